"""vr::AsyncMultiMapper::set_pixel_formats (include/octvr.hpp) from a C++ caller (tests/cpp/vr_async_nv12_test.cpp,
built by build() as opencv-octvr_amd/lib/vr_async_nv12_test): rigA through AsyncMultiMapper::New, NV12 planes in
and out with the U,V planes as CV_8UC2 Mats, 4 frames pushed before the first pop, each output file against the
oracle's stitch of the planar frames with the chroma rearranged by this file's own numpy."""
import os
import subprocess

import numpy as np
import pytest

import oracle_py as O
from test_gpu_cpp_api import _spans

pytestmark = pytest.mark.gpu
BIN = os.path.join(O.ROOT, "opencv-octvr_amd", "lib", "vr_async_nv12_test")


def _nv12(f, w, h):
    m = np.empty((h * 3 // 2, w), np.uint8)
    m[:h] = f[:h]
    m[h:, 0::2] = f[h:, :w // 2]
    m[h:, 1::2] = f[h:, w // 2:]
    return m


def test_gpu_cpp_async_nv12(product_lib, tmp_path):
    assert os.path.exists(BIN), "build() builds opencv-octvr_amd/lib/vr_async_nv12_test"
    from octvr_amd import synthetic
    name, blend, nf = "rigA", 0, 4
    text = open(os.path.join(O.ROOT, "tests", "golden", name + ".json")).read()
    rig, z = O.load_rig(name)
    W, H = (int(v) for v in z["out_size"])
    n = len(rig["inputs"])
    sp = _spans(text)
    d = str(tmp_path)
    with open(os.path.join(d, "case.txt"), "w") as f:
        f.write("%s %d %d %d %d %d %d %d\n" % (rig["output"]["type"], W, H, n, blend, 0, 0, 1))
    a, b = sp[("output", "options")]
    open(os.path.join(d, "out_opts.json"), "w").write(text[a:b])
    sizes = []
    for i, cam in enumerate(rig["inputs"]):
        w, h = cam["options"]["width"], cam["options"]["height"]
        sizes.append((w, h))
        a, b = sp[("inputs", i, "options")]
        open(os.path.join(d, "in%d_opts.json" % i), "w").write(text[a:b])
        open(os.path.join(d, "in%d.txt" % i), "w").write("%s %d %d\n" % (cam["type"], w, h))
    frames = []
    for f in range(nf):
        fr = [synthetic.smooth_yuv_frame(w, h, 6100 + 10 * f + i) for i, (w, h) in enumerate(sizes)]
        for i, (w, h) in enumerate(sizes):
            _nv12(fr[i], w, h).tofile(os.path.join(d, "frame%d_%d.yuv" % (i, f)))
        frames.append(fr)
    r = subprocess.run([BIN, d, str(nf)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and os.path.exists(os.path.join(d, "ok_async_nv12")), r.stderr[-3000:]
    for f in range(nf):
        want, _ = O.stitch_frame(frames[f], sizes, z["rois"].tolist(), [z[f"map1_{i}"] for i in range(n)],
                                 [z[f"map2_{i}"] for i in range(n)], [z[f"mask_{i}"] for i in range(n)], W, H,
                                 enable_gain=True, blend=blend, threads=8)
        got = np.fromfile(os.path.join(d, "out_async_nv12_%d.yuv" % f), np.uint8).reshape(H * 3 // 2, W)
        diff = got != _nv12(want, W, H)
        assert not diff.any(), (f, int(diff.sum()), np.argwhere(diff)[:5].tolist())
