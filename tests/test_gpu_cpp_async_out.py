"""vr::AsyncMultiMapper::set_output_format (include/octvr.hpp) from a C++ caller (tests/cpp/vr_async_out_test.cpp,
built by build() as opencv-octvr_amd/lib/vr_async_out_test): rigA through AsyncMultiMapper::New, planar frames in, one
frame merged as UYVY and one as P010 into padded planes; each output file against tests/async_out_ref.py's out rule
applied to the oracle's stitch."""
import os
import subprocess

import numpy as np
import pytest

import async_out_ref as R
import oracle_py as O
from test_gpu_cpp_api import _spans

pytestmark = pytest.mark.gpu
BIN = os.path.join(O.ROOT, "opencv-octvr_amd", "lib", "vr_async_out_test")


def test_gpu_cpp_async_out(product_lib, tmp_path):
    assert os.path.exists(BIN), "build() builds opencv-octvr_amd/lib/vr_async_out_test"
    from octvr_amd import synthetic
    name, blend = "rigA", 0
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
    for f in range(2):
        fr = [synthetic.smooth_yuv_frame(w, h, 6300 + 10 * f + i) for i, (w, h) in enumerate(sizes)]
        for i, (w, h) in enumerate(sizes):
            np.ascontiguousarray(fr[i][:, :w]).tofile(os.path.join(d, "frame%d_%d.yuv" % (i, f)))
        frames.append(fr)
    r = subprocess.run([BIN, d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and os.path.exists(os.path.join(d, "ok_async_out")), r.stderr[-3000:]
    for f, (fmt, out) in enumerate((("uyvy422", "out_async_uyvy.bin"), ("p010", "out_async_p010.bin"))):
        want, _ = O.stitch_frame(frames[f], sizes, z["rois"].tolist(), [z[f"map1_{i}"] for i in range(n)],
                                 [z[f"map2_{i}"] for i in range(n)], [z[f"mask_{i}"] for i in range(n)], W, H,
                                 enable_gain=True, blend=blend, threads=8)
        expect = R.merged_frame(fmt, W, H, [(0, 0, want)])
        got = np.fromfile(os.path.join(d, out), np.uint8).reshape(expect.shape)
        diff = got != expect
        assert not diff.any(), (fmt, int(diff.sum()), np.argwhere(diff)[:5].tolist())
