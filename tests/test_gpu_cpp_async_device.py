"""vr::AsyncMultiMapper::push_device (include/octvr.hpp) from a C++ caller (tests/cpp/vr_async_device_test.cpp,
built by build() as opencv-octvr_amd/lib/vr_async_device_test): rigA twice through AsyncMultiMapper::New, top
and bottom halves of a W x 2H merged frame, device frames from octvr_dev_malloc at padded pitches, 3 frames
pushed before the first pop; each merged frame the program downloads against the oracle's stitch per region,
the pitch padding still holding the fill byte."""
import os
import subprocess

import numpy as np
import pytest

import oracle_py as O
from test_gpu_cpp_api import _spans

pytestmark = pytest.mark.gpu
BIN = os.path.join(O.ROOT, "opencv-octvr_amd", "lib", "vr_async_device_test")


def test_gpu_cpp_async_device(product_lib, tmp_path):
    assert os.path.exists(BIN), "build() builds opencv-octvr_amd/lib/vr_async_device_test"
    from octvr_amd import synthetic
    name, blend, nf = "rigA", 0, 3
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
        fr = [synthetic.smooth_yuv_frame(w, h, 8300 + 10 * f + i) for i, (w, h) in enumerate(sizes)]
        for i in range(n):
            np.ascontiguousarray(fr[i]).tofile(os.path.join(d, "frame%d_%d.yuv" % (i, f)))
        frames.append(fr)
    r = subprocess.run([BIN, d, str(nf)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and os.path.exists(os.path.join(d, "ok_async_device")), r.stderr[-3000:]
    pitch = W + 32
    for f in range(nf):
        want, _ = O.stitch_frame(frames[f], sizes, z["rois"].tolist(), [z[f"map1_{i}"] for i in range(n)],
                                 [z[f"map2_{i}"] for i in range(n)], [z[f"mask_{i}"] for i in range(n)], W, H,
                                 enable_gain=True, blend=blend, threads=8)
        got = np.fromfile(os.path.join(d, "out_async_device_%d.yuv" % f), np.uint8).reshape(3 * H, pitch)
        assert (got[:, W:] == 0x5A).all(), (f, "pitch padding written")
        # both regions hold the same stitch (the second mapper takes the first one's gains): region k's Y rows
        # at k H, its chroma rows at 2 H + k H / 2, U in the left and V in the right half of the merged rows
        for k in range(2):
            assert np.array_equal(got[k * H:(k + 1) * H, :W], want[:H]), (f, k, "Y")
            c0 = 2 * H + k * H // 2
            assert np.array_equal(got[c0:c0 + H // 2, :W], want[H:]), (f, k, "UV")
