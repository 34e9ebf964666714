"""vr::Mapper::set_pixel_formats with OCTVR_PIX_V210 (include/octvr.hpp) from a C++ caller (tests/cpp/vr_v210_test.cpp,
built by build() as opencv-octvr_amd/lib/vr_v210_test): v210 frames in, v210 out into a frame the mapper creates, on rigA
with blend 0, against the oracle's stitch of the frames converted by tests/v210_ref.py's in rule, stored by its out
rule."""
import os
import subprocess

import numpy as np
import pytest

import oracle_py as O
import v210_ref as V
import yuv10_ref as R10
from test_gpu_cpp_api import _spans

pytestmark = pytest.mark.gpu
BIN = os.path.join(O.ROOT, "opencv-octvr_amd", "lib", "vr_v210_test")


def test_gpu_cpp_v210(product_lib, tmp_path):
    assert os.path.exists(BIN), "build() builds opencv-octvr_amd/lib/vr_v210_test"
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
    sizes, frames = [], []
    for i, cam in enumerate(rig["inputs"]):
        w, h = cam["options"]["width"], cam["options"]["height"]
        sizes.append((w, h))
        a, b = sp[("inputs", i, "options")]
        open(os.path.join(d, "in%d_opts.json" % i), "w").write(text[a:b])
        open(os.path.join(d, "in%d.txt" % i), "w").write("%s %d %d\n" % (cam["type"], w, h))
        pic = R10.noise_picture(synthetic.smooth_yuv_frame(w, h, 640 + i), w, h, 30 + i, edges=i == 0)
        laid = V.lay_out(*pic, seed=70 + i)
        frames.append(V.in_rule(laid, w, h))
        laid.tofile(os.path.join(d, "frame%d.v210" % i))
    r = subprocess.run([BIN, d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and os.path.exists(os.path.join(d, "ok_v210")), r.stderr[-3000:]
    want, g_orc = O.stitch_frame(frames, sizes, z["rois"].tolist(), [z[f"map1_{i}"] for i in range(n)],
                                 [z[f"map2_{i}"] for i in range(n)], [z[f"mask_{i}"] for i in range(n)], W, H,
                                 enable_gain=True, blend=blend, threads=8)
    expect = V.out_rule(want, W, H)
    got = np.fromfile(os.path.join(d, "out.v210"), np.uint8).reshape(expect.shape)
    g = [float(v) for v in open(os.path.join(d, "gains_v210.txt")).read().split()]
    np.testing.assert_array_equal(np.array(g), np.array(g_orc))
    diff = got != expect
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5].tolist())
