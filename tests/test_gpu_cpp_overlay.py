"""A template with overlays from a reference-style C++ caller of include/octvr.hpp
(tests/cpp/vr_overlay_test.cpp, built by build() as opencv-octvr_amd/lib/vr_overlay_test): the dump.cpp:84-93
flow (add_input for the inputs and the overlays, create_masks, dump), the .dat loaded back, then
vr::Mapper::stitch over the N + K frames.  Its output file and gains against tests/overlay_ref.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import overlay_ref as OR
import test_gpu_overlay as T

pytestmark = pytest.mark.gpu
BIN = os.path.join(OR.O.ROOT, "opencv-octvr_amd", "lib", "vr_overlay_test")


@pytest.mark.parametrize("blend", [0, 5])
def test_gpu_cpp_overlay(product_lib, tmp_path, blend):
    assert os.path.exists(BIN), "build() builds opencv-octvr_amd/lib/vr_overlay_test"
    ox = product_lib
    rig = T.rig_two()
    W, H = T.W, T.H
    n, k = len(rig["inputs"]), len(rig["overlays"])
    sizes = T._sizes(rig)
    frames = T._frames(sizes, 770)
    d = str(tmp_path)
    with open(os.path.join(d, "case.txt"), "w") as f:
        f.write("%s %d %d %d %d %d %d\n" % (rig["output"]["type"], W, H, n, k, blend, 1))
    open(os.path.join(d, "out_opts.json"), "w").write(json.dumps(rig["output"]["options"]))
    for i, cam in enumerate(rig["inputs"] + rig["overlays"]):
        open(os.path.join(d, "cam%d_opts.json" % i), "w").write(json.dumps(cam["options"]))
        open(os.path.join(d, "cam%d.txt" % i), "w").write("%s %d %d\n" % (cam["type"], sizes[i][0], sizes[i][1]))
        frames[i].tofile(os.path.join(d, "frame%d.yuv" % i))
    r = subprocess.run([BIN, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and os.path.exists(os.path.join(d, "ok_overlay")), r.stderr[-3000:]
    t = OR.prepare(ox.MapperTemplate.from_json(json.dumps(rig), W, H), blend)
    want, g_want = OR.expected(t, frames, sizes, blend=blend)
    got = np.fromfile(os.path.join(d, "out_overlay.yuv"), np.uint8).reshape(H * 3 // 2, W)
    g = np.array([float(v) for v in open(os.path.join(d, "gains_overlay.txt")).read().split()])
    assert len(g) == n
    np.testing.assert_array_equal(g, np.asarray(g_want))
    diff = got != want
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5].tolist())
