"""tests/overlay_ref.py against itself and the oracle, on the CPU: the two constructions of the expected
overlay output agree on a blend-0 rig (output, scaled output, preview), and the composed one with K = 0 is
orc_stitch_frame for the multi-band and the feather blender.  That licenses composed() as the expectation of
the blend != 0 GPU tests (tests/test_gpu_overlay.py).  Independent of the product: it passes without it."""
import copy

import numpy as np
import pytest

import camera_rigs as R
import oracle_py as O
import overlay_ref as OR

W, H = 512, 256


def _frames(sizes, seed):
    return [O.rand_img(w, h * 3 // 2, 1, seed + i) for i, (w, h) in enumerate(sizes)]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and np.array_equal(x, y), int((x != y).sum())


@pytest.mark.parametrize("remap_tex", [False, True])
def test_chain_equals_composed_blend0(remap_tex):
    rig = R.mask_rigs()["overlay_include"]
    t = OR.prepare_oracle(rig, W, H)
    assert t["n"] == 2 and t["k"] == 1 and (t["masks"][2] != 0).any()
    sizes = [(640, 360)] * 2 + [(192, 128)]
    frames = _frames(sizes, 11)
    vig = [None, None, O.resize_linear_cuda_f32(O.vignette_map({"vignette": [1.1, -0.35, 0.12, -0.04]}), 192, 128)]
    for kw in ({}, {"scale": (384, 192), "preview": (200, 100)}, {"vig": vig}, {"enable_gain": False}):
        _same(OR.chain(t, frames, sizes, remap_tex=remap_tex, **kw),
              OR.composed(t, frames, sizes, blend=0, remap_tex=remap_tex, **kw))


@pytest.mark.parametrize("blend", [5, -4])
def test_composed_without_overlays_is_stitch_frame(blend):
    rig = copy.deepcopy(R.mask_rigs()["overlay_include"])
    del rig["overlays"]
    t = OR.prepare_oracle(rig, W, H, blend=blend)
    assert t["k"] == 0
    sizes = [(640, 360)] * 2
    frames = _frames(sizes, 23)
    for kw in ({}, {"scale": (384, 192), "preview": (200, 100)}):
        want = O.stitch_frame(frames, sizes, t["rois"], t["map1"], t["map2"], t["masks"], W, H, enable_gain=True,
                              blend=blend, seams=t["seams"], threads=8, **kw)
        _same(OR.composed(t, frames, sizes, blend=blend, **kw), want)
