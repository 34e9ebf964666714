"""octvr_rig_morph_controlpoints on the case families of tests/morph_cases.py (test_morph_cases_host.py proves from the
oracle that each reaches its path): destination triangles off the ROI raster, folds, more than 255 triangles, every
frame clamp, masked control points, a camera without points, snapped duplicates, an ROI larger than the warp
kernel's grid, odd ROIs — then a second morph of a morphed template, a failed call, the seam masks, gains and all
three blenders downstream of a morphed mask, and the .dat round trip.  Bit-exact against the oracle, which morphs the
product's own pre-morph LUT (so only the morph is compared).  Parity unpinned, as in test_gpu_morph.py."""
import json

import numpy as np
import pytest

import morph_cases as MC
import oracle_py as O

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _luts(mt):
    return [mt.input(i)[:4] for i in range(len(mt))]


def _template(ox, name):
    rig, W, H, cps = MC.case(name)
    return ox.MapperTemplate.from_json(json.dumps(rig), W, H), rig, W, H, cps


def _oracle(name, before):
    """The oracle's morph of the product's pre-morph LUT, computed once per family and left unchanged."""
    if name not in _ORACLE:
        rig, W, H, cps = MC.case(name)
        _ORACLE[name] = O.morph_controlpoints(rig, before, W, H, cps)
    return _ORACLE[name]


def _assert_same(mt, want, want_tris):
    for i in range(len(mt)):
        st, dt = mt.triangles(i)
        assert np.array_equal(st.view(np.uint32), want_tris[i][0].view(np.uint32)), i
        assert np.array_equal(dt.view(np.uint32), want_tris[i][1].view(np.uint32)), i
        roi, g1, g2, gm, _ = mt.input(i)
        assert roi == tuple(want[i][0]), i
        assert np.array_equal(g1.view(np.uint32), want[i][1].view(np.uint32)), i
        assert np.array_equal(g2.view(np.uint32), want[i][2].view(np.uint32)), i
        assert np.array_equal(gm, want[i][3]), i


def _assert_untouched(mt, before, tris):
    for i in range(len(mt)):
        roi, g1, g2, gm, _ = mt.input(i)
        assert roi == before[i][0], i
        assert np.array_equal(g1.view(np.uint32), before[i][1].view(np.uint32)), i
        assert np.array_equal(g2.view(np.uint32), before[i][2].view(np.uint32)), i
        assert np.array_equal(gm, before[i][3]), i
        st, dt = mt.triangles(i)
        assert np.array_equal(st.view(np.uint32), tris[i][0].view(np.uint32)), i
        assert np.array_equal(dt.view(np.uint32), tris[i][1].view(np.uint32)), i


@pytest.mark.parametrize("name", MC.NAMES)
def test_gpu_morph_family_vs_oracle(product_lib, name):
    mt, rig, W, H, cps = _template(product_lib, name)
    before = _luts(mt)
    rc, want, want_tris = _oracle(name, before)
    assert rc == len(cps)
    assert mt.morph_controlpoints(cps) == rc
    _assert_same(mt, want, want_tris)
    assert sum(int((mt.input(i)[1] != before[i][1]).sum()) for i in range(len(mt))) > 1000


@pytest.mark.parametrize("name", ["big_jitter", "large_roi"])
def test_gpu_morph_twice(product_lib, name):
    """A morphed template morphed again: maps that already leave [0, 1), hold blends towards the border's 0 and
    graded masks are the warp's input."""
    mt, rig, W, H, cps = _template(product_lib, name)
    rc, want, _ = _oracle(name, _luts(mt))
    assert mt.morph_controlpoints(cps) == rc
    cps2 = MC.second(name)
    rc2, want2, tris2 = O.morph_controlpoints(rig, want, W, H, cps2)
    assert rc2 == len(cps2)
    assert mt.morph_controlpoints(cps2) == rc2
    _assert_same(mt, want2, tris2)
    assert sum(int((want2[i][1].view(np.uint32) != want[i][1].view(np.uint32)).sum()) for i in range(len(mt))) > 1000


@pytest.mark.parametrize("kind", ["outside_roi", "order", "camera"])
def test_gpu_morph_failed_call_changes_nothing(product_lib, kind):
    """A list whose last point is illegal fails as a whole (CV_Assert in the reference): the LUTs and the triangles
    of the previous morph stay, and the legal call afterwards gives what it would have given."""
    ox = product_lib
    name = "odd_size"
    mt, rig, W, H, cps = _template(ox, name)
    first = MC.second(name)
    assert mt.morph_controlpoints(first) == len(first)  # so that there are triangles to keep
    before = _luts(mt)
    tris = [mt.triangles(i) for i in range(len(mt))]
    with pytest.raises(ox.OctvrError) as e:
        mt.morph_controlpoints(cps + [MC.illegal_points(name)[kind]])
    assert e.value.code == ox.E_INVALID
    _assert_untouched(mt, before, tris)
    rc, want, want_tris = O.morph_controlpoints(rig, before, W, H, cps)
    assert mt.morph_controlpoints(cps) == rc == len(cps)
    _assert_same(mt, want, want_tris)


def test_gpu_morph_seams_of_a_graded_mask(product_lib):
    """create_masks on a morphed template: masks with values strictly between 0 and 255."""
    mt, rig, W, H, cps = _template(product_lib, "big_jitter")
    rc, want, _ = _oracle("big_jitter", _luts(mt))
    assert mt.morph_controlpoints(cps) == rc
    assert any(((w[3] > 0) & (w[3] < 255)).any() for w in want)
    mt.create_masks()
    seams = O.create_masks([w[0] for w in want], [w[3] for w in want], W)
    for i in range(len(mt)):
        np.testing.assert_array_equal(mt.input(i)[4], seams[i])


@pytest.mark.parametrize("blend", [0, 16, -8])
def test_gpu_morph_stitch_with_gain(product_lib, blend):
    """Gain plan, composite, multi-band and feather on the big_jitter template's morphed maps and graded masks."""
    ox = product_lib
    import torch
    mt, rig, W, H, cps = _template(ox, "big_jitter")
    rc, want, _ = _oracle("big_jitter", _luts(mt))
    assert mt.morph_controlpoints(cps) == rc
    sizes = [(480, 320)] * 3 + [(384, 192)]
    frames = [O.rand_img(w, h * 3 // 2, 1, 140 + i).reshape(h * 3 // 2, w) for i, (w, h) in enumerate(sizes)]
    seams = None
    if blend:
        mt.create_masks()
        seams = O.create_masks([w[0] for w in want], [w[3] for w in want], W)
    m = ox.Mapper(mt, sizes, blend=blend, enable_gain=True)
    out = torch.full((H * 3 // 2, W), 0xA5, dtype=torch.uint8, device="cuda")
    m.stitch([torch.from_numpy(f).cuda() for f in frames], out)
    torch.cuda.synchronize()
    frame, gains = O.stitch_frame(frames, sizes, [w[0] for w in want], [w[1] for w in want], [w[2] for w in want],
                                  [w[3] for w in want], W, H, enable_gain=True, blend=blend, seams=seams)
    np.testing.assert_array_equal(np.array(m.gains()), gains)
    np.testing.assert_array_equal(out.cpu().numpy(), frame)


def test_gpu_morph_dat_round_trip(product_lib, tmp_path):
    """.dat persists the morphed LUT of the dense family: more than 255 triangles, vertices beyond the clamp."""
    ox = product_lib
    mt, rig, W, H, cps = _template(ox, "dense")
    rc, want, _ = _oracle("dense", _luts(mt))
    assert mt.morph_controlpoints(cps) == rc
    p = tmp_path / "dense.dat"
    mt.dump(str(p))
    back = ox.MapperTemplate.load(str(p))
    assert len(back) == len(mt)
    for i in range(len(mt)):
        roi, g1, g2, gm, _ = back.input(i)
        assert roi == tuple(want[i][0])
        assert np.array_equal(g1.view(np.uint32), want[i][1].view(np.uint32)), i
        assert np.array_equal(g2.view(np.uint32), want[i][2].view(np.uint32)), i
        assert np.array_equal(gm, want[i][3]), i
