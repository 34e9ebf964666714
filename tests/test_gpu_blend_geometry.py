"""Multi-band and feather blends at geometries off the tile grid: output sizes that are no multiple of the
128 x 8 tile, the 32 x 8 sub-tile or the 8 x 8 block, ROI unions that start away from the frame's origin and
do not cover the frame, aligned result ROIs that round_up carries past the frame (the crop), per-camera ROIs
at their own offsets, and feather ROIs of odd origin and odd size.

Every rig is a ring of fisheye cameras (160 x 120 inputs) projected to 200 x 100 by the oracle's LUT build --
bit-equal to the library's own (test_gpu_base_arrays_are_the_librarys here, test_gpu_parity.py) -- whose
per-camera arrays are then optionally sliced to sub-rectangles, shifted by an offset and placed into an even
output frame with MapperTemplate.from_arrays.  The expected frame is the oracle's stitch of the same arrays:
bit-exact, Y and both chroma planes, and the estimated gains too.  Each test also asserts, from
Mapper.info() and from the rectangles of blenders.cpp:595-618 restated here, that its geometry reaches the
code path it is meant for.  Output tensors start as 0x5A bytes, so a byte the stitch leaves unwritten shows.

test_blend_geometry_oracle_properties needs no GPU: it runs the oracle over every geometry and checks what
the reference alone must satisfy."""
import json
import math

import numpy as np
import pytest

import oracle_py as O

gpu = pytest.mark.gpu
IN_W, IN_H = 160, 120
BASE_W, BASE_H = 200, 100  # 200: no multiple of 128 or 32; 100: no multiple of 8

# ---- geometries: n cameras, per-camera slices (x0, y0, x1, y1) of the base arrays, an offset, a frame ----
SLICES3 = [(54, 0, 182, 92), (0, 10, 200, 100), (0, 0, 200, 90)]     # even rectangles, union 200 x 100
SLICES3_MIXED = [(55, 0, 146, 91), (0, 11, 199, 100), (0, 0, 200, 90)]  # odd and even corners mixed
GEOMETRIES = {
    "full":        dict(n=3, offset=(0, 0), frame=(200, 100)),
    "full_sliced": dict(n=3, slices=SLICES3, offset=(0, 0), frame=(200, 100)),
    "shift40":     dict(n=3, slices=SLICES3, offset=(40, 24), frame=(300, 150)),
    "shift7":      dict(n=3, offset=(7, 3), frame=(236, 118)),
    "shift16":     dict(n=3, offset=(16, 8), frame=(232, 116)),
    "odd_x":       dict(n=3, offset=(7, 4), frame=(208, 104)),
    "odd_y":       dict(n=3, offset=(6, 3), frame=(206, 104)),
    "odd_xy":      dict(n=3, offset=(7, 3), frame=(208, 104)),
    "odd_size":    dict(n=3, slices=[(0, 0, 199, 99)] * 3, offset=(0, 0), frame=(200, 100)),
    "odd_size_xy": dict(n=3, slices=[(0, 0, 199, 99)] * 3, offset=(1, 1), frame=(200, 100)),
    "odd_mixed":   dict(n=3, slices=SLICES3_MIXED, offset=(3, 5), frame=(204, 106)),
    "single_odd":  dict(n=1, slices=[(0, 0, 199, 99)], offset=(5, 3), frame=(206, 104)),
}

_BASE, _RIGS, _WANT = {}, {}, {}


def ring_json(n):
    from octvr_amd import synthetic
    return synthetic.fisheye_rig(IN_W, IN_H, [2 * math.pi * k / n for k in range(n)],
                                 [0.35 * (-1) ** k for k in range(n)])


def base_arrays(n):
    if n not in _BASE:
        _BASE[n] = O.lut_build(O.json_loads_rj(json.dumps(ring_json(n))), BASE_W, BASE_H, threads=4)
    return _BASE[n]


def make_rig(name):
    """The rig of GEOMETRIES[name]: base arrays -> slices -> offset -> frame; seams from the oracle."""
    if name in _RIGS:
        return _RIGS[name]
    g = GEOMETRIES[name]
    n, (dx, dy), (W, H) = g["n"], g["offset"], g["frame"]
    assert W % 2 == 0 and H % 2 == 0
    t = dict(name=name, W=W, H=H, n=n, sizes=[(IN_W, IN_H)] * n, rois=[], maps1=[], maps2=[], masks=[])
    for i, (roi, m1, m2, mk) in enumerate(base_arrays(n)):
        x0, y0, x1, y1 = g["slices"][i] if g.get("slices") else (0, 0, roi[2], roi[3])
        assert 0 <= x0 < x1 <= roi[2] and 0 <= y0 < y1 <= roi[3]
        t["rois"].append((roi[0] + x0 + dx, roi[1] + y0 + dy, x1 - x0, y1 - y0))
        for key, a in (("maps1", m1), ("maps2", m2), ("masks", mk)):
            t[key].append(np.ascontiguousarray(a[y0:y1, x0:x1]))
    t["seams"] = O.create_masks(t["rois"], t["masks"], W)
    _RIGS[name] = t
    return t


# ---- the rectangles of blenders.cpp:479-486, 595-618 (feather: the ROIs themselves, B = 0) ----------------
def bands_of(blend):
    return O.blend_bands(blend) if blend > 0 else 0


def aligned_rois(rois, blend):
    """(align_result_roi, [per-camera align_roi]) as (x, y, w, h)."""
    B = bands_of(blend)
    dn = lambda v: (v >> B) << B
    up = lambda v: -((-v >> B) << B)
    x0, y0 = min(r[0] for r in rois), min(r[1] for r in rois)
    x1, y1 = max(r[0] + r[2] for r in rois), max(r[1] + r[3] for r in rois)
    arr = (dn(x0), dn(y0), up(x1) - dn(x0), up(y1) - dn(y0))
    gap = 5 << B if blend > 0 else 0
    ar = []
    for x, y, w, h in rois:
        l, t = max(arr[0], dn(x) - gap), max(arr[1], dn(y) - gap)
        r, b = min(arr[0] + arr[2], up(x + w) + gap), min(arr[1] + arr[3], up(y + h) + gap)
        ar.append((l, t, r - l, b - t))
    return arr, ar


def outside_masks(t, blend, W=None, H=None):
    """(luma pixels, chroma cells) of the frame wholly outside align_result_roi, as bool arrays."""
    W, H = W or t["W"], H or t["H"]
    (ax, ay, aw, ah), _ = aligned_rois(t["rois"], blend)
    luma = np.ones((H, W), bool)
    luma[ay:ay + ah, ax:ax + aw] = False
    return luma, luma[0::2, 0::2] & luma[0::2, 1::2] & luma[1::2, 0::2] & luma[1::2, 1::2]


def assert_black_outside(frame, t, blend, what, W=None, H=None):
    """Nothing is blended outside align_result_roi: Y 0, U = V = 128 (the zeroed result image converted)."""
    W, H = W or t["W"], H or t["H"]
    luma, cells = outside_masks(t, blend, W, H)
    assert luma.any(), (what, "the ROI union covers the frame")  # (an odd last column alone: no whole cell)
    assert (frame[:H][luma] == 0).all(), (what, "luma outside align_result_roi")
    assert (frame[H:, :W // 2][cells] == 128).all() and (frame[H:, W // 2:W][cells] == 128).all(), \
        (what, "chroma outside align_result_roi")


# ---- frames and the oracle's frame (computed once per case, never modified) -------------------------------
def frames_of(t, kind, seed=0):
    from octvr_amd import synthetic
    if kind == "smooth":  # estimated gains
        return [synthetic.smooth_yuv_frame(w, h, 3100 + seed + i) for i, (w, h) in enumerate(t["sizes"])], None
    if kind == "contrast":  # 0 / 255 luma checkerboards of period 1, 2, 4 px per camera, chroma 128; gains 1
        frames = []
        for i, (w, h) in enumerate(t["sizes"]):
            yy, xx = np.mgrid[0:h, 0:w]
            per = 1 << (i + seed) % 3
            f = np.full((h * 3 // 2, w), 128, np.uint8)
            f[:h] = ((xx // per + yy // per + seed) & 1) * 255
            frames.append(f)
        return frames, [1.0] * t["n"]
    frames = [O.rand_img(w, h * 3 // 2, 1, 7700 + seed + i) for i, (w, h) in enumerate(t["sizes"])]
    return frames, ([1.0 + 0.012 * k * (-1) ** k for k in range(t["n"])] if t["n"] > 1 else None)


def oracle_case(name, blend, kind, scale=None, tex=False, seed=0):
    key = (name, blend, kind, scale, tex, seed)
    if key not in _WANT:
        t = make_rig(name)
        frames, gains = frames_of(t, kind, seed)
        want, g = O.stitch_frame(frames, t["sizes"], t["rois"], t["maps1"], t["maps2"], t["masks"], t["W"], t["H"],
                                 enable_gain=True, gains=gains, blend=blend, seams=t["seams"], threads=4, scale=scale,
                                 remap_tex=tex)
        want.setflags(write=False)
        _WANT[key] = (frames, gains, want, np.array(g))
    return _WANT[key]


# ---- the host half: runs without a GPU --------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_blend_geometry_oracle_properties(name):
    """The reference side of every geometry: the oracle stitches it for every blend mode used below, leaves
    Y 0 / U = V = 128 outside align_result_roi, and -- with fixed gains, in a frame that holds the whole
    aligned ROI -- gives the same bytes whichever larger even frame the rig is embedded in."""
    t = make_rig(name)
    W, H = t["W"], t["H"]
    frames, gains = frames_of(t, "noise")
    for blend in (4, 16, 40, -3, -8):
        if t["n"] == 1 and blend > 0:
            continue
        (ax, ay, aw, ah), ar = aligned_rois(t["rois"], blend)
        for (x, y, w, h), (l, tp, cw, ch) in zip(t["rois"], ar):  # each ROI inside its aligned ROI inside arr
            assert ax <= l <= x and ay <= tp <= y and x + w <= l + cw <= ax + aw and y + h <= tp + ch <= ay + ah
        kw = dict(enable_gain=True, gains=gains, blend=blend, seams=t["seams"], threads=4)
        want, _ = O.stitch_frame(frames, t["sizes"], t["rois"], t["maps1"], t["maps2"], t["masks"], W, H, **kw)
        luma, _ = outside_masks(t, blend)
        if luma.any():
            assert_black_outside(want, t, blend, (name, blend))
        if ax + aw > W or ay + ah > H:
            continue  # the crop: a larger frame shows more of the aligned ROI
        W2, H2 = W + 22, H + 10
        big, _ = O.stitch_frame(frames, t["sizes"], t["rois"], t["maps1"], t["maps2"], t["masks"], W2, H2, **kw)
        assert_black_outside(big, t, blend, (name, blend, "larger frame"), W2, H2)
        assert np.array_equal(big[:H, :W], want[:H]), (name, blend)
        for x0s, x0b in ((0, 0), (W // 2, W2 // 2)):  # U, V
            assert np.array_equal(big[H2:H2 + H // 2, x0b:x0b + W // 2], want[H:, x0s:x0s + W // 2]), (name, blend)


# ---- the GPU half -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ox(product_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return product_lib


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _out(w, h):
    import torch
    return torch.full((h * 3 // 2, w), 0x5A, dtype=torch.uint8, device="cuda")


_TEMPLATES = {}


def template(ox, t):
    """from_arrays + create_masks(0); the seams read back equal the oracle's."""
    if t["name"] not in _TEMPLATES:
        mt = ox.MapperTemplate.from_arrays(t["W"], t["H"], t["rois"], t["maps1"], t["maps2"], t["masks"])
        mt.create_masks(0)
        for i in range(t["n"]):
            assert mt.input(i)[0] == tuple(t["rois"][i])
            assert np.array_equal(mt.input(i)[4], t["seams"][i]), (t["name"], i)
        _TEMPLATES[t["name"]] = mt
    return _TEMPLATES[t["name"]]


def check_rects(info, t, blend):
    """info() reports the reference's align_result_roi for these ROIs, and the band count."""
    arr, _ = aligned_rois(t["rois"], blend)
    assert info["align_result_roi"] == list(arr), (info["align_result_roi"], arr)
    assert info["bands"] == bands_of(blend)
    return arr


def stitch_case(ox, name, blend, kind, scale=None, out_fmt="yuv420p", remap="remap", rig=None, case=None, mt=None):
    """One stitch of geometry `name` against the oracle: (info, align_result_roi, got, want).  rig, case, mt:
    the rig's arrays, its oracle_case and its template where they are not make_rig(name)'s (other seams)."""
    import torch
    from test_gpu_nv12 import check
    t = rig or make_rig(name)
    frames, gains, want, g_orc = case or oracle_case(name, blend, kind, scale, remap == "texture")
    m = ox.Mapper(mt or template(ox, t), t["sizes"], blend=blend, enable_gain=True, scale_output=scale, remap=remap)
    if out_fmt != "yuv420p":
        m.set_pixel_formats("yuv420p", out_fmt)
    info = m.info()
    arr = check_rects(info, t, blend) if t["n"] > 1 else None
    ow, oh = scale or (t["W"], t["H"])
    out = _out(ow, oh)
    m.stitch([_cuda(f) for f in frames], out, gains=gains)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(np.array(m.gains()), g_orc)
    got = out.cpu().numpy()
    check(got, want, t, out_fmt, (name, blend, kind, scale, remap))
    return info, arr, got, want


@gpu
def test_gpu_base_arrays_are_the_librarys(ox):
    """The base arrays (the oracle's LUT build) are what the library's template of the same ring gives."""
    for n in (1, 3):
        mt = ox.MapperTemplate.from_json(json.dumps(ring_json(n)), BASE_W, BASE_H)
        for i, (roi, m1, m2, mk) in enumerate(base_arrays(n)):
            r, g1, g2, gk, _ = mt.input(i)
            assert r == tuple(roi) and np.array_equal(gk, mk)
            assert np.array_equal(g1.view(np.int32), m1.view(np.int32))
            assert np.array_equal(g2.view(np.int32), m2.view(np.int32))


# 1. off the tile grid, the ROI union is the frame ----------------------------------------------------------
@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("blend", [4, 8, 40, -5])
@gpu
def test_gpu_offgrid_full_cover(ox, blend, kind):
    """200 x 100: partial last tiles, sub-tiles and 8 x 8 blocks at every level; blend 40 (5 bands) aligns the
    result ROI to 224 x 128, past the frame both ways (the level-0 crop)."""
    W, H = GEOMETRIES["full"]["frame"]
    assert W % 128 and W % 32 and H % 8
    info, arr, _, _ = stitch_case(ox, "full", blend, kind)
    assert arr[:2] == (0, 0) and arr[2] >= W and arr[3] >= H and info["full_cover"] == 1
    B = info["bands"]
    assert any((arr[2] >> l) % 8 or (arr[3] >> l) % 8 for l in range(B + 1))
    if blend == 40:
        assert B == 5 and arr[2] > W and arr[3] > H and arr[2:] == (224, 128)
        assert info["crop"] == [W, H]


# 2. shifted, not covering the frame; per-camera aligned ROIs off the 8 x 8 blocks --------------------------
@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("blend", [4, 16])
@pytest.mark.parametrize("name", ["shift40", "shift7"])
@gpu
def test_gpu_multiband_shifted_not_covering(ox, name, blend, kind):
    t = make_rig(name)
    info, arr, got, want = stitch_case(ox, name, blend, kind)
    assert info["full_cover"] == 0
    if name == "shift40":
        assert arr[0] > 0 and arr[1] > 0
        _, ar = aligned_rois(t["rois"], blend)
        # some camera starts off the 8 x 8 block grid of some level (block_activity's ox & 7)
        assert any((((l - arr[0]) >> lv) & 7) or (((tp - arr[1]) >> lv) & 7)
                   for (l, tp, _, _) in ar for lv in range(info["bands"] + 1))
    assert_black_outside(want, t, blend, (name, blend, "oracle"))
    assert_black_outside(got, t, blend, (name, blend, "gpu"))


# 3. deep sub-tiles written by the remap at a non-zero origin, and the ones it must leave to the blend ------
def _deep0(info):
    return info["level_tiles"][0]["deep_subtiles"]  # written by the remap or not


@pytest.mark.parametrize("name", ["shift40", "shift16"])
@gpu
def test_gpu_deep_subtiles_in_remap_at_nonzero_origin(ox, name, monkeypatch):
    """The remap writes deep level-0 sub-tiles into the result at align_result_roi's origin (RgbaOut::res and
    the chroma offsets); without that (OCTVR_MB_NO_REMAP_RESULT) and without deep tiles at all
    (OCTVR_MB_NO_DEEP) the same bytes come out."""
    info, arr, got, _ = stitch_case(ox, name, 4, "smooth")
    assert arr[0] > 0 and arr[1] > 0 and info["remap_result_subtiles"] > 0
    assert all(lt["deep_subtiles"] <= lt["owned_subtiles"] for lt in info["level_tiles"])
    monkeypatch.setenv("OCTVR_MB_NO_REMAP_RESULT", "1")
    info2, _, got2, _ = stitch_case(ox, name, 4, "smooth")
    assert info2["remap_result_subtiles"] == 0 and _deep0(info2) == _deep0(info) > 0
    monkeypatch.delenv("OCTVR_MB_NO_REMAP_RESULT")
    monkeypatch.setenv("OCTVR_MB_NO_DEEP", "1")
    info3, _, got3, _ = stitch_case(ox, name, 4, "smooth")
    assert _deep0(info3) == 0 and info3["remap_result_subtiles"] == 0
    assert np.array_equal(got, got2) and np.array_equal(got, got3)


@pytest.mark.parametrize("name,blend", [("full", 4), ("shift40", 4), ("shift40", 16)])
@gpu
def test_gpu_deep_subtiles_across_the_crop_edge(ox, name, blend, monkeypatch):
    """A deep sub-tile whose 32 x 8 extent crosses the crop (the level's last, partial sub-tiles) is not given
    to the remap, whose result stores take no bounds: the level-0 blend writes it, clipped.  Bit-exact with
    and without the remap's result stores."""
    info, arr, got, _ = stitch_case(ox, name, blend, "noise")
    crop = info["crop"]
    assert crop[0] % 32 or crop[1] % 8
    # every deep level-0 sub-tile inside the crop goes to the remap: the rest cross its edge
    assert 0 < info["remap_result_subtiles"] < _deep0(info), (info["remap_result_subtiles"], _deep0(info))
    monkeypatch.setenv("OCTVR_MB_NO_REMAP_RESULT", "1")
    info2, _, got2, _ = stitch_case(ox, name, blend, "noise")
    assert info2["remap_result_subtiles"] == 0 and _deep0(info2) == _deep0(info)
    assert np.array_equal(got, got2)


# 4. feather: odd origins and sizes -------------------------------------------------------------------------
FEATHER_ODD = {"odd_x": (1, 0, 0, 0), "odd_y": (0, 1, 0, 0), "odd_xy": (1, 1, 0, 0), "odd_size": (0, 0, 1, 1),
               "odd_size_xy": (1, 1, 1, 1)}


@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("blend", [-3, -8])
@pytest.mark.parametrize("name", sorted(FEATHER_ODD))
@gpu
def test_gpu_feather_odd_geometry(ox, name, blend, kind):
    """FeatherGPUBlender takes the ROI union as it is: an odd origin puts its pixel pairs across the output's
    chroma cells, an odd size leaves the last column / row without a partner."""
    t = make_rig(name)
    info, arr, got, want = stitch_case(ox, name, blend, kind)
    assert info.get("feather") == 1 and tuple(v & 1 for v in arr) == FEATHER_ODD[name]
    gx, gy, gw, gh = info["grid_roi"]  # the even rectangle the kernels work on
    assert (gx | gy | gw | gh) & 1 == 0 and gx <= arr[0] and gy <= arr[1]
    assert gx + gw >= arr[0] + arr[2] and gy + gh >= arr[1] + arr[3]
    if outside_masks(t, blend)[0].any():
        assert_black_outside(got, t, blend, (name, blend, "gpu"))


@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("blend", [-3, -8])
@gpu
def test_gpu_feather_cameras_of_mixed_parity(ox, blend, kind):
    """Cameras whose ROIs start and end on odd and on even pixels of one result ROI: the quads of the level-0
    grid cannot be whole pixel pairs of every camera."""
    t = make_rig("odd_mixed")
    assert len({(x & 1, y & 1) for x, y, _, _ in t["rois"]}) > 1
    assert any(w & 1 for _, _, w, _ in t["rois"]) and any(h & 1 for _, _, _, h in t["rois"])
    # the cut edges carry weight: a mask set along a ROI's first and last column, deeper than the border
    for mk in t["masks"][:2]:
        assert (mk[:, 0] > 0).sum() > 20 and (mk[:, -1] > 0).sum() > 20
    _, _, got, _ = stitch_case(ox, "odd_mixed", blend, kind)
    assert_black_outside(got, t, blend, ("odd_mixed", blend, "gpu"))


@pytest.mark.parametrize("blend", [-3, 0])
@gpu
def test_gpu_single_camera_odd_roi(ox, blend):
    """n = 1 (the Mapper then stitches without blend or gain, mapper.cpp:78-82) at an odd origin and size."""
    import torch
    t = make_rig("single_odd")
    assert all(v & 1 for v in t["rois"][0])
    frames, _, want, _ = oracle_case("single_odd", blend, "noise")
    m = ox.Mapper(template(ox, t), t["sizes"], blend=blend, enable_gain=True)
    out = _out(t["W"], t["H"])
    m.stitch([_cuda(f) for f in frames], out)
    torch.cuda.synchronize()
    assert m.gains() == [1.0]
    got = out.cpu().numpy()
    d = got != want
    assert not d.any(), (int(d.sum()), np.argwhere(d)[:6].tolist())
    assert_black_outside(got, t, -3, "single_odd")


# 5. scaled output: the RGBA result image ------------------------------------------------------------------
@pytest.mark.parametrize("name,blend", [("shift40", 4), ("shift40", 16), ("odd_xy", -3), ("odd_size_xy", -8),
                                        ("odd_mixed", -3)])
@gpu
def test_gpu_scaled_output_off_origin(ox, name, blend):
    """Half the frame (rounded down to even sizes, which a YUV420 output needs)."""
    t = make_rig(name)
    scale = (t["W"] // 2 & ~1, t["H"] // 2 & ~1)
    info, _, _, _ = stitch_case(ox, name, blend, "smooth", scale=scale)
    assert info["scaled_out"] == list(scale)
    # (odd_size_xy: the even rectangle around x, y = 1 .. 200, 1 .. 100 is the whole frame)
    assert info["full_cover"] == (1 if name == "odd_size_xy" else 0)


# 6. NV12 output -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,blend", [("shift40", 4), ("shift7", 16), ("odd_xy", -3), ("odd_mixed", -8)])
@gpu
def test_gpu_nv12_output_off_origin(ox, name, blend):
    info, arr, _, _ = stitch_case(ox, name, blend, "smooth", out_fmt="nv12")
    assert info["full_cover"] == 0
    if name == "shift40":
        assert info["remap_result_subtiles"] > 0 and arr[0] > 0  # the remap's U,V pairs at arr.x & ~1


# 7. frames in flight --------------------------------------------------------------------------------------
@gpu
def test_gpu_frames_in_flight_shifted(ox):
    """Two slots, four frames on two streams: each slot clears and blends its own frame."""
    import torch
    name, blend, k = "shift40", 4, 2
    t = make_rig(name)
    m = ox.Mapper(template(ox, t), t["sizes"], blend=blend, enable_gain=True)
    info = m.info()
    assert info["full_cover"] == 0 and info["remap_result_subtiles"] > 0
    m.set_frames_in_flight(k)
    cases = [oracle_case(name, blend, "smooth", seed=10 * f) for f in range(2 * k)]
    dev = [[_cuda(x) for x in c[0]] for c in cases]
    outs = [_out(t["W"], t["H"]) for _ in range(2 * k)]
    streams = [torch.cuda.Stream() for _ in range(k)]
    torch.cuda.synchronize()
    for f in range(2 * k):
        m.stitch(dev[f], outs[f], stream=streams[f % k])
    g_last = np.array(m.gains())
    torch.cuda.synchronize()
    for f in range(2 * k):
        assert np.array_equal(outs[f].cpu().numpy(), cases[f][2]), f
    np.testing.assert_array_equal(g_last, cases[-1][3])


# 8. texture-convention remap ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,blend", [("full", 8), ("shift7", 4)])
@gpu
def test_gpu_texture_remap_off_grid(ox, name, blend):
    _, _, _, want = stitch_case(ox, name, blend, "smooth", remap="texture")
    assert (want != oracle_case(name, blend, "smooth")[2]).any()  # a different sampling


# ---- constructor errors -----------------------------------------------------------------------------------
@gpu
def test_gpu_aligned_result_roi_leaving_the_frame_is_rejected(ox):
    """ROIs inside the frame whose aligned result ROI is not: x 10 .. 210 in a 210-wide frame aligns to
    8 .. 216 with 3 bands (blenders.cpp:727-729 would throw on the result's sub-rectangle)."""
    t = make_rig("full")
    rois = [(x + 10, y, w, h) for x, y, w, h in t["rois"]]
    arr, _ = aligned_rois(rois, 16)
    assert arr[0] + min(arr[2], 210) > 210
    mt = ox.MapperTemplate.from_arrays(210, 100, rois, t["maps1"], t["maps2"], t["masks"], t["seams"])
    with pytest.raises(ox.OctvrError) as e:
        ox.Mapper(mt, t["sizes"], blend=16)
    assert e.value.code == -1 and "aligned result ROI leaves the output frame" in str(e.value)
    ox.Mapper(mt, t["sizes"], blend=4)  # 1 band: 10 .. 210 stays
