"""Multi-band blends over seam masks that are not a 0 / 255 partition of the output.

Seam masks are caller data (octvr_rig_create_from_arrays takes them verbatim, .dat files carry them), any u8
value anywhere inside a camera's ROI, while multiband_create derives its whole plan from their values: the
kind of every 32 x 8 sub-tile, the 8 x 8 blocks of each Gaussian level that get computed at all, the remap's
G0 and result flags.  create_masks only ever gives seams of 0 and 255 that split the output, one compact blob
per camera; the families below leave that in every direction.  Each is derived from a rig's create_masks
partition P_i and LUT masks M_i, on the rigs of test_gpu_blend_geometry.py, and stitched against the oracle's
frame of the same arrays: bit-exact, Y and both chroma planes, and the gains.  Each case also asserts, from
Mapper.info() and from numpy restatements on the seams themselves, that it reaches what it is for.

The host half (no GPU) pins the oracle on these seams: a numpy float32 restatement of the one-band blend, and
two properties the reference alone must satisfy."""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O
import test_gpu_blend_geometry as G

gpu = pytest.mark.gpu
FAMILIES = ["soft", "overlap", "gap", "empty_cam", "islands", "checker8", "lowvals", "seam_outside_mask",
            "seam_outside_mask12"]
VARIANT_FAMILIES = ["soft", "overlap", "gap", "islands"]
GEOS = ["full", "shift40"]
EMPTY_CAM = 1
GAP = (70, 40, 60, 20)  # x, y, w, h from the ROI union's corner: x 70..129, y 40..59 on "full"
# islands put on purpose (from the ROI union's corner) on both sides of 8 x 8 block, 32 x 8 sub-tile and 128 x 8
# tile corners of the level-0 grid; the second line are the same corners where 5 bands move the grid's origin
# of "shift40" to (-8, -24) of the union's
ISLAND_CORNERS = [(127, 7), (128, 8), (31, 23), (32, 24), (95, 39), (96, 40), (63, 55), (64, 56),
                  (119, 15), (120, 16), (23, 47), (24, 48), (55, 63), (56, 64)]
INV255 = np.float32(1. / 255)
EPS = np.float32(1e-5)

_SEAMS, _WANT, _TEMPLATES, _PART_INFO = {}, {}, {}, {}


def union_origin(t):
    return min(r[0] for r in t["rois"]), min(r[1] for r in t["rois"])


def frame_coords(roi):
    """(X, Y) frame coordinates of every pixel of a ROI-sized array."""
    x, y, w, h = roi
    yy, xx = np.mgrid[0:h, 0:w]
    return xx + x, yy + y


def box_sum(a, r):
    """Sum over the (2r + 1)^2 window, zero outside the array."""
    h, w = a.shape
    p = np.zeros((h + 2 * r, w + 2 * r), np.int64)
    p[r:r + h, r:r + w] = a
    return sum(p[dy:dy + h, dx:dx + w] for dy in range(2 * r + 1) for dx in range(2 * r + 1))


def island_points(t, i):
    """[(x, y, value)] in ROI coordinates: 40 random ones (seeded per camera), then the listed corners."""
    x0, y0, w, h = t["rois"][i]
    ux, uy = union_origin(t)
    rng = np.random.default_rng(9100 + i)
    pts, taken = [], np.zeros((h, w), bool)
    while len(pts) < 40:
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        if taken[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3].any():
            continue  # isolated: nothing of this camera's islands within 2 px
        taken[y, x] = True
        pts.append((x, y, int(rng.integers(1, 256))))
    for k, (cx, cy) in enumerate(ISLAND_CORNERS):
        x, y = ux + cx - x0, uy + cy - y0
        if 0 <= x < w and 0 <= y < h:
            pts.append((x, y, 1 + (37 * k + 101 * i) % 255))
    return pts


def seams_of(name, family):
    """The family's seams for geometry `name`: u8 arrays of each camera's ROI size, read-only."""
    key = (name, family)
    if key in _SEAMS:
        return _SEAMS[key]
    t = G.make_rig(name)
    P, M, n = t["seams"], t["masks"], t["n"]
    ux, uy = union_origin(t)
    out = []
    for i in range(n):
        X, Y = frame_coords(t["rois"][i])
        p, m = P[i], M[i]
        if family == "partition":
            s = p.copy()
        elif family == "soft":  # 9 x 9 box blur, rounded half up
            s = ((2 * box_sum(p, 4) + 81) // 162).astype(np.uint8)
        elif family == "overlap":
            s = np.where(m != 0, 255, 0).astype(np.uint8)
        elif family == "gap":
            gx, gy, gw, gh = GAP
            s = p.copy()
            s[(X >= ux + gx) & (X < ux + gx + gw) & (Y >= uy + gy) & (Y < uy + gy + gh)] = 0
        elif family == "empty_cam":
            s = np.zeros_like(p) if i == EMPTY_CAM else p.copy()
        elif family == "islands":
            s = p.copy()
            for x, y, v in island_points(t, i):
                s[y, x] = v
        elif family == "checker8":
            s = np.where(((X // 8 + Y // 8) % n == i) & (m != 0), 255, 0).astype(np.uint8)
        elif family == "lowvals":
            s = np.where(p != 0, 1 + i, 0).astype(np.uint8)
        elif family in ("seam_outside_mask", "seam_outside_mask12"):
            # P dilated by 3 px (7 x 7 square) into the pixels the mask leaves out: a handful here, where the
            # partition keeps away from the masks' edges, so a second family takes 12 px
            s = p.copy()
            s[(box_sum(p != 0, 12 if family.endswith("12") else 3) > 0) & (m == 0)] = 255
        else:
            raise KeyError(family)
        s = np.ascontiguousarray(s, np.uint8)
        s.setflags(write=False)
        out.append(s)
    _SEAMS[key] = out
    return out


def seam_rig(name, family):
    t = G.make_rig(name)
    return dict(t, seams=seams_of(name, family), name="%s/%s" % (name, family))


def oracle_case(name, family, blend, kind, scale=None, tex=False, seed=0):
    """(frames, gains, the oracle's frame, its gains), computed once per case and never modified."""
    key = (name, family, blend, kind, scale, tex, seed)
    if key not in _WANT:
        t = seam_rig(name, family)
        frames, gains = G.frames_of(t, kind, seed)
        want, g = O.stitch_frame(frames, t["sizes"], t["rois"], t["maps1"], t["maps2"], t["masks"], t["W"], t["H"],
                                 enable_gain=True, gains=gains, blend=blend, seams=t["seams"], threads=4, scale=scale,
                                 remap_tex=tex)
        want.setflags(write=False)
        _WANT[key] = (frames, gains, want, np.array(g))
    return _WANT[key]


# ---- numpy restatements on the seams ----------------------------------------------------------------------
def weight_levels(t, blend):
    """(align_result_roi, per level a list per camera of (ox, oy, f32 weights over its align_roi >> level)):
    level 0 = seam / 255 (convertTo's alpha * v), the levels above by the reference's f32 pyrDown."""
    B = O.blend_bands(blend)
    arr, ar = G.aligned_rois(t["rois"], blend)
    lv = [[] for _ in range(B + 1)]
    for (x, y, w, h), (l, tp, cw, ch), s in zip(t["rois"], ar, t["seams"]):
        wt = np.zeros((ch, cw), np.float32)
        wt[y - tp:y - tp + h, x - l:x - l + w] = INV255 * s.astype(np.float32)
        for k in range(B + 1):
            lv[k].append(((l - arr[0]) >> k, (tp - arr[1]) >> k, wt))
            if k < B:
                wt = O.pyr_down_f32(wt)
    return arr, lv


def on_grid(arr, level, cams, dtype=np.float32):
    """Each camera's level array placed on the level grid (0 outside its align_roi): (n, H, W)."""
    W, H = arr[2] >> level, arr[3] >> level
    g = np.zeros((len(cams), H, W), dtype)
    for i, (ox, oy, a) in enumerate(cams):
        g[i, oy:oy + a.shape[0], ox:ox + a.shape[1]] = a
    return g


def weight_sums0(t, blend):
    """The level-0 f32 weight sums 1e-5f + w_0 + w_1 + ... in camera order, as the kernel and the reference."""
    arr, lv = weight_levels(t, blend)
    s = np.full((arr[3], arr[2]), EPS, np.float32)
    for g in on_grid(arr, 0, lv[0]):
        s = s + g
    return s


def subtile_view(a, th=8, tw=32):
    """(n, H, W) -> (n, ty, tx, th, tw), zero padded to whole sub-tiles, and the same of an 'inside' mask."""
    n, H, W = a.shape
    Hp, Wp = -(-H // th) * th, -(-W // tw) * tw
    p = np.zeros((n, Hp, Wp), a.dtype)
    p[:, :H, :W] = a
    ins = np.zeros((Hp, Wp), bool)
    ins[:H, :W] = True
    v = lambda q: q.reshape(q.shape[:-2] + (Hp // th, th, Wp // tw, tw)).swapaxes(-3, -2)
    return v(p), v(ins)


def weight_cam_tiles(t, blend):
    """Per level: sum over cameras of the 128 x 8 tiles that hold a non-zero weight of the camera."""
    arr, lv = weight_levels(t, blend)
    return [int((subtile_view(on_grid(arr, k, cams) != 0, 8, 128)[0].any(axis=(-2, -1))).sum())
            for k, cams in enumerate(lv)]


def subtiles0(t, blend):
    """Level 0, per 32 x 8 sub-tile: (cameras with a non-zero seam there, owned: one such camera, 255 on every
    pixel of the sub-tile inside the level)."""
    arr, lv = weight_levels(t, blend)
    s = np.rint(on_grid(arr, 0, lv[0]) * np.float32(255)).astype(np.uint8)  # the seams on the level-0 grid
    v, ins = subtile_view(s)
    ncam = (v != 0).any(axis=(-2, -1)).sum(axis=0)
    full = ((v == 255) | ~ins).all(axis=(-2, -1)).any(axis=0)
    return ncam, (ncam == 1) & full


def reach(bands):
    """How far (level-0 pixels, Chebyshev) a seam or image pixel can lie from a result pixel it influences.
    Level-l positions within rho_l of p >> l matter: rho_0 = 0, and a pyrUp output x reads sources
    x / 2 - 1 .. x / 2 + 2 (the + 2: the 8-row block quirk), so rho_(l+1) = ceil(rho_l / 2) + 2.  A level-l
    position x is built by l pyrDowns (taps 2x - 2 .. 2x + 2) from level-0 pixels within 2 (2^l - 1) of
    x 2^l, and p lies less than 2^l from (p >> l) 2^l."""
    rho, r = 0, 0
    for l in range(1, bands + 1):
        rho = -(-rho // 2) + 2
        r = max(r, (rho + 1) * (1 << l) + 2 * ((1 << l) - 1))
    return r


def multiband_rgb(t, warped, bands, threads=4):
    """orc_multiband_blend's RGB result (H, W, 3) for ROI-sized u8x4 images."""
    n = t["n"]
    warped = [np.ascontiguousarray(a, np.uint8) for a in warped]
    seams = [np.ascontiguousarray(a, np.uint8) for a in t["seams"]]
    r = np.ascontiguousarray(np.asarray(t["rois"], np.int32).reshape(-1))
    res = np.zeros((t["H"], t["W"], 3), np.uint8)
    rc = O.lib().orc_multiband_blend(n, O._p(r), (C.c_void_p * n)(*[a.ctypes.data for a in seams]),
                                     (C.c_void_p * n)(*[a.ctypes.data for a in warped]), bands, O._p(res), t["W"],
                                     t["H"], C.c_size_t(t["W"] * 3), threads)
    assert rc == 0
    return res


def warped_of(t, frames):
    return [O.remap_u8(O.yuv420_to_rgba(f, w, h), m1, m2, float(w), float(h))
            for f, (w, h), m1, m2 in zip(frames, t["sizes"], t["maps1"], t["maps2"])]


def clamp_counts(want, t, blend):
    """Luma samples at 0 and at 255 inside align_result_roi (outside it, the frame is black anyway)."""
    y = want[:t["H"]][~G.outside_masks(t, blend)[0]]
    return int((y == 0).sum()), int((y == 255).sum())


# ---- the host half: runs without a GPU --------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", GEOS)
def test_seam_families_are_what_they_claim(name, family):
    """The seams themselves, in numpy: each family leaves the 0 / 255 partition in the way it is meant to."""
    t, part = seam_rig(name, family), G.make_rig(name)
    S, P, M = t["seams"], part["seams"], part["masks"]
    assert all(s.shape == p.shape and s.dtype == np.uint8 for s, p in zip(S, P))
    assert any((s != p).any() for s, p in zip(S, P))
    for blend in (4, 16, 40):
        arr, lv = weight_levels(t, blend)
        g0 = on_grid(arr, 0, lv[0])
        ws = weight_sums0(t, blend)
        other = (ws != EPS) & (ws != EPS + np.float32(1))
        ncam, owned = subtiles0(t, blend)
        _, owned_p = subtiles0(part, blend)
        if family in ("soft", "lowvals"):
            assert other.sum() > 500, (family, int(other.sum()))  # 1.0f / wsum at level 0
        if family == "soft":
            assert len(np.unique(np.concatenate([s.ravel() for s in S]))) == 82  # every rint(255 k / 81), k = 0..81
        if family == "overlap":
            two = (g0 == 1).sum(axis=0)
            assert (two == 2).any() and two.max() == t["n"], int(two.max())  # sum w = 2 and 3
            assert owned.sum() < owned_p.sum()
        if family == "gap":
            assert (ncam == 0).sum() >= 2 and ((ncam == 0) & (subtiles0(part, blend)[0] > 0)).sum() >= 2
        if family == "empty_cam":
            assert not S[EMPTY_CAM].any() and all(w.max() == 0 for k in range(len(lv)) for w in [lv[k][EMPTY_CAM][2]])
        if family == "checker8":
            assert owned.sum() < owned_p.sum() // 4
        if family == "lowvals":
            assert max(int(s.max()) for s in S) == t["n"] and ws.max() < 0.05
        if family == "islands":
            isl = np.zeros(g0.shape[1:], bool)
            for i in range(t["n"]):
                x0, y0 = t["rois"][i][:2]
                for x, y, _ in island_points(t, i):
                    isl[y + y0 - arr[1], x + x0 - arr[0]] = True
            yy, xx = np.nonzero(isl)
            edge = lambda v, m: (v % m == 0) | (v % m == m - 1)
            for what, mx in (("block", 8), ("sub-tile", 32), ("tile", 128)):
                hit = edge(xx, mx) & edge(yy, 8)
                assert (hit & (xx % mx == 0)).any() and (hit & (xx % mx == mx - 1)).any(), (what, blend)
    if family.startswith("seam_outside_mask"):
        k = sum(int(((s != 0) & (m == 0)).sum()) for s, m in zip(S, M))
        assert k > (400 if family.endswith("12") else 0), k
    if family == "islands":
        for i in range(t["n"]):  # other cameras' territory included
            assert sum(1 for x, y, _ in island_points(t, i) if P[i][y, x] == 0) >= 5


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", GEOS)
def test_contrast_frames_reach_the_clamp_in_the_oracle(name, family):
    """The 0 / 255 checkerboards put the oracle's luma into the level-0 clamp at both ends (lowvals: weights of
    k / 255 leave no 255), which the noise frames do not."""
    t = G.make_rig(name)
    for blend in (4, 16):
        lo, hi = clamp_counts(oracle_case(name, family, blend, "contrast")[2], t, blend)
        assert lo >= 64 and (hi >= 64 or family == "lowvals"), (name, family, blend, lo, hi)


@pytest.mark.parametrize("family", ["soft", "overlap"])
def test_one_band_blend_restated_in_float32(family):
    """blenders.cpp:686-735 at one band on the 'full' rig, from the oracle's exported pyramid steps and numpy
    float32: D = sum trunc(g_n w_n) in camera order, L = clamp(rint(D (1 / (1e-5 + sum w)))), then the collapse.
    Bit-equal to orc_multiband_blend's RGB result."""
    t = seam_rig("full", family)
    frames, _ = G.frames_of(t, "contrast")
    warped = warped_of(t, frames)
    blend, B = 4, 1
    assert O.blend_bands(blend) == B
    arr, ar = G.aligned_rois(t["rois"], blend)
    _, lv = weight_levels(t, blend)
    D = [np.zeros((arr[3] >> k, arr[2] >> k, 3), np.float32) for k in (0, 1)]
    wsum = [np.full((arr[3] >> k, arr[2] >> k), EPS, np.float32) for k in (0, 1)]
    for i, ((x, y, w, h), (l, tp, cw, ch)) in enumerate(zip(t["rois"], ar)):
        g0 = np.zeros((ch, cw, 4), np.uint8)
        g0[y - tp:y - tp + h, x - l:x - l + w] = warped[i]
        g1 = O.fast_pyr_down_u8x4(g0)
        lap = [g0.astype(np.int32) - O.pyr_up_u8x4(g1).astype(np.int32), g1.astype(np.int32)]
        for k in (0, 1):
            ox, oy, wt = lv[k][i]
            hh, ww = wt.shape
            D[k][oy:oy + hh, ox:ox + ww] += np.trunc(lap[k][:, :, :3].astype(np.float32) * wt[:, :, None])
            wsum[k][oy:oy + hh, ox:ox + ww] += wt
    assert all(np.abs(d).max() < 32768 for d in D)  # the reference's short sum does not wrap
    L = [np.clip(np.rint(D[k] * (np.float32(1) / wsum[k])[:, :, None]), -32768, 32767).astype(np.int16) for k in (0, 1)]
    R0 = np.clip(O.pyr_up_s16x3(L[1]).astype(np.int32) + L[0], -32768, 32767)
    mine = np.zeros((t["H"], t["W"], 3), np.uint8)
    hh, ww = min(arr[3], t["H"] - arr[1]), min(arr[2], t["W"] - arr[0])
    mine[arr[1]:arr[1] + hh, arr[0]:arr[0] + ww] = np.clip(R0[:hh, :ww], 0, 255)
    ws0 = wsum[0]
    assert ((ws0 != EPS) & (ws0 != EPS + np.float32(1))).any()  # the restated division is not the constant one
    want = multiband_rgb(t, warped, B)
    assert np.array_equal(mine, want), int((mine != want).sum())
    assert (want == 0).sum() > 64 and (want == 255).sum() > 64


def test_overlap_of_equal_content_reproduces_it():
    """'overlap' seams (weights 0 and 1) over cameras that all show one constant colour c.  (Constant, because
    pyrUp's 8-row block pattern follows each camera's own align_roi: equal images do not give equal Laplacians.)
    At a pixel p whose reach() square lies inside the mask of one camera and, for every other camera, wholly
    inside or wholly outside its ROI, every Gaussian value that matters is c (a clamped border tap moves towards
    p) and the weight sum is >= 1 at every level.  Level 0: the weights are 0 or 1, the products exact, and
    rint(k d / (k + 1e-5)) = d.  Levels >= 1: each of the n truncations loses less than 1 and the weight sum is
    >= 1, so |L - (G - up)| <= n; a pyrUp of values within e of another's lies within e + 1 of its pyrUp.  So
    |result - c| <= bands (n + 1)."""
    t = seam_rig("full", "overlap")
    n, blend = t["n"], 4
    B = O.blend_bands(blend)
    r = reach(B)
    assert (B, r) == (1, 8)
    c = np.array([201, 77, 30, 0], np.uint8)
    warped = [np.broadcast_to(c, (h, w, 4)).copy() for _, _, w, h in t["rois"]]
    got = multiband_rgb(t, warped, B).astype(np.int32)
    W, H = t["W"], t["H"]
    inside = np.zeros((n, H, W), bool)   # the square around p lies in the camera's mask
    in_roi = np.zeros((n, H, W), bool)   # ... in its ROI
    off_roi = np.ones((n, H, W), bool)   # ... outside its ROI
    k = (2 * r + 1) ** 2
    for i, (x, y, w, h) in enumerate(t["rois"]):
        m = np.zeros((H, W), bool)
        m[y:y + h, x:x + w] = t["masks"][i] != 0
        roi = np.zeros((H, W), bool)
        roi[y:y + h, x:x + w] = True
        # (the frame is the align_result_roi here: squares leaving it count what lies inside, as clamped taps do)
        cnt = box_sum(np.ones((H, W), np.int64), r)
        inside[i], in_roi[i], off_roi[i] = box_sum(m, r) == cnt, box_sum(roi, r) == cnt, box_sum(roi, r) == 0
    assert k >= cnt.max()
    ok = inside.any(axis=0) & (in_roi | off_roi).all(axis=0)
    assert ok.sum() > 1000 and (ok & (inside.sum(axis=0) >= 2)).sum() > 100  # with two cameras of weight 1
    bound = B * (n + 1)
    err = np.abs(got - c[:3].astype(np.int32))[ok]
    assert err.max() <= bound, (int(err.max()), bound)


def test_gap_is_black_beyond_the_pyramids_reach():
    """'gap' seams: a result pixel farther than reach(bands) from every non-zero seam pixel sees weight 0 on
    every camera at every position that matters: D = 0 and L = 0 at every level, so the collapse gives 0."""
    t = seam_rig("full", "gap")
    frames, _ = G.frames_of(t, "noise")
    warped = warped_of(t, frames)
    for blend, some in ((4, True), (16, False)):
        B = O.blend_bands(blend)
        r = reach(B)
        nz = np.zeros((t["H"], t["W"]), bool)
        for (x, y, w, h), s in zip(t["rois"], t["seams"]):
            nz[y:y + h, x:x + w] |= s != 0
        far = box_sum(nz, r) == 0
        assert far.any() == some, (blend, r)  # (3 bands reach across the whole gap: nothing to check)
        res = multiband_rgb(t, warped, B)
        assert (res[far] == 0).all()
        if some:
            gx, gy, gw, gh = GAP
            assert far[gy + r:gy + gh - r, gx + r:gx + gw - r].all() and gh > 2 * r
            assert (res[box_sum(nz, 1) == 0] != 0).any()  # the gap's rim is not black: the collapse fills it


def test_seams_survive_the_dat_round_trip(product_lib, tmp_path):
    """MapperTemplate.dump / load carry arbitrary u8 seams byte for byte."""
    t = seam_rig("full", "soft")
    mt = product_lib.MapperTemplate.from_arrays(t["W"], t["H"], t["rois"], t["maps1"], t["maps2"], t["masks"], t["seams"])
    p = tmp_path / "soft.dat"
    mt.dump(str(p))
    mt2 = product_lib.MapperTemplate.load(str(p))
    for i in range(t["n"]):
        assert mt2.input(i)[0] == tuple(t["rois"][i])
        assert np.array_equal(mt2.input(i)[4], t["seams"][i]) and np.array_equal(mt.input(i)[4], t["seams"][i])


# ---- the GPU half -----------------------------------------------------------------------------------------
ox = G.ox


def template(ox, t):
    """from_arrays with the seams; read back, they are the bytes given."""
    if t["name"] not in _TEMPLATES:
        mt = ox.MapperTemplate.from_arrays(t["W"], t["H"], t["rois"], t["maps1"], t["maps2"], t["masks"], t["seams"])
        for i in range(t["n"]):
            assert np.array_equal(mt.input(i)[4], t["seams"][i]), (t["name"], i)
        _TEMPLATES[t["name"]] = mt
    return _TEMPLATES[t["name"]]


def stitch_case(ox, name, family, blend, kind, scale=None, out_fmt="yuv420p", remap="remap"):
    t = seam_rig(name, family)
    case = oracle_case(name, family, blend, kind, scale, remap == "texture")
    info, arr, got, want = G.stitch_case(ox, name, blend, kind, scale, out_fmt, remap, rig=t, case=case,
                                         mt=template(ox, t))
    return t, info, arr, got, want


def partition_info(ox, name, blend):
    """Mapper.info() of the create_masks partition on the same rig and blend (no knobs set)."""
    if (name, blend) not in _PART_INFO:
        t = G.make_rig(name)
        _PART_INFO[(name, blend)] = ox.Mapper(G.template(ox, t), t["sizes"], blend=blend, enable_gain=True).info()
    return _PART_INFO[(name, blend)]


def check_plan(t, info, blend):
    """info() against the numpy restatements: the level's camera tile sets, the owned level-0 sub-tiles, and
    that every level-0 sub-tile is either blended or written by the remap."""
    lt = info["level_tiles"]
    assert [l["weight_cam_tiles"] for l in lt] == weight_cam_tiles(t, blend)
    ncam, owned = subtiles0(t, blend)
    assert lt[0]["owned_subtiles"] == int(owned.sum())
    assert lt[0]["unread_subtiles"] == 0 and info["remap_result_subtiles"] <= lt[0]["deep_subtiles"] <= int(owned.sum())
    todo = lt[0]["tiles"] * 4 - info["remap_result_subtiles"]
    assert lt[0]["blend_subtiles"] == -(-todo // 4) * 4, (lt[0], info["remap_result_subtiles"])
    return ncam, owned


def check_family(ox, name, family, blend, t, info, arr, got, want):
    """The path assertions of one family, against the partition's plan on the same rig."""
    part = partition_info(ox, name, blend)
    lt, lp = info["level_tiles"], part["level_tiles"]
    ncam, owned = check_plan(t, info, blend)
    if family == "overlap":
        assert lt[0]["owned_subtiles"] < lp[0]["owned_subtiles"]
        d, dp = lt[0]["deep_subtiles"], lp[0]["deep_subtiles"]  # (5 bands leave the partition none on these frames)
        assert d < dp or d == dp == 0, (d, dp)
    if family == "gap":  # sub-tiles without a camera are blended (the collapse alone): written, and the oracle's
        H, hit = t["H"], 0
        for ty, tx in np.argwhere(ncam == 0):
            x0, y0 = arr[0] + 32 * tx, arr[1] + 8 * ty
            if x0 + 32 > min(arr[0] + arr[2], t["W"]) or y0 + 8 > min(arr[1] + arr[3], H):
                continue
            ys, xs = slice(y0, y0 + 8), slice(x0, x0 + 32)
            cy, cx = slice(H + y0 // 2, H + y0 // 2 + 4), slice(x0 // 2, x0 // 2 + 16)
            assert np.array_equal(got[ys, xs], want[ys, xs]) and np.array_equal(got[cy, cx], want[cy, cx])
            hit += bool((want[ys, xs] != 0x5A).all())  # written: no byte there is the output's fill value
        assert hit >= 2
    if family == "empty_cam":
        assert all(a["weight_cam_tiles"] < b["weight_cam_tiles"] for a, b in zip(lt, lp))
        two = dict(t, seams=[s for i, s in enumerate(t["seams"]) if i != EMPTY_CAM],
                   rois=[r for i, r in enumerate(t["rois"]) if i != EMPTY_CAM])
        arr2, lv2 = weight_levels(two, blend)
        if tuple(arr2) == tuple(arr):  # the other cameras alone account for every tile set
            assert [l["weight_cam_tiles"] for l in lt] == weight_cam_tiles(two, blend)
    if family == "islands":
        # more required tiles than the partition's, level 0 and the levels above -- unless the partition already
        # requires every 128 x 8 tile of every camera there, which these small frames' upper levels come to
        for lo, hi in ((0, 1), (1, len(lt))):
            req, req_p = (sum(l["required"] for l in x[lo:hi]) for x in (lt, lp))
            every = t["n"] * sum(l["tiles"] for l in lt[lo:hi])
            assert req > req_p or req == req_p == every, (lo, req, req_p, every)
        assert lt[0]["owned_subtiles"] < lp[0]["owned_subtiles"]
    if family == "checker8":
        assert lt[0]["owned_subtiles"] < lp[0]["owned_subtiles"]
    if family in ("soft", "lowvals"):  # level-0 weight sums that are neither constant: 1.0f / wsum
        ws = weight_sums0(t, blend)
        assert ((ws != EPS) & (ws != EPS + np.float32(1))).any()
    if family == "lowvals":
        assert all(l["owned_subtiles"] == 0 and l["deep_subtiles"] == 0 for l in lt) and info["remap_result_subtiles"] == 0


BLENDS = [(f, b) for f in FAMILIES for b in (4, 16, 40)]


@pytest.mark.parametrize("kind", ["noise", "smooth", "contrast"])
@pytest.mark.parametrize("family,blend", BLENDS)
@pytest.mark.parametrize("name", GEOS)
@gpu
def test_gpu_seam_families(ox, name, family, blend, kind):
    """Every family on both geometries at 1, 3 and 5 bands: fixed gains over noise, estimated gains over smooth
    frames, and the 0 / 255 checkerboards that reach the level-0 clamp."""
    assert O.blend_bands(blend) == {4: 1, 16: 3, 40: 5}[blend]
    if kind == "contrast" and blend != 40:
        lo, hi = clamp_counts(oracle_case(name, family, blend, kind)[2], G.make_rig(name), blend)
        assert lo >= 64 and (hi >= 64 or family == "lowvals"), (lo, hi)
    t, info, arr, got, want = stitch_case(ox, name, family, blend, kind)
    assert info["bands"] == O.blend_bands(blend)
    check_family(ox, name, family, blend, t, info, arr, got, want)
    if name == "shift40":
        G.assert_black_outside(got, t, blend, (name, family, blend, "gpu"))


# ---- variants, on a reduced set ---------------------------------------------------------------------------
@pytest.mark.parametrize("family", VARIANT_FAMILIES)
@gpu
def test_gpu_seams_nv12_output(ox, family):
    _, info, _, _, _ = stitch_case(ox, "shift40", family, 16, "smooth", out_fmt="nv12")
    assert info["full_cover"] == 0


@pytest.mark.parametrize("family", VARIANT_FAMILIES)
@gpu
def test_gpu_seams_scaled_output(ox, family):
    """The RGBA result path: the blend's and the remap's result stores go to the result image."""
    t = G.make_rig("shift40")
    scale = (t["W"] // 2 & ~1, t["H"] // 2 & ~1)
    _, info, _, _, _ = stitch_case(ox, "shift40", family, 4, "contrast", scale=scale)
    assert info["scaled_out"] == list(scale)


@pytest.mark.parametrize("family", VARIANT_FAMILIES)
@gpu
def test_gpu_seams_texture_remap(ox, family):
    _, _, _, _, want = stitch_case(ox, "full", family, 16, "smooth", remap="texture")
    assert (want != oracle_case("full", family, 16, "smooth")[2]).any()  # a different sampling


@pytest.mark.parametrize("family", VARIANT_FAMILIES)
@gpu
def test_gpu_seams_without_remap_result(ox, family, monkeypatch):
    """With and without the remap's result stores (OCTVR_MB_NO_REMAP_RESULT) the oracle's bytes come out."""
    _, info, _, got, _ = stitch_case(ox, "shift40", family, 4, "contrast")
    monkeypatch.setenv("OCTVR_MB_NO_REMAP_RESULT", "1")
    t, info2, _, got2, _ = stitch_case(ox, "shift40", family, 4, "contrast")
    assert info2["remap_result_subtiles"] == 0
    assert info2["level_tiles"][0]["deep_subtiles"] == info["level_tiles"][0]["deep_subtiles"]
    check_plan(t, info2, 4)
    assert np.array_equal(got, got2)


@pytest.mark.parametrize("family", VARIANT_FAMILIES)
@gpu
def test_gpu_seams_two_frames_in_flight(ox, family):
    """Two slots, two different frames on two streams: each slot clears and blends its own frame ('gap' leaves
    sub-tiles that no camera writes)."""
    import torch
    name, blend = "shift40", 16
    t = seam_rig(name, family)
    m = ox.Mapper(template(ox, t), t["sizes"], blend=blend, enable_gain=True)
    m.set_frames_in_flight(2)
    cases = [oracle_case(name, family, blend, kind) for kind in ("contrast", "noise")]
    dev = [[G._cuda(x) for x in c[0]] for c in cases]
    outs = [G._out(t["W"], t["H"]) for _ in cases]
    streams = [torch.cuda.Stream() for _ in cases]
    torch.cuda.synchronize()
    for f, c in enumerate(cases):
        m.stitch(dev[f], outs[f], gains=c[1], stream=streams[f])
    torch.cuda.synchronize()
    for f, c in enumerate(cases):
        got = outs[f].cpu().numpy()
        d = got != c[2]
        assert not d.any(), (f, int(d.sum()), np.argwhere(d)[:6].tolist())


@pytest.mark.parametrize("family", FAMILIES)
@gpu
def test_gpu_seams_second_frame_on_the_same_mapper(ox, family):
    """Frame 2 on the mapper that stitched frame 1: a pyramid block that is read but not written would still
    hold frame 1's bytes.  Frame 1 is the checkerboards, frame 2 noise, then the checkerboards again."""
    import torch
    name, blend = "full", 16
    t = seam_rig(name, family)
    m = ox.Mapper(template(ox, t), t["sizes"], blend=blend, enable_gain=True)
    for kind in ("contrast", "noise", "contrast"):
        frames, gains, want, g_orc = oracle_case(name, family, blend, kind)
        out = G._out(t["W"], t["H"])
        m.stitch([G._cuda(f) for f in frames], out, gains=gains)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        d = got != want
        assert not d.any(), (kind, int(d.sum()), np.argwhere(d)[:6].tolist())
        np.testing.assert_array_equal(np.array(m.gains()), g_orc)


@gpu
def test_gpu_seams_from_a_dat_file(ox, tmp_path):
    """A rig carrying the 'soft' seams through dump / load stitches to the bytes of the one from the arrays."""
    import torch
    name, blend = "shift40", 16
    t = seam_rig(name, "soft")
    p = tmp_path / "soft.dat"
    template(ox, t).dump(str(p))
    mt2 = ox.MapperTemplate.load(str(p))
    for i in range(t["n"]):
        assert np.array_equal(mt2.input(i)[4], t["seams"][i])
    frames, gains, want, _ = oracle_case(name, "soft", blend, "noise")
    outs = []
    for mt in (template(ox, t), mt2):
        m = ox.Mapper(mt, t["sizes"], blend=blend, enable_gain=True)
        out = G._out(t["W"], t["H"])
        m.stitch([G._cuda(f) for f in frames], out, gains=gains)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], want)
