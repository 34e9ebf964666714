"""Control-point sets that drive MapperTemplate::morph_controlpoints (template_morph.cpp:69-237) onto the
paths the mild sets of test_gpu_morph.py never reach — plain Python over camera_rigs.py and the oracle,
no GPU.  case(name) -> (rig, W, H, control_points); every point is legal (legal_points below), so the
oracle's return value is len(control_points).

  big_jitter     20 points per pair moved by up to 0.03 of the input image: destination triangles with
                 rounded corners off the ROI raster, folds, taps outside the ROI, partial mask values
  dense          40 points per pair, and points in the output's first column: more than 255 triangles
                 in a camera, source vertices left of the frame's clamp at 1e-3
  borders        points within 0.05 of each of the output's four borders: every frame clamp
  masked_points  points whose two output pixels are masked out in both cameras (exclude polygons drawn
                 round coordinates read from the same rig without masks): both distances 0, w0 = w1 = 1
  idle_camera    four cameras, points among the three fisheyes only: the fourth has no triangle
  duplicates     one camera-0 point used twice with different partners (Subdiv2D snaps it, the first
                 point's mid wins), and three points of the equirect camera on one output row bit for bit
  large_roi      1536 x 768: the equirect ROI has more pixels than the warp kernel's grid has lanes
  odd_size       500 x 250: odd ROI widths and origins

second(name): a second point set for morphing an already morphed template (legality depends on the ROIs
and camera models only, which a morph leaves alone)."""
import copy
import functools

import numpy as np

import camera_rigs as R
import oracle_py as O

F = np.float32
NAMES = ["big_jitter", "dense", "borders", "masked_points", "idle_camera", "duplicates", "large_roi", "odd_size"]
LANES = 256 * 16 * 256  # launch_morph_warp's largest grid: pixels of index >= LANES take a second iteration


@functools.lru_cache(maxsize=None)
def _luts_cached(rig_json, W, H):
    import json
    return O.lut_build(json.loads(rig_json), W, H, threads=8)


def luts_of(rig, W, H):
    """The oracle's pre-morph LUTs of a rig; shared, so callers must not write into them."""
    import json
    return _luts_cached(json.dumps(rig, sort_keys=True), W, H)


def translate(rig, cp):
    """_translate of both ends (template_morph.cpp:86-90) in float: (dst0, dst1), None where it throws."""
    n0, n1 = int(cp[0]), int(cp[1])
    d0 = O.project(rig["inputs"][n0], rig["output"], float(F(cp[2])), float(F(cp[3])))
    d1 = O.project(rig["inputs"][n1], rig["output"], float(F(cp[4])), float(F(cp[5])))
    if d0 is None or d1 is None:
        return None
    return (F(d0[0]), F(d0[1])), (F(d1[0]), F(d1[1]))


def local_pixels(rig, luts, W, H, cp):
    """(x0, y0, x1, y1): the ROI pixels whose distances weigh the point (:107-110, float truncated)."""
    (d0, d1) = translate(rig, cp)
    r0, r1 = luts[int(cp[0])][0], luts[int(cp[1])][0]
    return (int(d0[0] * F(W) - F(r0[0])), int(d0[1] * F(H) - F(r0[1])),
            int(d1[0] * F(W) - F(r1[0])), int(d1[1] * F(H) - F(r1[1])))


def is_legal(rig, luts, W, H, cp):
    """The point is kept and no assertion fires: n0 < n1 in range, both projections exist, are no NaN and lie in
    [0, 1)^2 (Subdiv2D's rectangle), their L1 distance in float is <= 0.1, both land inside their ROIs."""
    n0, n1 = int(cp[0]), int(cp[1])
    if not (0 <= n0 < n1 < len(rig["inputs"])):
        return False
    t = translate(rig, cp)
    if t is None:
        return False
    d0, d1 = t
    v = np.array([d0[0], d0[1], d1[0], d1[1]], F)
    if np.isnan(v).any() or (v < 0).any() or (v >= 1).any():
        return False
    if float(F(abs(d0[0] - d1[0])) + F(abs(d0[1] - d1[1]))) > 0.1:
        return False
    x0, y0, x1, y1 = local_pixels(rig, luts, W, H, cp)
    r0, r1 = luts[n0][0], luts[n1][0]
    return 0 <= x0 < r0[2] and 0 <= y0 < r0[3] and 0 <= x1 < r1[2] and 0 <= y1 < r1[3]


def legal_points(rig, luts, W, H, cps):
    return [cp for cp in cps if is_legal(rig, luts, W, H, cp)]


def _points(rig, W, H, **kw):
    luts = luts_of(rig, W, H)
    return legal_points(rig, luts, W, H, R.morph_points(luts, **kw))


def _big_jitter():
    rig = R.morph_rig(True)
    return rig, 512, 256, _points(rig, 512, 256, per_pair=20, seed=3, jitter=0.03)


def _dense():
    rig = R.morph_rig(True)
    cps = _points(rig, 512, 256, per_pair=40, seed=7, jitter=0.01)
    # column 0 projects to x < 1e-3, left of the frame's clamp
    cps += _points(rig, 512, 256, per_pair=2, seed=8, jitter=0.001, region=lambda X, Y: X == 0)
    return rig, 512, 256, cps


def _borders():
    """The fisheyes' ROIs end 18 rows short of the output's top and 24 short of its bottom, so only the
    equirect camera (3) has pixels within 0.05 of every border: each point pairs a fisheye pixel with the
    camera-3 pixel of the same column at most 0.1 nearer the border (left and right: the same pixel).  All
    of camera 3's vertices stay inside [1e-3, 1 - 1e-3], so its extremes are the clamps themselves."""
    rig = R.morph_rig(True)
    W, H = 512, 256
    luts = luts_of(rig, W, H)
    (_, _, w3, h3), e1, e2, _ = luts[3]
    assert (w3, h3) == (W, H)
    cps = []
    # (fisheye, its top-most or bottom-most claimed pixel, camera 3's row): rows 10, 11 are within 0.05 of
    # the top, rows 243, 244 of the bottom, each less than 0.1 of the height from the fisheye's pixel
    for k, top, Y3 in ((1, True, 10), (2, True, 11), (0, False, 244), (1, False, 243)):
        (kx, ky, kw, kh), k1, k2, km = luts[k]
        ys, xs = np.nonzero(km)
        j = int(np.argmin(ys) if top else np.argmax(ys))
        Xk, Yk = int(xs[j]), int(ys[j])
        assert abs(Yk + ky - Y3) < 0.095 * H
        cps.append([k, 3, float(k1[Yk, Xk]), float(k2[Yk, Xk]), float(e1[Y3, Xk + kx]), float(e2[Y3, Xk + kx])])
    inner = lambda X, Y: (Y > 0.3 * H) & (Y < 0.7 * H)
    for s, region in enumerate([lambda X, Y: (X >= 3) & (X < 0.04 * W) & inner(X, Y),
                                lambda X, Y: (X > 0.96 * W) & (X <= W - 5) & inner(X, Y)]):
        cps += R.morph_points(luts, per_pair=2, seed=20 + s, jitter=0.001, pairs=[(1, 3), (2, 3)], region=region)
    return rig, W, H, legal_points(rig, luts, W, H, cps)


MASK_HALF = 14  # half side of an exclude square, input pixels


def _masked_points():
    plain = R.morph_rig(False)
    W, H = 512, 256
    luts = luts_of(plain, W, H)
    inner = lambda X, Y: (Y > 0.3 * H) & (Y < 0.7 * H)
    hidden = R.morph_points(luts, per_pair=2, seed=31, jitter=0.002, region=inner)
    rig = copy.deepcopy(plain)
    for cam in rig["inputs"]:
        cam["options"]["exclude_masks"] = []
    for n0, n1, x0, y0, x1, y1 in hidden:
        for n, u, v in ((n0, x0, y0), (n1, x1, y1)):
            o = rig["inputs"][n]["options"]
            cx, cy = int(u * o["width"]), int(v * o["height"])
            sq = [cx - MASK_HALF, cy - MASK_HALF, cx + MASK_HALF, cy - MASK_HALF, cx + MASK_HALF, cy + MASK_HALF,
                  cx - MASK_HALF, cy + MASK_HALF]
            o["exclude_masks"].append({"type": "polygonal", "args": [float(c) + 0.25 for c in sq]})
    masked = luts_of(rig, W, H)
    assert [l[0] for l in masked] == [l[0] for l in luts], "the exclude squares must leave the ROIs alone"
    # the hidden points first, then ordinary ones of the masked rig so that its visible part moves too
    cps = legal_points(rig, masked, W, H, hidden) + legal_points(rig, masked, W, H,
                                                                  R.morph_points(masked, per_pair=4, seed=32))
    return rig, W, H, cps


def _idle_camera():
    rig = R.morph_rig(True)
    return rig, 512, 256, _points(rig, 512, 256, per_pair=6, seed=41, jitter=0.01, pairs=[(0, 1), (0, 2), (1, 2)])


def _snap_row(rig, cam, x1, y1, target):
    """A float y near y1 for which camera `cam`'s point (x1, y) projects to output row `target` bit for bit."""
    def row(y):
        return O.project(rig["inputs"][cam], rig["output"], float(F(x1)), float(y))[1]
    lo, hi = y1 - 0.02, y1 + 0.02
    up = row(hi) > row(lo)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if (row(mid) < float(target)) == up:
            lo = mid
        else:
            hi = mid
    y = F(lo)
    for cand in [y] + [np.nextafter(y, F(s * np.inf), dtype=F) for s in (-1, 1)]:
        if F(row(float(cand))) == target:
            return float(cand)
    return None


ROW = 120  # duplicates: the output row the three collinear points share


def _duplicates():
    rig = R.morph_rig(True)
    W, H = 512, 256
    luts = luts_of(rig, W, H)
    mid = lambda X, Y: (Y > 0.35 * H) & (Y < 0.65 * H)
    base = R.morph_points(luts, per_pair=3, seed=51, jitter=0.004, region=mid, pairs=[(0, 1), (0, 2), (1, 2)])
    # (0, 1) and (0, 3) points sharing camera 0's coordinates bit for bit, the partners' jitter differing
    a = next(cp for cp in base if cp[0] == 0 and cp[1] == 1)
    d0 = translate(rig, a)[0]
    X, Y = int(round(float(d0[0]) * W)) - luts[3][0][0], int(round(float(d0[1]) * H)) - luts[3][0][1]
    twin = [0, 3, a[2], a[3], float(luts[3][1][Y, X]) + 0.006, float(luts[3][2][Y, X]) - 0.005]
    cps = [a, twin] + [cp for cp in base if cp is not a]
    # (k, 3) points of output row ROW; the camera-3 ends of three of them moved onto one row bit for bit
    row3 = R.morph_points(luts, per_pair=4, seed=52, jitter=0.004, region=lambda X, Y: Y == ROW,
                          pairs=[(0, 3), (1, 3), (2, 3)])
    target = translate(rig, row3[0])[1][1]
    done = 1
    for cp in row3[1:]:
        y = _snap_row(rig, 3, cp[4], cp[5], target) if done < 3 else None
        if y is not None:
            cp[5] = y
            done += 1
    assert done == 3, "no three points on one row"
    return rig, W, H, legal_points(rig, luts, W, H, cps + row3)


def _large_roi():
    rig = R.morph_rig(True)
    W, H = 1536, 768
    cps = _points(rig, W, H, per_pair=6, seed=61, jitter=0.01)
    # pixel LANES of the equirect ROI lies in row 682, below every fisheye's mask: as in borders, each fisheye's
    # bottom-most claimed pixel is paired with the camera-3 pixel 0.06 of the height further down
    luts = luts_of(rig, W, H)
    for k in range(3):
        (kx, ky, kw, kh), k1, k2, km = luts[k]
        ys, xs = np.nonzero(km)
        j = int(np.argmax(ys))
        Xk, Yk = int(xs[j]), int(ys[j])
        Y3 = Yk + ky + int(0.06 * H)
        cps.append([k, 3, float(k1[Yk, Xk]), float(k2[Yk, Xk]), float(luts[3][1][Y3, Xk + kx]),
                    float(luts[3][2][Y3, Xk + kx])])
    return rig, W, H, legal_points(rig, luts, W, H, cps)


def _odd_size():
    rig = R.morph_rig(True)
    return rig, 500, 250, _points(rig, 500, 250, per_pair=8, seed=71, jitter=0.01)


_BUILD = {"big_jitter": _big_jitter, "dense": _dense, "borders": _borders, "masked_points": _masked_points,
          "idle_camera": _idle_camera, "duplicates": _duplicates, "large_roi": _large_roi, "odd_size": _odd_size}


@functools.lru_cache(maxsize=None)
def case(name):
    """(rig, W, H, control_points) of a family; cached, so callers must not modify it."""
    return _BUILD[name]()


@functools.lru_cache(maxsize=None)
def second(name):
    """Another legal point set for case(name)'s rig: the second morph of an already morphed template."""
    rig, W, H, _ = case(name)
    return _points(rig, W, H, per_pair=5, seed=97, jitter=0.01)


def illegal_points(name):
    """Points that make the call fail (a four-camera family): kind -> point.  outside_roi: camera 0's left-most
    claimed pixel, its coordinates moved 0.06 of the image width further left — the projection is a number
    inside [0, 1)^2 less than 0.1 from camera 3's, but left of camera 0's ROI."""
    rig, W, H, cps = case(name)
    luts = luts_of(rig, W, H)
    (x0, y0, _, _), a1, a2, am = luts[0]
    ys, xs = np.nonzero(am)
    j = int(np.argmin(xs))
    X, Y = int(xs[j]) + x0, int(ys[j]) + y0
    out = [0, 3, float(a1[ys[j], xs[j]]) - 0.06, float(a2[ys[j], xs[j]]), float(luts[3][1][Y, X]),
           float(luts[3][2][Y, X])]
    d0, d1 = translate(rig, out)
    v = np.array([d0[0], d0[1], d1[0], d1[1]], F)
    assert not np.isnan(v).any() and (v >= 0).all() and (v < 1).all()
    assert float(F(abs(d0[0] - d1[0])) + F(abs(d0[1] - d1[1]))) <= 0.1
    assert local_pixels(rig, luts, W, H, out)[0] < 0
    good = cps[0]
    return {"outside_roi": out, "order": [good[1], good[0]] + good[2:], "camera": [good[0], len(luts)] + good[2:]}


def fill_points(tri, roi, W, H):
    """A destination triangle's rounded ROI-local corners as fillPoly receives them (:208-214): T(x, y)
    in float, std::round (halves away from zero)."""
    q = []
    for c in range(3):
        for v in (F(tri[2 * c]) * F(W) - F(roi[0]), F(tri[2 * c + 1]) * F(H) - F(roi[1])):
            q.append(int(np.sign(v) * np.floor(abs(v) + F(0.5))))
    return q

