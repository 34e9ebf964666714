"""The morph case families (tests/morph_cases.py) reach the paths they are named for — proven from the CPU oracle
(oracle/octvr_oracle_morph.c) alone, so a family cannot silently miss its path.  No GPU."""
import functools

import numpy as np
import pytest

import morph_cases as MC
import oracle_py as O

F = np.float32


@functools.lru_cache(maxsize=None)
def morphed(name):
    """(rc, luts before, luts after, triangles) of the oracle on a family; shared, read-only."""
    rig, W, H, cps = MC.case(name)
    luts = MC.luts_of(rig, W, H)
    rc, new, tris = O.morph_controlpoints(rig, luts, W, H, cps)
    return rc, luts, new, tris


def _corners(tris):
    return np.asarray(tris, F).reshape(-1, 2)


@pytest.mark.parametrize("name", MC.NAMES)
def test_every_point_is_kept(name):
    rig, W, H, cps = MC.case(name)
    rc = morphed(name)[0]
    assert rc == len(cps) > 0
    assert all(MC.is_legal(rig, MC.luts_of(rig, W, H), W, H, cp) for cp in cps)
    rc2, _, _ = O.morph_controlpoints(rig, morphed(name)[2], W, H, MC.second(name))
    assert rc2 == len(MC.second(name)) > 0


@pytest.mark.parametrize("kind", ["outside_roi", "order", "camera"])
def test_illegal_points_fail_the_call(kind):
    rig, W, H, cps = MC.case("odd_size")
    bad = MC.illegal_points("odd_size")[kind]
    assert not MC.is_legal(rig, MC.luts_of(rig, W, H), W, H, bad)
    rc, new, _ = O.morph_controlpoints(rig, MC.luts_of(rig, W, H), W, H, cps + [bad])
    assert rc == -1  # CV_Assert


def _off_raster(name):
    """Per camera: destination triangles with a rounded corner outside [0, rw) x [0, rh)."""
    _, W, H, _ = MC.case(name)
    _, luts, _, tris = morphed(name)
    out = []
    for (roi, _, _, _), (_, dt) in zip(luts, tris):
        k = 0
        for t in dt:
            q = MC.fill_points(t, roi, W, H)
            k += any(not (0 <= q[2 * c] < roi[2] and 0 <= q[2 * c + 1] < roi[3]) for c in range(3))
        out.append(k)
    return out


def _partial_mask(name):
    return [int(((l[3] > 0) & (l[3] < 255)).sum()) for l in morphed(name)[2]]


def _folded_pixels(name):
    """Per camera: pixels inside the fillPoly of two destination triangles that have no corner in common (so no
    edge either) — where the order of the reference's copyTo's decides the result."""
    _, W, H, _ = MC.case(name)
    _, luts, _, tris = morphed(name)
    out = []
    for (roi, _, _, _), (_, dt) in zip(luts, tris):
        pix, owner, corners = [], [], []
        for k, t in enumerate(dt):
            q = MC.fill_points(t, roi, W, H)
            corners.append({(q[0], q[1]), (q[2], q[3]), (q[4], q[5])})
            cover = np.zeros((roi[3], roi[2]), np.uint8)
            O.fill_poly(cover, q, 1)
            idx = np.flatnonzero(cover)
            pix.append(idx)
            owner.append(np.full(len(idx), k))
        if not pix:
            out.append(0)
            continue
        pix, owner = np.concatenate(pix), np.concatenate(owner)
        order = np.argsort(pix, kind="stable")
        pix, owner = pix[order], owner[order]
        start = np.flatnonzero(np.r_[True, pix[1:] != pix[:-1], True])
        folded = 0
        for a, b in zip(start[:-1], start[1:]):
            ks = owner[a:b]
            folded += any(not (corners[ks[i]] & corners[ks[j]]) for i in range(len(ks)) for j in range(i + 1, len(ks)))
        out.append(folded)
    return out


def test_big_jitter_leaves_the_raster_and_grades_the_mask():
    off, part = _off_raster("big_jitter"), _partial_mask("big_jitter")
    print("big_jitter: off-raster triangles per camera", off, "partial-mask pixels per camera", part)
    assert max(off) > 0, off
    assert max(part) > 0, part


def test_overwrite_order_matters():
    folded = _folded_pixels("big_jitter")
    print("big_jitter: folded pixels per camera", folded)
    assert max(folded) > 0, "folded pixels per camera: %s" % folded


def test_dense_has_many_triangles_and_a_vertex_beyond_the_clamp():
    tris = morphed("dense")[3]
    nts = [len(st) for st, _ in tris]
    print("dense: triangles per camera", nts)
    assert max(nts) > 255, nts
    # the frame is clamped to [1e-3, 1 - 1e-3], so a source vertex beyond either value lies outside it
    assert any(len(st) and ((_corners(st) < F(1e-3)).any() or (_corners(st) > F(1 - 1e-3)).any()) for st, _ in tris)


def test_borders_reach_all_four_clamps():
    ok = []
    for st, _ in morphed("borders")[3]:
        c = _corners(st)
        ok.append(len(c) > 0 and c[:, 0].min() == F(1e-3) and c[:, 1].min() == F(1e-3) and
                  c[:, 0].max() == F(1 - 1e-3) and c[:, 1].max() == F(1 - 1e-3))
    assert any(ok), ok


def test_masked_points_have_no_distance():
    rig, W, H, cps = MC.case("masked_points")
    luts = morphed("masked_points")[1]
    hidden = 0
    for cp in cps:
        x0, y0, x1, y1 = MC.local_pixels(rig, luts, W, H, cp)
        both = luts[cp[0]][3][y0, x0] == 0 and luts[cp[1]][3][y1, x1] == 0
        either = luts[cp[0]][3][y0, x0] == 0 or luts[cp[1]][3][y1, x1] == 0
        assert both == either, cp  # the ordinary points are visible to both cameras
        hidden += both
    assert hidden >= 3, hidden  # every pair of the three fisheyes has two; the filter may drop some
    # the mid of such a point is the plain mean: a vertex of n0's destination triangles
    for cp in cps[:hidden]:
        d0, d1 = MC.translate(rig, cp)
        mid = ((d0[0] * F(1) + d1[0] * F(1)) / F(2), (d0[1] * F(1) + d1[1] * F(1)) / F(2))
        assert (_corners(morphed("masked_points")[3][cp[0]][1]) == np.array(mid, F)).all(1).any(), cp


def test_idle_camera_keeps_its_lut():
    _, luts, new, tris = morphed("idle_camera")
    assert len(luts) == 4
    for k in (1, 2, 3):
        assert np.array_equal(luts[3][k].view(np.uint8), new[3][k].view(np.uint8))
    assert len(tris[3][0]) == 0 and len(tris[3][1]) == 0
    assert all(len(tris[i][0]) > 0 for i in range(3))


def test_duplicates_snap_and_first_mid_wins():
    rig, W, H, cps = MC.case("duplicates")
    a, twin = cps[0], cps[1]
    assert a[0] == twin[0] == 0 and a[1] != twin[1] and a[2:4] == twin[2:4]
    st, dt = morphed("duplicates")[3][0]
    d0 = np.array(MC.translate(rig, a)[0], F)
    sc, dc = _corners(st), _corners(dt)
    hit = (sc == d0).all(1)
    assert hit.any()
    # one vertex: every triangle corner at that position moves to one destination, the first point's mid — a
    # vertex of camera a[1]'s destination triangles, not of camera twin[1]'s
    dests = {tuple(v) for v in dc[hit]}
    assert len(dests) == 1
    mid = np.array(dests.pop(), F)
    assert (_corners(morphed("duplicates")[3][a[1]][1]) == mid).all(1).any()
    assert not (_corners(morphed("duplicates")[3][twin[1]][1]) == mid).all(1).any()
    # three control vertices of camera 3 on one row bit for bit, all of them triangle corners
    ends = [MC.translate(rig, cp)[1] for cp in cps if cp[1] == 3]
    rows = [float(y) for _, y in ends]
    row = max(rows, key=rows.count)
    assert rows.count(row) >= 3, sorted(rows)
    s3 = _corners(morphed("duplicates")[3][3][0])
    assert all((s3 == np.array(e, F)).all(1).any() for e in ends if float(e[1]) == row)


def test_large_roi_changes_past_the_grid():
    _, luts, new, _ = morphed("large_roi")
    big = [i for i, l in enumerate(luts) if l[0][2] * l[0][3] > MC.LANES]
    assert big
    tail = sum(int(((new[i][1] != luts[i][1]) | (new[i][2] != luts[i][2])).reshape(-1)[MC.LANES:].sum()) for i in big)
    print("large_roi: changed map values of index >= %d: %d" % (MC.LANES, tail))
    assert tail > 0


def test_odd_size_is_odd():
    rois = [l[0] for l in morphed("odd_size")[1]]
    assert any(r[2] % 2 for r in rois) and any(r[0] % 2 and r[1] % 2 for r in rois), rois
    assert all(r[2] % 64 for r in rois), rois
