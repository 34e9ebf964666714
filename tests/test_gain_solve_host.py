"""The gain path's solver on the CPU (no GPU): lu_trace (tests/gain_systems.py, LUImpl in plain float64 with its
row swaps reported) against the oracle's orc_solve, which the 12 golden systems pin to the reference — bit for
bit on every matrix family the device test (tests/test_gpu_gain_extremes.py) sends through the device solver,
so that test may take the swaps a system needs from lu_trace.  And the oracle's gain system (orc_gain_system)
against the feed it was split from.
"""
import numpy as np
import pytest

import gain_systems as G
import oracle_py as O


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("n", range(4, 17))
def test_lu_trace_equals_oracle_bit_for_bit(n):
    fams = G.families(n)
    names = {f[0] for f in fams}
    assert {"diag_dominant", "dense", "anti_diagonal", "tie_pm_col0", "tie_pm_col1", "tie_diagonal", "zero_column",
            "identical_rows", "last_pivot_99eps", "last_pivot_100eps", "gain_shaped"} <= names
    assert ("golden" in names) == (n <= 12)
    for k, (name, A, b, expect) in enumerate(fams):
        x, swaps, ok = G.lu_trace(A, b)
        want = O.solve(A, b)
        assert ok == (want is not None), (name, n, k)
        if ok:
            assert np.array_equal(_bits(x), _bits(want)), (name, n, k, x, want)
        G.check_expect(name, n, swaps, ok, expect)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_closed_form_families_flags(n):
    """n <= 3 (cv::solve's closed forms): a determinant of exactly 0 fails, a tiny one solves."""
    fams = G.families(n)
    assert {"golden", "det_zero", "det_tiny", "dense"} <= {f[0] for f in fams}
    for name, A, b, expect in fams:
        assert (O.solve(A, b) is not None) == expect["ok"], (name, n)


def test_golden_systems_through_lu_trace():
    """The reference's own answers (solve_kat) for n >= 4, from lu_trace."""
    for n, (A, b, x) in G.golden_systems().items():
        if n >= 4:
            got, _, ok = G.lu_trace(A, b)
            assert ok and np.array_equal(_bits(got), _bits(x)), n


@pytest.mark.parametrize("n", [4, 8, 9, 16])
def test_gain_shaped_systems_swap_rows(n):
    """A dark camera beside a bright one: the off-diagonal term 2 alpha I(i,j) I(j,i) N exceeds the diagonal
    beta (N(i,i) + N) + 2 alpha I(i,j)^2 N, and LUImpl swaps rows (the feed's solvers' `k != i` branch)."""
    traces = [G.lu_trace(A, b)[1] for name, A, b, _ in G.families(n) if name == "gain_shaped"]
    assert traces and any(traces), traces


def test_gain_system_is_the_feeds_system():
    """orc_gain_system + orc_solve = orc_gain_feed (and the stitch's gains), on a golden rig; A and b follow
    from N and I by the feed's formula."""
    from octvr_amd import synthetic
    rig, z = O.load_rig("rigB")
    n = len(z["rois"])
    W, H = (int(v) for v in z["out_size"])
    sizes = [(rig["inputs"][i]["options"]["width"], rig["inputs"][i]["options"]["height"]) for i in range(n)]
    frames = [synthetic.smooth_yuv_frame(w, h, 70 + i) for i, (w, h) in enumerate(sizes)]
    rois = z["rois"].tolist()
    m1 = [z[f"map1_{i}"] for i in range(n)]
    m2 = [z[f"map2_{i}"] for i in range(n)]
    mk = [z[f"mask_{i}"] for i in range(n)]
    warped = O.warp_inputs(frames, sizes, m1, m2)
    N, I, A, b = O.gain_system(rois, warped, mk, W, H)
    g = O.gain_feed(rois, warped, mk, W, H)
    assert np.array_equal(_bits(O.solve(A, b)), _bits(g))
    _, g_stitch = O.stitch_frame(frames, sizes, rois, m1, m2, mk, W, H, enable_gain=True, gains=None)
    assert np.array_equal(_bits(g_stitch), _bits(g))
    assert (N == N.T).all() and (N >= 1).all() and (np.diag(I) == 0).all()
    for i in range(n):
        aii = bi = 0.0
        for j in range(n):
            bi += 100.0 * N[i, j]
            aii += 100.0 * N[i, j]
            if j != i:
                aii += 2 * 0.01 * I[i, j] * I[i, j] * N[i, j]
                assert A[i, j] == 0.0 - 2 * 0.01 * I[i, j] * I[j, i] * N[i, j]
        assert A[i, i] == aii and b[i] == bi
