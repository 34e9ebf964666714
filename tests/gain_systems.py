"""Linear systems for the gain path's solver tests (tests/test_gain_solve_host.py on the CPU,
tests/test_gpu_gain_extremes.py on the device), and lu_trace: LUImpl (core/src/matrix_decomp.cpp:50-110, as
oracle/octvr_oracle.c orc_solve restates it) in plain float64 that also reports its row swaps.  lu_trace is
trusted only because test_gain_solve_host.py pins its x to O.solve bit for bit on every system built here.
"""
import os

import numpy as np

import oracle_py as O

EPS = float(np.finfo(np.float64).eps)  # DBL_EPSILON
LU_EPS = EPS * 100                     # LUImpl's singularity threshold: fails where |pivot| < LU_EPS


def lu_trace(A, b):
    """(x, swaps, ok): cv::solve's LU for n >= 4 in float64, every operation rounded as written (no FMA);
    swaps = [(column, pivot_row)] for every column whose pivot is not its diagonal.  x is None where ok is
    False."""
    A = np.array(A, np.float64)
    b = np.array(b, np.float64)
    n = len(b)
    assert A.shape == (n, n) and n >= 4
    swaps = []
    for i in range(n):
        k = i
        for j in range(i + 1, n):
            if abs(A[j, i]) > abs(A[k, i]):
                k = j
        if abs(A[k, i]) < LU_EPS:
            return None, swaps, False
        if k != i:
            swaps.append((i, k))
            A[[i, k], i:] = A[[k, i], i:]
            b[[i, k]] = b[[k, i]]
        d = -1 / A[i, i]
        for j in range(i + 1, n):
            alpha = A[j, i] * d
            A[j, i + 1:] += alpha * A[i, i + 1:]  # two rounded operations per element
            b[j] += alpha * b[i]
        A[i, i] = -d
    for i in range(n - 1, -1, -1):
        s = b[i]
        for k in range(i + 1, n):
            s -= A[i, k] * b[k]
        b[i] = s * A[i, i]
    return b, swaps, True


def golden_systems():
    """{n: (A, b, x)}: the 12 reference-pinned systems of tests/golden/kats.npz (solve_kat)."""
    s = np.load(os.path.join(O.ROOT, "tests", "golden", "kats.npz"))["solve_kat"]
    out, i = {}, 0
    while i < len(s):
        n = int(s[i]); i += 1
        A = s[i:i + n * n].reshape(n, n).copy(); i += n * n
        b = s[i:i + n].copy(); i += n
        x = s[i:i + n].copy(); i += n
        out[n] = (A, b, x)
    assert len(out) == 12
    return out


def gain_shaped(n, seed, paired=True):
    """A, b of GainCompensatorGPU::feed's system (exposure_compensate.cpp:279-296, alpha = 0.01, beta = 100) from
    a random symmetric N with N(i,j) <= min(N(i,i), N(j,j)) and I(i,j) = camera i's level (dark 20..100 or
    bright 350..441, alternating) with a little per-pair variation.  paired: cameras 2k and 2k+1 overlap
    almost completely and the other pairs hardly (one dominant partner, the case that swaps rows)."""
    rng = np.random.default_rng(seed)
    diag = rng.integers(20000, 60000, n)
    N = np.zeros((n, n), np.int64)
    for i in range(n):
        N[i, i] = diag[i]
        for j in range(i + 1, n):
            cap = min(diag[i], diag[j])
            if paired:
                frac = rng.uniform(0.85, 1.0) if (j == i + 1 and i % 2 == 0) else rng.uniform(0.0, 0.03)
            else:
                frac = rng.uniform(0.0, 1.0)
            N[i, j] = N[j, i] = max(1, int(frac * cap))
    dark_first = bool(seed & 1)
    level = np.array([rng.uniform(20, 100) if (i % 2 == 0) == dark_first else rng.uniform(350, 441) for i in range(n)])
    I = level[:, None] * (1 + rng.uniform(-0.03, 0.03, (n, n)))
    np.fill_diagonal(I, 0.0)
    alpha, beta = 0.01, 100.0
    A = np.zeros((n, n))
    b = np.zeros(n)
    for i in range(n):
        bi = aii = 0.0
        for j in range(n):
            bi += beta * N[i, j]
            aii += beta * N[i, j]
            if j == i:
                continue
            aii += 2 * alpha * I[i, j] * I[i, j] * N[i, j]
            A[i, j] = 0.0 - 2 * alpha * I[i, j] * I[j, i] * N[i, j]
        A[i, i] = aii
        b[i] = bi
    return A, b


def _upper(n, rng, last):
    """Unit-diagonal upper-triangular matrix with a dense upper part and last pivot `last`: LUImpl's
    multipliers are all 0, so the last pivot it tests is exactly `last`."""
    A = np.triu(rng.normal(size=(n, n)), 1) + np.eye(n)
    A[n - 1, n - 1] = last
    return A


def families(n):
    """[(family, A, b, expect)] for n x n: expect = None, or a dict of what the family is built to show
    ("ok": the success flag; "no_swaps": True; "swaps_at": {column: pivot_row}; "min_swaps": count)."""
    rng = np.random.default_rng(9000 + n)
    out = []

    def add(name, A, b=None, **expect):
        A = np.ascontiguousarray(A, np.float64)
        b = rng.normal(size=n) * 10 if b is None else np.ascontiguousarray(b, np.float64)
        out.append((name, A, b, expect or None))

    gold = golden_systems()
    if n in gold:
        add("golden", gold[n][0], gold[n][1], ok=True)
    if n <= 3:
        # closed forms: a determinant of exactly 0 fails, a tiny one solves
        zero = {1: [[0.0]], 2: [[2.0, 4.0], [1.0, 2.0]], 3: [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]]}[n]
        add("det_zero", zero, ok=False)
        add("det_zero_b", np.array(zero) * 3.0, ok=False)
        tiny = {1: [[1e-300]], 2: [[1.0, 1.0], [1.0, 1.0 + EPS]],
                3: [[1.0, 1.0, 0.0], [1.0, 1.0 + EPS, 0.0], [0.0, 0.0, 1.0]]}[n]
        add("det_tiny", tiny, ok=True)
        add("det_tiny_diag", np.eye(n) * 1e-100, ok=True)
        for _ in range(6):
            add("dense", rng.normal(size=(n, n)), ok=True)
        if n >= 2:
            for s in range(4):
                add("gain_shaped", *gain_shaped(n, 100 * n + s), ok=True)
        return out
    for _ in range(3):
        add("diag_dominant", rng.normal(size=(n, n)) + np.eye(n) * (4.0 * n), ok=True, no_swaps=True)
    for _ in range(4):
        while True:  # dense Gaussian: drawn again until at least half the columns swap (most draws do)
            A, b = rng.normal(size=(n, n)), rng.normal(size=n) * 10
            if len(lu_trace(A, b)[1]) >= (n + 1) // 2:
                break
        add("dense", A, b, ok=True, min_swaps=(n + 1) // 2)
    for _ in range(2):
        # the first pivot is the LAST row; columns 0 .. n/2 - 1 each swap with their mirror row
        add("anti_diagonal", rng.normal(size=(n, n)) + np.fliplr(np.eye(n)) * (4.0 * n), ok=True,
            swaps_at={c: n - 1 - c for c in range(n // 2)})
    # ties: the scan keeps the FIRST of equal magnitudes (strict >)
    for r1, r2 in ((1, 2), (2, n - 1)):
        A = rng.normal(size=(n, n))
        A[r1, 0], A[r2, 0] = 7.5, -7.5  # above every |normal| drawn here
        add("tie_pm_col0", A, ok=True, swaps_at={0: r1})
    for r1, r2 in ((2, 3), (2, n - 1)):
        A = rng.normal(size=(n, n))
        A[0, 0], A[1:, 0] = 1.0, 0.0    # column 0 eliminates nothing: column 1 is scanned as written
        A[r1, 1], A[r2, 1] = -7.5, 7.5
        add("tie_pm_col1", A, ok=True, swaps_at={1: r1})
    for sign in (1.0, -1.0):
        A = rng.normal(size=(n, n))
        A[0, 0], A[n - 2, 0] = 7.5, sign * 7.5  # a candidate equal to the diagonal in magnitude: no swap
        add("tie_diagonal", A, ok=True, swaps_at={0: None})
    # failure and near-failure
    for c in (0, n // 2, n - 1):
        A = rng.normal(size=(n, n))
        A[:, c] = 0.0
        add("zero_column", A, ok=False)
    A = rng.integers(-5, 6, (n, n)).astype(np.float64)
    A[0, 0] = 8.0  # the largest of column 0, a power of two: row 1's multiplier is exactly -1
    A[1] = A[0]
    add("identical_rows", A, ok=False)
    for rev in (False, True):
        U = _upper(n, rng, 99 * EPS)
        add("last_pivot_99eps", U[::-1] if rev else U, ok=False)
        U = _upper(n, rng, 100 * EPS)
        add("last_pivot_100eps", U[::-1] if rev else U, ok=True)
    for s in range(4):
        add("gain_shaped", *gain_shaped(n, 100 * n + s), ok=True)
    for s in range(2):
        add("gain_shaped_dense", *gain_shaped(n, 100 * n + 50 + s, paired=False), ok=True)
    return out


def check_expect(name, n, swaps, ok, expect):
    """Assert what a family was built to show, from lu_trace's swaps and flag."""
    if not expect:
        return
    assert ok == expect["ok"], (name, n, ok)
    if expect.get("no_swaps"):
        assert swaps == [], (name, n, swaps)
    if "min_swaps" in expect:
        assert len(swaps) >= expect["min_swaps"], (name, n, swaps)
    got = dict(swaps)
    for c, r in expect.get("swaps_at", {}).items():
        assert got.get(c) == r, (name, n, c, r, swaps)
