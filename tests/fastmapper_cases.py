"""The FastMapper configurations of tests/test_gpu_fastmapper_layouts.py (kernels against the oracle) and
tests/test_fastmapper_layouts_host.py (the host index audit and the oracle-side conditions of the same
configurations): templates made of arrays (maps, masks, input sizes), not of library-made rigs.  Every builder
is cached and its arrays are read-only, so the tests of both files share one copy and one oracle result."""
import collections
import functools

import numpy as np

import oracle_py as O

Case = collections.namedtuple("Case", "key W H sizes m1 m2 mk")

IN_PADS = (0, 1, 2, 3, 8, 64)           # input pitch = w + pad
TINY_SHAPES = ((2, 2), (6, 4), (100, 50), (258, 2), (254, 6))
MANY_N = (7, 9, 16, 17, 32)
WRAP_N = (12, 32)
INTERIOR_KINDS = ("A", "B", "C", "D")


def _frozen(arrays):
    out = []
    for a in arrays:
        a = np.ascontiguousarray(a)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def _case(key, W, H, sizes, m1, m2, mk):
    return Case(key, W, H, tuple(sizes), _frozen(m1), _frozen(m2), _frozen(mk))


def template(ox, c):
    return ox.MapperTemplate.from_arrays(c.W, c.H, [[0, 0, c.W, c.H]] * len(c.sizes), list(c.m1), list(c.m2), list(c.mk))


def _rand_maps(rng, n, W, H, lo=0.0, hi=1.0):
    m1 = [rng.uniform(lo, hi, (H, W)).astype(np.float32) for _ in range(n)]
    m2 = [rng.uniform(lo, hi, (H, W)).astype(np.float32) for _ in range(n)]
    return m1, m2


def _full(n, W, H):
    return [np.full((H, W), 255, np.uint8) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def layouts():
    """The edge-tap maps of test_gpu_fastmapper_edge_taps (taps at -1, 0, w - 1, w and beyond on both planes; the
    42 x 39 byte frame ends mid-dword), full masks."""
    W, H, sizes = 96, 48, [(40, 24), (42, 26)]
    m1, m2 = _rand_maps(np.random.default_rng(7), 2, W, H, -0.06, 1.06)
    return _case("layouts", W, H, sizes, m1, m2, _full(2, W, H))


# the one-camera source of each tiny shape: 2 x 2 (chroma 1 x 1, needs a pitch of 4), 4 x 2 (chroma 2 x 1), 18 x 10
_TINY_ONE = {(2, 2): (2, 2), (6, 4): (4, 2), (100, 50): (18, 10), (258, 2): (4, 2), (254, 6): (2, 2)}
_TINY_THREE = ((4, 2), (2, 2), (18, 10))


@functools.lru_cache(maxsize=None)
def tiny(W, H, ncam):
    """Outputs below one run and with ragged last runs: 100 x 50 = 19 x 256 + 136 luma pixels, 50 x 25 = 4 x 256 +
    226 chroma pixels in rows of 50 (a run spans more than five rows); 258 x 2: the first run ends two pixels
    into row 1.  Random maps in [0, 1], full masks."""
    sizes = [_TINY_ONE[(W, H)]] if ncam == 1 else list(_TINY_THREE)
    m1, m2 = _rand_maps(np.random.default_rng(1000 * W + 10 * H + ncam), ncam, W, H)
    return _case("tiny%dx%dn%d" % (W, H, ncam), W, H, sizes, m1, m2, _full(ncam, W, H))


def tiny_pads(c):
    """An input pitch pad per camera that keeps every frame at 8 bytes or more (a 2 x 2 source: pitch 4)."""
    return [2 if s == (2, 2) else 0 for s in c.sizes]


@functools.lru_cache(maxsize=None)
def uncovered(all_zero):
    """Masks that leave whole 256-pixel runs without a camera (all_zero: every run of both planes, so neither
    plane has a block): the layouts maps; camera 0 covers rows 24.., camera 1 the right half of rows 30..."""
    c = layouts()
    mk = [np.zeros((c.H, c.W), np.uint8) for _ in c.sizes]
    if not all_zero:
        mk[0][24:, :] = 255
        mk[1][30:, c.W // 2:] = 255
    return _case("uncovered%d" % all_zero, c.W, c.H, c.sizes, c.m1, c.m2, mk)


def _cycle_sizes(n):
    return [((16, 8), (18, 10), (64, 32))[i % 3] for i in range(n)]


def _one_zero_masks(rng, n, W, H):
    mk = _full(n, W, H)
    for m in mk:
        m[int(rng.integers(H)), int(rng.integers(W))] = 0
    return mk


@functools.lru_cache(maxsize=None)
def many(n):
    """n cameras (camera bits up to 31, up to eight groups of four) on a 100 x 50 output: random maps, every mask
    full except one zero pixel, so every camera has weight in every run."""
    W, H = 100, 50
    rng = np.random.default_rng(4100 + n)
    m1, m2 = _rand_maps(rng, n, W, H)
    return _case("many%d" % n, W, H, _cycle_sizes(n), m1, m2, _one_zero_masks(rng, n, W, H))


WRAP_SEED = 5200


@functools.lru_cache(maxsize=None)
def wrap(n):
    """The accumulator wrap: constant maps 0.5 and (wrap_frames) all-255 frames, so every camera adds 255 * its u8
    weight; where the rounded weights of the n cameras sum to 258 or more the u16 sum passes 65535 and the pixel
    wraps to 1..4 instead of 255."""
    W, H = 100, 50
    rng = np.random.default_rng(WRAP_SEED + n)
    m1 = [np.full((H, W), 0.5, np.float32) for _ in range(n)]
    m2 = [np.full((H, W), 0.5, np.float32) for _ in range(n)]
    return _case("wrap%d" % n, W, H, _cycle_sizes(n), m1, m2, _one_zero_masks(rng, n, W, H))


def _interior_maps(kind):
    """One 64 x 32 source on a 64 x 8 output (two luma runs of four rows).  Maps (k + 0.25) / 64 and (k + 0.25) / 32
    are exact in f32 and give tap k with fraction 8 / 32.  Run 0: x taps 0..62, y taps 26..29, i.e. its largest
    tap is (w - 2, h - 3), the last interior one (A); one pixel moved to x tap w - 1 (B), to y tap h - 2 (C), to
    x tap -1 (D).  Run 1 always reaches y tap 31 (an edge block)."""
    W, H = 64, 8
    tx = np.tile(np.minimum(np.arange(W), 62), (H, 1)).astype(np.float64)
    ty = np.tile(np.array([26, 27, 28, 29, 28, 29, 30, 31], np.float64)[:, None], (1, W))
    if kind == "B":
        tx[1, 5] = 63
    elif kind == "C":
        ty[2, 7] = 30
    elif kind == "D":
        tx[0, 9] = -1
    else:
        assert kind == "A"
    return ((tx + 0.25) / 64).astype(np.float32), ((ty + 0.25) / 32).astype(np.float32)


@functools.lru_cache(maxsize=None)
def interior(kind):
    m1, m2 = _interior_maps(kind)
    return _case("interior" + kind, 64, 8, [(64, 32)], [m1], [m2], _full(1, 64, 8))


@functools.lru_cache(maxsize=None)
def interior_group():
    """Five cameras, every mask full: run 0's first group of four holds interior blocks (cameras 0, 2, 3) and an
    edge block (camera 1, case B), so the whole group takes the general path; camera 4 (interior) is alone in the
    second group, which takes the interior path in run 0 and the general one in run 1."""
    kinds = "ABAAA"
    maps = [_interior_maps(k) for k in kinds]
    return _case("interior_group", 64, 8, [(64, 32)] * 5, [m[0] for m in maps], [m[1] for m in maps], _full(5, 64, 8))


def expected_interior_blocks(c):
    """Per plane ("y", "uv") the number of (run, camera) blocks whose taps all lie at 0 <= x <= pw - 2,
    0 <= y <= ph - 3 of the camera's plane, from the maps alone (convertMaps' scalar rule, the f32 area halving
    of the chroma maps); every mask of `c` is full, so every entry of a block is in use."""
    out = {}
    for plane in ("y", "uv"):
        count = 0
        for (w, h), m1, m2 in zip(c.sizes, c.m1, c.m2):
            if plane == "uv":
                assert (c.W // 2) % 4 == 0  # every column in the vector grouping ((a + b) + (c + d)) * 0.25
                half = lambda m: ((m[0::2, 0::2] + m[0::2, 1::2]) + (m[1::2, 0::2] + m[1::2, 1::2])) * np.float32(0.25)
                m1, m2, w, h = half(m1), half(m2), w // 2, h // 2
            sx = np.rint((m1 * np.float32(w)) * np.float32(32)).astype(np.int64) >> 5
            sy = np.rint((m2 * np.float32(h)) * np.float32(32)).astype(np.int64) >> 5
            ok = ((sx >= 0) & (sx <= w - 2) & (sy >= 0) & (sy <= h - 3)).ravel()
            count += sum(bool(ok[k:k + 256].all()) for k in range(0, ok.size, 256))
        out[plane] = count
    return out


@functools.lru_cache(maxsize=None)
def nonfinite():
    """1 % of the map values (all under a non-zero weight: full masks) overwritten with NaN, +-inf, +-1e9 and the
    values whose taps are 32767 and -32768: convertMaps saturates them to INT_MIN or +-32768, a block then spans
    2048 source pixels or more and the plane keeps the 8-byte entries."""
    W, H, sizes = 96, 48, [(40, 24), (42, 26)]
    rng = np.random.default_rng(77)
    m1, m2 = _rand_maps(rng, 2, W, H)
    for (w, h), a, b in zip(sizes, m1, m2):
        for m, s in ((a, w), (b, h)):
            bad = [np.nan, np.inf, -np.inf, 1e9, -1e9, 32767.25 / s, -32767.75 / s]
            at = rng.choice(W * H, W * H // 100, replace=False)
            m.ravel()[at] = np.resize(np.array(bad, np.float32), at.size)
    return _case("nonfinite", W, H, sizes, m1, m2, _full(2, W, H))


def rand_frames(c, seed):
    return [O.rand_img(w, h * 3 // 2, 1, seed + i) for i, (w, h) in enumerate(c.sizes)]


def white_frames(c):
    return [np.full((h * 3 // 2, w), 255, np.uint8) for (w, h) in c.sizes]


_WANT = {}


def want(c, seed):
    """The oracle's stitch of rand_frames(c, seed), or of white_frames(c) for seed None: (frames, output), computed
    once per (case, seed) and read-only.  The oracle gets contiguous frames whatever layout the kernels are given."""
    k = (c.key, seed)
    if k not in _WANT:
        frames = white_frames(c) if seed is None else rand_frames(c, seed)
        out = O.fastmapper_nv12(frames, c.sizes, c.m1, c.m2, c.mk, c.W, c.H)
        out.setflags(write=False)
        _WANT[k] = (_frozen(frames), out)
    return _WANT[k]


def wrapped_counts(c, out):
    """(luma pixels, chroma bytes) of value <= 4 in the oracle's stitch of white frames: pixels whose u16 sum wrapped."""
    return int((out[:c.H] <= 4).sum()), int((out[c.H:] <= 4).sum())
