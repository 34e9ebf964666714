"""Case builders of tests/test_tile_limits_host.py (the tiler's statistics, no GPU) and tests/test_gpu_tile_limits.py
(the composite against the oracle): affine maps on a 256 x 64 output (eight items of 128 x 16 pixels) whose items
reach what the fisheye rigs of the other tests never do: more than kGroupFirst = 4 staging chunks (the
overflow table grp1), slots that start among the overflow chunks (stage_slot's search), black groups past the
image's edge inside them, boxes 256 pixels wide, LDS up to kTileLdsBytes, and the 4 -> 5 camera step between staged
and gathered ("wide") tiles.

A camera is (sx, sy, x0, y0, swap): output pixel (x, y) reads source (x0 + x sx, y0 + y sy), or with swap
(x0 + y sx, y0 + x sy) (u from y: tall boxes), divided by the input size and rounded to f32.  Camera c of n owns the
column blocks (x % 128) // ceil(128 / n) == c of every 128-pixel tile, so every item holds every camera.  All ROIs
are the whole frame.  Every builder is cached and its arrays are read-only; the oracle's results are computed once
per (case, arguments) and shared by the tests."""
import collections
import functools
import hashlib

import numpy as np

import oracle_py as O

Cam = collections.namedtuple("Cam", "sx sy x0 y0 swap")
Case = collections.namedtuple("Case", "key W H sizes rois m1 m2 mk cams")

W, H = 256, 64
TILE_W = 128
K_GROUP_FIRST = 4                 # kernels.hpp kGroupFirst
K_TILE_LDS_BYTES = 16 * 1024 - 176  # kernels.hpp kTileLdsBytes


def _frozen(arrays):
    out = []
    for a in arrays:
        a = np.ascontiguousarray(a)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def affine_maps(out_w, out_h, size, cam):
    """(map1, map2) of one camera: f32(source coordinate / input size)."""
    x = np.arange(out_w, dtype=np.float64)[None, :].repeat(out_h, 0)
    y = np.arange(out_h, dtype=np.float64)[:, None].repeat(out_w, 1)
    a, b = (y, x) if cam.swap else (x, y)
    u, v = cam.x0 + a * cam.sx, cam.y0 + b * cam.sy
    return (u / size[0]).astype(np.float32), (v / size[1]).astype(np.float32)


def block_masks(out_w, out_h, n):
    """Camera c's mask: 255 on its column block of every 128-pixel tile (blocks of ceil(128 / n) columns)."""
    owner = (np.arange(out_w) % TILE_W) // -(-TILE_W // n)
    return [np.where(owner == c, 255, 0).astype(np.uint8)[None, :].repeat(out_h, 0) for c in range(n)]


def affine_rig(key, out_w, out_h, sizes, cams, masks):
    """The from_arrays arguments of an affine rig: Case(key, W, H, sizes, rois, m1, m2, mk, cams)."""
    assert len(sizes) == len(cams) == len(masks)
    maps = [affine_maps(out_w, out_h, s, c) for s, c in zip(sizes, cams)]
    return Case(key, out_w, out_h, tuple(sizes), tuple([0, 0, out_w, out_h] for _ in sizes),
                _frozen(m[0] for m in maps), _frozen(m[1] for m in maps), _frozen(masks), tuple(cams))


def _ring(key, n, s, size=(512, 160), swap=False, sx=None, sy=None):
    """n cameras of scale s (or sx, sy), camera c at x0 = 1.25 + 2 c, y0 = 0.5 + c."""
    cams = [Cam(s if sx is None else sx, s if sy is None else sy, 1.25 + 2 * c, 0.5 + c, swap) for c in range(n)]
    return affine_rig(key, W, H, [size] * n, cams, block_masks(W, H, n))


# (cameras, scale): the plain rings
_RINGS = {"one_cam_13": (1, 1.3), "cams2_10": (2, 1.0), "cams3_10": (3, 1.0), "cams4_10": (4, 1.0),
          "cams2_115": (2, 1.15), "cams3_115": (3, 1.15), "cams4_115": (4, 1.15), "cams5": (5, 1.0)}
_TALL = {"tall2_10": (2, 1.0), "tall4_10": (4, 1.0), "tall2_115": (2, 1.15)}

# wide_box: sx such that camera 0's last tap of a tile is column 255 of its box (1.25 + 127 sx + 1 in [255, 256));
# wide_box_over: one more source column, a box of 264
WIDE_BOX_SX, WIDE_BOX_OVER_SX = 1.995, 2.0

STATIC_NAMES = tuple(_RINGS) + tuple(_TALL) + ("edge", "edge2", "mixed", "wide_box", "wide_box_over")
LDS_NAMES = ("lds_edge", "lds_over")
ALL_NAMES = STATIC_NAMES + LDS_NAMES


@functools.lru_cache(maxsize=None)
def static_case(name):
    if name in _RINGS:
        n, s = _RINGS[name]
        return _ring(name, n, s)
    if name in _TALL:  # axes swapped: boxes ~20 wide and up to 128 s + 4 tall
        n, s = _TALL[name]
        return _ring(name, n, s, size=(160, 512), swap=True)
    if name == "edge":
        # u reaches 1.25 + 255 * 1.3 = 332.75 > 320 and v 0.5 + 63 * 1.2 = 76.1 > 64: output columns from 246 and
        # rows from 53 have every tap outside the image
        return _ring(name, 1, None, size=(320, 64), sx=1.3, sy=1.2)
    if name == "edge2":
        # two cameras past the right and bottom edge, for the blends too (a single input disables the blend, as in
        # the reference); 320 x 56 inputs at sy = 1.0 (v reaches 64.5), so that two slots of 18 rows fit the LDS
        return _ring(name, 2, None, size=(320, 56), sx=1.3, sy=1.0)
    if name == "cams2_115_full":
        # cams2_115 with full masks, for the blends: no entry carries "no gain", so the remap LUT holds 24-bit entries;
        # create_masks gives camera 0 every pixel (seams all 255 and all 0): every level-0 sub-tile is deep, the remap
        # writes the result itself and no level has blend work
        c = static_case("cams2_115")
        return c._replace(key=name, mk=_frozen(np.full((H, W), 255, np.uint8) for _ in c.sizes))
    if name == "mixed":
        # camera 0 (s = 0.9: 15 groups x at most 17 rows, 4 chunks) owns the left tile column, camera 1 (s = 1.3) the right
        cams = [Cam(0.9, 0.9, 1.25, 0.5, False), Cam(1.3, 1.3, 1.25, 0.5, False)]
        left = np.zeros((H, W), np.uint8)
        left[:, :TILE_W] = 255
        return affine_rig(name, W, H, [(512, 160)] * 2, cams, [left, 255 - left])
    if name in ("wide_box", "wide_box_over"):
        sx = WIDE_BOX_SX if name == "wide_box" else WIDE_BOX_OVER_SX
        return _ring(name, 1, None, size=(528, 64), sx=sx, sy=0.5)
    raise KeyError(name)


LDS_SY = 1.3  # the vertical scale of lds_edge / lds_over: boxes of 22 or 24 rows


def one_cam(key, s):
    """One camera of horizontal scale s and vertical scale LDS_SY."""
    return _ring(key, 1, None, sx=s, sy=LDS_SY)


_OVERLAPPED = {}


def overlapped(c):
    """The case with camera i's mask widened to every pixel a camera >= i owns.  The copy chain takes the last camera
    whose mask is set, so every pixel keeps its camera and the tiled LUT is the same; but the masks now overlap, and
    the estimated gains (all 1 for a partition: no camera pair shares a pixel) depend on the frames."""
    if c.key not in _OVERLAPPED:
        mk = [np.maximum.reduce([np.asarray(m) for m in c.mk[i:]]) for i in range(len(c.mk))]
        _OVERLAPPED[c.key] = c._replace(key=c.key + "+overlap", mk=_frozen(mk))
    return _OVERLAPPED[c.key]


def template(ox, c, seams=None):
    return ox.MapperTemplate.from_arrays(c.W, c.H, [list(r) for r in c.rois], list(c.m1), list(c.m2), list(c.mk), seams)


_SEAMS = {}


def seams(c):
    """The oracle's create_masks seams of the case's masks, once per case."""
    if c.key not in _SEAMS:
        _SEAMS[c.key] = _frozen(O.create_masks([list(r) for r in c.rois], list(c.mk), c.W))
    return _SEAMS[c.key]


_INFO = {}


def lut_info(ox, c, remap="remap"):
    """octvr_debug_tiled_lut_info of the case's blend = 0 LUT (host only), once per (case, remap)."""
    k = (c.key, remap)
    if k not in _INFO:
        _INFO[k] = ox.debug_tiled_lut_info(template(ox, c), list(c.sizes), remap=remap)
    return _INFO[k]


_LDS = {}


def lds_pair(ox):
    """(lds_edge, lds_over): one camera of horizontal scale s, searched downward from 1.45 in steps of 1/64 for the
    largest s at which every item is staged; lds_over is the step above it (some item gathered).  The vertical scale
    stays at LDS_SY: a step of s then moves a box's width by at most one 8-pixel group (768 bytes of a 24-row box),
    while a common scale would move widths and heights together, in steps of more than 1 KiB."""
    if not _LDS:
        info = lambda s: ox.debug_tiled_lut_info(template(ox, one_cam("probe", s)), [(512, 160)])
        hi, step = 1.45, 1.0 / 64
        assert info(hi)["wide_tiles"] > 0
        lo = hi - step
        while info(lo)["wide_tiles"] > 0:
            hi, lo = lo, lo - step
            assert lo > 1.0
        _LDS["lds_edge"], _LDS["lds_over"] = one_cam("lds_edge", lo), one_cam("lds_over", hi)
        _LDS["s"] = (lo, hi)
    return _LDS["lds_edge"], _LDS["lds_over"]


def case(ox, name):
    if name in LDS_NAMES:
        return lds_pair(ox)[LDS_NAMES.index(name)]
    return static_case(name)


@functools.lru_cache(maxsize=None)
def noise_frames(sizes, seed):
    """Random-byte YUV420P frames: every staged group has its own content."""
    fr = tuple(O.rand_img(w, h * 3 // 2, 1, seed + i).reshape(h * 3 // 2, w) for i, (w, h) in enumerate(sizes))
    for f in fr:
        f.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def smooth_frames(sizes, seed):
    """Smooth frames: neighbouring cameras' samples correlate, so the estimated gains are well conditioned."""
    from octvr_amd import synthetic
    fr = tuple(np.ascontiguousarray(synthetic.smooth_yuv_frame(w, h, seed + i)) for i, (w, h) in enumerate(sizes))
    for f in fr:
        f.setflags(write=False)
    return fr


def given_gains(n, f=0):
    return [0.8 + 0.05 * ((f + 2 * i) % 7) for i in range(n)]


_WANT = {}


def _digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(repr((a.shape, a.dtype.str)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def want(c, frames, **kw):
    """The oracle's stitch_frame of the case, computed once per distinct input and read-only: (output, gains).  The
    cache key holds the case's key and masks, a digest of the frames and of the seams and vignette maps, and the
    other arguments."""
    arrays = list(frames) + list(c.mk) + list(kw.get("seams") or [])
    vig = kw.get("vig")
    vig_key = None if vig is None else tuple(None if v is None else _digest(v) for v in vig)
    k = (c.key, _digest(*arrays), vig_key, tuple(sorted((a, repr(b)) for a, b in kw.items() if a not in ("seams", "vig"))))
    if k not in _WANT:
        r = O.stitch_frame(list(frames), list(c.sizes), [list(r) for r in c.rois], list(c.m1), list(c.m2), list(c.mk),
                           c.W, c.H, threads=8, **kw)
        for a in r:
            a.setflags(write=False)
        _WANT[k] = r
    return _WANT[k]


def black_region(c, i=0):
    """Boolean (H, W) image of the output pixels at which all four taps of camera i lie outside its image
    (cv::remap's cell from the fixed-point coordinate, as the oracle and the tiler take it)."""
    (w, h), m1, m2 = c.sizes[i], c.m1[i], c.m2[i]
    sx = np.rint((m1 * np.float32(w)) * np.float32(32)).astype(np.int64) >> 5
    sy = np.rint((m2 * np.float32(h)) * np.float32(32)).astype(np.int64) >> 5
    return (sx >= w) | (sy >= h) | (sx + 1 < 0) | (sy + 1 < 0)
