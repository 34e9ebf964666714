"""Host-side checks of the NV12 AsyncMultiMapper pipeline (no GPU): the copy-in's packing of a footprint run
(octvr_debug_pack_runs runs the pipeline's own pack_run) gives the same luma bytes and run sizes for the
planar and the NV12 planes of the same pixels, with chroma bytes that are each other's interleave; and the
two new entry points reject bad arguments without a device."""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O

SIZES = [(324, 240), (256, 144), (16, 2)]  # w % 8 == 4 (a partial last group), w % 8 == 0, one row pair


def _planes(seed):
    planar, nv12 = [], []
    for i, (w, h) in enumerate(SIZES):
        # pitches above the widths, different per plane
        y = O.rand_img(w + 12, h, 1, seed + 3 * i)[:, :w]
        u = O.rand_img(w // 2 + 6, h // 2, 1, seed + 3 * i + 1)[:, :w // 2]
        v = O.rand_img(w // 2 + 10, h // 2, 1, seed + 3 * i + 2)[:, :w // 2]
        uv = np.zeros((h // 2, w + 4), np.uint8)[:, :w]
        uv[:, 0::2] = u
        uv[:, 1::2] = v
        planar.append((y, u, v))
        nv12.append((y, uv))
    return planar, nv12


def _runs(seed):
    rng = np.random.RandomState(seed)
    runs = []
    for cam, (w, h) in enumerate(SIZES):
        G = (w + 7) // 8
        runs.append((cam, h // 2 - 1, G - 1, 1))  # the last group (partial for 324) of the last row pair
        runs.append((cam, 0, 0, G))                # a whole row pair
        runs.append((cam, h // 2 - 1, 0, 1))
        for _ in range(40):
            g0 = int(rng.randint(0, G))
            runs.append((cam, int(rng.randint(0, h // 2)), g0, int(rng.randint(1, G - g0 + 1))))
    order = rng.permutation(len(runs))
    return [runs[k] for k in order]


def test_pack_run_layouts_agree(product_lib):
    ox = product_lib
    assert hasattr(ox.lib(), "octvr_debug_pack_runs"), "octvr_debug_pack_runs is missing"
    planar, nv12 = _planes(5100)
    runs = _runs(7)
    pp, ps = ox.debug_pack_runs(SIZES, runs, planar, "yuv420p")
    pn, ns = ox.debug_pack_runs(SIZES, runs, nv12, "nv12")
    assert np.array_equal(ps, ns), "run sizes differ between the layouts"
    assert len(pp) == len(pn) == int(ps.sum())
    off = 0
    for (cam, rp, g0, ng), n in zip(runs, ps):
        w, h = SIZES[cam]
        y, u, v = planar[cam]
        x0 = 8 * g0
        yb = min(8 * (g0 + ng), w) - x0
        assert n == 3 * yb, (cam, rp, g0, ng)
        a, b = pp[off:off + n], pn[off:off + n]
        # luma: rows 2 rp and 2 rp + 1, equal in both and equal to the source
        assert np.array_equal(a[:yb], y[2 * rp, x0:x0 + yb]) and np.array_equal(a[yb:2 * yb], y[2 * rp + 1, x0:x0 + yb])
        assert np.array_equal(a[:2 * yb], b[:2 * yb])
        # chroma: planar packs U then V (yb / 2 bytes each), NV12 their interleave
        cb = yb // 2
        assert np.array_equal(a[2 * yb:2 * yb + cb], u[rp, 4 * g0:4 * g0 + cb])
        assert np.array_equal(a[2 * yb + cb:], v[rp, 4 * g0:4 * g0 + cb])
        assert np.array_equal(b[2 * yb::2], a[2 * yb:2 * yb + cb]), "NV12 chroma is not the interleave (U)"
        assert np.array_equal(b[2 * yb + 1::2], a[2 * yb + cb:]), "NV12 chroma is not the interleave (V)"
        off += n


def test_pack_runs_rejects_bad_arguments(product_lib):
    ox = product_lib
    planar, nv12 = _planes(5200)
    with pytest.raises(ox.OctvrError):  # row pair past the frame
        ox.debug_pack_runs(SIZES, [(0, 120, 0, 1)], nv12, "nv12")
    with pytest.raises(ox.OctvrError):  # groups past the row
        ox.debug_pack_runs(SIZES, [(0, 0, 40, 2)], nv12, "nv12")
    with pytest.raises(ox.OctvrError):  # planar needs the third plane
        ox.debug_pack_runs(SIZES, [(0, 0, 0, 1)], nv12, "yuv420p")
    with pytest.raises(ox.OctvrError):  # unknown format
        ox.debug_pack_runs(SIZES, [(0, 0, 0, 1)], nv12, 2)
    with pytest.raises(ox.OctvrError):  # a U,V pitch below W
        ox.debug_pack_runs(SIZES, [(0, 0, 0, 1)], [(y, np.zeros((h // 2, w - 2), np.uint8))
                                                   for (y, uv), (w, h) in zip(nv12, SIZES)], "nv12")


def test_async_pixel_format_entry_points_reject_bad_arguments(product_lib):
    ox = product_lib
    lib = ox.lib()
    assert hasattr(lib, "octvr_async_set_pixel_formats") and hasattr(lib, "octvr_async_pixel_formats")
    a, b = C.c_int(-7), C.c_int(-7)
    assert lib.octvr_async_set_pixel_formats(None, ox.PIX_NV12, ox.PIX_NV12) == ox.E_INVALID
    assert lib.octvr_async_set_pixel_formats(None, 2, ox.PIX_YUV420P) == ox.E_INVALID
    assert lib.octvr_async_set_pixel_formats(None, ox.PIX_NV12, -1) == ox.E_INVALID
    assert lib.octvr_async_pixel_formats(None, C.byref(a), C.byref(b)) == ox.E_INVALID
    assert (a.value, b.value) == (-7, -7)
    assert lib.octvr_last_error()
