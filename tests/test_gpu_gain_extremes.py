"""The gain path at its numeric edges, on the device: the solvers' row swaps, pivot ties and failure branch
(octvr_debug_gain_solve runs the function the feed kernels end in), feeds whose systems swap rows (a dark
camera beside a bright one), and the gain application at exact rounding ties and far past saturation through
every path that has its own finish.  Everything is compared bit for bit with the oracle, whose solver the
golden systems pin to the reference; the matrix families and lu_trace come from tests/gain_systems.py, which
tests/test_gain_solve_host.py pins to the oracle on the CPU.
"""
import numpy as np
import pytest

import gain_systems as G
import oracle_py as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ox(product_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    assert hasattr(product_lib.lib(), "octvr_debug_gain_solve"), "octvr_debug_gain_solve is missing"
    return product_lib


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ---- a. the device solver, directly ----------------------------------------------------------------------
@pytest.mark.parametrize("lean", [0, 1], ids=["full", "lean"])
@pytest.mark.parametrize("n", range(1, 17))
def test_gpu_gain_solve_families(ox, n, lean):
    """Full feed's choice (closed forms n <= 3, register LU 4..8, workgroup LU 9..16) and lean feed's (closed
    forms, workgroup LU 4..16): flag and x equal to the oracle's, bit for bit (-0.0 and the last ulp count)."""
    fams = G.families(n)
    A = np.stack([f[1] for f in fams])
    b = np.stack([f[2] for f in fams])
    want = [O.solve(f[1], f[2]) for f in fams]
    if n >= 4:  # a green run proves the swap branch, the tie rule and the failure branch ran
        traces = [G.lu_trace(f[1], f[2]) for f in fams]
        for f, (_, swaps, ok) in zip(fams, traces):
            G.check_expect(f[0], n, swaps, ok, f[3])
        assert sum(1 for t in traces if t[1]) >= 10 and sum(1 for t in traces if not t[2]) >= 5
    assert any(w is None for w in want) and any(w is not None for w in want)
    x, ok = ox.debug_gain_solve(A, b, lean=bool(lean))
    for k, f in enumerate(fams):
        assert bool(ok[k]) == (want[k] is not None), (f[0], n, lean, k)
        if want[k] is not None:
            assert np.array_equal(_bits(x[k]), _bits(want[k])), (f[0], n, lean, k, x[k], want[k])


# ---- b. feeds whose systems swap rows ----------------------------------------------------------------------
IN_W, IN_H, OUT_W, OUT_H = 320, 240, 512, 256
DARK, BRIGHT = (35, 58), (231, 255)  # luma bands: grey of norm sqrt(3) Y = 60..100 and 400..441
HIGHLIGHT = 236                      # dark cameras' highlights: below 255 as shot, at 255 under a gain above 1.08


def band_frame(w, h, seed, band, highlight=0):
    """synthetic.smooth_yuv_frame with its luma mapped into `band`, its chroma pulled to 128 +- 7, and (dark
    cameras) a grid of 6 x 6 highlights that a gain above 1 saturates."""
    from octvr_amd import synthetic
    f = synthetic.smooth_yuv_frame(w, h, seed)
    y = np.rint(band[0] + (band[1] - band[0]) * f[:h].astype(np.float32) / 255.0).astype(np.uint8)
    if highlight:
        for yy in range(8, h - 6, 24):
            for xx in range(8, w - 6, 24):
                y[yy:yy + 6, xx:xx + 6] = highlight
    out = f.copy()
    out[:h] = y
    out[h:] = np.rint(128 + (f[h:].astype(np.float32) - 128) * 0.15).astype(np.uint8)
    return out


def pairs_rig(n):
    """n cameras as near-coincident pairs (yaws t, t + 0.06) spread round the ring, a single camera last where n
    is odd, with a field of view small enough that the groups do not overlap: every camera of a pair has one
    dominant partner."""
    import math
    from octvr_amd import synthetic
    groups = n // 2 + n % 2
    yaws, pitches = [], []
    for k in range(groups):
        for j in range(2 if k < n // 2 else 1):
            yaws.append(2 * math.pi * k / groups + 0.06 * j)
            pitches.append(0.1 * (-1) ** k)
    return synthetic.fisheye_rig(IN_W, IN_H, yaws, pitches, hfov=min(2.4, 0.7 * 2 * math.pi / groups))


_FEED = {}


def feed_case(n):
    """The rig's LUT (the oracle's, built on the CPU), two frames of alternating dark and bright cameras (the
    second with the roles exchanged), and the oracle's stitch of each; the preconditions are asserted here, on
    the CPU, before anything is launched."""
    import json
    if n in _FEED:
        return _FEED[n]
    res = O.lut_build(O.json_loads_rj(json.dumps(pairs_rig(n))), OUT_W, OUT_H, use_roi=True, threads=8)
    t = dict(W=OUT_W, H=OUT_H, n=n, sizes=[(IN_W, IN_H)] * n, rois=[list(r[0]) for r in res], maps1=[r[1] for r in res],
             maps2=[r[2] for r in res], masks=[r[3] for r in res], seams=None)
    frames, wants = [], []
    for fno in range(2):
        fr = []
        for i in range(n):
            dark = (i % 2 == 1) ^ (i // 2 % 2 == 1) ^ (fno == 1)
            fr.append(band_frame(IN_W, IN_H, 900 + 10 * fno + i, DARK if dark else BRIGHT, HIGHLIGHT if dark else 0))
        N, I, A, b = O.gain_system(t["rois"], O.warp_inputs(fr, t["sizes"], t["maps1"], t["maps2"]), t["masks"], OUT_W, OUT_H)
        want, g = O.stitch_frame(fr, t["sizes"], t["rois"], t["maps1"], t["maps2"], t["masks"], OUT_W, OUT_H,
                                 enable_gain=True, gains=None, threads=8)
        assert np.array_equal(_bits(O.solve(A, b)), _bits(g))
        if n >= 4:  # every case with an LU swaps rows (n = 3 is the closed form)
            x, swaps, ok = G.lu_trace(A, b)
            assert ok and swaps and np.array_equal(_bits(x), _bits(g)), (n, fno, swaps)
        assert g.min() > 0 and g.max() / g.min() >= 2.0, (n, fno, g)
        plain, _ = O.stitch_frame(fr, t["sizes"], t["rois"], t["maps1"], t["maps2"], t["masks"], OUT_W, OUT_H,
                                  enable_gain=True, gains=[1.0] * n, threads=8)
        assert ((want[:OUT_H] == 255) & (plain[:OUT_H] < 255)).sum() >= 16, (n, fno)  # the gain saturates
        want.setflags(write=False)
        frames.append(fr)
        wants.append((want, g))
    _FEED[n] = (t, frames, wants)
    return _FEED[n]


FEED_CASES = [(n, k, "yuv420p") for n in (3, 4, 8, 9, 16) for k in (1, 2)] + [(4, 2, "nv12"), (9, 1, "nv12")]


@pytest.mark.parametrize("n,inflight,fmt", FEED_CASES, ids=["n%d-inflight%d-%s" % c for c in FEED_CASES])
def test_gpu_feed_swapping_systems(ox, n, inflight, fmt):
    """A dark camera beside a bright one per pair: the feed's system swaps rows in cv::solve's LU (register LU
    n = 4, 8 with one frame in flight; workgroup LU n = 9, 16, and n >= 4 in the lean feed that frames in flight
    select; n = 3 the closed form), the gains span more than a factor of 2 and saturate highlights.  Two frames in
    a row (totals and tickets reset): gains and output equal to the oracle's."""
    import torch
    import test_gpu_nv12 as NV
    t, frames, wants = feed_case(n)  # CPU: oracle and preconditions first
    mt = ox.MapperTemplate.from_arrays(OUT_W, OUT_H, t["rois"], t["maps1"], t["maps2"], t["masks"])
    m = ox.Mapper(mt, t["sizes"], blend=0, enable_gain=True)
    m.set_frames_in_flight(inflight)
    m.set_pixel_formats(fmt, fmt)
    for fno in range(2):
        out = torch.zeros((OUT_H * 3 // 2, OUT_W), dtype=torch.uint8, device="cuda")
        m.stitch(NV.dev_frames(frames[fno], t["sizes"], fmt), out)
        torch.cuda.synchronize()
        want, g = wants[fno]
        assert np.array_equal(_bits(m.gains()), _bits(g)), (n, fno, m.gains(), g)
        NV.check(out.cpu().numpy(), want, t, fmt, (n, inflight, fno))


# ---- c. gain application at rounding ties and far past saturation --------------------------------------------
GAINS = [0.5, 1.5, 2.5, 0.25, 255.0, 0.0, -0.5, 1.0]


def tie_gains(n, off=0):
    return [GAINS[(i + off) % len(GAINS)] for i in range(n)]


_TIE = {}


def tie_frames(key, sizes, seed=5200):
    if key not in _TIE:
        _TIE[key] = [O.rand_img(w, h * 3 // 2, 1, seed + 13 * i) for i, (w, h) in enumerate(sizes)]
    return _TIE[key]


def test_gpu_tie_gains_hit_ties_and_saturate(ox):
    """The inputs of the tests below, on the oracle's side: under g = 0.5 every odd channel value is an exact
    .5 tie in f32 (at least 10 % of a 0.5 camera's gained values), and 255.0 saturates."""
    import test_gpu_nv12 as NV
    t = NV.golden("rigB")
    g = tie_gains(t["n"])
    warped = O.warp_inputs(tie_frames("rigB", t["sizes"]), t["sizes"], t["maps1"], t["maps2"])
    c = warped[g.index(0.5)][t["masks"][g.index(0.5)] > 0][:, :3].astype(np.float32)
    prod = c * np.float32(0.5)
    assert (prod - np.floor(prod) == 0.5).mean() >= 0.10
    c = warped[g.index(255.0)][t["masks"][g.index(255.0)] > 0][:, :3].astype(np.float32)
    assert (c * np.float32(255.0) > 255.5).mean() > 0.9
    want, _ = NV.oracle(t, tie_frames("rigB", t["sizes"]), enable_gain=True, gains=g)
    plain, _ = NV.oracle(t, tie_frames("rigB", t["sizes"]), enable_gain=True, gains=[1.0] * t["n"])
    assert ((want[:t["H"]] == 255) & (plain[:t["H"]] < 255)).sum() > 100


TIE_PATHS = ["quad", "quad_forced", "entry32", "wide", "nv12", "batch2", "batch4", "texture", "multiband16", "feather5", "scaled_preview",
             "prepared_preview"]


@pytest.mark.parametrize("path", TIE_PATHS)
def test_gpu_tie_gains_every_finish(ox, path, monkeypatch):
    """Fixed gains k + 0.5, 0.25, 255, 0, negative and 1 per camera on independent random bytes through every
    path with a finish of its own: sat_u8(rne(c * (float)g)), bit-equal to the oracle."""
    import torch
    import test_gpu_nv12 as NV
    off = TIE_PATHS.index(path)
    kw, okw, fmt, blend = {}, {}, "yuv420p", 0
    monkeypatch.delenv("OCTVR_ENTRY32", raising=False)
    monkeypatch.delenv("OCTVR_ENTRY_QUAD", raising=False)
    if path == "entry32":
        monkeypatch.setenv("OCTVR_ENTRY32", "1")
    if path == "quad_forced":  # rigB packs no item by default (fewer than half qualify)
        monkeypatch.setenv("OCTVR_ENTRY_QUAD", "1")
    if path == "wide":
        mt, t = NV.ring(ox, 5, in_w=324, in_h=240)  # the ring of test_gpu_nv12_unaligned: gathered (wide) tiles
    else:
        key = {"feather5": "rigC", "quad": "rigA"}.get(path, "rigB")  # rigA packs quads by default
        t = NV.golden(key)
        mt = NV.template(ox, t)
    if path == "wide":
        key = "wide"
    if path == "nv12":
        fmt = "nv12"
    if path == "texture":
        kw["remap"], okw["remap_tex"] = "texture", True
    if path == "multiband16":
        blend = 16
    if path == "feather5":
        blend = -5
    if blend:
        okw.update(blend=blend, seams=t["seams"])
    scale = preview = None
    if path == "scaled_preview":
        scale, preview = (t["W"] // 2, t["H"] // 2), (200, 100)
        kw["scale_output"] = scale
        okw.update(scale=scale, preview=preview)
    if path == "prepared_preview":
        preview = (320, 180)
        okw.update(preview=preview)
    m = ox.Mapper(mt, t["sizes"], blend=blend, enable_gain=True, **kw)
    info = m.info()
    if path in ("quad", "quad_forced"):
        assert info["items_packed"] > 0
    if path == "entry32":
        assert info["items_packed"] == 0
    if path == "wide":
        assert info["wide_tiles"] > 0
    m.set_pixel_formats(fmt, fmt)
    W, H = scale if scale else (t["W"], t["H"])
    if path in ("batch2", "batch4"):
        nb = int(path[5:])
        m.set_frames_in_flight(4)
        sets = [tie_frames((key, f), t["sizes"], 5200 + 100 * f) for f in range(nb)]
        outs = [NV._out(W, H) for _ in range(nb)]
        gl = [tie_gains(t["n"], off + f) for f in range(nb)]
        m.stitch_batch([NV.dev_frames(fr, t["sizes"], fmt) for fr in sets], outs, gains=gl)
        torch.cuda.synchronize()
        for f in range(nb):
            want, _ = NV.oracle(t, sets[f], enable_gain=True, gains=gl[f])
            NV.check(outs[f].cpu().numpy(), want, t, fmt, (path, f))
        return
    frames = tie_frames(key, t["sizes"])
    out = NV._out(W, H)
    pv = None
    if preview:
        if path == "prepared_preview":
            m.prepare_preview(*preview)
            assert m.info()["preview_prepared"] == list(preview)
        pv = torch.full((preview[1], preview[0], 3), 0x5A, dtype=torch.uint8, device="cuda")
    dev = NV.dev_frames(frames, t["sizes"], fmt)
    # rigs with fewer than 8 cameras: further stitches until every gain of the cycle was applied
    for o in range(off, off + len(GAINS), t["n"]):
        gains = tie_gains(t["n"], o)
        m.stitch(dev, out, gains=gains, preview=pv)
        torch.cuda.synchronize()
        res = NV.oracle(t, frames, enable_gain=True, gains=gains, **okw)
        np.testing.assert_array_equal(np.array(m.gains()), np.array(gains))
        NV.check(out.cpu().numpy(), res[0], t, fmt, (path, o))
        if preview:
            d = pv.cpu().numpy() != res[2]
            assert not d.any(), (path, o, int(d.sum()), np.argwhere(d)[:5].tolist())
