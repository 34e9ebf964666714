"""The prepared preview of a blend-0 mapper (octvr_mapper_prepare_preview, preview_gather_kernel): the preview
gathered from the source frames through a tap list, no result frame, any number of frames in flight.  Bit-exact
against the oracle's Mapper::stitch preview (tests/overlay_ref.py for the overlay rig), never against the
library's own result-frame path.  rigB (384 x 192, six inputs), rigA (512 x 256)."""
import copy
import functools
import json

import numpy as np
import pytest

import camera_rigs as R
import oracle_py as O
import overlay_ref as OR

pytestmark = pytest.mark.gpu

SMALL = (320, 180)  # the smallest prepared size of the parity case


@functools.lru_cache(maxsize=None)
def _rig(name):
    rig, z = O.load_rig(name)
    n = len(z["rois"])
    W, H = (int(v) for v in z["out_size"])
    return {"rig": rig, "W": W, "H": H, "n": n, "rois": z["rois"].tolist(),
            "sizes": [(rig["inputs"][i]["options"]["width"], rig["inputs"][i]["options"]["height"]) for i in range(n)],
            "map1": [z[f"map1_{i}"] for i in range(n)], "map2": [z[f"map2_{i}"] for i in range(n)],
            "masks": [z[f"mask_{i}"] for i in range(n)], "seams": [z[f"seam_{i}"] for i in range(n)]}


def _template(ox, t, seams=True):
    return ox.MapperTemplate.from_arrays(t["W"], t["H"], t["rois"], t["map1"], t["map2"], t["masks"],
                                         t["seams"] if seams else None)


@functools.lru_cache(maxsize=None)
def _frames(name, seed):
    from octvr_amd import synthetic
    return tuple(synthetic.smooth_yuv_frame(w, h, seed + i) for i, (w, h) in enumerate(_rig(name)["sizes"]))


@functools.lru_cache(maxsize=None)
def _want(name, seed, preview, gains=None, remap_tex=False):
    """(output, gains, preview) of the oracle for rig `name`, blend 0; computed once per case, never changed."""
    t = _rig(name)
    out, g, pv = O.stitch_frame(list(_frames(name, seed)), t["sizes"], t["rois"], t["map1"], t["map2"], t["masks"],
                                t["W"], t["H"], enable_gain=True, gains=list(gains) if gains else None, blend=0,
                                threads=8, preview=preview, remap_tex=remap_tex)
    for a in (out, pv):
        a.setflags(write=False)
    return out, np.asarray(g, np.float64), pv


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    d = got != want
    assert got.shape == want.shape and not d.any(), (what, int(d.sum()), np.argwhere(d)[:5].tolist())


def _cuda(frames):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames]


def _bufs(W, H, preview):
    import torch
    return (torch.zeros((H * 3 // 2, W), dtype=torch.uint8, device="cuda"),
            torch.full((preview[1], preview[0], 3), 0x5A, dtype=torch.uint8, device="cuda"))


def _entries(preview):
    return (4 * preview[0] * preview[1] + 255) // 256 * 256


# ---- 1. parity and path --------------------------------------------------------------------------------
@pytest.mark.parametrize("preview", [SMALL, (384, 192), (1000, 500), (301, 201)])
def test_gpu_prepared_preview_bit_exact(product_lib, preview):
    """Down-scale, identity, up-scale (where most pixels' upper taps clamp to the last row and column and the
    weights still come from the unclamped coordinate) and an odd width at pitch 3 * 301: gains estimated, then
    set.  Preview and output equal the oracle's, the output equals a stitch without a preview."""
    import torch
    ox = product_lib
    t = _rig("rigB")
    m = ox.Mapper(_template(ox, t), t["sizes"], blend=0, enable_gain=True)
    assert m.info()["preview_prepared"] == [0, 0] and m.info()["preview_entries"] == 0
    m.prepare_preview(*preview)
    info = m.info()
    assert info["preview_prepared"] == list(preview) and info["preview_entries"] == _entries(preview)
    dev = _cuda(_frames("rigB", 900))
    for gains in (None, tuple(1.0 + 0.017 * k * (-1) ** k for k in range(t["n"]))):
        out, pv = _bufs(t["W"], t["H"], preview)
        assert pv.stride(0) == 3 * preview[0]
        m.stitch(dev, out, gains=list(gains) if gains else None, preview=pv)
        plain = torch.zeros_like(out)
        m.stitch(dev, plain, gains=list(gains) if gains else None)
        torch.cuda.synchronize()
        want, g, want_pv = _want("rigB", 900, preview, gains)
        _same(np.asarray(m.gains()).view(np.int64), g.view(np.int64), "gains")
        _same(out.cpu().numpy(), want, ("output", gains))
        assert torch.equal(out, plain)
        _same(pv.cpu().numpy(), want_pv, ("preview", preview, gains))


# ---- 2. frames in flight -------------------------------------------------------------------------------
def test_gpu_prepared_preview_frames_in_flight(product_lib):
    """Three frame slots, six distinct frame sets round-robin on three streams, each with its own output and
    preview: every one equals the oracle's, and so do the last frame's gains."""
    import torch
    ox = product_lib
    t = _rig("rigB")
    m = ox.Mapper(_template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.prepare_preview(*SMALL)
    m.set_frames_in_flight(3)
    assert m.info()["preview_prepared"] == list(SMALL)  # the slots do not touch the list
    seeds = [900 + 10 * f for f in range(6)]
    dev = [_cuda(_frames("rigB", s)) for s in seeds]
    bufs = [_bufs(t["W"], t["H"], SMALL) for _ in seeds]
    streams = [torch.cuda.Stream() for _ in range(3)]
    torch.cuda.synchronize()
    for f in range(6):
        m.stitch(dev[f], bufs[f][0], stream=streams[f % 3], preview=bufs[f][1])
    torch.cuda.synchronize()
    for f, s in enumerate(seeds):
        want, g, want_pv = _want("rigB", s, SMALL)
        _same(bufs[f][0].cpu().numpy(), want, ("output", f))
        _same(bufs[f][1].cpu().numpy(), want_pv, ("preview", f))
    _same(np.asarray(m.gains()).view(np.int64), _want("rigB", seeds[-1], SMALL)[1].view(np.int64), "last gains")


# ---- 3. the layouts and modes the gather helper branches on ---------------------------------------------
def test_gpu_prepared_preview_nv12(product_lib):
    """NV12 frames in and out; the preview stays RGB."""
    ox = product_lib
    t = _rig("rigB")
    m = ox.Mapper(_template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats("nv12", "nv12")
    m.prepare_preview(*SMALL)
    import torch
    out, pv = _bufs(t["W"], t["H"], SMALL)
    m.stitch(_cuda([ox.nv12_from_yuv420p(f, w, h) for f, (w, h) in zip(_frames("rigB", 900), t["sizes"])]), out,
             preview=pv)
    torch.cuda.synchronize()
    want, g, want_pv = _want("rigB", 900, SMALL)
    _same(ox.yuv420p_from_nv12(out.cpu().numpy(), t["W"], t["H"]), want, "output")
    _same(pv.cpu().numpy(), want_pv, "preview")
    _same(np.asarray(m.gains()).view(np.int64), g.view(np.int64), "gains")


def test_gpu_prepared_preview_vignette(product_lib):
    """Vignetted inputs (some cameras without one): the correction is applied to every source tap before the
    filter, as the composite's staging does."""
    import torch
    ox = product_lib
    t = _rig("rigB")
    rig = json.loads(json.dumps(t["rig"]))
    for k, c in enumerate(rig["inputs"]):
        if k % 3 != 2:
            c["options"]["vignette"] = [1.0 + 0.05 * k, -0.35, 0.12 - 0.01 * k, -0.04]
    W, H, sizes = t["W"], t["H"], t["sizes"]
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
    vig = []
    for c, (w, h) in zip(rig["inputs"], sizes):
        v = O.vignette_map(c["options"])
        vig.append(None if v is None else O.resize_linear_cuda_f32(v, w, h))
    rois, m1, m2, mk = [], [], [], []
    for i in range(len(mt)):
        roi, a, b, c, _ = mt.input(i)
        rois.append(roi); m1.append(a); m2.append(b); mk.append(c)
    m = ox.Mapper(mt, sizes, blend=0, enable_gain=True)
    m.prepare_preview(*SMALL)
    frames = list(_frames("rigB", 900))
    out, pv = _bufs(W, H, SMALL)
    m.stitch(_cuda(frames), out, preview=pv)
    torch.cuda.synchronize()
    want, g, want_pv = O.stitch_frame(frames, sizes, rois, m1, m2, mk, W, H, enable_gain=True, blend=0, vig=vig,
                                      threads=8, preview=SMALL)
    _same(out.cpu().numpy(), want, "output")
    _same(pv.cpu().numpy(), want_pv, "preview")
    _same(np.asarray(m.gains()).view(np.int64), np.asarray(g, np.float64).view(np.int64), "gains")


def test_gpu_prepared_preview_texture_mode(product_lib):
    """remap="texture": the entries carry the texture convention and the kernel filters them with its model."""
    import torch
    ox = product_lib
    t = _rig("rigB")
    m = ox.Mapper(_template(ox, t), t["sizes"], blend=0, enable_gain=True, remap="texture")
    m.prepare_preview(*SMALL)
    out, pv = _bufs(t["W"], t["H"], SMALL)
    m.stitch(_cuda(_frames("rigB", 900)), out, preview=pv)
    torch.cuda.synchronize()
    want, g, want_pv = _want("rigB", 900, SMALL, remap_tex=True)
    _same(out.cpu().numpy(), want, "output")
    _same(pv.cpu().numpy(), want_pv, "preview")
    _same(np.asarray(m.gains()).view(np.int64), g.view(np.int64), "gains")


def test_gpu_prepared_preview_unaligned_pitch(product_lib):
    """Every input inside a wider byte tensor from flat offset 2 (base pointer + 2, pitch w + 2), and a preview
    whose rows are 7 bytes apart from tight: nothing outside the preview's pixels is written."""
    import torch
    ox = product_lib
    t = _rig("rigB")
    m = ox.Mapper(_template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.prepare_preview(*SMALL)
    dev = []
    for f, (w, h) in zip(_frames("rigB", 900), t["sizes"]):
        rows = h * 3 // 2
        buf = torch.full(((rows + 1) * (w + 2),), 0xA5, dtype=torch.uint8, device="cuda")
        v = buf[2:2 + rows * (w + 2)].view(rows, w + 2)[:, :w]
        v.copy_(torch.from_numpy(f).cuda())
        assert v.data_ptr() % 8 == 2 and v.stride(0) == w + 2
        dev.append(v)
    out, _ = _bufs(t["W"], t["H"], SMALL)
    pw, ph = SMALL
    wide = torch.full((ph, 3 * pw + 7), 0x5A, dtype=torch.uint8, device="cuda")
    pv = wide[:, :3 * pw].unflatten(1, (pw, 3))
    assert pv.stride(0) == 3 * pw + 7 and pv.stride(1) == 3
    m.stitch(dev, out, preview=pv)
    torch.cuda.synchronize()
    want, g, want_pv = _want("rigB", 900, SMALL)
    _same(out.cpu().numpy(), want, "output")
    got = wide.cpu().numpy()
    _same(got[:, :3 * pw].reshape(ph, pw, 3), want_pv, "preview")
    assert (got[:, 3 * pw:] == 0x5A).all(), "bytes between the preview's rows were written"


# ---- 4. overlay at blend 0 -----------------------------------------------------------------------------
def test_gpu_prepared_preview_overlay(product_lib):
    """The overlay_include rig: the overlay is a camera of the same LUT, so the list covers it with no extra
    work; where it wins the preview shows it un-gained (the inputs' gains are not 1)."""
    import torch
    ox = product_lib
    W, H, preview = 512, 256, (200, 100)
    rig = copy.deepcopy(R.mask_rigs()["overlay_include"])
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
    tt = OR.prepare(mt)
    sizes = [(640, 360)] * len(rig["inputs"]) + [(192, 128)]
    frames = [O.rand_img(w, h * 3 // 2, 1, 40 + i) for i, (w, h) in enumerate(sizes)]
    want = OR.expected(tt, frames, sizes, blend=0, enable_gain=True, preview=preview)
    m = ox.Mapper(mt, sizes, blend=0, enable_gain=True)
    m.prepare_preview(*preview)
    assert m.info()["overlays"] == 1 and m.info()["preview_prepared"] == list(preview)
    out, pv = _bufs(W, H, preview)
    m.stitch(_cuda(frames), out, preview=pv)
    torch.cuda.synchronize()
    g = np.asarray(m.gains(), np.float64)
    assert len(g) == tt["n"] and (g != 1.0).any()
    _same(g.view(np.int64), np.asarray(want[1], np.float64).view(np.int64), "gains")
    _same(out.cpu().numpy(), want[0], "output")
    _same(pv.cpu().numpy(), want[2], "preview")
    assert (np.asarray(tt["masks"][tt["n"]]) != 0).sum() > 1000, "the overlay wins next to nothing"


# ---- 5. arbitrary map values ----------------------------------------------------------------------------
def test_gpu_prepared_preview_out_of_range_maps(product_lib):
    """Claimed pixels whose maps are < 0, >= 1 and NaN (test_gpu_morph's construction), and unclaimed ones: taps
    outside the image read 0, unclaimed pixels are black.  Identity (every result pixel on its own) and a
    down-scale, prepared one after the other on one mapper."""
    import torch
    ox = product_lib
    rng = np.random.default_rng(11)
    Wo, Ho = 256, 128
    sizes = [(64, 48), (96, 64)]
    rois, m1s, m2s, mks = [], [], [], []
    for i, (w, h) in enumerate(sizes):
        roi = (0, 0, Wo, Ho) if i == 0 else (32, 16, 160, 96)
        m1 = rng.uniform(-0.08, 1.08, (roi[3], roi[2])).astype(np.float32)
        m2 = rng.uniform(-0.08, 1.08, (roi[3], roi[2])).astype(np.float32)
        m1[rng.random(m1.shape) < 0.01] = np.nan
        m2[rng.random(m2.shape) < 0.01] = -5.0
        m1[::7, ::5] = np.float32(-0.5 / w)
        mk = np.where(rng.random(m1.shape) < 0.9, 255, 0).astype(np.uint8)
        rois.append(roi); m1s.append(m1); m2s.append(m2); mks.append(mk)
    mt = ox.MapperTemplate.from_arrays(Wo, Ho, rois, m1s, m2s, mks)
    frames = [O.rand_img(w, h * 3 // 2, 1, 70 + i).reshape(h * 3 // 2, w) for i, (w, h) in enumerate(sizes)]
    m = ox.Mapper(mt, sizes, blend=0, enable_gain=True)
    dev = _cuda(frames)
    for preview in ((Wo, Ho), (200, 90)):
        m.prepare_preview(*preview)  # the second call replaces the first list
        assert m.info()["preview_prepared"] == list(preview)
        out, pv = _bufs(Wo, Ho, preview)
        m.stitch(dev, out, preview=pv)
        torch.cuda.synchronize()
        want, g, want_pv = O.stitch_frame(frames, sizes, rois, m1s, m2s, mks, Wo, Ho, enable_gain=True, blend=0,
                                          preview=preview)
        np.testing.assert_array_equal(np.array(m.gains()), g)
        _same(out.cpu().numpy(), want, ("output", preview))
        _same(pv.cpu().numpy(), want_pv, ("preview", preview))
        assert (want_pv == 0).all(axis=2).any(), "no black preview pixel in the expectation"


# ---- 6. fallback and errors -----------------------------------------------------------------------------
def test_gpu_prepared_preview_fallback(product_lib):
    """A preview of another size than the prepared one takes the result-frame path: the oracle's bytes, one
    frame in flight only; prepare_preview(0, 0) returns every size to that path."""
    import torch
    ox = product_lib
    t = _rig("rigB")
    other = (200, 100)
    m = ox.Mapper(_template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.prepare_preview(*SMALL)
    dev = _cuda(_frames("rigB", 900))
    want, g, want_pv = _want("rigB", 900, other)
    out, pv = _bufs(t["W"], t["H"], other)
    m.stitch(dev, out, preview=pv)
    torch.cuda.synchronize()
    _same(out.cpu().numpy(), want, "output, other size")
    _same(pv.cpu().numpy(), want_pv, "preview, other size")
    m.set_frames_in_flight(2)
    with pytest.raises(ox.OctvrError) as e:
        m.stitch(dev, out, preview=pv)
    assert e.value.code == ox.E_INVALID and "one frame in flight" in str(e.value)
    out2, pv2 = _bufs(t["W"], t["H"], SMALL)
    m.stitch(dev, out2, preview=pv2)  # the prepared size is not bound to one slot
    torch.cuda.synchronize()
    _same(pv2.cpu().numpy(), _want("rigB", 900, SMALL)[2], "preview, prepared size, two in flight")
    m.prepare_preview(0, 0)
    assert m.info()["preview_prepared"] == [0, 0] and m.info()["preview_entries"] == 0
    with pytest.raises(ox.OctvrError) as e:
        m.stitch(dev, out2, preview=pv2)
    assert e.value.code == ox.E_INVALID and "one frame in flight" in str(e.value)
    m.set_frames_in_flight(1)
    out2, pv2 = _bufs(t["W"], t["H"], SMALL)
    m.stitch(dev, out2, preview=pv2)
    torch.cuda.synchronize()
    _same(out2.cpu().numpy(), _want("rigB", 900, SMALL)[0], "output, list dropped")
    _same(pv2.cpu().numpy(), _want("rigB", 900, SMALL)[2], "preview, list dropped")


def test_gpu_prepare_preview_errors(product_lib):
    ox = product_lib
    t = _rig("rigB")
    mt = _template(ox, t)
    for kw, word in (({"blend": 16}, "blend"), ({"blend": -5}, "blend"), ({"scale_output": (512, 256)}, "scaled")):
        m = ox.Mapper(mt, t["sizes"], enable_gain=True, **kw)
        with pytest.raises(ox.OctvrError) as e:
            m.prepare_preview(*SMALL)
        assert e.value.code == ox.E_UNSUPPORTED and word in str(e.value), kw
        assert m.info()["preview_prepared"] == [0, 0]
    m = ox.Mapper(mt, t["sizes"], blend=0, enable_gain=True)
    a = _rig("rigA")
    fewer = ox.MapperTemplate.from_arrays(t["W"], t["H"], t["rois"][:5], t["map1"][:5], t["map2"][:5], t["masks"][:5])
    cut = [list(r) for r in t["rois"]]
    cut[0][2] -= 2  # input 0's ROI two columns narrower, its arrays cut to match
    narrow = lambda arrs: [np.ascontiguousarray(arrs[0][:, :cut[0][2]])] + list(arrs[1:])
    shifted = ox.MapperTemplate.from_arrays(t["W"], t["H"], cut, narrow(t["map1"]), narrow(t["map2"]),
                                            narrow(t["masks"]))
    lib = ox.lib()
    for bad in (_template(ox, a, seams=False), fewer, shifted):  # another size, another input count, another ROI
        assert lib.octvr_mapper_prepare_preview(m._h, bad._h, SMALL[0], SMALL[1]) == ox.E_INVALID
        assert b"rig" in lib.octvr_last_error()
    for w, h in ((-1, 10), (10, 0), (0, 10)):
        with pytest.raises(ox.OctvrError) as e:
            m.prepare_preview(w, h)
        assert e.value.code == ox.E_INVALID
    assert m.info()["preview_prepared"] == [0, 0]
    m.prepare_preview(*SMALL)
    assert m.info()["preview_prepared"] == list(SMALL)


# ---- 7. AsyncMultiMapper --------------------------------------------------------------------------------
def test_gpu_async_prepared_preview(product_lib):
    """One blend-0 mapper over the whole output at template size, with a preview: the pipeline prepares it, and
    the published previews and the planes equal the oracle's over three frames."""
    ox = product_lib
    t = _rig("rigB")
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([_template(ox, t)], t["sizes"], (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)],
                             preview_size=SMALL)
    info = am.info()
    assert info["preview"] == list(SMALL) and info["preview_prepared"] == [list(SMALL)]
    sunk = []
    am.set_preview_sink(lambda a, h: sunk.append(a))
    seeds = [900, 910, 920]
    outs = []
    for s in seeds:
        out = (np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8))
        am.push([(f[:h], f[h:, :w // 2], f[h:, w // 2:]) for f, (w, h) in zip(_frames("rigB", s), t["sizes"])], out)
        outs.append(out)
    while am.pending():
        am.pop()
    assert len(sunk) == len(seeds)
    for f, s in enumerate(seeds):
        want, _, want_pv = _want("rigB", s, SMALL)
        _same(outs[f][0], want[:H], ("Y", f))
        _same(outs[f][1], want[H:, :W // 2], ("U", f))
        _same(outs[f][2], want[H:, W // 2:], ("V", f))
        _same(sunk[f], want_pv, ("preview", f))
    _same(am.preview()[0], _want("rigB", seeds[-1], SMALL)[2], "the latest preview")
    am.set_preview_sink(None)
    am.close()
