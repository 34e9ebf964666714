"""NV12 host planes in and out of the AsyncMultiMapper pipeline (octvr_async_set_pixel_formats): copy-in,
unpack kernel, mappers, region downloads, copy-out and registered outputs all carry the layout.  The expected
bytes are always the oracle's planar stitch of the planar frames; the layout permutation is this file's own
numpy (never the library's helpers).  Outputs are prefilled with 0x5A, so bytes that must stay untouched
(outside every region, between a plane's width and its pitch) are checked too."""
import json
import math

import numpy as np
import pytest

import oracle_py as O

pytestmark = pytest.mark.gpu

PAIRS = [("yuv420p", "yuv420p"), ("nv12", "yuv420p"), ("yuv420p", "nv12"), ("nv12", "nv12")]
FILL = 0x5A


@pytest.fixture(scope="module")
def ox(product_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    assert hasattr(product_lib.lib(), "octvr_async_set_pixel_formats"), "octvr_async_set_pixel_formats is missing"
    return product_lib


def interleave(u, v):
    uv = np.empty((u.shape[0], 2 * u.shape[1]), np.uint8)
    uv[:, 0::2] = u
    uv[:, 1::2] = v
    return uv


def in_planes(f, w, h, fmt):
    """Host planes of a "Y over [U|V]" frame for push(): (Y, U, V), or (Y, UV) for NV12."""
    y, u, v = f[:h, :w], f[h:, :w // 2], f[h:, w // 2:w]
    return (y, interleave(u, v)) if fmt == "nv12" else (y, u, v)


def new_out(OW, OH, fmt, pad=0):
    """Output planes full of FILL with pitch = width + pad: (Y, U, V), or (Y, UV) for NV12."""
    y = np.full((OH, OW + pad), FILL, np.uint8)[:, :OW]
    if fmt == "nv12":
        return (y, np.full((OH // 2, OW + pad), FILL, np.uint8)[:, :OW])
    return (y, np.full((OH // 2, OW // 2 + pad), FILL, np.uint8)[:, :OW // 2],
            np.full((OH // 2, OW // 2 + pad), FILL, np.uint8)[:, :OW // 2])


def want_out(OW, OH, regions, fmt):
    """The expected output planes: FILL, then each (x, y, planar stitch `want` of rw x rh) region put in."""
    y = np.full((OH, OW), FILL, np.uint8)
    u = np.full((OH // 2, OW // 2), FILL, np.uint8)
    v = np.full((OH // 2, OW // 2), FILL, np.uint8)
    for x0, y0, want in regions:
        rw, rh = want.shape[1], want.shape[0] * 2 // 3
        y[y0:y0 + rh, x0:x0 + rw] = want[:rh]
        u[y0 // 2:(y0 + rh) // 2, x0 // 2:(x0 + rw) // 2] = want[rh:, :rw // 2]
        v[y0 // 2:(y0 + rh) // 2, x0 // 2:(x0 + rw) // 2] = want[rh:, rw // 2:]
    # NV12: pair c of a chroma row at bytes 2c, 2c + 1 (unwritten pairs stay FILL, FILL)
    return (y, interleave(u, v)) if fmt == "nv12" else (y, u, v)


def padding_of(p):
    """The bytes between the plane's width and its pitch."""
    base = p.base if p.base is not None else p
    return base[:, p.shape[1]:]


def check(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        d = g != w
        assert not d.any(), (what, "plane %d" % k, int(d.sum()), np.argwhere(d)[:6].tolist())
        assert (padding_of(g) == FILL).all(), (what, "plane %d: bytes past the width were written" % k)


_GOLD = {}


def golden(name):
    if name not in _GOLD:
        rig, z = O.load_rig(name)
        W, H = (int(v) for v in z["out_size"])
        n = len(z["rois"])
        _GOLD[name] = dict(
            W=W, H=H, n=n, rois=z["rois"].tolist(),
            sizes=[(rig["inputs"][i]["options"]["width"], rig["inputs"][i]["options"]["height"]) for i in range(n)],
            maps1=[z[f"map1_{i}"] for i in range(n)], maps2=[z[f"map2_{i}"] for i in range(n)],
            masks=[z[f"mask_{i}"] for i in range(n)], seams=[z[f"seam_{i}"] for i in range(n)])
    return _GOLD[name]


def template(ox, t):
    return ox.MapperTemplate.from_arrays(t["W"], t["H"], t["rois"], t["maps1"], t["maps2"], t["masks"], t["seams"])


def oracle(t, frames, **kw):
    return O.stitch_frame(frames, t["sizes"], t["rois"], t["maps1"], t["maps2"], t["masks"], t["W"], t["H"], threads=8,
                          **kw)[0]


def smooth_frames(t, seed):
    from octvr_amd import synthetic
    return [synthetic.smooth_yuv_frame(w, h, seed + i) for i, (w, h) in enumerate(t["sizes"])]


def push(am, t, frames, out, in_fmt):
    am.push([in_planes(f, w, h, in_fmt) for f, (w, h) in zip(frames, t["sizes"])], out)


# ---- 1. all four format pairs --------------------------------------------------------------------------
_RIGA = {}


def riga_case():
    """Five frames of rigA and their oracle stitches, computed once for the four pairs."""
    if not _RIGA:
        t = golden("rigA")
        frames = [smooth_frames(t, 4300 + 10 * f) for f in range(5)]
        _RIGA["frames"] = frames
        _RIGA["want"] = [oracle(t, fr, enable_gain=True) for fr in frames]
    return _RIGA["frames"], _RIGA["want"]


@pytest.mark.parametrize("fmt", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_gpu_async_nv12_format_pairs(ox, fmt):
    t = golden("rigA")  # 2 x 256x144 -> 512x256: widths that are multiples of 8, the unpack kernel's 8-byte path
    frames, want = riga_case()
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([template(ox, t)], t["sizes"], (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])
    assert am.pixel_formats == PAIRS[0]
    am.set_pixel_formats(*fmt)
    assert am.pixel_formats == fmt
    assert am.info()["pixel_formats"] == [("yuv420p", "nv12").index(f) for f in fmt]
    outs = [new_out(W, H, fmt[1]) for _ in frames]
    for fr, out in zip(frames, outs):  # more frames than pipeline slots, all pushed before the first pop
        push(am, t, fr, out, fmt[0])
    assert am.pending() == len(frames)
    for f, out in enumerate(outs):
        assert am.pop() is out
        check(out, want_out(W, H, [(0, 0, want[f])], fmt[1]), (fmt, f))
    am.close()


# ---- 2. the unpack kernel's byte path ------------------------------------------------------------------
def test_gpu_async_nv12_byte_path(ox):
    """324-wide inputs (w % 8 == 4): every run takes the byte path, the last group of a row is partial, the
    composite has wide (gathered) tiles and the feed reads row ends.  The device frames hold a pattern
    outside the footprint, so a used byte that was not uploaded shows as a mismatch."""
    from octvr_amd import synthetic
    n, in_w, in_h, W, H = 5, 324, 240, 512, 256
    rig = synthetic.fisheye_rig(in_w, in_h, [2 * math.pi * k / n for k in range(n)], [0.35 * (-1) ** k for k in range(n)])
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
    t = dict(W=W, H=H, n=n, sizes=[(in_w, in_h)] * n, rois=[], maps1=[], maps2=[], masks=[], seams=None)
    for i in range(n):
        roi, m1, m2, mk, _ = mt.input(i)
        t["rois"].append(roi); t["maps1"].append(m1); t["maps2"].append(m2); t["masks"].append(mk)
    am = ox.AsyncMultiMapper([mt], t["sizes"], (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])
    am.set_pixel_formats("nv12", "nv12")
    frames = [smooth_frames(t, 4500 + 10 * f) for f in range(4)]
    outs = [new_out(W, H, "nv12") for _ in frames]
    for fr, out in zip(frames, outs):
        push(am, t, fr, out, "nv12")
    for f, out in enumerate(outs):
        am.pop()
        check(out, want_out(W, H, [(0, 0, oracle(t, frames[f], enable_gain=True))], "nv12"), f)
    am.close()


# ---- 3. regions and pitches ----------------------------------------------------------------------------
def test_gpu_async_nv12_side_by_side_regions(ox):
    """Two mappers (blend 0 and multi-band 16, the second on the first's gains) side by side at x = 0.5, output
    pitch = width + 64: each region's Y at its column, its chroma at byte 2 c.x, the padding untouched."""
    t = golden("rigB")
    W, H = t["W"], t["H"]
    OW, OH = 2 * W, H
    blends = [0, 16]
    am = ox.AsyncMultiMapper([template(ox, t) for _ in blends], t["sizes"], (OW, OH), blends, [0, 0],
                             [(0.0, 0.0, 0.5, 1.0), (0.5, 0.0, 0.5, 1.0)])
    am.set_pixel_formats("nv12", "nv12")
    frames = [smooth_frames(t, 4700 + 10 * f) for f in range(2)]
    outs = [new_out(OW, OH, "nv12", pad=64) for _ in frames]
    for fr, out in zip(frames, outs):
        assert out[0].strides[0] == OW + 64 and out[1].strides[0] == OW + 64
        push(am, t, fr, out, "nv12")
    for f, out in enumerate(outs):
        am.pop()
        w0, g = O.stitch_frame(frames[f], t["sizes"], t["rois"], t["maps1"], t["maps2"], t["masks"], W, H, threads=8,
                               enable_gain=True)
        w1 = oracle(t, frames[f], enable_gain=True, gains=g, blend=16, seams=t["seams"])
        check(out, want_out(OW, OH, [(0, 0, w0), (W, 0, w1)], "nv12"), f)
    am.close()


def test_gpu_async_nv12_stacked_scaled_regions(ox):
    """Stacked regions, each scaled from the template size to 1024x512 (feather -5 with gain, blend 0 without),
    padded pitches."""
    t = golden("rigB")
    W, H = t["W"], t["H"]
    OW, OH = 1024, 1024
    blends, gain_modes = [-5, 0], [0, -1]
    am = ox.AsyncMultiMapper([template(ox, t) for _ in blends], t["sizes"], (OW, OH), blends, gain_modes,
                             [(0.0, 0.0, 1.0, 0.5), (0.0, 0.5, 1.0, 0.5)])
    am.set_pixel_formats("nv12", "nv12")
    frames = [smooth_frames(t, 4900 + 10 * f) for f in range(2)]
    outs = [new_out(OW, OH, "nv12", pad=64) for _ in frames]
    for fr, out in zip(frames, outs):
        push(am, t, fr, out, "nv12")
    for f, out in enumerate(outs):
        am.pop()
        regs = []
        for k, (bl, gm) in enumerate(zip(blends, gain_modes)):
            regs.append((0, k * OH // 2, oracle(t, frames[f], enable_gain=gm >= 0, blend=bl, seams=t["seams"],
                                                scale=(OW, OH // 2))))
        check(out, want_out(OW, OH, regs, "nv12"), f)
    am.close()


# ---- 4. registered outputs -----------------------------------------------------------------------------
def test_gpu_async_nv12_registered_outputs(ox):
    """One contiguous (3H/2, W) NV12 frame registered as (a[:H], a[H:]) — its two plane ranges are adjacent and
    share a page — a second registered set, and an unregistered one: 7 frames over the three, all bit-exact."""
    t = golden("rigA")
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([template(ox, t)], t["sizes"], (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])
    am.set_pixel_formats("nv12", "nv12")
    a = np.full((H * 3 // 2, W), FILL, np.uint8)
    ring = [(a[:H], a[H:]), new_out(W, H, "nv12", pad=64), new_out(W, H, "nv12")]
    am.register_output(ring[0])
    am.register_output(ring[1])
    am.register_output(ring[0])  # again: a no-op
    with pytest.raises(ox.OctvrError):  # the sets' geometry depends on the output format
        am.set_pixel_formats("nv12", "yuv420p")
    am.set_pixel_formats("yuv420p", "nv12")  # the input format alone may change
    am.set_pixel_formats("nv12", "nv12")
    for f in range(7):
        fr = smooth_frames(t, 5100 + 10 * f)
        out = ring[f % 3]  # ring[2] is not registered: staging path
        for p in out:
            p[:] = FILL
        push(am, t, fr, out, "nv12")
        am.pop()
        want = want_out(W, H, [(0, 0, oracle(t, fr, enable_gain=True))], "nv12")
        for k in range(2):
            assert np.array_equal(out[k], want[k]), (f, k)
        if f % 3 == 1:
            assert (padding_of(out[0]) == FILL).all() and (padding_of(out[1]) == FILL).all()
    am.unregister_output(ring[0])
    am.unregister_output(ring[1])
    am.set_pixel_formats("nv12", "yuv420p")  # nothing registered any more
    am.close()


def test_gpu_async_planar_registers_column_halves(ox):
    """A planar pipeline whose U and V planes are the two column halves of one array (overlapping byte ranges):
    registered through one merged range, and bit-exact."""
    t = golden("rigA")
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([template(ox, t)], t["sizes"], (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])
    y = np.full((H, W), FILL, np.uint8)
    c = np.full((H // 2, W), FILL, np.uint8)
    out = (y, c[:, :W // 2], c[:, W // 2:])
    am.register_output(out)
    for f in range(2):
        fr = smooth_frames(t, 5300 + 10 * f)
        push(am, t, fr, out, "yuv420p")
        am.pop()
        want = oracle(t, fr, enable_gain=True)
        assert np.array_equal(y, want[:H]) and np.array_equal(c, want[H:]), f
    am.unregister_output(out)
    am.close()


@pytest.mark.parametrize("out_fmt", ["yuv420p", "nv12"])
def test_gpu_async_registered_odd_chroma_column(ox, out_fmt):
    """Output 268 x 128 in two halves: r.x = r.w = 134 and an odd chroma column c.x = c.w = 67, the mappers scaling
    rigA's 512 x 256 to 134 x 128.  The same frame through registered planes (pitch = width + 6: the region
    downloads write them) and through unregistered ones (staging and copy-out): byte-identical, and nothing but
    the regions' bytes is written.  (push_device with such regions: test_gpu_async_device_ragged_regions.)"""
    t = golden("rigA")
    OW, OH = 268, 128
    am = ox.AsyncMultiMapper([template(ox, t) for _ in range(2)], t["sizes"], (OW, OH), [0, 0], [0, 0],
                             [(0.0, 0.0, 0.5, 1.0), (0.5, 0.0, 0.5, 1.0)])
    am.set_pixel_formats("yuv420p", out_fmt)
    reg, plain = new_out(OW, OH, out_fmt, pad=6), new_out(OW, OH, out_fmt, pad=6)
    am.register_output(reg)
    fr = smooth_frames(t, 5500)
    for out in (reg, plain):
        push(am, t, fr, out, "yuv420p")
    assert am.pop() is reg and am.pop() is plain
    for k, (a, b) in enumerate(zip(reg, plain)):
        assert np.array_equal(a, b), (out_fmt, "plane %d" % k, np.argwhere(a != b)[:6].tolist())
        assert (padding_of(a) == FILL).all() and (padding_of(b) == FILL).all(), (out_fmt, k)
    assert (plain[0] != FILL).any() and (plain[1][:, 2 * 67 if out_fmt == "nv12" else 67:] != FILL).any()
    am.unregister_output(reg)
    am.close()


# ---- 5. preview ----------------------------------------------------------------------------------------
def test_gpu_async_nv12_preview(ox):
    """NV12 in and out with a preview and two regions: the preview stays RGB and equals the planar pipeline's
    expected preview; the outputs are bit-exact."""
    import test_gpu_async as A
    t = golden("rigB")
    W, H = t["W"], t["H"]
    blends, gain_modes, psize = [0, 0], [0, 0], (200, 100)
    regions = [(0.0, 0.0, 1.0, 0.5), (0.0, 0.5, 1.0, 0.5)]
    OW, OH = W, 2 * H  # two template-size regions
    am = ox.AsyncMultiMapper([template(ox, t) for _ in blends], t["sizes"], (OW, OH), blends, gain_modes, regions,
                             preview_size=psize)
    am.set_pixel_formats("nv12", "nv12")
    sunk = []
    am.set_preview_sink(lambda a, h: sunk.append(a))
    frames = [smooth_frames(t, 5500 + 10 * f) for f in range(2)]
    outs = [new_out(OW, OH, "nv12") for _ in frames]
    for fr, out in zip(frames, outs):
        push(am, t, fr, out, "nv12")
    for f, out in enumerate(outs):
        am.pop()
        (y, u, v), want_pv = A.preview_oracle(frames[f], t["sizes"], t["rois"], t["maps1"], t["maps2"], t["masks"], W, H,
                                              blends, gain_modes, regions, (OW, OH), psize, seams=t["seams"])
        check(out, (y, interleave(u, v)), f)
        assert np.array_equal(sunk[f], want_pv), (f, int((sunk[f] != want_pv).sum()))
    rgb, hdr = am.preview()
    assert (hdr.width, hdr.height) == psize and np.array_equal(rgb, sunk[-1])
    am.set_preview_sink(None)
    am.close()


# ---- 6. switching and errors ---------------------------------------------------------------------------
def test_gpu_async_nv12_switching_and_errors(ox):
    import ctypes as C
    t = golden("rigA")
    W, H = t["W"], t["H"]
    lib = ox.lib()
    am = ox.AsyncMultiMapper([template(ox, t)], t["sizes"], (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])
    for k, fmt in enumerate(["yuv420p", "nv12", "yuv420p"]):  # one pipeline, a frame in each layout
        am.set_pixel_formats(fmt, fmt)
        assert am.pixel_formats == (fmt, fmt)
        fr = smooth_frames(t, 5700 + 10 * k)
        out = new_out(W, H, fmt)
        push(am, t, fr, out, fmt)
        if k == 1:  # a frame is pending: refused, and that frame's output is not damaged
            assert lib.octvr_async_set_pixel_formats(am._h, ox.PIX_YUV420P, ox.PIX_YUV420P) == ox.E_INVALID
            assert am.pixel_formats == ("nv12", "nv12")
        am.pop()
        check(out, want_out(W, H, [(0, 0, oracle(t, fr, enable_gain=True))], fmt), (k, fmt))
    # bad values
    for bad in [(2, 0), (0, 2), (-1, 1), (1, 7)]:
        assert lib.octvr_async_set_pixel_formats(am._h, *bad) == ox.E_INVALID, bad
    assert am.pixel_formats == ("yuv420p", "yuv420p")
    # the output format cannot change while a set is registered
    reg = new_out(W, H, "yuv420p")
    am.register_output(reg)
    assert lib.octvr_async_set_pixel_formats(am._h, ox.PIX_NV12, ox.PIX_NV12) == ox.E_INVALID
    am.set_pixel_formats("nv12", "yuv420p")
    assert am.pixel_formats == ("nv12", "yuv420p")
    am.unregister_output(reg)
    # a NULL third plane: rejected for planar ...
    fr = smooth_frames(t, 5800)
    am.set_pixel_formats("yuv420p", "yuv420p")
    planar_in = [in_planes(f, w, h, "yuv420p") for f, (w, h) in zip(fr, t["sizes"])]
    nv12_in = [in_planes(f, w, h, "nv12") for f, (w, h) in zip(fr, t["sizes"])]
    with pytest.raises(ox.OctvrError):
        am.push([p[:2] for p in planar_in], new_out(W, H, "yuv420p"))
    with pytest.raises(ox.OctvrError):
        am.push(planar_in, new_out(W, H, "yuv420p")[:2])
    assert am.pending() == 0
    # ... and accepted for NV12, on both sides
    am.set_pixel_formats("nv12", "nv12")
    out = new_out(W, H, "nv12")
    am.push([(y, uv, None) for y, uv in nv12_in], (out[0], out[1], None))
    am.pop()
    check(out, want_out(W, H, [(0, 0, oracle(t, fr, enable_gain=True))], "nv12"), "NULL third planes")
    # a U,V pitch below W is rejected, input or output
    with pytest.raises(ox.OctvrError):
        am.push([(y, np.zeros((h // 2, w - 2), np.uint8)) for (y, uv), (w, h) in zip(nv12_in, t["sizes"])], out)
    with pytest.raises(ox.OctvrError):
        am.push(nv12_in, (out[0], np.zeros((H // 2, W // 2), np.uint8)))
    with pytest.raises(ox.OctvrError):
        am.register_output((out[0], np.zeros((H // 2, W // 2), np.uint8)))
    assert am.pending() == 0
    a, b = C.c_int(), C.c_int()
    assert lib.octvr_async_pixel_formats(am._h, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (1, 1)
    am.close()
