"""NV12 frames in and out of the Mapper path (octvr_mapper_set_pixel_formats): the kernels read NV12 sources
and write NV12 output themselves, and the result is always the planar ("Y over [U|V]") stitch of the same
pixels, bit for bit, with the chroma bytes rearranged.  The expected bytes come from the oracle's stitch of
the planar frames; the layout permutation is this file's own numpy (never the library's helpers)."""
import json
import math

import numpy as np
import pytest

import oracle_py as O

pytestmark = pytest.mark.gpu

PAIRS = [("yuv420p", "yuv420p"), ("nv12", "yuv420p"), ("yuv420p", "nv12"), ("nv12", "nv12")]


def to_nv12(f, w, h):
    """"Y over [U|V]" (h rows of Y, then h/2 rows of U in bytes [0, w/2) and V in [w/2, w)) -> NV12."""
    m = np.empty((h * 3 // 2, w), np.uint8)
    m[:h] = f[:h, :w]
    m[h:, 0::2] = f[h:, :w // 2]
    m[h:, 1::2] = f[h:, w // 2:w]
    return m


def as_fmt(f, w, h, fmt):
    return to_nv12(f, w, h) if fmt == "nv12" else np.ascontiguousarray(f[:, :w])


@pytest.fixture(scope="module")
def ox(product_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    assert hasattr(product_lib.Mapper, "set_pixel_formats"), "octvr_mapper_set_pixel_formats is missing"
    return product_lib


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _out(W, H, pitch=None):
    import torch
    return torch.zeros((H * 3 // 2, pitch or W), dtype=torch.uint8, device="cuda")


_GOLD = {}


def golden(name):
    if name not in _GOLD:
        rig, z = O.load_rig(name)
        W, H = (int(v) for v in z["out_size"])
        n = len(z["rois"])
        t = dict(W=W, H=H, n=n, rois=z["rois"].tolist(),
                 sizes=[(rig["inputs"][i]["options"]["width"], rig["inputs"][i]["options"]["height"]) for i in range(n)],
                 maps1=[z[f"map1_{i}"] for i in range(n)], maps2=[z[f"map2_{i}"] for i in range(n)],
                 masks=[z[f"mask_{i}"] for i in range(n)], seams=[z[f"seam_{i}"] for i in range(n)])
        _GOLD[name] = t
    return _GOLD[name]


def template(ox, t):
    return ox.MapperTemplate.from_arrays(t["W"], t["H"], t["rois"], t["maps1"], t["maps2"], t["masks"], t["seams"])


def oracle(t, frames, **kw):
    return O.stitch_frame(frames, t["sizes"], t["rois"], t["maps1"], t["maps2"], t["masks"], t["W"], t["H"], threads=8, **kw)


def ring(ox, n, in_w=320, in_h=240, W=512, H=256):
    from octvr_amd import synthetic
    rig = synthetic.fisheye_rig(in_w, in_h, [2 * math.pi * k / n for k in range(n)], [0.35 * (-1) ** k for k in range(n)])
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
    t = dict(W=W, H=H, n=n, sizes=[(in_w, in_h)] * n, rois=[], maps1=[], maps2=[], masks=[], seams=None)
    for i in range(n):
        roi, m1, m2, mk, _ = mt.input(i)
        t["rois"].append(roi); t["maps1"].append(m1); t["maps2"].append(m2); t["masks"].append(mk)
    return mt, t


def check(got, want, t, out_fmt, what=""):
    want = as_fmt(want, want.shape[1], want.shape[0] * 2 // 3, out_fmt)
    d = got != want
    assert not d.any(), (what, out_fmt, int(d.sum()), np.argwhere(d)[:6].tolist())


def dev_frames(frames, sizes, fmt):
    return [_cuda(as_fmt(f, w, h, fmt)) for f, (w, h) in zip(frames, sizes)]


# ---- 1. fixed gains, independent random bytes ----------------------------------------------------------
_FIXED = {}


def fixed_case(name):
    if name not in _FIXED:
        t = golden(name)
        frames = [O.rand_img(w, h * 3 // 2, 1, 4100 + 17 * i) for i, (w, h) in enumerate(t["sizes"])]
        gains = [0.85 + 0.07 * ((3 * i) % 5) for i in range(t["n"])]
        want, _ = oracle(t, frames, enable_gain=True, gains=gains)
        _FIXED[name] = (frames, gains, want)
    return _FIXED[name]


@pytest.mark.parametrize("fmt", PAIRS, ids=["%s-%s" % p for p in PAIRS])
@pytest.mark.parametrize("name", ["rigA", "rigB", "rigC", "rigD"])
def test_gpu_nv12_fixed_gains(ox, name, fmt):
    import torch
    t = golden(name)
    frames, gains, want = fixed_case(name)
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    before = None
    if fmt == PAIRS[0]:  # the default, before set_pixel_formats was ever called
        before = _out(t["W"], t["H"])
        m.stitch(dev_frames(frames, t["sizes"], "yuv420p"), before, gains=gains)
    m.set_pixel_formats(*fmt)
    assert m.pixel_formats == fmt
    out = _out(t["W"], t["H"])
    m.stitch(dev_frames(frames, t["sizes"], fmt[0]), out, gains=gains)
    torch.cuda.synchronize()
    check(out.cpu().numpy(), want, t, fmt[1], name)
    if before is not None:
        assert torch.equal(before, out)


# ---- 2. estimated gains --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rigA", "rigB", "rigC", "rigD"])
def test_gpu_nv12_estimated_gains(ox, name):
    import torch
    from octvr_amd import synthetic
    t = golden(name)
    frames = [synthetic.smooth_yuv_frame(w, h, 730 + i) for i, (w, h) in enumerate(t["sizes"])]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats("nv12", "nv12")
    out = _out(t["W"], t["H"])
    m.stitch(dev_frames(frames, t["sizes"], "nv12"), out)
    torch.cuda.synchronize()
    want, g_orc = oracle(t, frames, enable_gain=True, gains=None)
    np.testing.assert_array_equal(np.array(m.gains()), np.array(g_orc))
    check(out.cpu().numpy(), want, t, "nv12", name)


# ---- 3. ring rigs: the workgroup LU (n = 9) and the lean feed (frames in flight) -------------------------
@pytest.mark.parametrize("n,inflight", [(9, 1), (4, 2)])
def test_gpu_nv12_ring_rig(ox, n, inflight):
    import torch
    from octvr_amd import synthetic
    mt, t = ring(ox, n)
    m = ox.Mapper(mt, t["sizes"], blend=0, enable_gain=True)
    m.set_frames_in_flight(inflight)
    m.set_pixel_formats("nv12", "nv12")
    for k in range(inflight):  # frames in a row, one per slot
        frames = [synthetic.smooth_yuv_frame(w, h, 1200 + 31 * k + i) for i, (w, h) in enumerate(t["sizes"])]
        out = _out(t["W"], t["H"])
        m.stitch(dev_frames(frames, t["sizes"], "nv12"), out)
        torch.cuda.synchronize()
        want, g_orc = oracle(t, frames, enable_gain=True, gains=None)
        np.testing.assert_array_equal(np.array(m.gains()), np.array(g_orc))
        check(out.cpu().numpy(), want, t, "nv12", (n, k))


# ---- 4. unaligned frames -------------------------------------------------------------------------------
def _unaligned_inputs(frames, sizes, fmt):
    """Each frame inside a (rows, w + 2) byte tensor from flat offset 2: base pointer + 2, pitch w + 2."""
    import torch
    dev = []
    for f, (w, h) in zip(frames, sizes):
        rows = h * 3 // 2
        buf = torch.full(((rows + 1) * (w + 2),), 0xA5, dtype=torch.uint8, device="cuda")
        v = buf[2:2 + rows * (w + 2)].view(rows, w + 2)[:, :w]
        v.copy_(_cuda(as_fmt(f, w, h, fmt)))
        assert v.data_ptr() % 8 == 2 and v.stride(0) == w + 2
        dev.append(v)
    return dev


@pytest.mark.parametrize("out_fmt", ["nv12", "yuv420p"])
@pytest.mark.parametrize("case", ["rigB", "ring324"])
def test_gpu_nv12_unaligned(ox, case, out_fmt):
    import torch
    from octvr_amd import synthetic
    if case == "rigB":
        t = golden("rigB")
        mt = template(ox, t)
    else:
        mt, t = ring(ox, 5, in_w=324, in_h=240)  # w % 8 == 4: gathered (wide) tiles, and the feed's row ends
    frames = [synthetic.smooth_yuv_frame(w, h, 2100 + i) for i, (w, h) in enumerate(t["sizes"])]
    m = ox.Mapper(mt, t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats("nv12", out_fmt)
    W, H = t["W"], t["H"]
    out = torch.full((H * 3 // 2, W + 6), 0x5A, dtype=torch.uint8, device="cuda")
    m.stitch(_unaligned_inputs(frames, t["sizes"], "nv12"), out[:, :W])
    torch.cuda.synchronize()
    want, g_orc = oracle(t, frames, enable_gain=True, gains=None)
    np.testing.assert_array_equal(np.array(m.gains()), np.array(g_orc))
    got = out.cpu().numpy()
    assert (got[:, W:] == 0x5A).all(), "bytes between W and the pitch were written"
    check(got[:, :W], want, t, out_fmt, case)


# ---- 5. batches ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [2, 4])
def test_gpu_nv12_batch(ox, nb):
    import torch
    from octvr_amd import synthetic
    t = golden("rigA")
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_frames_in_flight(4)
    m.set_pixel_formats("nv12", "nv12")
    frames = [[synthetic.smooth_yuv_frame(w, h, 3000 + 40 * nb + 7 * f + i) for i, (w, h) in enumerate(t["sizes"])]
              for f in range(nb)]
    outs = [_out(t["W"], t["H"]) for _ in range(nb)]
    m.stitch_batch([dev_frames(fr, t["sizes"], "nv12") for fr in frames], outs)
    torch.cuda.synchronize()
    for f in range(nb):
        want, _ = oracle(t, frames[f], enable_gain=True, gains=None)
        check(outs[f].cpu().numpy(), want, t, "nv12", (nb, f))


# ---- 6. other mapper kinds -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,blend", [("rigB", 16), ("rigC", -5)])
def test_gpu_nv12_blend(ox, name, blend):
    import torch
    from octvr_amd import synthetic
    t = golden(name)
    frames = [synthetic.smooth_yuv_frame(w, h, 3400 + i) for i, (w, h) in enumerate(t["sizes"])]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=blend, enable_gain=True)
    m.set_pixel_formats("nv12", "nv12")
    out = _out(t["W"], t["H"])
    m.stitch(dev_frames(frames, t["sizes"], "nv12"), out)
    torch.cuda.synchronize()
    want, g_orc = oracle(t, frames, enable_gain=True, gains=None, blend=blend, seams=t["seams"])
    np.testing.assert_array_equal(np.array(m.gains()), np.array(g_orc))
    check(out.cpu().numpy(), want, t, "nv12", (name, blend))


def test_gpu_nv12_scaled_and_preview(ox):
    import torch
    from octvr_amd import synthetic
    t = golden("rigA")
    scale, (pw, ph) = (256, 128), (200, 100)
    frames = [synthetic.smooth_yuv_frame(w, h, 3500 + i) for i, (w, h) in enumerate(t["sizes"])]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True, scale_output=scale)
    m.set_pixel_formats("nv12", "nv12")
    out = _out(*scale)
    pv = torch.zeros((ph, pw, 3), dtype=torch.uint8, device="cuda")
    m.stitch(dev_frames(frames, t["sizes"], "nv12"), out, preview=pv)
    torch.cuda.synchronize()
    want, _, want_pv = oracle(t, frames, enable_gain=True, gains=None, scale=scale, preview=(pw, ph))
    assert np.array_equal(pv.cpu().numpy(), want_pv), "the preview stays RGB"
    check(out.cpu().numpy(), want, t, "nv12", "scaled")


def test_gpu_nv12_texture_mode(ox):
    import torch
    from octvr_amd import synthetic
    t = golden("rigA")
    frames = [synthetic.smooth_yuv_frame(w, h, 3600 + i) for i, (w, h) in enumerate(t["sizes"])]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True, remap="texture")
    m.set_pixel_formats("nv12", "nv12")
    out = _out(t["W"], t["H"])
    m.stitch(dev_frames(frames, t["sizes"], "nv12"), out)
    torch.cuda.synchronize()
    want, g_orc = oracle(t, frames, enable_gain=True, gains=None, remap_tex=True)
    np.testing.assert_array_equal(np.array(m.gains()), np.array(g_orc))
    check(out.cpu().numpy(), want, t, "nv12", "texture")


def test_gpu_nv12_vignette(ox):
    import torch
    from octvr_amd import synthetic
    rig, _ = O.load_rig("rigB")
    rig = json.loads(json.dumps(rig))
    for k, c in enumerate(rig["inputs"]):  # the rig of tests/test_gpu_vignette.py
        o = c["options"]
        if k % 3 == 2:
            continue
        o["vignette"] = [1.0 + 0.05 * k, -0.35, 0.12 - 0.01 * k, -0.04]
        if k % 2:
            o["exposure"] = 0.25 * k - 0.5
    W, H = 768, 384
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
    n = len(mt)
    sizes = [(c["options"]["width"], c["options"]["height"]) for c in rig["inputs"]]
    vig = []
    for i, c in enumerate(rig["inputs"]):
        v = O.vignette_map(c["options"])
        vig.append(None if v is None else O.resize_linear_cuda_f32(v, sizes[i][0], sizes[i][1]))
    t = dict(W=W, H=H, n=n, sizes=sizes, rois=[], maps1=[], maps2=[], masks=[])
    for i in range(n):
        roi, m1, m2, mk, _ = mt.input(i)
        t["rois"].append(roi); t["maps1"].append(m1); t["maps2"].append(m2); t["masks"].append(mk)
    frames = [synthetic.smooth_yuv_frame(w, h, 3700 + i) for i, (w, h) in enumerate(sizes)]
    m = ox.Mapper(mt, sizes, blend=0, enable_gain=True)
    m.set_pixel_formats("nv12", "nv12")
    out = _out(W, H)
    m.stitch(dev_frames(frames, sizes, "nv12"), out)
    torch.cuda.synchronize()
    want, g_orc = oracle(t, frames, enable_gain=True, gains=None, vig=vig)
    np.testing.assert_array_equal(np.array(m.gains()), np.array(g_orc))
    check(out.cpu().numpy(), want, t, "nv12", "vignette")


# ---- 7. switching formats on one mapper ------------------------------------------------------------------
def test_gpu_nv12_format_switching(ox):
    import torch
    t = golden("rigA")
    frames, gains, want = fixed_case("rigA")
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    for fmt in ("yuv420p", "nv12", "yuv420p"):
        m.set_pixel_formats(fmt, fmt)
        out = _out(t["W"], t["H"])
        m.stitch(dev_frames(frames, t["sizes"], fmt), out, gains=gains)
        torch.cuda.synchronize()
        check(out.cpu().numpy(), want, t, fmt, fmt)


# ---- 8. errors -------------------------------------------------------------------------------------------
def test_gpu_nv12_errors_and_getter(ox):
    import ctypes as C
    t = golden("rigA")
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=False)
    assert m.pixel_formats == ("yuv420p", "yuv420p")
    lib = ox.lib()
    E_INVALID = -1
    for bad in (2, -1):
        assert lib.octvr_mapper_set_pixel_formats(m._h, bad, 0) == E_INVALID
        assert lib.octvr_mapper_set_pixel_formats(m._h, 0, bad) == E_INVALID
        with pytest.raises(ox.OctvrError):
            m.set_pixel_formats(bad, "nv12")
    assert m.pixel_formats == ("yuv420p", "yuv420p"), "a rejected call changes nothing"
    for fmt in PAIRS:
        m.set_pixel_formats(*fmt)
        assert m.pixel_formats == fmt
        a, b = C.c_int(-7), C.c_int(-7)
        assert lib.octvr_mapper_pixel_formats(m._h, C.byref(a), C.byref(b)) == 0
        assert (a.value, b.value) == (int(fmt[0] == "nv12"), int(fmt[1] == "nv12"))
    assert ox.abi_version() == 1
