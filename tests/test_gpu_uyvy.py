"""Packed UYVY 4:2:2 frames in and out of the Mapper (OCTVR_PIX_UYVY422): a UYVY stitch is the planar stitch of
the frames converted by the two rules of include/octvr_hip.h —
  in:  chroma row r = (c[2r] + c[2r + 1] + 1) >> 1 per byte of the packed rows 2r and 2r + 1, luma copied;
  out: packed rows 2r and 2r + 1 both carry chroma row r, luma copied —
bit for bit.  The expected bytes always come from the oracle's stitch of frames converted by this file's own
numpy (never the library's helpers, never the code under test)."""
import json
import math

import numpy as np
import pytest

import oracle_py as O

pytestmark = pytest.mark.gpu

FILL = 0xA5


# ---- the two rules, in numpy -----------------------------------------------------------------------------
def pack_rule(f, w, h):
    """out rule: "Y over [U|V]" -> packed, every chroma row on two packed rows."""
    p = np.empty((h, 2 * w), np.uint8)
    p[:, 1::2] = f[:h, :w]
    p[:, 0::4] = np.repeat(f[h:, :w // 2], 2, axis=0)
    p[:, 2::4] = np.repeat(f[h:, w // 2:w], 2, axis=0)
    return p


def unpack_rule(p, w, h):
    """in rule: packed -> "Y over [U|V]", chroma rows averaged with rounding up."""
    f = np.empty((h * 3 // 2, w), np.uint8)
    f[:h] = p[:, 1:2 * w:2]
    u = p[:, 0:2 * w:4].astype(np.int32)
    v = p[:, 2:2 * w:4].astype(np.int32)
    f[h:, :w // 2] = (u[0::2] + u[1::2] + 1) >> 1
    f[h:, w // 2:] = (v[0::2] + v[1::2] + 1) >> 1
    return f


def noise_packed(f, w, h, seed):
    """The luma of f with independent noise chroma on every packed row."""
    p = pack_rule(f, w, h)
    rng = np.random.RandomState(seed)
    p[:, 0::2] = rng.randint(0, 256, (h, w), dtype=np.int64).astype(np.uint8)
    return p


@pytest.fixture(scope="module")
def ox(product_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    assert hasattr(product_lib, "PIX_UYVY422"), "OCTVR_PIX_UYVY422 is missing"
    return product_lib


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _window(a, pad, offset):
    """a on the device as a window of a larger tensor: pitch = width + pad, base `offset` bytes into it."""
    import torch
    rows, cols = a.shape
    buf = torch.full(((rows + 1) * (cols + pad) + offset,), FILL, dtype=torch.uint8, device="cuda")
    v = buf[offset:offset + rows * (cols + pad)].view(rows, cols + pad)[:, :cols]
    v.copy_(_cuda(a))
    return v


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
    return O.stitch_frame(frames, t["sizes"], t["rois"], t["maps1"], t["maps2"], t["masks"], t["W"], t["H"], threads=8, **kw)


def ring(ox, n, in_w, in_h=120, W=256, H=128):
    from octvr_amd import synthetic
    rig = synthetic.fisheye_rig(in_w, in_h, [2 * math.pi * k / n for k in range(n)], [0.35 * (-1) ** k for k in range(n)])
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
    t = dict(W=W, H=H, n=n, sizes=[(in_w, in_h)] * n, rois=[], maps1=[], maps2=[], masks=[], seams=None)
    for i in range(n):
        roi, m1, m2, mk, _ = mt.input(i)
        t["rois"].append(roi); t["maps1"].append(m1); t["maps2"].append(m2); t["masks"].append(mk)
    return mt, t


def smooth(t, seed):
    from octvr_amd import synthetic
    return [synthetic.smooth_yuv_frame(w, h, seed + i) for i, (w, h) in enumerate(t["sizes"])]


def same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    d = got != want
    assert got.shape == want.shape and not d.any(), (what, int(d.sum()), np.argwhere(d)[:6].tolist())


def same_gains(m, g_orc):
    same(np.asarray(m.gains(), np.float64).view(np.int64), np.asarray(g_orc, np.float64).view(np.int64), "gains")


def planar_out(W, H):
    import torch
    return torch.zeros((H * 3 // 2, W), dtype=torch.uint8, device="cuda")


_NOISE = {}


def noise_case():
    """rigA: packed frames with noise chroma (frame 0 with the carry rows), the converted frames, the oracle."""
    if not _NOISE:
        t = golden("rigA")
        packed = [noise_packed(f, w, h, 77 + i) for i, (f, (w, h)) in enumerate(zip(smooth(t, 510), t["sizes"]))]
        w, h = t["sizes"][0]
        for r in range(h // 4, h // 4 + 8):  # chroma pairs 255/254 and 0/1: the carries of the packed-byte average
            packed[0][2 * r, 0::4], packed[0][2 * r + 1, 0::4] = 255, 254
            packed[0][2 * r, 2::4], packed[0][2 * r + 1, 2::4] = 0, 1
            packed[0][2 * r + 16, 0::4], packed[0][2 * r + 17, 0::4] = 1, 0
            packed[0][2 * r + 16, 2::4], packed[0][2 * r + 17, 2::4] = 254, 255
        frames = [unpack_rule(p, w, h) for p, (w, h) in zip(packed, t["sizes"])]
        want, g = oracle(t, frames, enable_gain=True, gains=None)
        _NOISE.update(t=t, packed=packed, frames=frames, want=want, gains=g)
    return _NOISE


# ---- input ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rigA", "rigB"])
def test_gpu_uyvy_in_replicated_chroma_is_the_planar_stitch(ox, name):
    import torch
    t = golden(name)
    frames = smooth(t, 300)
    want, g_orc = oracle(t, frames, enable_gain=True, gains=None)
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats("uyvy422", "yuv420p")
    assert m.pixel_formats == ("uyvy422", "yuv420p")
    out = planar_out(t["W"], t["H"])
    m.stitch([_cuda(pack_rule(f, w, h)) for f, (w, h) in zip(frames, t["sizes"])], out)
    torch.cuda.synchronize()
    same_gains(m, g_orc)
    same(out.cpu().numpy(), want, name)


def test_gpu_uyvy_in_noise_chroma_averages_and_carries(ox):
    import torch
    c = noise_case()
    t = c["t"]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats("uyvy422", "yuv420p")
    out = planar_out(t["W"], t["H"])
    m.stitch([_cuda(p) for p in c["packed"]], out)
    torch.cuda.synchronize()
    same_gains(m, c["gains"])
    same(out.cpu().numpy(), c["want"])


@pytest.mark.parametrize("in_w", [330, 328], ids=["w=2mod8", "w=8mod16"])
def test_gpu_uyvy_in_widths_pitch_and_odd_base(ox, in_w):
    """Pitch 2 W + 6, the base an odd byte offset into a larger tensor; a width with a short last group (every
    group on the byte path) and one that is a multiple of 8 but not of 16."""
    import torch
    mt, t = ring(ox, 3, in_w)
    packed = [noise_packed(f, w, h, 900 + i) for i, (f, (w, h)) in enumerate(zip(smooth(t, 620), t["sizes"]))]
    frames = [unpack_rule(p, w, h) for p, (w, h) in zip(packed, t["sizes"])]
    want, g_orc = oracle(t, frames, enable_gain=True, gains=None)
    m = ox.Mapper(mt, t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats("uyvy422", "yuv420p")
    dev = [_window(p, 6, 3) for p in packed]
    assert all(d.data_ptr() % 2 == 1 and d.stride(0) == 2 * in_w + 6 for d in dev)
    out = planar_out(t["W"], t["H"])
    m.stitch(dev, out)
    torch.cuda.synchronize()
    same_gains(m, g_orc)
    same(out.cpu().numpy(), want, in_w)


def test_gpu_uyvy_in_three_frames_in_flight(ox):
    import torch
    c = noise_case()
    t = c["t"]
    sets = [c["packed"]] + [[noise_packed(f, w, h, 40 * k + i) for i, (f, (w, h)) in enumerate(zip(smooth(t, 700 + 9 * k), t["sizes"]))]
                            for k in (1, 2)]
    wants = [c["want"]] + [oracle(t, [unpack_rule(p, w, h) for p, (w, h) in zip(s, t["sizes"])], enable_gain=True, gains=None)[0]
                           for s in sets[1:]]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats("uyvy422", "yuv420p")
    m.set_frames_in_flight(3)
    assert m.pixel_formats == ("uyvy422", "yuv420p")
    streams = [torch.cuda.Stream() for _ in range(3)]
    dev = [[_cuda(p) for p in s] for s in sets]
    outs = [planar_out(t["W"], t["H"]) for _ in range(6)]
    torch.cuda.synchronize()
    for k in range(6):  # every slot twice
        m.stitch(dev[k % 3], outs[k], stream=streams[k % 3])
    torch.cuda.synchronize()
    for k in range(6):
        same(outs[k].cpu().numpy(), wants[k % 3], k)


def test_gpu_uyvy_stitch_batch_of_two(ox):
    import torch
    c = noise_case()
    t = c["t"]
    second = [noise_packed(f, w, h, 66 + i) for i, (f, (w, h)) in enumerate(zip(smooth(t, 810), t["sizes"]))]
    want2 = oracle(t, [unpack_rule(p, w, h) for p, (w, h) in zip(second, t["sizes"])], enable_gain=True, gains=None)[0]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_frames_in_flight(2)
    m.set_pixel_formats("uyvy422", "uyvy422")
    W, H = t["W"], t["H"]
    outs = [torch.zeros((H, 2 * W), dtype=torch.uint8, device="cuda") for _ in range(2)]
    m.stitch_batch([[_cuda(p) for p in c["packed"]], [_cuda(p) for p in second]], outs)
    torch.cuda.synchronize()
    same(outs[0].cpu().numpy(), pack_rule(c["want"], W, H), "frame 0")
    same(outs[1].cpu().numpy(), pack_rule(want2, W, H), "frame 1")


@pytest.mark.parametrize("blend", [0, 5])
def test_gpu_uyvy_overlay_rig(ox, blend):
    """The overlay frame goes through the same conversion: blend 0 (the overlays are cameras of the composite)
    and multi-band (overlay_apply_kernel reads the slot's frames), against tests/overlay_ref.py."""
    import copy
    import torch
    import camera_rigs as R
    import overlay_ref as OR
    rig = copy.deepcopy(R.mask_rigs()["overlay_include"])
    W, H = 512, 256
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
    t = OR.prepare(mt, blend)
    sizes = [(640, 360)] * len(rig["inputs"]) + [(192, 128)]
    packed = [noise_packed(O.rand_img(w, h * 3 // 2, 1, 40 + i), w, h, 5 + i) for i, (w, h) in enumerate(sizes)]
    frames = [unpack_rule(p, w, h) for p, (w, h) in zip(packed, sizes)]
    want = OR.expected(t, frames, sizes, blend=blend, enable_gain=True)
    m = ox.Mapper(mt, sizes, blend=blend, enable_gain=True)
    m.set_pixel_formats("uyvy422", "yuv420p")
    out = planar_out(W, H)
    m.stitch([_cuda(p) for p in packed], out)
    torch.cuda.synchronize()
    same(out.cpu().numpy(), want[0], blend)
    same_gains(m, want[1])


@pytest.mark.parametrize("blend", [5, -4])
def test_gpu_uyvy_in_blended(ox, blend):
    import torch
    c = noise_case()
    t = c["t"]
    want, g_orc = oracle(t, c["frames"], enable_gain=True, gains=None, blend=blend, seams=t["seams"])
    m = ox.Mapper(template(ox, t), t["sizes"], blend=blend, enable_gain=True)
    m.set_pixel_formats("uyvy422", "yuv420p")
    out = planar_out(t["W"], t["H"])
    m.stitch([_cuda(p) for p in c["packed"]], out)
    torch.cuda.synchronize()
    same_gains(m, g_orc)
    same(out.cpu().numpy(), want, blend)


def test_gpu_uyvy_in_texture_mode(ox):
    import torch
    c = noise_case()
    t = c["t"]
    want, g_orc = oracle(t, c["frames"], enable_gain=True, gains=None, remap_tex=True)
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True, remap="texture")
    m.set_pixel_formats("uyvy422", "yuv420p")
    out = planar_out(t["W"], t["H"])
    m.stitch([_cuda(p) for p in c["packed"]], out)
    torch.cuda.synchronize()
    same_gains(m, g_orc)
    same(out.cpu().numpy(), want, "texture")


def test_gpu_uyvy_in_prepared_preview(ox):
    import torch
    c = noise_case()
    t = c["t"]
    pw, ph = 128, 64
    want, _, want_pv = oracle(t, c["frames"], enable_gain=True, gains=None, preview=(pw, ph))
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats("uyvy422", "yuv420p")
    m.prepare_preview(pw, ph)
    out = planar_out(t["W"], t["H"])
    pv = torch.zeros((ph, pw, 3), dtype=torch.uint8, device="cuda")
    m.stitch([_cuda(p) for p in c["packed"]], out, preview=pv)
    torch.cuda.synchronize()
    same(out.cpu().numpy(), want, "frame")
    same(pv.cpu().numpy(), want_pv, "preview")


# ---- output --------------------------------------------------------------------------------------------------
def check_packed_out(got, want, W, H, what):
    """got: H x 2W packed bytes; want: the planar stitch."""
    same(got[:, 1::2], want[:H, :W], (what, "Y"))
    for k in (0, 1):  # every chroma row on both of its packed rows
        same(got[k::2, 0::4], want[H:, :W // 2], (what, "U on packed rows 2r + %d" % k))
        same(got[k::2, 2::4], want[H:, W // 2:W], (what, "V on packed rows 2r + %d" % k))
    same(unpack_rule(got, W, H), want, (what, "round trip through the input rule"))


@pytest.mark.parametrize("in_fmt", ["yuv420p", "nv12", "uyvy422"])
def test_gpu_uyvy_out_template_size_pitch_and_untouched_bytes(ox, in_fmt):
    """Pitch 2 W + 10 in a window at an odd byte offset; the bytes between 2 W and the pitch stay as they were."""
    import torch
    c = noise_case()
    t = c["t"]
    W, H = t["W"], t["H"]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats(in_fmt, "uyvy422")
    assert m.pixel_formats == (in_fmt, "uyvy422")
    if in_fmt == "uyvy422":
        dev = [_cuda(p) for p in c["packed"]]
    elif in_fmt == "nv12":
        dev = []
        for f, (w, h) in zip(c["frames"], t["sizes"]):
            nv = f.copy()
            nv[h:, 0::2], nv[h:, 1::2] = f[h:, :w // 2], f[h:, w // 2:]
            dev.append(_cuda(nv))
    else:
        dev = [_cuda(f) for f in c["frames"]]
    out = _window(np.full((H, 2 * W), FILL, np.uint8), 10, 5)
    whole = out.as_strided((H, 2 * W + 10), (2 * W + 10, 1))[: H - 1]  # rows with their padding (the last row has none)
    m.stitch(dev, out)
    torch.cuda.synchronize()
    check_packed_out(out.cpu().numpy(), c["want"], W, H, in_fmt)
    assert (whole.cpu().numpy()[:, 2 * W:] == FILL).all(), "bytes between 2 W and the pitch were written"
    same_gains(m, c["gains"])


def test_gpu_uyvy_out_scaled_with_preview(ox):
    import torch
    c = noise_case()
    t = c["t"]
    scale, (pw, ph) = (256, 128), (200, 100)
    want, _, want_pv = oracle(t, c["frames"], enable_gain=True, gains=None, scale=scale, preview=(pw, ph))
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True, scale_output=scale)
    m.set_pixel_formats("uyvy422", "uyvy422")
    out = torch.zeros((scale[1], 2 * scale[0]), dtype=torch.uint8, device="cuda")
    pv = torch.zeros((ph, pw, 3), dtype=torch.uint8, device="cuda")
    m.stitch([_cuda(p) for p in c["packed"]], out, preview=pv)
    torch.cuda.synchronize()
    check_packed_out(out.cpu().numpy(), want, scale[0], scale[1], "scaled")
    same(pv.cpu().numpy(), want_pv, "the preview stays RGB")


def test_gpu_uyvy_out_odd_output_width(ox):
    """An output width that is no multiple of 8 (2 W = 4 mod 16): row heads and tails of the pack kernel."""
    import torch
    mt, t = ring(ox, 3, 328, W=250, H=126)
    frames = smooth(t, 1500)
    want, _ = oracle(t, frames, enable_gain=True, gains=None)
    m = ox.Mapper(mt, t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats("yuv420p", "uyvy422")
    out = _window(np.full((126, 500), FILL, np.uint8), 2, 7)
    m.stitch([_cuda(f) for f in frames], out)
    torch.cuda.synchronize()
    check_packed_out(out.cpu().numpy(), want, 250, 126, "250 wide")


# ---- API -----------------------------------------------------------------------------------------------------
def test_gpu_uyvy_api_values_pitches_and_info(ox):
    import ctypes as C
    import torch
    c = noise_case()
    t = c["t"]
    W, H = t["W"], t["H"]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=False)
    lib = ox.lib()
    E_INVALID = -1
    assert ox.PIX_UYVY422 == 16
    m.set_pixel_formats("uyvy422", "nv12")
    for bad in (2, 7, -1):
        assert lib.octvr_mapper_set_pixel_formats(m._h, bad, 16) == E_INVALID
        assert lib.octvr_mapper_set_pixel_formats(m._h, 16, bad) == E_INVALID
    assert m.pixel_formats == ("uyvy422", "nv12"), "a rejected call changes nothing"
    a, b = C.c_int(-7), C.c_int(-7)
    assert lib.octvr_mapper_pixel_formats(m._h, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (16, 1)
    info = m.info()
    assert info["uyvy_out_bytes"] == 0 and info["uyvy_runs"] > 0
    # uyvy_in_bytes: 2 B x 8 pixels x 2 rows per set group of the footprint, clipped at the width — the sizes the
    # pipeline's own run packing reports for the mapper's runs
    runs = ox.debug_mapper_uyvy_runs(m)
    assert len(runs) == info["uyvy_runs"]
    _, sizes = ox.debug_pack_runs(t["sizes"], runs, [(p,) for p in c["packed"]], "uyvy422")
    px = sum(min(8 * (int(g0) + int(ng)), t["sizes"][int(cam)][0]) - 8 * int(g0) for cam, _, g0, ng in runs)
    assert int(sizes.sum()) == 2 * 2 * px == info["uyvy_in_bytes"]
    assert info["uyvy_in_bytes"] * 3 == info["footprint_bytes"] * 4, "the runs are exactly the footprint's set groups"
    # pitches below 2 W: E_INVALID, before any launch (the output keeps its bytes)
    m.set_pixel_formats("uyvy422", "uyvy422")
    assert m.info()["uyvy_out_bytes"] == 2 * W * H
    out = torch.full((H, 2 * W), FILL, dtype=torch.uint8, device="cuda")
    dev = [_cuda(p) for p in c["packed"]]
    narrow = torch.full((H, 2 * W - 2), FILL, dtype=torch.uint8, device="cuda")
    with pytest.raises(ox.OctvrError) as e:
        m.stitch(dev, narrow)
    assert e.value.code == E_INVALID
    assert (narrow == FILL).all()
    w0 = t["sizes"][0][0]
    with pytest.raises(ox.OctvrError) as e:
        m.stitch([dev[0][:, :2 * w0 - 2].contiguous()] + dev[1:], out)
    assert e.value.code == E_INVALID
    torch.cuda.synchronize()
    assert (out == FILL).all()
    m.set_pixel_formats("yuv420p", "yuv420p")  # unset: the frames are freed, the plain path is back
    assert m.info()["uyvy_in_bytes"] == 0 and m.pixel_formats == ("yuv420p", "yuv420p")
    out = planar_out(W, H)
    m.stitch([_cuda(f) for f in c["frames"]], out)
    torch.cuda.synchronize()
    same(out.cpu().numpy(), oracle(t, c["frames"], enable_gain=False)[0], "back on planar")
