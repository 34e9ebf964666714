"""10-bit frames in and out of the Mapper (OCTVR_PIX_P010 / _YUV420P10 / _P210 / _YUV422P10): a stitch in any of them is
the planar 8-bit stitch of the frames converted by the in rule of include/octvr_hip.h, stored by the out rule —
  in:  v8 = min(255, (v10 + 2) >> 2) per sample, the 4:2:2 layouts then (c8[2r] + c8[2r + 1] + 1) >> 1;
  out: v10 = v8 << 2, the 4:2:2 layouts with chroma row r on rows 2r and 2r + 1 —
bit for bit.  The expected bytes always come from the oracle's stitch of frames converted by tests/yuv10_ref.py's numpy
(never the library's helpers, never an 8-bit 4:2:2 device path).  The pictures are made once as 10-bit 4:2:2 planes and
laid out per layout (the 4:2:0 ones through the picture with the same 8-bit frame), so one oracle stitch serves the
four layouts: each test converts its own laid-out frames with the rule and checks that they are the frames the
oracle stitched."""
import json
import math

import numpy as np
import pytest

import oracle_py as O
import yuv10_ref as R10
from yuv10_ref import LAYOUTS, VALUES, shape10, in_rule, out_rule

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def ox(product_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    assert hasattr(product_lib, "PIX_P010"), "OCTVR_PIX_P010 is missing"
    return product_lib


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _window(a, pad, offset):
    """a on the device as a window of a larger tensor: pitch = width + pad, base `offset` bytes into it."""
    import torch
    rows, cols = a.shape
    buf = torch.full(((rows + 1) * (cols + pad) + offset + 16,), FILL, dtype=torch.uint8, device="cuda")
    offset += (-buf.data_ptr()) % 16  # `offset` bytes past a 16-byte boundary
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


_RING = {}


def ring(ox, n, in_w, in_h=120, W=256, H=128):
    key = (n, in_w, in_h, W, H)
    if key not in _RING:
        from octvr_amd import synthetic
        rig = synthetic.fisheye_rig(in_w, in_h, [2 * math.pi * k / n for k in range(n)], [0.35 * (-1) ** k for k in range(n)])
        mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
        t = dict(W=W, H=H, n=n, sizes=[(in_w, in_h)] * n, rois=[], maps1=[], maps2=[], masks=[], seams=None)
        for i in range(n):
            roi, m1, m2, mk, _ = mt.input(i)
            t["rois"].append(roi); t["maps1"].append(m1); t["maps2"].append(m2); t["masks"].append(mk)
        _RING[key] = (mt, t)
    return _RING[key]


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


def out10(fmt, W, H):
    import torch
    return torch.zeros(shape10(fmt, W, H), dtype=torch.uint8, device="cuda")


_MEMO = {}


def memo(key, make):
    """A reference computed once and shared (never modified) by the tests and layouts that need it."""
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def picture_set(t, smooth_seed, noise_seed, edges=False):
    """A 10-bit 4:2:2 picture per camera of t (camera 0 with the edge rows) and their 8-bit frames by the in rule."""
    pics = [R10.noise_picture(f, w, h, noise_seed + i, edges=edges and i == 0)
            for i, (f, (w, h)) in enumerate(zip(smooth(t, smooth_seed), t["sizes"]))]
    return pics, [R10.frame8(p) for p in pics]


def noise_case():
    """rigA: noise pictures (camera 0 with the edge rows), the converted frames, the oracle."""
    def make():
        t = golden("rigA")
        pics, frames = picture_set(t, 510, 77, edges=True)
        want, g = oracle(t, frames, enable_gain=True, gains=None)
        return dict(t=t, pics=pics, frames=frames, want=want, gains=g)
    return memo("noise", make)


def laid(fmt, c, sizes=None):
    """The case's pictures in layout fmt with random ignored bits; their conversion by the rule is what the oracle
    stitched."""
    sizes = sizes or c["t"]["sizes"]
    frames = [R10.laid_out(fmt, p, 1000 + i) for i, p in enumerate(c["pics"])]
    for p, f, (w, h) in zip(frames, c["frames"], sizes):
        assert p.shape == shape10(fmt, w, h)
        same(in_rule(fmt, p, w, h), f, "the layouts carry one picture")
    return frames


# ---- input ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", LAYOUTS)
@pytest.mark.parametrize("name", ["rigA", "rigB"])
def test_gpu_yuv10_in_replicated_content_is_the_planar_stitch(ox, name, fmt):
    import torch
    t = golden(name)
    frames = memo(("smooth", name), lambda: smooth(t, 300))
    want, g_orc = memo(("smooth-oracle", name), lambda: oracle(t, frames, enable_gain=True, gains=None))
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats(fmt, "yuv420p")
    assert m.pixel_formats == (fmt, "yuv420p")
    out = planar_out(t["W"], t["H"])
    m.stitch([_cuda(out_rule(fmt, f, w, h)) for f, (w, h) in zip(frames, t["sizes"])], out)
    torch.cuda.synchronize()
    same_gains(m, g_orc)
    same(out.cpu().numpy(), want, name)


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_yuv10_in_noise_pictures_edge_values_and_ignored_bits(ox, fmt):
    import torch
    c = noise_case()
    t = c["t"]
    frames = laid(fmt, c)
    y, u, v = R10.planes10(fmt, frames[0], *t["sizes"][0])
    assert set(R10.EDGE) <= set(np.unique(y)) and set(R10.EDGE) <= set(np.unique(u)), "the edge values are in the frame"
    words = frames[0].view("<u2")
    assert ((words >> 10 if R10.planar(fmt) else words & 0x3F) != 0).any(), "the ignored bits are not all 0"
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats(fmt, "yuv420p")
    out = planar_out(t["W"], t["H"])
    m.stitch([_cuda(p) for p in frames], out)
    torch.cuda.synchronize()
    same_gains(m, c["gains"])
    same(out.cpu().numpy(), c["want"])


def _width_cases():
    cases = [(fmt, w) for fmt in LAYOUTS for w in (330, 328)]
    return cases + [(fmt, 332) for fmt in LAYOUTS if R10.planar(fmt)]  # the V half starts at byte 332: no multiple of 8


@pytest.mark.parametrize("fmt,in_w", _width_cases())
def test_gpu_yuv10_in_widths_pitch_and_base(ox, fmt, in_w):
    """Pitch + 6, the base 2 bytes into a larger tensor; a width with a short last group (every group on the
    per-sample path), one that is a multiple of 8 but not of 16 and, planar, one whose V half is not 8-byte aligned."""
    import torch
    mt, t = ring(ox, 3, in_w)

    def make():
        pics, frames = picture_set(t, 620, 900, edges=True)
        return dict(t=t, pics=pics, frames=frames, ref=oracle(t, frames, enable_gain=True, gains=None))
    c = memo(("width", in_w), make)
    want, g_orc = c["ref"]
    m = ox.Mapper(mt, t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats(fmt, "yuv420p")
    dev = [_window(p, 6, 2) for p in laid(fmt, c)]
    assert all(d.data_ptr() % 16 == 2 and d.stride(0) == 2 * in_w + 6 for d in dev)
    out = planar_out(t["W"], t["H"])
    m.stitch(dev, out)
    torch.cuda.synchronize()
    same_gains(m, g_orc)
    same(out.cpu().numpy(), want, (fmt, in_w))


def _more_sets():
    """Two more noise picture sets of rigA with their converted frames and oracle stitches."""
    def make():
        t = golden("rigA")
        sets = []
        for k in (1, 2):
            pics, frames = picture_set(t, 700 + 9 * k, 40 * k)
            sets.append(dict(t=t, pics=pics, frames=frames, want=oracle(t, frames, enable_gain=True, gains=None)[0]))
        return sets
    return memo("more", make)


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_yuv10_in_three_frames_in_flight(ox, fmt):
    import torch
    c = noise_case()
    t = c["t"]
    sets = [c] + _more_sets()
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats(fmt, "yuv420p")
    m.set_frames_in_flight(3)
    assert m.pixel_formats == (fmt, "yuv420p")
    streams = [torch.cuda.Stream() for _ in range(3)]
    dev = [[_cuda(p) for p in laid(fmt, s)] for s in sets]
    outs = [planar_out(t["W"], t["H"]) for _ in range(6)]
    torch.cuda.synchronize()
    for k in range(6):  # every slot twice
        m.stitch(dev[k % 3], outs[k], stream=streams[k % 3])
    torch.cuda.synchronize()
    for k in range(6):
        same(outs[k].cpu().numpy(), sets[k % 3]["want"], k)


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_yuv10_stitch_batch_of_two(ox, fmt):
    import torch
    c = noise_case()
    t = c["t"]
    second = _more_sets()[0]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_frames_in_flight(2)
    m.set_pixel_formats(fmt, fmt)
    W, H = t["W"], t["H"]
    outs = [out10(fmt, W, H) for _ in range(2)]
    m.stitch_batch([[_cuda(p) for p in laid(fmt, c)], [_cuda(p) for p in laid(fmt, second)]], outs)
    torch.cuda.synchronize()
    same(outs[0].cpu().numpy(), out_rule(fmt, c["want"], W, H), "frame 0")
    same(outs[1].cpu().numpy(), out_rule(fmt, second["want"], W, H), "frame 1")


@pytest.mark.parametrize("fmt", LAYOUTS)
@pytest.mark.parametrize("blend", [0, 5])
def test_gpu_yuv10_overlay_rig(ox, blend, fmt):
    """The overlay frame goes through the same conversion: blend 0 (the overlays are cameras of the composite)
    and multi-band (overlay_apply_kernel reads the slot's frames), against tests/overlay_ref.py."""
    import copy
    import torch
    import camera_rigs as R
    import overlay_ref as OR
    rig = copy.deepcopy(R.mask_rigs()["overlay_include"])
    W, H = 512, 256
    sizes = [(640, 360)] * len(rig["inputs"]) + [(192, 128)]

    def make():  # the template too: OR.prepare gives it the seam masks a multi-band mapper needs
        mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
        pics = [R10.noise_picture(O.rand_img(w, h * 3 // 2, 1, 40 + i), w, h, 5 + i) for i, (w, h) in enumerate(sizes)]
        frames = [R10.frame8(p) for p in pics]
        return dict(mt=mt, pics=pics, frames=frames,
                    want=OR.expected(OR.prepare(mt, blend), frames, sizes, blend=blend, enable_gain=True))
    c = memo(("overlay", blend), make)
    m = ox.Mapper(c["mt"], sizes, blend=blend, enable_gain=True)
    m.set_pixel_formats(fmt, "yuv420p")
    out = planar_out(W, H)
    m.stitch([_cuda(p) for p in laid(fmt, c, sizes)], out)
    torch.cuda.synchronize()
    same(out.cpu().numpy(), c["want"][0], blend)
    same_gains(m, c["want"][1])


@pytest.mark.parametrize("fmt", LAYOUTS)
@pytest.mark.parametrize("blend", [5, -4])
def test_gpu_yuv10_in_blended(ox, blend, fmt):
    import torch
    c = noise_case()
    t = c["t"]
    want, g_orc = memo(("blend", blend),
                       lambda: oracle(t, c["frames"], enable_gain=True, gains=None, blend=blend, seams=t["seams"]))
    m = ox.Mapper(template(ox, t), t["sizes"], blend=blend, enable_gain=True)
    m.set_pixel_formats(fmt, "yuv420p")
    out = planar_out(t["W"], t["H"])
    m.stitch([_cuda(p) for p in laid(fmt, c)], out)
    torch.cuda.synchronize()
    same_gains(m, g_orc)
    same(out.cpu().numpy(), want, blend)


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_yuv10_in_texture_mode(ox, fmt):
    import torch
    c = noise_case()
    t = c["t"]
    want, g_orc = memo("texture", lambda: oracle(t, c["frames"], enable_gain=True, gains=None, remap_tex=True))
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True, remap="texture")
    m.set_pixel_formats(fmt, "yuv420p")
    out = planar_out(t["W"], t["H"])
    m.stitch([_cuda(p) for p in laid(fmt, c)], out)
    torch.cuda.synchronize()
    same_gains(m, g_orc)
    same(out.cpu().numpy(), want, "texture")


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_yuv10_in_prepared_preview(ox, fmt):
    import torch
    c = noise_case()
    t = c["t"]
    pw, ph = 128, 64
    want, _, want_pv = memo("preview", lambda: oracle(t, c["frames"], enable_gain=True, gains=None, preview=(pw, ph)))
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats(fmt, "yuv420p")
    m.prepare_preview(pw, ph)
    out = planar_out(t["W"], t["H"])
    pv = torch.zeros((ph, pw, 3), dtype=torch.uint8, device="cuda")
    m.stitch([_cuda(p) for p in laid(fmt, c)], out, preview=pv)
    torch.cuda.synchronize()
    same(out.cpu().numpy(), want, "frame")
    same(pv.cpu().numpy(), want_pv, "preview")


# ---- output --------------------------------------------------------------------------------------------------
def check_out(fmt, got, want, W, H, what):
    """got: the frame in layout fmt as bytes; want: the planar 8-bit stitch."""
    same(got, out_rule(fmt, want, W, H), (what, "the numpy out rule of the oracle's stitch"))
    words = np.ascontiguousarray(got).view("<u2")
    assert not (words & (0xFC00 if R10.planar(fmt) else 0x003F)).any(), (what, "the ignored bits are written as 0")
    y, u, v = R10.planes10(fmt, got, W, H)
    same(y, want[:H, :W].astype(np.int32) << 2, (what, "Y"))
    for k in range(2 if R10.is422(fmt) else 1):  # every chroma row on both of its rows
        step = 2 if R10.is422(fmt) else 1
        same(u[k::step], want[H:, :W // 2].astype(np.int32) << 2, (what, "U", k))
        same(v[k::step], want[H:, W // 2:W].astype(np.int32) << 2, (what, "V", k))
    same(in_rule(fmt, got, W, H), want, (what, "round trip through the input rule"))


@pytest.mark.parametrize("fmt", LAYOUTS)
@pytest.mark.parametrize("in_fmt", ["yuv420p", "same"])
def test_gpu_yuv10_out_template_size_pitch_and_untouched_bytes(ox, in_fmt, fmt):
    """Pitch + 10 in a window 6 bytes past a 16-byte boundary; the bytes between a row's 2 W bytes and the pitch stay
    as they were."""
    import torch
    c = noise_case()
    t = c["t"]
    W, H = t["W"], t["H"]
    in_fmt = fmt if in_fmt == "same" else in_fmt
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats(in_fmt, fmt)
    assert m.pixel_formats == (in_fmt, fmt)
    dev = [_cuda(p) for p in (laid(fmt, c) if in_fmt == fmt else c["frames"])]
    rows, cols = shape10(fmt, W, H)
    out = _window(np.full((rows, cols), FILL, np.uint8), 10, 6)
    whole = out.as_strided((rows, cols + 10), (cols + 10, 1))[: rows - 1]  # rows with their padding (the last row has none)
    m.stitch(dev, out)
    torch.cuda.synchronize()
    check_out(fmt, out.cpu().numpy(), c["want"], W, H, (in_fmt, fmt))
    assert (whole.cpu().numpy()[:, cols:] == FILL).all(), "bytes between a row's width and the pitch were written"
    same_gains(m, c["gains"])


@pytest.mark.parametrize("in_fmt,out_fmt", [("p010", "uyvy422"), ("nv12", "yuv422p10"), ("yuv420p10", "p210")])
def test_gpu_yuv10_mixed_formats(ox, in_fmt, out_fmt):
    """The two sides are independent, across the 8-bit and the 10-bit layouts."""
    import torch
    c = noise_case()
    t = c["t"]
    W, H = t["W"], t["H"]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats(in_fmt, out_fmt)
    assert m.pixel_formats == (in_fmt, out_fmt)
    if in_fmt == "nv12":
        dev = []
        for f, (w, h) in zip(c["frames"], t["sizes"]):
            nv = f.copy()
            nv[h:, 0::2], nv[h:, 1::2] = f[h:, :w // 2], f[h:, w // 2:]
            dev.append(_cuda(nv))
    else:
        dev = [_cuda(p) for p in laid(in_fmt, c)]
    want = c["want"]
    if out_fmt == "uyvy422":  # the 8-bit out rule, written out: chroma row r on packed rows 2r and 2r + 1
        out = torch.zeros((H, 2 * W), dtype=torch.uint8, device="cuda")
        m.stitch(dev, out)
        torch.cuda.synchronize()
        exp = np.empty((H, 2 * W), np.uint8)
        exp[:, 1::2] = want[:H, :W]
        exp[:, 0::4] = np.repeat(want[H:, :W // 2], 2, axis=0)
        exp[:, 2::4] = np.repeat(want[H:, W // 2:W], 2, axis=0)
        same(out.cpu().numpy(), exp, (in_fmt, out_fmt))
    else:
        out = out10(out_fmt, W, H)
        m.stitch(dev, out)
        torch.cuda.synchronize()
        check_out(out_fmt, out.cpu().numpy(), want, W, H, (in_fmt, out_fmt))
    same_gains(m, c["gains"])


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_yuv10_out_scaled_with_preview(ox, fmt):
    import torch
    c = noise_case()
    t = c["t"]
    scale, (pw, ph) = (256, 128), (200, 100)
    want, _, want_pv = memo("scaled", lambda: oracle(t, c["frames"], enable_gain=True, gains=None, scale=scale,
                                                     preview=(pw, ph)))
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True, scale_output=scale)
    m.set_pixel_formats(fmt, fmt)
    out = out10(fmt, scale[0], scale[1])
    pv = torch.zeros((ph, pw, 3), dtype=torch.uint8, device="cuda")
    m.stitch([_cuda(p) for p in laid(fmt, c)], out, preview=pv)
    torch.cuda.synchronize()
    check_out(fmt, out.cpu().numpy(), want, scale[0], scale[1], "scaled")
    same(pv.cpu().numpy(), want_pv, "the preview stays RGB")


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_yuv10_out_odd_output_width(ox, fmt):
    """An output width whose half is odd (250: rows of 500 bytes, a planar V half at byte 250): row heads and tails of
    the pack kernel at a base 14 bytes past a 16-byte boundary."""
    import torch
    mt, t = ring(ox, 3, 328, W=250, H=126)
    frames = memo("odd-frames", lambda: smooth(t, 1500))
    want, _ = memo("odd", lambda: oracle(t, frames, enable_gain=True, gains=None))
    m = ox.Mapper(mt, t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats("yuv420p", fmt)
    rows, cols = shape10(fmt, 250, 126)
    out = _window(np.full((rows, cols), FILL, np.uint8), 2, 14)
    m.stitch([_cuda(f) for f in frames], out)
    torch.cuda.synchronize()
    check_out(fmt, out.cpu().numpy(), want, 250, 126, "250 wide")


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_yuv10_out_then_in_is_the_identity(ox, fmt):
    """Two mappers: the first writes the stitch of the 8-bit frames in the layout, and the in rule reads the planar
    stitch back from it; the second reads the same frames widened by the out rule as inputs of the layout and writes
    the first mapper's frame, with the same gains."""
    import torch
    c = noise_case()
    t = c["t"]
    W, H = t["W"], t["H"]
    first = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    first.set_pixel_formats("yuv420p", fmt)
    out = out10(fmt, W, H)
    first.stitch([_cuda(f) for f in c["frames"]], out)
    torch.cuda.synchronize()
    same(in_rule(fmt, out.cpu().numpy(), W, H), c["want"], "out, then the in rule")
    second = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    second.set_pixel_formats(fmt, fmt)
    out2 = out10(fmt, W, H)
    second.stitch([_cuda(out_rule(fmt, f, w, h)) for f, (w, h) in zip(c["frames"], t["sizes"])], out2)
    torch.cuda.synchronize()
    same(out2.cpu().numpy(), out.cpu().numpy(), "in of out-rule frames, then out: the first mapper's frame")
    same_gains(second, c["gains"])


# ---- API -----------------------------------------------------------------------------------------------------
def test_gpu_yuv10_api_names_values_and_helpers(ox):
    assert (ox.PIX_P010, ox.PIX_YUV420P10, ox.PIX_P210, ox.PIX_YUV422P10) == (32, 33, 34, 35)
    assert ox.frame_shape("p010", 64, 32) == (48, 128) and ox.frame_shape("yuv420p10", 64, 32) == (48, 128)
    assert ox.frame_shape("p210", 64, 32) == (64, 128) and ox.frame_shape("yuv422p10", 64, 32) == (64, 128)
    assert ox.frame_shape(33, 64, 32) == (48, 128)
    assert ox.frame_shape("nv16", 64, 32) == (64, 64) and ox.frame_shape("nv12", 64, 32) == (48, 64)
    f = O.rand_img(64, 48, 1, 3)
    rng = np.random.RandomState(4)
    for fmt in LAYOUTS:
        p = ox.yuv10_from_yuv420p(fmt, f, 64, 32)
        assert p.dtype == np.uint16
        same(p.view(np.uint8), out_rule(fmt, f, 64, 32), fmt)
        same(ox.yuv420p_from_yuv10(fmt, p, 64, 32), f, (fmt, "out-then-in is the identity"))
        crows = 32 if R10.is422(fmt) else 16
        noisy = R10.lay_out(fmt, rng.randint(0, 1024, (32, 64)), rng.randint(0, 1024, (crows, 32)),
                            rng.randint(0, 1024, (crows, 32)), seed=8)
        same(ox.yuv420p_from_yuv10(fmt, noisy, 64, 32), in_rule(fmt, noisy, 64, 32), fmt)
        same(ox.yuv420p_from_yuv10(fmt, noisy.view(np.uint16), 64, 32), in_rule(fmt, noisy, 64, 32), (fmt, "words"))
    # the rule's own example: 10-bit 3 and 6 narrow to 1 and 2 and average to 2 (averaging in 10 bits would give 1)
    y = np.zeros((2, 2), np.int32)
    got = in_rule("p210", R10.lay_out("p210", y, np.array([[3], [6]]), np.array([[1023], [1021]])), 2, 2)
    assert got[2].tolist() == [2, 255]


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_yuv10_api_values_alignment_pitches_and_info(ox, fmt):
    import ctypes as C
    import torch
    c = noise_case()
    t = c["t"]
    W, H = t["W"], t["H"]
    val = VALUES[fmt]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=False)
    lib = ox.lib()
    E_INVALID = -1
    m.set_pixel_formats(val, "nv12")  # by value
    for bad in (2, 7, -1, 20, 15):
        assert lib.octvr_mapper_set_pixel_formats(m._h, bad, val) == E_INVALID
        assert lib.octvr_mapper_set_pixel_formats(m._h, val, bad) == E_INVALID
    assert m.pixel_formats == (fmt, "nv12"), "a rejected call changes nothing"
    a, b = C.c_int(-7), C.c_int(-7)
    assert lib.octvr_mapper_pixel_formats(m._h, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (val, 1)
    info = m.info()
    assert info["yuv10_out_bytes"] == 0 and info["yuv10_runs"] > 0
    assert [info[k] for k in ("uyvy_runs", "uyvy_in_bytes", "uyvy_out_bytes", "yuv422_runs", "yuv422_in_bytes",
                              "yuv422_out_bytes")] == [0] * 6, "the 8-bit keys are 0 for a 10-bit side"
    # footprint_bytes is 1.5 B per pixel of the footprint (8 bits, 4:2:0); 10-bit 4:2:0 is 3 B per pixel, 4:2:2 is 4
    if R10.is422(fmt):
        assert info["yuv10_in_bytes"] * 3 == info["footprint_bytes"] * 8
    else:
        assert info["yuv10_in_bytes"] == info["footprint_bytes"] * 2
    m.set_pixel_formats("nv16", "nv16")  # the 8-bit keys keep their values for the other formats
    info = m.info()
    assert (info["yuv10_runs"], info["yuv10_in_bytes"], info["yuv10_out_bytes"]) == (0, 0, 0)
    assert info["yuv422_runs"] > 0 and info["yuv422_in_bytes"] * 3 == info["footprint_bytes"] * 4
    assert info["yuv422_out_bytes"] == 2 * W * H
    m.set_pixel_formats(fmt, fmt)
    rows, cols = shape10(fmt, W, H)
    assert m.info()["yuv10_out_bytes"] == rows * cols == (4 if R10.is422(fmt) else 3) * W * H
    dev = [_cuda(p) for p in laid(fmt, c)]

    def refused(ins, out):
        with pytest.raises(ox.OctvrError) as e:
            m.stitch(ins, out)
        assert e.value.code == E_INVALID
        torch.cuda.synchronize()

    # a pitch below 2 W, on either side
    narrow = torch.full((rows, cols - 2), FILL, dtype=torch.uint8, device="cuda")
    refused(dev, narrow)
    assert (narrow == FILL).all()
    out = torch.full((rows, cols), FILL, dtype=torch.uint8, device="cuda")
    refused([dev[0][:, :dev[0].shape[1] - 2].contiguous()] + dev[1:], out)
    # an odd base or an odd pitch, on either side: E_INVALID before any launch, the output untouched
    (w0, h0), p0 = t["sizes"][0], laid(fmt, c)[0]
    refused([_window(p0, 6, 3)] + dev[1:], out)
    refused([_window(p0, 5, 2)] + dev[1:], out)
    assert (out == FILL).all()
    for pad, off in ((6, 3), (5, 2)):
        odd = _window(np.full((rows, cols), FILL, np.uint8), pad, off)
        assert odd.data_ptr() % 2 == off % 2 and odd.stride(0) % 2 == pad % 2
        refused(dev, odd)
        assert (odd == FILL).all()
    m.set_pixel_formats("yuv420p", "yuv420p")  # unset: the frames are freed, the plain path is back
    assert m.info()["yuv10_in_bytes"] == 0 and m.pixel_formats == ("yuv420p", "yuv420p")
    out = planar_out(W, H)
    m.stitch([_cuda(f) for f in c["frames"]], out)
    torch.cuda.synchronize()
    same(out.cpu().numpy(), memo("plain", lambda: oracle(t, c["frames"], enable_gain=False)[0]), "back on planar")
