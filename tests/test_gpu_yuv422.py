"""YUYV, planar YUV422P and NV16 frames in and out of the Mapper (OCTVR_PIX_YUYV422 / _YUV422P / _NV16): a stitch in
any of them is the planar stitch of the frames converted by the two rules of include/octvr_hip.h —
  in:  chroma row r = (c[2r] + c[2r + 1] + 1) >> 1 per byte of chroma rows 2r and 2r + 1, luma copied;
  out: chroma rows 2r and 2r + 1 both carry chroma row r, luma copied —
bit for bit.  The expected bytes always come from the oracle's stitch of frames converted by this file's own numpy
(never the library's helpers, never the library's UYVY path).  The 4:2:2 pictures are made as (Y, U, V) planes and
laid out per layout, so one oracle stitch serves the three layouts: each test converts its own laid-out frames
with the rule and checks that they are the frames the oracle stitched."""
import json
import math

import numpy as np
import pytest

import oracle_py as O

pytestmark = pytest.mark.gpu

FILL = 0xA5
LAYOUTS = ["yuyv422", "yuv422p", "nv16"]
VALUES = {"yuyv422": 17, "yuv422p": 18, "nv16": 19}


# ---- the layouts and the two rules, in numpy ---------------------------------------------------------------
def shape422(fmt, w, h):
    return (h, 2 * w) if fmt in ("yuyv422", "uyvy422") else (2 * h, w)


def planes422(fmt, p, w, h):
    """(Y, U, V) views of the frame p: h rows each, U and V w / 2 columns."""
    if fmt == "yuyv422":
        return p[:, 0:2 * w:2], p[:, 1:2 * w:4], p[:, 3:2 * w:4]
    if fmt == "uyvy422":
        return p[:, 1:2 * w:2], p[:, 0:2 * w:4], p[:, 2:2 * w:4]
    if fmt == "yuv422p":
        return p[:h, :w], p[h:, :w // 2], p[h:, w // 2:w]
    assert fmt == "nv16"
    return p[:h, :w], p[h:, 0:w:2], p[h:, 1:w:2]


def lay_out(fmt, y, u, v):
    h, w = y.shape
    p = np.empty(shape422(fmt, w, h), np.uint8)
    py, pu, pv = planes422(fmt, p, w, h)
    py[...], pu[...], pv[...] = y, u, v
    return p


def out_rule(fmt, f, w, h):
    """out rule: "Y over [U|V]" -> 4:2:2, every chroma row on two rows."""
    return lay_out(fmt, f[:h, :w], np.repeat(f[h:, :w // 2], 2, axis=0), np.repeat(f[h:, w // 2:w], 2, axis=0))


def in_rule(fmt, p, w, h):
    """in rule: 4:2:2 -> "Y over [U|V]", chroma rows averaged with rounding up."""
    y, u, v = planes422(fmt, p, w, h)
    f = np.empty((h * 3 // 2, w), np.uint8)
    f[:h] = y
    u, v = u.astype(np.int32), v.astype(np.int32)
    f[h:, :w // 2] = (u[0::2] + u[1::2] + 1) >> 1
    f[h:, w // 2:] = (v[0::2] + v[1::2] + 1) >> 1
    return f


def noise_yuv(f, w, h, seed):
    """(Y, U, V): the luma of f with independent noise chroma on every row."""
    rng = np.random.RandomState(seed)
    c = rng.randint(0, 256, (h, w), dtype=np.int64).astype(np.uint8)
    return f[:h, :w].copy(), c[:, :w // 2].copy(), c[:, w // 2:].copy()


def to_format(fmt, f, w, h):
    """A 4:2:0 frame in the input format `fmt` (the 4:2:0 layouts, or a 4:2:2 one by the out rule)."""
    if fmt == "yuv420p":
        return f
    if fmt == "nv12":
        nv = f.copy()
        nv[h:, 0::2], nv[h:, 1::2] = f[h:, :w // 2], f[h:, w // 2:]
        return nv
    return out_rule(fmt, f, w, h)


@pytest.fixture(scope="module")
def ox(product_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    assert hasattr(product_lib, "PIX_YUYV422"), "OCTVR_PIX_YUYV422 is missing"
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


_MEMO = {}


def memo(key, make):
    """A reference computed once and shared (never modified) by the tests and layouts that need it."""
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def noise_set(t, smooth_seed, noise_seed, carries=False):
    """(Y, U, V) planes per camera of t; with `carries`, camera 0 gets the chroma row pairs 255/254, 0/1, 1/0 and
    254/255: the carries of the four-bytes-at-a-time average."""
    yuv = [noise_yuv(f, w, h, noise_seed + i) for i, (f, (w, h)) in enumerate(zip(smooth(t, smooth_seed), t["sizes"]))]
    if carries:
        _, u, v = yuv[0]
        h = t["sizes"][0][1]
        for r in range(h // 4, h // 4 + 8):
            u[2 * r], u[2 * r + 1], v[2 * r], v[2 * r + 1] = 255, 254, 0, 1
            u[2 * r + 16], u[2 * r + 17], v[2 * r + 16], v[2 * r + 17] = 1, 0, 254, 255
    return yuv


def noise_case():
    """rigA: 4:2:2 planes with noise chroma (camera 0 with the carry rows), the converted frames, the oracle."""
    def make():
        t = golden("rigA")
        yuv = noise_set(t, 510, 77, carries=True)
        frames = [in_rule("yuv422p", lay_out("yuv422p", *p), w, h) for p, (w, h) in zip(yuv, t["sizes"])]
        want, g = oracle(t, frames, enable_gain=True, gains=None)
        return dict(t=t, yuv=yuv, frames=frames, want=want, gains=g)
    return memo("noise", make)


def laid(fmt, c):
    """The case's pictures in layout fmt; their conversion by the rule is what the oracle stitched."""
    t = c["t"]
    frames = [lay_out(fmt, *p) for p in c["yuv"]]
    for p, f, (w, h) in zip(frames, c["frames"], t["sizes"]):
        same(in_rule(fmt, p, w, h), f, "the layouts carry one picture")
    return frames


# ---- input ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", LAYOUTS)
@pytest.mark.parametrize("name", ["rigA", "rigB"])
def test_gpu_yuv422_in_replicated_chroma_is_the_planar_stitch(ox, name, fmt):
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
def test_gpu_yuv422_in_noise_chroma_averages_and_carries(ox, fmt):
    import torch
    c = noise_case()
    t = c["t"]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats(fmt, "yuv420p")
    out = planar_out(t["W"], t["H"])
    m.stitch([_cuda(p) for p in laid(fmt, c)], out)
    torch.cuda.synchronize()
    same_gains(m, c["gains"])
    same(out.cpu().numpy(), c["want"])


def _width_cases():
    cases = [(fmt, w) for fmt in LAYOUTS for w in (330, 328)]
    return cases + [("yuv422p", 332)]  # W / 2 = 166: the V half starts at a byte that is no multiple of 4


@pytest.mark.parametrize("fmt,in_w", _width_cases())
def test_gpu_yuv422_in_widths_pitch_and_odd_base(ox, fmt, in_w):
    """Pitch + 6, the base an odd byte offset into a larger tensor; a width with a short last group (every group
    on the byte path), one that is a multiple of 8 but not of 16 and, planar, one whose half is not 4-byte aligned."""
    import torch
    mt, t = ring(ox, 3, in_w)

    def make():
        yuv = noise_set(t, 620, 900)
        frames = [in_rule("nv16", lay_out("nv16", *p), w, h) for p, (w, h) in zip(yuv, t["sizes"])]
        return yuv, frames, oracle(t, frames, enable_gain=True, gains=None)
    yuv, frames, (want, g_orc) = memo(("width", in_w), make)
    laid_out = [lay_out(fmt, *p) for p in yuv]
    for p, f, (w, h) in zip(laid_out, frames, t["sizes"]):
        same(in_rule(fmt, p, w, h), f)
    m = ox.Mapper(mt, t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats(fmt, "yuv420p")
    dev = [_window(p, 6, 3) for p in laid_out]
    assert all(d.data_ptr() % 2 == 1 and d.stride(0) == shape422(fmt, in_w, 120)[1] + 6 for d in dev)
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
            yuv = noise_set(t, 700 + 9 * k, 40 * k)
            frames = [in_rule("yuv422p", lay_out("yuv422p", *p), w, h) for p, (w, h) in zip(yuv, t["sizes"])]
            sets.append(dict(t=t, yuv=yuv, frames=frames, want=oracle(t, frames, enable_gain=True, gains=None)[0]))
        return sets
    return memo("more", make)


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_yuv422_in_three_frames_in_flight(ox, fmt):
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
def test_gpu_yuv422_stitch_batch_of_two(ox, fmt):
    import torch
    c = noise_case()
    t = c["t"]
    second = _more_sets()[0]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_frames_in_flight(2)
    m.set_pixel_formats(fmt, fmt)
    W, H = t["W"], t["H"]
    outs = [torch.zeros(shape422(fmt, W, H), dtype=torch.uint8, device="cuda") for _ in range(2)]
    m.stitch_batch([[_cuda(p) for p in laid(fmt, c)], [_cuda(p) for p in laid(fmt, second)]], outs)
    torch.cuda.synchronize()
    same(outs[0].cpu().numpy(), out_rule(fmt, c["want"], W, H), "frame 0")
    same(outs[1].cpu().numpy(), out_rule(fmt, second["want"], W, H), "frame 1")


@pytest.mark.parametrize("fmt", LAYOUTS)
@pytest.mark.parametrize("blend", [0, 5])
def test_gpu_yuv422_overlay_rig(ox, blend, fmt):
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
        yuv = [noise_yuv(O.rand_img(w, h * 3 // 2, 1, 40 + i), w, h, 5 + i) for i, (w, h) in enumerate(sizes)]
        frames = [in_rule("nv16", lay_out("nv16", *p), w, h) for p, (w, h) in zip(yuv, sizes)]
        return mt, yuv, frames, OR.expected(OR.prepare(mt, blend), frames, sizes, blend=blend, enable_gain=True)
    mt, yuv, frames, want = memo(("overlay", blend), make)
    laid_out = [lay_out(fmt, *p) for p in yuv]
    for p, f, (w, h) in zip(laid_out, frames, sizes):
        same(in_rule(fmt, p, w, h), f)
    m = ox.Mapper(mt, sizes, blend=blend, enable_gain=True)
    m.set_pixel_formats(fmt, "yuv420p")
    out = planar_out(W, H)
    m.stitch([_cuda(p) for p in laid_out], out)
    torch.cuda.synchronize()
    same(out.cpu().numpy(), want[0], blend)
    same_gains(m, want[1])


@pytest.mark.parametrize("fmt", LAYOUTS)
@pytest.mark.parametrize("blend", [5, -4])
def test_gpu_yuv422_in_blended(ox, blend, fmt):
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
def test_gpu_yuv422_in_texture_mode(ox, fmt):
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
def test_gpu_yuv422_in_prepared_preview(ox, fmt):
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
    """got: the frame in layout fmt; want: the planar stitch."""
    same(got, out_rule(fmt, want, W, H), (what, "the numpy pack of the oracle's stitch"))
    y, u, v = planes422(fmt, got, W, H)
    same(y, want[:H, :W], (what, "Y"))
    for k in (0, 1):  # every chroma row on both of its rows
        same(u[k::2], want[H:, :W // 2], (what, "U on rows 2r + %d" % k))
        same(v[k::2], want[H:, W // 2:W], (what, "V on rows 2r + %d" % k))
    same(in_rule(fmt, got, W, H), want, (what, "round trip through the input rule"))


@pytest.mark.parametrize("fmt", LAYOUTS)
@pytest.mark.parametrize("in_fmt", ["yuv420p", "same"])
def test_gpu_yuv422_out_template_size_pitch_and_untouched_bytes(ox, in_fmt, fmt):
    """Pitch + 10 in a window at an odd byte offset; the bytes between a row's width and the pitch stay as they
    were."""
    import torch
    c = noise_case()
    t = c["t"]
    W, H = t["W"], t["H"]
    in_fmt = fmt if in_fmt == "same" else in_fmt
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats(in_fmt, fmt)
    assert m.pixel_formats == (in_fmt, fmt)
    dev = [_cuda(p) for p in (laid(fmt, c) if in_fmt == fmt else c["frames"])]
    rows, cols = shape422(fmt, W, H)
    out = _window(np.full((rows, cols), FILL, np.uint8), 10, 5)
    assert out.data_ptr() % 2 == 1
    whole = out.as_strided((rows, cols + 10), (cols + 10, 1))[: rows - 1]  # rows with their padding (the last row has none)
    m.stitch(dev, out)
    torch.cuda.synchronize()
    check_out(fmt, out.cpu().numpy(), c["want"], W, H, (in_fmt, fmt))
    assert (whole.cpu().numpy()[:, cols:] == FILL).all(), "bytes between a row's width and the pitch were written"
    same_gains(m, c["gains"])


@pytest.mark.parametrize("in_fmt,out_fmt", [("yuyv422", "uyvy422"), ("nv16", "yuv422p"), ("yuv420p", "nv16"),
                                            ("uyvy422", "yuyv422"), ("yuv422p", "nv12")])
def test_gpu_yuv422_mixed_formats(ox, in_fmt, out_fmt):
    """The two sides are independent, across the old and the new layouts."""
    import torch
    c = noise_case()
    t = c["t"]
    W, H = t["W"], t["H"]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats(in_fmt, out_fmt)
    assert m.pixel_formats == (in_fmt, out_fmt)
    if in_fmt in ("yuv420p", "nv12"):
        dev = [_cuda(to_format(in_fmt, f, w, h)) for f, (w, h) in zip(c["frames"], t["sizes"])]
    else:
        dev = [_cuda(p) for p in laid(in_fmt, c)]
    if out_fmt == "nv12":
        out = planar_out(W, H)
        m.stitch(dev, out)
        torch.cuda.synchronize()
        same(out.cpu().numpy(), to_format("nv12", c["want"], W, H), (in_fmt, out_fmt))
    else:
        out = torch.zeros(shape422(out_fmt, W, H), dtype=torch.uint8, device="cuda")
        m.stitch(dev, out)
        torch.cuda.synchronize()
        check_out(out_fmt, out.cpu().numpy(), c["want"], W, H, (in_fmt, out_fmt))
    same_gains(m, c["gains"])


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_yuv422_out_scaled_with_preview(ox, fmt):
    import torch
    c = noise_case()
    t = c["t"]
    scale, (pw, ph) = (256, 128), (200, 100)
    want, _, want_pv = memo("scaled", lambda: oracle(t, c["frames"], enable_gain=True, gains=None, scale=scale,
                                                     preview=(pw, ph)))
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True, scale_output=scale)
    m.set_pixel_formats(fmt, fmt)
    out = torch.zeros(shape422(fmt, scale[0], scale[1]), dtype=torch.uint8, device="cuda")
    pv = torch.zeros((ph, pw, 3), dtype=torch.uint8, device="cuda")
    m.stitch([_cuda(p) for p in laid(fmt, c)], out, preview=pv)
    torch.cuda.synchronize()
    check_out(fmt, out.cpu().numpy(), want, scale[0], scale[1], "scaled")
    same(pv.cpu().numpy(), want_pv, "the preview stays RGB")


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_yuv422_out_odd_output_width(ox, fmt):
    """An output width that is no multiple of 8 (250: W = 10 mod 16, W / 2 = 13 mod 16): row heads and tails of
    the pack kernel, and for the planar layout a V half at an odd byte."""
    import torch
    mt, t = ring(ox, 3, 328, W=250, H=126)
    frames = memo("odd-frames", lambda: smooth(t, 1500))
    want, _ = memo("odd", lambda: oracle(t, frames, enable_gain=True, gains=None))
    m = ox.Mapper(mt, t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats("yuv420p", fmt)
    rows, cols = shape422(fmt, 250, 126)
    out = _window(np.full((rows, cols), FILL, np.uint8), 2, 7)
    m.stitch([_cuda(f) for f in frames], out)
    torch.cuda.synchronize()
    check_out(fmt, out.cpu().numpy(), want, 250, 126, "250 wide")


# ---- API -----------------------------------------------------------------------------------------------------
def test_gpu_yuv422_api_names_values_and_helpers(ox):
    assert (ox.PIX_YUYV422, ox.PIX_YUV422P, ox.PIX_NV16) == (17, 18, 19)
    assert ox.frame_shape("yuyv422", 64, 32) == (32, 128)
    assert ox.frame_shape("yuv422p", 64, 32) == (64, 64) and ox.frame_shape("nv16", 64, 32) == (64, 64)
    assert ox.frame_shape("uyvy422", 64, 32) == (32, 128) and ox.frame_shape("nv12", 64, 32) == (48, 64)
    with pytest.raises(ValueError):
        ox.frame_shape("yuv444p", 64, 32)
    f = O.rand_img(64, 48, 1, 3)
    for fmt in LAYOUTS + ["uyvy422"]:
        p = ox.yuv422_from_yuv420p(fmt, f, 64, 32)
        same(p, out_rule(fmt, f, 64, 32), fmt)
        same(ox.yuv420p_from_yuv422(fmt, p, 64, 32), f, (fmt, "out-then-in is the identity"))
        noisy = lay_out(fmt, *noise_yuv(f, 64, 32, 9))
        same(ox.yuv420p_from_yuv422(fmt, noisy, 64, 32), in_rule(fmt, noisy, 64, 32), fmt)


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_yuv422_api_values_pitches_and_info(ox, fmt):
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
    with pytest.raises(ValueError):
        m.set_pixel_formats("yuv411p", "nv12")
    info = m.info()
    assert info["yuv422_out_bytes"] == 0 and info["yuv422_runs"] > 0
    assert (info["uyvy_runs"], info["uyvy_in_bytes"], info["uyvy_out_bytes"]) == (0, 0, 0), "the UYVY keys stay UYVY's"
    # every 4:2:2 layout is 2 B per pixel: 4 B per 4:2:0's 3 over the footprint's set groups
    assert info["yuv422_in_bytes"] * 3 == info["footprint_bytes"] * 4
    with pytest.raises(ox.OctvrError):  # the UYVY run dump is UYVY's
        ox.debug_mapper_uyvy_runs(m)
    # pitches below a row's width: E_INVALID, before any launch (the output keeps its bytes)
    m.set_pixel_formats(fmt, fmt)
    assert m.info()["yuv422_out_bytes"] == 2 * W * H
    rows, cols = shape422(fmt, W, H)
    out = torch.full((rows, cols), FILL, dtype=torch.uint8, device="cuda")
    dev = [_cuda(p) for p in laid(fmt, c)]
    narrow = torch.full((rows, cols - 2), FILL, dtype=torch.uint8, device="cuda")
    with pytest.raises(ox.OctvrError) as e:
        m.stitch(dev, narrow)
    assert e.value.code == E_INVALID
    assert (narrow == FILL).all()
    with pytest.raises(ox.OctvrError) as e:
        m.stitch([dev[0][:, :dev[0].shape[1] - 2].contiguous()] + dev[1:], out)
    assert e.value.code == E_INVALID
    torch.cuda.synchronize()
    assert (out == FILL).all()
    m.set_pixel_formats("yuv420p", "yuv420p")  # unset: the frames are freed, the plain path is back
    assert m.info()["yuv422_in_bytes"] == 0 and m.pixel_formats == ("yuv420p", "yuv420p")
    out = planar_out(W, H)
    m.stitch([_cuda(f) for f in c["frames"]], out)
    torch.cuda.synchronize()
    same(out.cpu().numpy(), memo("plain", lambda: oracle(t, c["frames"], enable_gain=False)[0]), "back on planar")
