"""v210 frames (OCTVR_PIX_V210 = 48: 10-bit 4:2:2, three components a 32-bit word, six pixels a 16-byte block, rows
padded to 48 pixels) in and out of the Mapper.  A v210 stitch is the planar 8-bit stitch of the frames converted by the
in rule, stored by the out rule, bit for bit: every comparison here is byte for byte against the oracle's stitch of
tests/v210_ref.py's in_rule frames, stored by its out_rule (numpy written from the format's definition, never the
library's helpers).  The pictures, rigs and oracle stitches are those of tests/test_gpu_yuv10.py where the shapes
agree (one reference, shared and never modified)."""
import json

import numpy as np
import pytest

import oracle_py as O
import v210_ref as V
import yuv10_ref as R10
from test_gpu_yuv10 import (FILL, _cuda, _more_sets, _window, golden, memo, noise_case, oracle, picture_set, planar_out, ring,
                            same, same_gains, smooth, template)

pytestmark = pytest.mark.gpu

E_INVALID = -1


@pytest.fixture(scope="module")
def ox(product_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    assert hasattr(product_lib, "PIX_V210"), "OCTVR_PIX_V210 is missing"
    return product_lib


def laid(c, sizes=None, seed=3000):
    """The case's 4:2:2 pictures as v210 frames with random bits wherever the format ignores them; their conversion by
    the in rule is what the oracle stitched."""
    sizes = sizes or c["t"]["sizes"]
    frames = [V.lay_out(*p, seed=seed + i) for i, p in enumerate(c["pics"])]
    for p, f, (w, h) in zip(frames, c["frames"], sizes):
        assert p.shape == V.shape(w, h)
        same(V.in_rule(p, w, h), f, "the v210 frame carries the picture")
    return frames


def out_v210(W, H):
    import torch
    return torch.zeros(V.shape(W, H), dtype=torch.uint8, device="cuda")


def check_out(got, want, W, H, what):
    """got: the v210 frame as bytes; want: the planar 8-bit stitch."""
    same(got, V.out_rule(want, W, H), (what, "the numpy out rule of the oracle's stitch, zeros included"))
    assert not (np.asarray(got) & V.ignored_mask(W, H)).any(), (what, "ignored bits, absent components and padding are 0")
    same(V.in_rule(got, W, H), want, (what, "round trip through the in rule"))


# ---- input ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_w", [96, 144, 146, 148, 150, 192])
def test_gpu_v210_in_widths_junk_pitch_and_base(ox, in_w):
    """Every W % 6, W % 8 and W % 48 class: all three group phases, the short last group and the per-sample path (146,
    148, 150), padding blocks (all but 96, 144 and 192).  Noise pictures with the edge values and the chroma row pairs,
    random junk in every ignored bit, absent component and padding block; windows of larger tensors with the base 4
    bytes past a 16-byte boundary and pitch row_bytes + 4."""
    import torch
    mt, t = ring(ox, 3, in_w)

    def make():
        pics, frames = picture_set(t, 620, 900, edges=True)
        return dict(t=t, pics=pics, frames=frames, ref=oracle(t, frames, enable_gain=True, gains=None))
    c = memo(("v210-width", in_w), make)
    want, g_orc = c["ref"]
    frames = laid(c)
    y, u, v = V.planes10(frames[0], in_w, 120)
    assert set(R10.EDGE) <= set(np.unique(y)) and set(R10.EDGE) <= set(np.unique(u)), "the edge values are in the frame"
    for a, b in R10.PAIRS:
        assert ((u[0::2] == a) & (u[1::2] == b)).any(), "the chroma row pairs are in the frame"
    assert (frames[0] & V.ignored_mask(in_w, 120)).any(), "the ignored bits are not all 0"
    m = ox.Mapper(mt, t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats("v210", "yuv420p")
    assert m.pixel_formats == ("v210", "yuv420p")
    dev = [_window(p, 4, 4) for p in frames]
    assert all(d.data_ptr() % 16 == 4 and d.stride(0) == V.row_bytes(in_w) + 4 for d in dev)
    out = planar_out(t["W"], t["H"])
    m.stitch(dev, out)
    torch.cuda.synchronize()
    same_gains(m, g_orc)
    same(out.cpu().numpy(), want, in_w)


def test_gpu_v210_in_three_frames_in_flight(ox):
    import torch
    c = noise_case()
    t = c["t"]
    sets = [c] + _more_sets()
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats("v210", "yuv420p")
    m.set_frames_in_flight(3)
    assert m.pixel_formats == ("v210", "yuv420p")
    streams = [torch.cuda.Stream() for _ in range(3)]
    dev = [[_cuda(p) for p in laid(s)] for s in sets]
    outs = [planar_out(t["W"], t["H"]) for _ in range(6)]
    torch.cuda.synchronize()
    for k in range(6):  # every slot twice
        m.stitch(dev[k % 3], outs[k], stream=streams[k % 3])
    torch.cuda.synchronize()
    for k in range(6):
        same(outs[k].cpu().numpy(), sets[k % 3]["want"], k)


def test_gpu_v210_stitch_batch_of_two(ox):
    import torch
    c = noise_case()
    t = c["t"]
    second = _more_sets()[0]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_frames_in_flight(2)
    m.set_pixel_formats("v210", "v210")
    W, H = t["W"], t["H"]
    outs = [out_v210(W, H) for _ in range(2)]
    m.stitch_batch([[_cuda(p) for p in laid(c)], [_cuda(p) for p in laid(second)]], outs)
    torch.cuda.synchronize()
    check_out(outs[0].cpu().numpy(), c["want"], W, H, "frame 0")
    check_out(outs[1].cpu().numpy(), second["want"], W, H, "frame 1")


@pytest.mark.parametrize("blend", [16, -5])
def test_gpu_v210_blended(ox, blend):
    import torch
    c = noise_case()
    t = c["t"]
    W, H = t["W"], t["H"]
    want, g_orc = memo(("blend", blend),
                       lambda: oracle(t, c["frames"], enable_gain=True, gains=None, blend=blend, seams=t["seams"]))
    m = ox.Mapper(template(ox, t), t["sizes"], blend=blend, enable_gain=True)
    m.set_pixel_formats("v210", "v210")
    out = out_v210(W, H)
    m.stitch([_cuda(p) for p in laid(c)], out)
    torch.cuda.synchronize()
    same_gains(m, g_orc)
    check_out(out.cpu().numpy(), want, W, H, blend)


def test_gpu_v210_texture_mode(ox):
    import torch
    c = noise_case()
    t = c["t"]
    W, H = t["W"], t["H"]
    want, g_orc = memo("texture", lambda: oracle(t, c["frames"], enable_gain=True, gains=None, remap_tex=True))
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True, remap="texture")
    m.set_pixel_formats("v210", "v210")
    out = out_v210(W, H)
    m.stitch([_cuda(p) for p in laid(c)], out)
    torch.cuda.synchronize()
    same_gains(m, g_orc)
    check_out(out.cpu().numpy(), want, W, H, "texture")


@pytest.mark.parametrize("blend", [0, 5])
def test_gpu_v210_overlay_rig(ox, blend):
    """The overlay frame is v210 of its own size and goes through the same conversion, against tests/overlay_ref.py."""
    import copy
    import torch
    import camera_rigs as R
    import overlay_ref as OR
    rig = copy.deepcopy(R.mask_rigs()["overlay_include"])
    W, H = 512, 256
    sizes = [(640, 360)] * len(rig["inputs"]) + [(192, 128)]

    def make():  # test_gpu_yuv10's case: OR.prepare gives the template the seam masks a multi-band mapper needs
        mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
        pics = [R10.noise_picture(O.rand_img(w, h * 3 // 2, 1, 40 + i), w, h, 5 + i) for i, (w, h) in enumerate(sizes)]
        frames = [R10.frame8(p) for p in pics]
        return dict(mt=mt, pics=pics, frames=frames,
                    want=OR.expected(OR.prepare(mt, blend), frames, sizes, blend=blend, enable_gain=True))
    c = memo(("overlay", blend), make)
    m = ox.Mapper(c["mt"], sizes, blend=blend, enable_gain=True)
    m.set_pixel_formats("v210", "v210")
    out = out_v210(W, H)
    m.stitch([_cuda(p) for p in laid(c, sizes)], out)
    torch.cuda.synchronize()
    check_out(out.cpu().numpy(), c["want"][0], W, H, blend)
    same_gains(m, c["want"][1])


def test_gpu_v210_prepared_preview_and_tensor(ox):
    import torch
    c = noise_case()
    t = c["t"]
    pw, ph = 128, 64
    want, _, want_pv = memo("preview", lambda: oracle(t, c["frames"], enable_gain=True, gains=None, preview=(pw, ph)))
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats("v210", "yuv420p")
    m.prepare_preview(pw, ph)
    dev = [_cuda(p) for p in laid(c)]
    out = planar_out(t["W"], t["H"])
    pv = torch.zeros((ph, pw, 3), dtype=torch.uint8, device="cuda")
    m.stitch(dev, out, preview=pv)
    torch.cuda.synchronize()
    same(out.cpu().numpy(), want, "frame")
    same(pv.cpu().numpy(), want_pv, "preview")
    ten = torch.zeros((3, ph, pw), dtype=torch.float16, device="cuda")
    m.stitch_tensor(dev, ten, scale=1 / 255.0)
    torch.cuda.synchronize()
    expect = (want_pv.astype(np.float32) * np.float32(1 / 255.0)).astype(np.float16).transpose(2, 0, 1)
    same(ten.cpu().numpy().view(np.uint16), np.ascontiguousarray(expect).view(np.uint16), "f16 tensor")


def test_gpu_v210_scaled_output_with_preview(ox):
    import torch
    c = noise_case()
    t = c["t"]
    scale, (pw, ph) = (256, 128), (200, 100)
    want, _, want_pv = memo("scaled", lambda: oracle(t, c["frames"], enable_gain=True, gains=None, scale=scale,
                                                     preview=(pw, ph)))
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True, scale_output=scale)
    m.set_pixel_formats("v210", "v210")
    out = out_v210(*scale)
    pv = torch.zeros((ph, pw, 3), dtype=torch.uint8, device="cuda")
    m.stitch([_cuda(p) for p in laid(c)], out, preview=pv)
    torch.cuda.synchronize()
    check_out(out.cpu().numpy(), want, scale[0], scale[1], "scaled")
    same(pv.cpu().numpy(), want_pv, "the preview stays RGB")


# ---- output --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad,base", [(0, 0), (4, 4), (20, 12)])
@pytest.mark.parametrize("W,H", [(256, 128), (240, 128), (250, 126)])
def test_gpu_v210_out_widths_sentinel_pitch_and_base(ox, W, H, pad, base):
    """256 (2 pixels in the last block with pixels, padding blocks), 240 (a whole number of 48-pixel units) and 250 (4
    pixels in the last block): every byte of row_bytes equals the reference, zeros included; every byte from row_bytes
    to the pitch keeps the sentinel; 16-byte aligned blocks and blocks 4 and 12 bytes past a boundary."""
    import torch
    mt, t = ring(ox, 3, 328, W=W, H=H)
    frames = memo(("v210-out-frames", W), lambda: smooth(t, 1500))
    want, g_orc = memo(("v210-out", W), lambda: oracle(t, frames, enable_gain=True, gains=None))
    m = ox.Mapper(mt, t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats("yuv420p", "v210")
    assert m.pixel_formats == ("yuv420p", "v210")
    rows, cols = V.shape(W, H)
    out = _window(np.full((rows, cols), FILL, np.uint8), pad, base)
    assert out.data_ptr() % 16 == base and out.stride(0) == cols + pad
    whole = out.as_strided((rows, cols + pad), (cols + pad, 1))[: rows - 1]  # rows with their padding (the last row has none)
    m.stitch([_cuda(f) for f in frames], out)
    torch.cuda.synchronize()
    check_out(out.cpu().numpy(), want, W, H, (W, pad, base))
    assert (whole.cpu().numpy()[:, cols:] == FILL).all(), "bytes between row_bytes and the pitch were written"
    same_gains(m, g_orc)


def test_gpu_v210_out_then_in_is_the_identity(ox):
    """Two mappers: the first writes the stitch of the 8-bit frames as v210, and the in rule reads the planar stitch
    back from it; the second reads the same frames widened by the out rule as v210 inputs and writes the first
    mapper's frame, with the same gains."""
    import torch
    c = noise_case()
    t = c["t"]
    W, H = t["W"], t["H"]
    first = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    first.set_pixel_formats("yuv420p", "v210")
    out = out_v210(W, H)
    first.stitch([_cuda(f) for f in c["frames"]], out)
    torch.cuda.synchronize()
    same(V.in_rule(out.cpu().numpy(), W, H), c["want"], "out, then the in rule")
    second = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    second.set_pixel_formats("v210", "v210")
    out2 = out_v210(W, H)
    second.stitch([_cuda(V.out_rule(f, w, h)) for f, (w, h) in zip(c["frames"], t["sizes"])], out2)
    torch.cuda.synchronize()
    same(out2.cpu().numpy(), out.cpu().numpy(), "in of out-rule frames, then out: the first mapper's frame")
    same_gains(second, c["gains"])


@pytest.mark.parametrize("in_fmt,out_fmt", [("v210", "nv12"), ("v210", "uyvy422"), ("v210", "p010"), ("yuv420p", "v210"),
                                            ("yuv422p10", "v210")])
def test_gpu_v210_format_mixes(ox, in_fmt, out_fmt):
    """The two sides are independent, across the 8-bit, the 16-bit-word and the v210 layouts."""
    import torch
    c = noise_case()
    t = c["t"]
    W, H = t["W"], t["H"]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=True)
    m.set_pixel_formats(in_fmt, out_fmt)
    assert m.pixel_formats == (in_fmt, out_fmt)
    if in_fmt == "v210":
        dev = [_cuda(p) for p in laid(c)]
    elif in_fmt == "yuv420p":
        dev = [_cuda(f) for f in c["frames"]]
    else:
        dev = [_cuda(R10.laid_out(in_fmt, p, 1000 + i)) for i, p in enumerate(c["pics"])]
    want = c["want"]
    if out_fmt == "v210":
        out = out_v210(W, H)
        m.stitch(dev, out)
        torch.cuda.synchronize()
        check_out(out.cpu().numpy(), want, W, H, (in_fmt, out_fmt))
    elif out_fmt == "p010":
        out = torch.zeros(R10.shape10("p010", W, H), dtype=torch.uint8, device="cuda")
        m.stitch(dev, out)
        torch.cuda.synchronize()
        same(out.cpu().numpy(), R10.out_rule("p010", want, W, H), (in_fmt, out_fmt))
    else:
        exp = want.copy()
        if out_fmt == "nv12":
            exp[H:, 0::2], exp[H:, 1::2] = want[H:, :W // 2], want[H:, W // 2:]
        else:  # the 8-bit out rule, written out: chroma row r on packed rows 2r and 2r + 1
            exp = np.empty((H, 2 * W), np.uint8)
            exp[:, 1::2] = want[:H, :W]
            exp[:, 0::4] = np.repeat(want[H:, :W // 2], 2, axis=0)
            exp[:, 2::4] = np.repeat(want[H:, W // 2:W], 2, axis=0)
        out = torch.zeros(exp.shape, dtype=torch.uint8, device="cuda")
        m.stitch(dev, out)
        torch.cuda.synchronize()
        same(out.cpu().numpy(), exp, (in_fmt, out_fmt))
    same_gains(m, c["gains"])


# ---- API -----------------------------------------------------------------------------------------------------
def test_gpu_v210_refusals(ox):
    import ctypes as C
    import torch
    c = noise_case()
    t = c["t"]
    W, H = t["W"], t["H"]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=False)
    lib = ox.lib()
    assert ox.PIX_V210 == 48 and ox.frame_shape("v210", 250, 126) == (126, 768) and ox.v210_row_bytes(48) == 128
    m.set_pixel_formats(48, 48)  # by value
    for bad in (49, 47, 2, 7, -1, 15, 20):
        assert lib.octvr_mapper_set_pixel_formats(m._h, bad, 48) == E_INVALID
        assert lib.octvr_mapper_set_pixel_formats(m._h, 48, bad) == E_INVALID
    assert m.pixel_formats == ("v210", "v210"), "a rejected call changes nothing"
    a, b = C.c_int(-7), C.c_int(-7)
    assert lib.octvr_mapper_pixel_formats(m._h, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (48, 48)
    frames = laid(c)
    dev = [_cuda(p) for p in frames]
    rows, cols = V.shape(W, H)

    def refused(ins, out):
        with pytest.raises(ox.OctvrError) as e:
            m.stitch(ins, out)
        assert e.value.code == E_INVALID
        torch.cuda.synchronize()

    # pitch row_bytes - 4, on either side
    narrow = torch.full((rows, cols - 4), FILL, dtype=torch.uint8, device="cuda")
    refused(dev, narrow)
    assert (narrow == FILL).all()
    out = torch.full((rows, cols), FILL, dtype=torch.uint8, device="cuda")
    refused([dev[0][:, :dev[0].shape[1] - 4].contiguous()] + dev[1:], out)
    # an odd base, a base 2 (mod 4), a pitch 2 (mod 4), on either side: E_INVALID before any launch, the output untouched
    for pad, off in ((4, 3), (4, 2), (6, 4), (4, 1)):
        refused([_window(frames[0], pad, off)] + dev[1:], out)
        assert (out == FILL).all()
        bad = _window(np.full((rows, cols), FILL, np.uint8), pad, off)
        assert (bad.data_ptr() % 4, bad.stride(0) % 4) == (off % 4, (cols + pad) % 4)
        refused(dev, bad)
        assert (bad == FILL).all()
    good = _window(np.full((rows, cols), FILL, np.uint8), 4, 4)
    m.stitch(dev, good)
    torch.cuda.synchronize()
    check_out(good.cpu().numpy(), memo("v210-nogain", lambda: oracle(t, c["frames"], enable_gain=False)[0]), W, H, "after the refusals")


def test_gpu_v210_info(ox):
    """The info keys against counts made here from the mapper's footprint runs (the debug dump of a UYVY-input mapper:
    the runs are the footprint's, the same for every layout)."""
    c = noise_case()
    t = c["t"]
    W, H = t["W"], t["H"]
    m = ox.Mapper(template(ox, t), t["sizes"], blend=0, enable_gain=False)
    m.set_pixel_formats("uyvy422", "nv12")
    runs = ox.debug_mapper_uyvy_runs(m)
    uyvy = m.info()
    assert all(uyvy[k] == 0 for k in ("v210_runs", "v210_in_bytes", "v210_out_bytes"))
    m.set_pixel_formats("v210", "nv12")
    info = m.info()
    blocks = 0
    for cam, rp, g0, ng in runs.tolist():
        w = t["sizes"][cam][0]
        blocks += 2 * (-(-min(8 * (g0 + ng), w) // 6) - 8 * g0 // 6)  # the covering blocks of the run's two rows
    assert info["v210_runs"] == len(runs) == uyvy["uyvy_runs"] > 0
    assert info["v210_in_bytes"] == 16 * blocks
    assert info["v210_out_bytes"] == 0
    zero = ("uyvy_runs", "uyvy_in_bytes", "uyvy_out_bytes", "yuv422_runs", "yuv422_in_bytes", "yuv422_out_bytes", "yuv10_runs",
            "yuv10_in_bytes", "yuv10_out_bytes")
    assert [info[k] for k in zero] == [0] * 9, "the other families' keys are 0 for a v210 side"
    m.set_pixel_formats("p210", "v210")
    info = m.info()
    assert info["v210_out_bytes"] == V.row_bytes(W) * H and (info["v210_runs"], info["v210_in_bytes"]) == (0, 0)
    assert info["yuv10_runs"] == len(runs) and info["yuv10_in_bytes"] * 3 == info["footprint_bytes"] * 8
    m.set_pixel_formats("uyvy422", "uyvy422")  # the existing keys keep their values
    again = m.info()
    assert (again["uyvy_runs"], again["uyvy_in_bytes"]) == (uyvy["uyvy_runs"], uyvy["uyvy_in_bytes"])
    assert again["uyvy_out_bytes"] == 2 * W * H and again["v210_out_bytes"] == 0
