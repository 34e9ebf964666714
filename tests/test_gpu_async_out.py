"""The merged frame of the AsyncMultiMapper pipeline in a converted output layout (octvr_async_set_output_format):
UYVY, YUYV, YUV422P, NV16, P010, YUV420P10, P210 and YUV422P10 out of push (host planes, registered or not) and
push_device (one device frame), written by one merge_pack_kernel launch per frame from the mappers' NV12 region
frames.  Everything is bit-exact: the expected bytes are tests/async_out_ref.py's out rules and region placement
(numpy, independent of the library) applied to the oracle's stitch per region.  Every destination starts full of
0x5A at a padded pitch, and every check covers the whole buffer: bytes outside every region and between a row's
width and its pitch must still hold the fill."""
import numpy as np
import pytest

import async_out_ref as R
import test_gpu_async as G
import test_gpu_async_device as D
import test_gpu_async_nv12 as A
import test_gpu_async_uyvy as U
import test_gpu_async_yuv10 as T10

pytestmark = pytest.mark.gpu

FILL = R.FILL
WHOLE = [(0.0, 0.0, 1.0, 1.0)]


@pytest.fixture(scope="module")
def ox(product_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    assert hasattr(product_lib.lib(), "octvr_async_set_output_format"), "octvr_async_set_output_format is missing"
    return product_lib


def new_device_frame(fmt, OW, OH, pad=6, offset=2):
    """A device frame of the layout full of FILL: a window of a larger tensor at pitch = row + pad whose first byte
    is `offset` bytes past a 16-byte boundary.  Returns (window, whole buffer)."""
    import torch
    rows, nbytes = R.frame_dims(fmt, OW, OH)
    pitch = nbytes + pad
    buf = torch.full((rows * pitch + 32,), FILL, dtype=torch.uint8, device="cuda")
    win = torch.as_strided(buf, (rows, nbytes), (pitch, 1), offset)
    assert win.data_ptr() % 16 == offset % 16 and win.stride(0) == pitch
    return win, buf


def check_device_frame(win, buf, want, what, offset=2):
    rows, nbytes = want.shape
    pitch = win.stride(0)
    host = buf.cpu().numpy()
    assert (host[:offset] == FILL).all() and (host[offset + rows * pitch:] == FILL).all(), (what, "bytes around the frame")
    got = host[offset:offset + rows * pitch].reshape(rows, pitch)
    d = got[:, :nbytes] != want
    assert not d.any(), (what, int(d.sum()), np.argwhere(d)[:6].tolist())
    assert (got[:, nbytes:] == FILL).all(), (what, "bytes between the row and the pitch were written")


# ---- 1. one whole-frame region, all eight layouts, more frames than slots -----------------------------------------
def _riga_inputs(in_fmt):
    """(frames' plane sets for push, oracle stitches) of five frames of rigA with inputs in in_fmt."""
    t = A.golden("rigA")
    if in_fmt == "yuv420p":
        frames, want = A.riga_case()
        return [[A.in_planes(f, w, h, "yuv420p") for f, (w, h) in zip(fr, t["sizes"])] for fr in frames], want
    if in_fmt == "uyvy422":  # four packed frame sets: the first again as the fifth
        c = U.case()
        planes = [[U.padded(p) for p in s] for s in c["packed"]]
        return planes + planes[:1], c["want"] + c["want"][:1]
    c = T10.case()
    return [T10.planes_of(in_fmt, c, f) for f in range(5)], c["want"]


CASES_1 = [("yuv420p", f) for f in R.LAYOUTS] + [("p010", "p010"), ("uyvy422", "uyvy422")]


@pytest.mark.parametrize("in_fmt,fmt", CASES_1, ids=["%s-%s" % c for c in CASES_1])
def test_gpu_async_out_whole_frame(ox, in_fmt, fmt):
    """Five frames of rigA, gain estimated, through push: every plane at a padded pitch, the first output registered
    (its rectangles downloaded straight into it), the others through the pinned staging and the copy-out."""
    t = A.golden("rigA")
    W, H = t["W"], t["H"]
    planes, want = _riga_inputs(in_fmt)
    am = ox.AsyncMultiMapper([A.template(ox, t)], t["sizes"], (W, H), [0], [0], WHOLE)
    if in_fmt != "yuv420p":
        am.set_pixel_formats(in_fmt, "yuv420p")
    am.set_output_format(fmt)
    assert am.pixel_formats == (in_fmt, fmt)
    assert am.info()["pixel_formats"][1] == R.VALUES[fmt]
    outs = [R.new_planes(fmt, W, H) for _ in range(5)]
    assert all(p.base.strides[0] > p.shape[1] for p in outs[0])
    am.register_output(outs[0])
    for f in range(3):
        am.push(planes[f], outs[f])
    assert am.pending() == 3
    for f in range(3, 5):  # every slot again
        assert am.pop() is outs[f - 3]
        am.push(planes[f], outs[f])
    for f in range(2, 5):
        assert am.pop() is outs[f]
    for f in range(5):
        R.check_planes(outs[f], R.merged_frame(fmt, W, H, [(0, 0, want[f])]), fmt, W, H, (in_fmt, fmt, f))
    info = am.info()
    assert info["merge_pack_launches"] == 5 and info["merge_launches"] == 0
    am.unregister_output(outs[0])
    am.close()


# ---- 2. two regions off every vector boundary, host planes and a device window ------------------------------------
@pytest.mark.parametrize("fmt", R.LAYOUTS)
def test_gpu_async_out_ragged_regions(ox, fmt):
    """The left and right half of 1036 x 512 (r.x = r.w = 518: a packed row of the right half starts 12 bytes past a
    16-byte boundary, an 8-bit U half at byte 259; the mappers scale 768 x 384 to 518 x 512): once by push into host
    planes, once by push_device into a window of a larger tensor at pitch + 6, 2 bytes past a 16-byte boundary."""
    t = A.golden("rigB")
    frames, want = D.scaled_want((518, 512))
    am = ox.AsyncMultiMapper([A.template(ox, t) for _ in range(2)], t["sizes"], (1036, 512), [0, 0], [0, 0], D.LEFT_RIGHT)
    am.set_output_format(fmt)
    expect = R.merged_frame(fmt, 1036, 512, [(0, 0, want), (518, 0, want)])
    out = R.new_planes(fmt, 1036, 512)
    A.push(am, t, frames, out, "yuv420p")
    assert am.pop() is out
    R.check_planes(out, expect, fmt, 1036, 512, (fmt, "host"))
    win, buf = new_device_frame(fmt, 1036, 512)
    ins = D.dev_inputs(frames, t["sizes"], "yuv420p")
    D.sync()
    am.push_device(ins, win)
    assert am.pop() is win
    check_device_frame(win, buf, expect, (fmt, "device"))
    info = am.info()
    assert info["merge_pack_launches"] == 2 and info["merge_launches"] == 0 and info["device_frames"] == 1
    am.close()


# ---- 3. a region that does not cover the output -------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["yuyv422", "nv16", "p210", "yuv422p", "yuv420p10"])
def test_gpu_async_out_gap_untouched(ox, fmt):
    """Two quarter regions on the diagonal of 768 x 768: the other two quarters keep the fill, luma and chroma, in the
    host planes and in the device frame."""
    t = A.golden("rigB")
    frames, want = D.scaled_want((384, 384))
    am = ox.AsyncMultiMapper([A.template(ox, t) for _ in range(2)], t["sizes"], (768, 768), [0, 0], [0, 0],
                             [(0.0, 0.0, 0.5, 0.5), (0.5, 0.5, 0.5, 0.5)])
    am.set_output_format(fmt)
    expect = R.merged_frame(fmt, 768, 768, [(0, 0, want), (384, 384, want)])
    assert (R.planes_of(fmt, expect, 768, 768)[0][:384, -16:] == FILL).all()
    out = R.new_planes(fmt, 768, 768, pad=10)
    A.push(am, t, frames, out, "yuv420p")
    am.pop()
    R.check_planes(out, expect, fmt, 768, 768, (fmt, "host"))
    win, buf = new_device_frame(fmt, 768, 768, pad=10, offset=0)
    ins = D.dev_inputs(frames, t["sizes"], "yuv420p")
    D.sync()
    am.push_device(ins, win)
    am.pop()
    check_device_frame(win, buf, expect, (fmt, "device"), offset=0)
    am.close()


# ---- 4. format switches on one pipeline ----------------------------------------------------------------------------
def test_gpu_async_out_format_switches(ox):
    """uyvy422 -> p210 -> yuv422p -> nv12 (through set_pixel_formats, which leaves converted output) -> yuv420p10, a
    checked frame after each."""
    t = A.golden("rigA")
    W, H = t["W"], t["H"]
    frames, want = A.riga_case()
    am = ox.AsyncMultiMapper([A.template(ox, t)], t["sizes"], (W, H), [0], [0], WHOLE)
    for f, fmt in enumerate(["uyvy422", "p210", "yuv422p", "nv12", "yuv420p10"]):
        if fmt == "nv12":
            am.set_pixel_formats("yuv420p", "nv12")
            assert am.pixel_formats == ("yuv420p", "nv12")
            out = A.new_out(W, H, "nv12", pad=4)
            A.push(am, t, frames[f], out, "yuv420p")
            assert am.pop() is out
            A.check(out, A.want_out(W, H, [(0, 0, want[f])], "nv12"), fmt)
            continue
        am.set_output_format(fmt)
        assert am.pixel_formats == ("yuv420p", fmt)
        out = R.new_planes(fmt, W, H)
        A.push(am, t, frames[f], out, "yuv420p")
        assert am.pop() is out
        R.check_planes(out, R.merged_frame(fmt, W, H, [(0, 0, want[f])]), fmt, W, H, fmt)
    assert am.info()["merge_pack_launches"] == 4
    am.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------
def test_gpu_async_out_odd_region_refused(ox):
    """x = 3 / 512: creation accepts the region (r.w even, c.w == r.w / 2) with r.x = 3 and c.x = 2; UYVY cannot
    place it (OCTVR_E_INVALID naming the region, formats unchanged) and NV12 output still stitches it."""
    t = A.golden("rigA")
    W, H = t["W"], t["H"]
    assert (W, H) == (512, 256)
    reg = (3 / W, 0.0, 0.5, 1.0)
    r, c = G._rect_mul_size(reg, W, H), G._rect_mul_size(reg, W // 2, H // 2)
    assert r == (3, 0, 256, 256) and c == (2, 0, 128, 128) and r[2] % 2 == 0 and c[2] == r[2] // 2
    frames, _ = A.riga_case()
    want = A.oracle(t, frames[0], enable_gain=True, scale=(256, 256))
    am = ox.AsyncMultiMapper([A.template(ox, t)], t["sizes"], (W, H), [0], [0], [reg])
    am.set_pixel_formats("yuv420p", "nv12")
    for fmt in ("uyvy422", "p010"):
        with pytest.raises(ox.OctvrError) as e:
            am.set_output_format(fmt)
        assert e.value.code == ox.E_INVALID and "region 0" in str(e.value)
        assert am.pixel_formats == ("yuv420p", "nv12")
    out = A.new_out(W, H, "nv12", pad=4)
    A.push(am, t, frames[0], out, "yuv420p")
    am.pop()
    y = np.full((H, W), FILL, np.uint8)
    uv = np.full((H // 2, W), FILL, np.uint8)
    y[:, 3:259] = want[:256]
    uv[:, 4:260] = A.interleave(want[256:, :128], want[256:, 128:])
    A.check(out, (y, uv), "nv12 at an odd origin")
    am.close()


def test_gpu_async_out_refusals(ox):
    import torch
    t = A.golden("rigA")
    W, H = t["W"], t["H"]
    frames, want = A.riga_case()
    am = ox.AsyncMultiMapper([A.template(ox, t)], t["sizes"], (W, H), [0], [0], WHOLE)
    ins = D.dev_inputs(frames[0], t["sizes"], "yuv420p")
    D.sync()

    def good_frame(fmt, f, what):
        out = R.new_planes(fmt, W, H)
        A.push(am, t, frames[f], out, "yuv420p")
        am.pop()
        R.check_planes(out, R.merged_frame(fmt, W, H, [(0, 0, want[f])]), fmt, W, H, what)

    # set_pixel_formats keeps refusing a converted output format, and an unknown value is refused
    with pytest.raises(ox.OctvrError) as e:
        am.set_pixel_formats("yuv420p", "uyvy422")
    assert e.value.code == ox.E_UNSUPPORTED and "output" in str(e.value)
    with pytest.raises(ox.OctvrError) as e:
        am.set_output_format(7)
    assert e.value.code == ox.E_INVALID and am.pixel_formats == ("yuv420p", "yuv420p")

    am.set_output_format("p010")
    # a 16-bit device frame at an odd base, at an odd pitch, at a pitch below a row
    rows, nbytes = R.frame_dims("p010", W, H)
    buf = torch.full((rows * (nbytes + 8) + 32,), FILL, dtype=torch.uint8, device="cuda")
    for pitch, offset in ((nbytes + 6, 1), (nbytes + 7, 0), (nbytes - 2, 0)):
        with pytest.raises(ox.OctvrError) as e:
            am.push_device(ins, torch.as_strided(buf, (rows, nbytes), (pitch, 1), offset))
        assert e.value.code == ox.E_INVALID and am.pending() == 0, (pitch, offset)
    assert (buf.cpu().numpy() == FILL).all(), "a refused push wrote the output"
    # host planes: an odd pitch; one column short (the wrapper's own check); a plane missing
    y, uv = R.new_planes("p010", W, H)
    odd = np.full((H // 2, nbytes + 3), FILL, np.uint8)[:, :nbytes]
    with pytest.raises(ox.OctvrError) as e:
        A.push(am, t, frames[0], (y, odd), "yuv420p")
    assert e.value.code == ox.E_INVALID and am.pending() == 0
    with pytest.raises(ValueError):
        A.push(am, t, frames[0], (y, uv[:, :nbytes - 2]), "yuv420p")
    with pytest.raises(ValueError):
        A.push(am, t, frames[0], (y,), "yuv420p")
    with pytest.raises(ValueError):
        am.push_device(ins, torch.zeros((rows, nbytes - 2), dtype=torch.uint8, device="cuda"))
    assert am.pending() == 0
    good_frame("p010", 0, "after the refused pushes")

    # the call with a frame pending
    out = R.new_planes("p010", W, H)
    A.push(am, t, frames[1], out, "yuv420p")
    with pytest.raises(ox.OctvrError) as e:
        am.set_output_format("uyvy422")
    assert e.value.code == ox.E_INVALID and am.pixel_formats == ("yuv420p", "p010")
    am.pop()
    R.check_planes(out, R.merged_frame("p010", W, H, [(0, 0, want[1])]), "p010", W, H, "the pending frame")

    # the call with planes registered in another format
    reg = R.new_planes("p010", W, H)
    am.register_output(reg)
    for fmt in ("uyvy422", "nv12"):
        with pytest.raises(ox.OctvrError) as e:
            am.set_output_format(fmt)
        assert e.value.code == ox.E_INVALID and am.pixel_formats == ("yuv420p", "p010")
    am.set_output_format("p010")  # the same format is no change
    A.push(am, t, frames[2], reg, "yuv420p")
    am.pop()
    R.check_planes(reg, R.merged_frame("p010", W, H, [(0, 0, want[2])]), "p010", W, H, "registered")
    am.unregister_output(reg)
    am.set_output_format("uyvy422")
    good_frame("uyvy422", 3, "after unregistering")
    assert am.pending() == 0
    am.close()
