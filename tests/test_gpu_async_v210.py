"""v210 as the input format of the AsyncMultiMapper pipeline (octvr_async_set_pixel_formats with OCTVR_PIX_V210 = 48):
push packs and uploads the 16-byte blocks that hold the footprint runs' pixels of the one host plane per camera,
push_device converts the caller's device frames, and the mappers stitch the pipeline's 8-bit NV12 frames.  The expected
bytes are the oracle's stitch of the frames converted by tests/v210_ref.py's in rule; the pictures and the oracle
stitches are tests/test_gpu_async_yuv10.py's (one reference, shared and never modified).  v210 as the pipeline's output
format is not built: OCTVR_E_UNSUPPORTED from both calls that could set it."""
import numpy as np
import pytest

import async_out_ref as RO
import v210_ref as V
from test_gpu_async_yuv10 import FILL, case, check_host, host_out, padded, template

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ox(product_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    assert hasattr(product_lib, "PIX_V210"), "OCTVR_PIX_V210 is missing"
    return product_lib


def laid(c, f):
    """Picture set f as v210 frames with random bits wherever the format ignores them; the in rule gives the oracle's
    frames."""
    frames = [V.lay_out(*p, seed=4000 + 10 * f + i) for i, p in enumerate(c["pics"][f])]
    for p, f8, (w, h) in zip(frames, c["frames"][f], c["t"]["sizes"]):
        assert p.shape == V.shape(w, h) and np.array_equal(V.in_rule(p, w, h), f8), "the v210 frame carries the picture"
    return frames


def planes_of(c, f, pad=4):
    return [(padded(p, pad),) for p in laid(c, f)]


def one_region(ox, t):
    return ox.AsyncMultiMapper([template(ox, t)], t["sizes"], (t["W"], t["H"]), [0], [0], [(0.0, 0.0, 1.0, 1.0)])


@pytest.mark.parametrize("out_fmt", ["yuv420p", "nv12"])
def test_gpu_async_v210_push_three_pending_pageable_padded(ox, out_fmt):
    """Five frames (more than the slots) from pageable host planes with pitch row_bytes + 4, three pending at a time."""
    c = case()
    t = c["t"]
    W, H = t["W"], t["H"]
    am = one_region(ox, t)
    am.set_pixel_formats("v210", out_fmt)
    assert am.pixel_formats == ("v210", out_fmt)
    assert am.info()["pixel_formats"] == [48, int(out_fmt == "nv12")]
    outs = [host_out(W, H, out_fmt) for _ in range(5)]
    planes = [planes_of(c, f) for f in range(5)]
    assert all(p.strides[0] == p.shape[1] + 4 for tri in planes[0] for p in tri)
    for f in range(3):
        am.push(planes[f], outs[f])
    assert am.pending() == 3
    for f in range(3, 5):  # every slot again
        assert am.pop() is outs[f - 3]
        am.push(planes[f], outs[f])
    for f in range(2, 5):
        assert am.pop() is outs[f]
    for f in range(5):
        check_host(outs[f], c["want"][f], W, H, out_fmt, (out_fmt, f))
    am.close()


def test_gpu_async_v210_two_regions_host_and_push_device(ox):
    """Two mappers over the same inputs (one conversion for both), side by side in the merged frame; minimal-pitch host
    planes and device frames (windows with pitch row_bytes + 4, 4 bytes past a 16-byte boundary)."""
    import torch
    c = case()
    t = c["t"]
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([template(ox, t), template(ox, t)], t["sizes"], (2 * W, H), [0, 0], [0, 0],
                             [(0.0, 0.0, 0.5, 1.0), (0.5, 0.0, 0.5, 1.0)])
    am.set_pixel_formats("v210", "yuv420p")
    want = c["want"][0]
    merged = np.empty((H * 3 // 2, 2 * W), np.uint8)  # "Y over [U|V]" of the 2 W wide frame
    merged[:H, :W], merged[:H, W:] = want[:H], want[:H]
    merged[H:, :W // 2], merged[H:, W // 2:W] = want[H:, :W // 2], want[H:, :W // 2]
    merged[H:, W:W + W // 2], merged[H:, W + W // 2:] = want[H:, W // 2:], want[H:, W // 2:]
    out = host_out(2 * W, H, "yuv420p")
    am.push(planes_of(c, 0, 0), out)
    dout = torch.full((H * 3 // 2, 2 * W), FILL, dtype=torch.uint8, device="cuda")
    dev = []
    for p in laid(c, 0):
        rows, cols = p.shape
        buf = torch.full(((rows + 1) * (cols + 4) + 32,), FILL, dtype=torch.uint8, device="cuda")
        off = (-buf.data_ptr()) % 16 + 4
        d = buf[off:off + rows * (cols + 4)].view(rows, cols + 4)[:, :cols]
        d.copy_(torch.from_numpy(p))
        dev.append(d)
    torch.cuda.synchronize()
    am.push_device(dev, dout)
    am.pop()
    check_host(out, merged, 2 * W, H, "yuv420p", "host")
    am.pop()
    assert np.array_equal(dout.cpu().numpy(), merged)
    with pytest.raises(ValueError):  # an 8-bit-shaped tensor is not a v210 frame
        am.push_device([torch.zeros((h * 3 // 2, w), dtype=torch.uint8, device="cuda") for w, h in t["sizes"]], dout)
    odd = [d for d in dev]
    odd[0] = torch.zeros((dev[0].shape[0], dev[0].shape[1] + 2), dtype=torch.uint8, device="cuda")[:, 2:]
    with pytest.raises(ox.OctvrError):  # a base 2 (mod 4)
        am.push_device(odd, dout)
    assert am.pending() == 0
    am.close()


@pytest.mark.parametrize("fmt", ["uyvy422", "p010"])
def test_gpu_async_v210_converted_output_formats(ox, fmt):
    """v210 in with the merged frame as UYVY and as P010 (octvr_async_set_output_format, merge_pack_kernel)."""
    c = case()
    t = c["t"]
    W, H = t["W"], t["H"]
    am = one_region(ox, t)
    am.set_pixel_formats("v210", "nv12")
    am.set_output_format(fmt)
    assert am.pixel_formats == ("v210", fmt)
    out = RO.new_planes(fmt, W, H)
    am.push(planes_of(c, 1), out)
    am.pop()
    RO.check_planes(out, RO.merged_frame(fmt, W, H, [(0, 0, c["want"][1])]), fmt, W, H, ("v210", fmt))
    am.close()


def test_gpu_async_v210_format_switches_rebuild_the_table(ox):
    """v210 -> planar -> v210 -> P210 -> v210 on one pipeline: the packed offsets are each format's own (v210's covering
    blocks against 3 and 8 bytes per pixel of a piece's row)."""
    import yuv10_ref as R10
    from test_gpu_async_yuv10 import planes_of as planes10
    c = case()
    t = c["t"]
    W, H = t["W"], t["H"]
    am = one_region(ox, t)
    for fmt, f in [("v210", 0), ("yuv420p", 1), ("v210", 2), ("p210", 3), ("v210", 4)]:
        am.set_pixel_formats(fmt, "yuv420p")
        assert am.pixel_formats == (fmt, "yuv420p")
        out = host_out(W, H, "yuv420p")
        if fmt == "v210":
            planes = planes_of(c, f)
        elif fmt == "p210":
            planes = planes10(fmt, c, f)
        else:
            planes = [(fr[:h, :w], fr[h:, :w // 2], fr[h:, w // 2:]) for fr, (w, h) in zip(c["frames"][f], t["sizes"])]
        am.push(planes, out)
        am.pop()
        check_host(out, c["want"][f], W, H, "yuv420p", (fmt, f))
    am.close()


def test_gpu_async_v210_out_is_unsupported_and_bad_planes(ox):
    c = case()
    t = c["t"]
    W, H = t["W"], t["H"]
    am = one_region(ox, t)
    lib = ox.lib()
    E_INVALID, E_UNSUPPORTED = -1, lib.octvr_async_set_pixel_formats(am._h, 0, 16)
    assert E_UNSUPPORTED not in (0, E_INVALID)
    am.set_pixel_formats("v210", "nv12")
    for call in (lambda: am.set_pixel_formats("v210", "v210"), lambda: am.set_pixel_formats("yuv420p", "v210"),
                 lambda: am.set_output_format("v210")):
        with pytest.raises(ox.OctvrError) as e:
            call()
        assert e.value.code == E_UNSUPPORTED and "v210 out" in str(e.value) and "not built" in str(e.value)
        assert am.pixel_formats == ("v210", "nv12"), "a rejected call changes nothing"
        assert am.info()["pixel_formats"] == [48, 1]
    for bad in (49, 47):
        assert lib.octvr_async_set_pixel_formats(am._h, bad, 0) == E_INVALID
        assert lib.octvr_async_set_output_format(am._h, bad) == E_INVALID
    assert am.pixel_formats == ("v210", "nv12")
    out = host_out(W, H, "nv12")
    good = planes_of(c, 0, 0)
    for cut in (4, 2):  # a plane narrower than row_bytes, a pitch 2 (mod 4)
        bad_planes = [(np.ascontiguousarray(p[0][:, :-cut]),) for p in good]
        with pytest.raises(ox.OctvrError):
            am.push(bad_planes, out)
    assert am.pending() == 0
    am.push(good, out)
    am.pop()
    check_host(out, c["want"][0], W, H, "nv12", "after the refused calls")
    am.close()


def test_gpu_async_v210_debug_pack_runs(ox):
    """octvr_debug_pack_runs for v210: a run is the blocks that hold its pixels, those of row 2 rp, then those of row
    2 rp + 1 (the last group of a 330 wide row is 2 pixels; runs at all three group phases)."""
    w, h = 330, 8
    rng = np.random.RandomState(31)
    frame = V.lay_out(rng.randint(0, 1024, (h, w)), rng.randint(0, 1024, (h, w // 2)), rng.randint(0, 1024, (h, w // 2)), seed=3)
    runs = [(0, 1, 3, 2), (0, 3, 40, 2), (0, 0, 0, 42), (0, 2, 1, 1), (0, 2, 2, 5)]
    packed, sizes = ox.debug_pack_runs([(w, h)], runs, [(padded(frame, 4),)], "v210")
    want, nblocks = [], []
    for _, rp, g0, ng in runs:
        b0, b1 = 8 * g0 // 6, -(-min(8 * (g0 + ng), w) // 6)
        want += [frame[r, 16 * b0:16 * b1] for r in (2 * rp, 2 * rp + 1)]
        nblocks.append(b1 - b0)
    assert np.array_equal(packed, np.concatenate(want))
    assert sizes.tolist() == [32 * n for n in nblocks]
