"""AsyncMultiMapper.push_device (octvr_async_push_device): device frames in, one merged device frame out, no
host copy.  The mappers read the caller's tensors in place and merge_regions_kernel places the region frames
into the merged frame.  Expected bytes are the oracle's stitch per region, merged by this file's own numpy the
way tests/test_gpu_async.py and tests/test_gpu_async_nv12.py build them, never the host push path of the
build under test.  Merged frames start as 0x5A at a pitch above the width, so bytes that must stay untouched
(outside every region, between the width and the pitch) are checked too."""
import json
import threading

import numpy as np
import pytest

import test_gpu_async as G
import test_gpu_async_nv12 as A

pytestmark = pytest.mark.gpu

FILL = A.FILL
TOP_BOTTOM = [(0.0, 0.0, 1.0, 0.5), (0.0, 0.5, 1.0, 0.5)]
LEFT_RIGHT = [(0.0, 0.0, 0.5, 1.0), (0.5, 0.0, 0.5, 1.0)]


@pytest.fixture(scope="module")
def ox(product_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    assert hasattr(product_lib.lib(), "octvr_async_push_device"), "octvr_async_push_device is missing"
    return product_lib


# ---- frames and expectations --------------------------------------------------------------------------------
def layout(f, w, h, fmt):
    """The "Y over [U|V]" host frame f in the layout fmt: NV12 interleaves the chroma rows' halves."""
    if fmt != "nv12":
        return np.ascontiguousarray(f[:, :w])
    return np.vstack([f[:h, :w], A.interleave(f[h:, :w // 2], f[h:, w // 2:w])])


def dev_inputs(frames, sizes, fmt):
    import torch
    return [torch.from_numpy(layout(f, w, h, fmt)).cuda() for f, (w, h) in zip(frames, sizes)]


def new_merged(OW, OH, pad=6):
    """A merged device frame full of FILL: a (3 OH / 2, OW) view of a tensor with pitch OW + pad."""
    import torch
    base = torch.full((OH * 3 // 2, OW + pad), FILL, dtype=torch.uint8, device="cuda")
    return base[:, :OW], base


def merged(planes):
    """Host output planes (Y, U, V) or (Y, UV) as one merged frame: the chroma rows under the Y rows."""
    return np.vstack([planes[0], planes[1] if len(planes) == 2 else np.hstack([planes[1], planes[2]])])


def check_merged(base, OW, want, what):
    got = base.cpu().numpy()
    d = got[:, :OW] != want
    assert not d.any(), (what, int(d.sum()), np.argwhere(d)[:6].tolist())
    assert (got[:, OW:] == FILL).all(), (what, "bytes between the width and the pitch were written")


_RIGB = {}


def rigb_case():
    """Three frames of rigB through two mappers, blends [0, 16], region 1 with region 0's gains, top and bottom
    of a 768 x 768 output with a 300 x 201 preview: the oracle's merged planes and preview per frame."""
    if not _RIGB:
        t = A.golden("rigB")
        frames = [A.smooth_frames(t, 9100 + 10 * f) for f in range(3)]
        res = [G.preview_oracle(fr, t["sizes"], t["rois"], t["maps1"], t["maps2"], t["masks"], t["W"], t["H"], [0, 16],
                                [0, 0], TOP_BOTTOM, (768, 768), (300, 201), seams=t["seams"]) for fr in frames]
        _RIGB.update(frames=frames, planes=[r[0] for r in res], preview=[r[1] for r in res])
    return _RIGB


def want_merged(planes, fmt):
    y, u, v = planes
    return merged((y, A.interleave(u, v)) if fmt == "nv12" else planes)


def rigb_pipeline(ox, fmt=("yuv420p", "yuv420p"), preview_size=(0, 0)):
    t = A.golden("rigB")
    am = ox.AsyncMultiMapper([A.template(ox, t) for _ in range(2)], t["sizes"], (768, 768), [0, 16], [0, 0], TOP_BOTTOM,
                             preview_size=preview_size)
    am.set_pixel_formats(*fmt)
    return am, t


def sync():
    import torch
    torch.cuda.synchronize()


# ---- 1. two regions, every format pair, pipelined ---------------------------------------------------------------
@pytest.mark.parametrize("fmt", A.PAIRS, ids=["%s-%s" % p for p in A.PAIRS])
def test_gpu_async_device_two_regions(ox, fmt):
    """Top and bottom at template size, blends [0, 16], gain chain [0, 0]: three frames pushed before the first
    pop, each bit-exact against the oracle (which estimates region 0's gains itself and hands them to region 1,
    so wrong gains show as wrong bytes); one merge launch per frame."""
    c = rigb_case()
    am, t = rigb_pipeline(ox, fmt)
    ins = [dev_inputs(fr, t["sizes"], fmt[0]) for fr in c["frames"]]
    outs = [new_merged(768, 768) for _ in c["frames"]]
    sync()
    for i, (o, _) in zip(ins, outs):
        am.push_device(i, o)
    assert am.pending() == 3
    for f, (o, base) in enumerate(outs):
        assert am.pop() is o
        check_merged(base, 768, want_merged(c["planes"][f], fmt[1]), (fmt, f))
    info = am.info()
    assert info["device_frames"] == 3 and info["merge_launches"] == 3
    with pytest.raises(ox.OctvrError):
        am.pop()
    am.close()


# ---- 2. regions off every vector boundary ---------------------------------------------------------------------
_SCALED = {}


def scaled_want(size):
    """One frame of rigB and its oracle stitch scaled to `size`, blend 0, own gains."""
    if "frames" not in _SCALED:
        _SCALED["frames"] = A.smooth_frames(A.golden("rigB"), 9400)
    if size not in _SCALED:
        _SCALED[size] = A.oracle(A.golden("rigB"), _SCALED["frames"], enable_gain=True, scale=size)
    return _SCALED["frames"], _SCALED[size]


@pytest.mark.parametrize("out_fmt", ["yuv420p", "nv12"])
@pytest.mark.parametrize("pad", [0, 6])
def test_gpu_async_device_ragged_regions(ox, out_fmt, pad):
    """Output 1036 x 512 in two halves: r.x = r.w = 518 = 6 (mod 16), c.x = c.w = 259, so the planar chroma
    halves start and end off every vector boundary (tests/test_async_device_host.py checks the region rule
    for these numbers); the mappers scale 768 x 384 to 518 x 512.  Pitch 1036 and 1036 + 6; nothing but the
    regions' bytes is written."""
    t = A.golden("rigB")
    frames, want = scaled_want((518, 512))
    am = ox.AsyncMultiMapper([A.template(ox, t) for _ in range(2)], t["sizes"], (1036, 512), [0, 0], [0, 0], LEFT_RIGHT)
    am.set_pixel_formats("yuv420p", out_fmt)
    o, base = new_merged(1036, 512, pad)
    ins = dev_inputs(frames, t["sizes"], "yuv420p")
    sync()
    am.push_device(ins, o)
    assert am.pop() is o
    check_merged(base, 1036, merged(A.want_out(1036, 512, [(0, 0, want), (518, 0, want)], out_fmt)), (out_fmt, pad))
    assert am.info()["merge_launches"] == 1
    am.close()


@pytest.mark.parametrize("out_fmt", ["yuv420p", "nv12"])
def test_gpu_async_device_gap_untouched(ox, out_fmt):
    """Two quarter regions on the diagonal of a 768 x 768 output: the other two quarters, luma and chroma,
    keep the fill byte."""
    t = A.golden("rigB")
    frames, want = scaled_want((384, 384))
    am = ox.AsyncMultiMapper([A.template(ox, t) for _ in range(2)], t["sizes"], (768, 768), [0, 0], [0, 0],
                             [(0.0, 0.0, 0.5, 0.5), (0.5, 0.5, 0.5, 0.5)])
    am.set_pixel_formats("yuv420p", out_fmt)
    o, base = new_merged(768, 768, 10)
    ins = dev_inputs(frames, t["sizes"], "yuv420p")
    sync()
    am.push_device(ins, o)
    am.pop()
    check_merged(base, 768, merged(A.want_out(768, 768, [(0, 0, want), (384, 384, want)], out_fmt)), out_fmt)
    am.close()


# ---- 3. one region covering the whole output: no merge ----------------------------------------------------------
@pytest.mark.parametrize("out_fmt", ["yuv420p", "nv12"])
def test_gpu_async_device_single_region_in_place(ox, out_fmt):
    t = A.golden("rigA")
    frames, want = A.riga_case()
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([A.template(ox, t)], t["sizes"], (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])
    am.set_pixel_formats("yuv420p", out_fmt)
    outs = [new_merged(W, H, 10) for _ in frames[:3]]
    ins = [dev_inputs(fr, t["sizes"], "yuv420p") for fr in frames[:3]]
    sync()
    for i, (o, _) in zip(ins, outs):
        am.push_device(i, o)
    for f, (o, base) in enumerate(outs):
        assert am.pop() is o
        check_merged(base, W, merged(A.want_out(W, H, [(0, 0, want[f])], out_fmt)), (out_fmt, f))
    info = am.info()
    assert info["merge_launches"] == 0 and info["device_frames"] == 3
    am.close()


# ---- 4. inputs that are views of larger tensors -------------------------------------------------------------------
@pytest.mark.parametrize("in_fmt", ["yuv420p", "nv12"])
def test_gpu_async_device_input_views(ox, in_fmt):
    """Each input is a window of a larger tensor (pitch = width + 24, first byte 8 columns and one row in),
    the surroundings full of another byte; two regions, so the merge runs as well."""
    import torch
    t = A.golden("rigA")
    frames, want = A.riga_case()
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([A.template(ox, t) for _ in range(2)], t["sizes"], (W, 2 * H), [0, 0], [0, 0], TOP_BOTTOM)
    am.set_pixel_formats(in_fmt, "yuv420p")
    ins = []
    for f, (w, h) in zip(frames[1], t["sizes"]):
        big = torch.full((h * 3 // 2 + 2, w + 24), 0xC3, dtype=torch.uint8, device="cuda")
        view = big[1:1 + h * 3 // 2, 8:8 + w]
        view.copy_(torch.from_numpy(layout(f, w, h, in_fmt)))
        assert view.stride(0) == w + 24 and view.data_ptr() == big.data_ptr() + w + 24 + 8
        ins.append(view)
    o, base = new_merged(W, 2 * H)
    sync()
    am.push_device(ins, o)
    am.pop()
    check_merged(base, W, merged(A.want_out(W, 2 * H, [(0, 0, want[1]), (0, H, want[1])], "yuv420p")), in_fmt)
    am.close()


# ---- 5. the ready event ---------------------------------------------------------------------------------------------
def test_gpu_async_device_ready_event(ox):
    """The inputs are filled on a side stream behind other work; the push follows the event's record with no
    synchronisation in between."""
    import torch
    t = A.golden("rigA")
    frames, want = A.riga_case()
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([A.template(ox, t) for _ in range(2)], t["sizes"], (W, 2 * H), [0, 0], [0, 0], TOP_BOTTOM)
    host = [torch.from_numpy(layout(f, w, h, "yuv420p")).pin_memory() for f, (w, h) in zip(frames[2], t["sizes"])]
    ins = [torch.zeros_like(h, device="cuda") for h in host]
    o, base = new_merged(W, 2 * H)
    busy = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    sync()
    side = torch.cuda.Stream()
    ready = torch.cuda.Event()
    with torch.cuda.stream(side):
        for k in range(16):  # about a gigabyte of stores ahead of the copies
            busy.fill_(k)
        for d, h in zip(ins, host):
            d.copy_(h, non_blocking=True)
        ready.record(side)
    am.push_device(ins, o, ready=ready)
    assert am.pop() is o
    check_merged(base, W, merged(A.want_out(W, 2 * H, [(0, 0, want[2]), (0, H, want[2])], "yuv420p")), "ready")
    am.close()


# ---- 6. a rig with an overlay: N + K frames ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [("yuv420p", "yuv420p"), ("nv12", "nv12")], ids=["planar", "nv12"])
def test_gpu_async_device_overlay(ox, fmt):
    """The overlay_include rig, blend 0 (the overlay in the composite LUT) on the left half and multi-band (the
    overlay applied to the result frame) on the right: the overlay's frame is the third device frame."""
    import overlay_ref as OR
    import test_gpu_overlay as T
    W, H = T.W, T.H
    rig = T.rig_one()
    sizes = T._sizes(rig)
    mts = [ox.MapperTemplate.from_json(json.dumps(rig), W, H) for _ in range(2)]
    frames = T._frames(sizes, 960)
    want = [OR.expected(OR.prepare(mts[k], b), frames, sizes, blend=b, scale=(W // 2, H))[0] for k, b in enumerate((0, 5))]
    am = ox.AsyncMultiMapper(mts, sizes, (W, H), [0, 5], [0, 0], LEFT_RIGHT)
    am.set_pixel_formats(*fmt)
    assert am.n == len(rig["inputs"]) + len(rig["overlays"])
    o, base = new_merged(W, H)
    ins = dev_inputs(frames, sizes, fmt[0])
    sync()
    am.push_device(ins, o)
    am.pop()
    check_merged(base, W, merged(A.want_out(W, H, [(0, 0, want[0]), (W // 2, 0, want[1])], fmt[1])), fmt)
    am.close()


# ---- 7. the preview ------------------------------------------------------------------------------------------------
def test_gpu_async_device_preview_and_reentrant_sink(ox):
    """The preview of a device frame is downloaded and published as for push: every sunk image equals the
    oracle's; and a sink that calls preview() — which takes the lock the publishing holds — returns."""
    c = rigb_case()
    am, t = rigb_pipeline(ox, preview_size=(300, 201))
    sunk = []

    def sink(rgb, hdr):
        inner, ihdr = am.preview()  # the frame being published
        sunk.append((rgb, inner, (hdr.width, hdr.height), (ihdr.width, ihdr.height)))

    am.set_preview_sink(sink)
    ins = [dev_inputs(fr, t["sizes"], "yuv420p") for fr in c["frames"]]
    outs = [new_merged(768, 768) for _ in c["frames"]]
    sync()
    for i, (o, _) in zip(ins, outs):
        am.push_device(i, o)
    errors = []

    def pops():
        try:
            for _ in outs:
                am.pop()
        except Exception as e:  # reported by the main thread
            errors.append(e)

    th = threading.Thread(target=pops, daemon=True)
    th.start()
    th.join(60)
    assert not th.is_alive(), "pop() hangs: the sink's preview() waits for the lock its caller holds"
    assert not errors, errors
    assert len(sunk) == 3
    for f, (rgb, inner, size, isize) in enumerate(sunk):
        assert size == isize == (300, 201)
        assert np.array_equal(rgb, c["preview"][f]), (f, int((rgb != c["preview"][f]).sum()))
        assert np.array_equal(inner, c["preview"][f]), (f, "preview() inside the sink")
        check_merged(outs[f][1], 768, want_merged(c["planes"][f], "yuv420p"), ("preview", f))
    rgb, hdr = am.preview()
    assert np.array_equal(rgb, c["preview"][2]) and (hdr.width, hdr.height) == (300, 201)
    am.set_preview_sink(None)
    am.close()


# ---- 8. host and device frames on one pipeline ---------------------------------------------------------------------
def test_gpu_async_device_interleaved_with_push(ox):
    t = A.golden("rigA")
    frames, want = A.riga_case()
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([A.template(ox, t) for _ in range(2)], t["sizes"], (W, 2 * H), [0, 0], [0, 0], TOP_BOTTOM)
    host0, host2 = A.new_out(W, 2 * H, "yuv420p"), A.new_out(W, 2 * H, "yuv420p", pad=8)
    o, base = new_merged(W, 2 * H)
    ins = dev_inputs(frames[1], t["sizes"], "yuv420p")
    sync()
    A.push(am, t, frames[0], host0, "yuv420p")
    am.push_device(ins, o)
    A.push(am, t, frames[2], host2, "yuv420p")
    assert am.pending() == 3
    assert am.pop() is host0
    assert am.pop() is o
    assert am.pop() is host2
    assert am.pending() == 0
    A.check(host0, A.want_out(W, 2 * H, [(0, 0, want[0]), (0, H, want[0])], "yuv420p"), "host frame 0")
    check_merged(base, W, merged(A.want_out(W, 2 * H, [(0, 0, want[1]), (0, H, want[1])], "yuv420p")), "device frame 1")
    A.check(host2, A.want_out(W, 2 * H, [(0, 0, want[2]), (0, H, want[2])], "yuv420p"), "host frame 2")
    assert am.info()["device_frames"] == 1
    am.close()


# ---- 9. refused pushes ------------------------------------------------------------------------------------------------
def test_gpu_async_device_rejects(ox):
    import ctypes as C
    import torch
    t = A.golden("rigA")
    frames, _ = A.riga_case()
    W, H = t["W"], t["H"]
    n = len(t["sizes"])
    am = ox.AsyncMultiMapper([A.template(ox, t) for _ in range(2)], t["sizes"], (W, 2 * H), [0, 0], [0, 0], TOP_BOTTOM)
    ins = dev_inputs(frames[0], t["sizes"], "yuv420p")
    o, base = new_merged(W, 2 * H)
    sync()
    lib = ox.lib()

    def raw(in_ptrs, in_pitches, out_ptr, out_pitch):
        """octvr_async_push_device itself: its status, with nothing queued on a refusal."""
        rc = lib.octvr_async_push_device(am._h, (C.c_void_p * n)(*in_ptrs) if in_ptrs is not None else None,
                                         (C.c_size_t * n)(*in_pitches) if in_pitches is not None else None,
                                         C.c_void_p(out_ptr), out_pitch, None)
        assert am.pending() == 0
        return rc

    ptrs, pitches = [x.data_ptr() for x in ins], [x.stride(0) for x in ins]
    with pytest.raises(ValueError):  # wrong count
        am.push_device(ins[:-1], o)
    assert am.pending() == 0
    with pytest.raises(ValueError):  # a host tensor never reaches the library through the wrapper
        am.push_device([x.cpu() for x in ins], o)
    # pitch too small: rows that overlap, legal for torch, refused by the library
    w0, h0 = t["sizes"][0]
    narrow = torch.as_strided(ins[0], (h0 * 3 // 2, w0), (w0 - 2, 1))
    with pytest.raises(ox.OctvrError) as e:
        am.push_device([narrow] + ins[1:], o)
    assert e.value.code == ox.E_INVALID and am.pending() == 0
    assert raw(ptrs, pitches, o.data_ptr(), W - 2) == ox.E_INVALID
    # NULL: the arrays, one frame, the output
    assert raw(None, pitches, o.data_ptr(), o.stride(0)) == ox.E_INVALID
    assert raw(ptrs, None, o.data_ptr(), o.stride(0)) == ox.E_INVALID
    assert raw([None] + ptrs[1:], pitches, o.data_ptr(), o.stride(0)) == ox.E_INVALID
    assert raw(ptrs, pitches, None, o.stride(0)) == ox.E_INVALID
    # an output frame of 2 GiB or more, by its pitch
    assert raw(ptrs, pitches, o.data_ptr(), 0x7FFFFF80 // (3 * H) + 1) == ox.E_INVALID
    # pinned host memory: the device could read it, the library refuses it all the same
    pinned = torch.from_numpy(layout(frames[0][0], w0, h0, "yuv420p")).pin_memory()
    assert raw([pinned.data_ptr()] + ptrs[1:], pitches, o.data_ptr(), o.stride(0)) == ox.E_INVALID
    pinned_out = torch.empty((3 * H, W), dtype=torch.uint8).pin_memory()
    assert raw(ptrs, pitches, pinned_out.data_ptr(), W) == ox.E_INVALID
    plain = np.zeros((3 * H, W), np.uint8)  # pageable host memory
    assert raw(ptrs, pitches, plain.ctypes.data, W) == ox.E_INVALID
    assert (base.cpu().numpy() == FILL).all(), "a refused push wrote the output"
    # and the pipeline still works
    am.push_device(ins, o)
    assert am.pending() == 1
    am.pop()
    assert am.info()["device_frames"] == 1
    am.close()
