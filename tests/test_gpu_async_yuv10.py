"""10-bit inputs of the AsyncMultiMapper pipeline (octvr_async_set_pixel_formats with OCTVR_PIX_P010 / _YUV420P10 /
_P210 / _YUV422P10 as the input format): push packs and uploads the footprint runs of the host planes at the format's
own offsets, push_device converts the caller's device frames, and the mappers stitch the pipeline's 8-bit NV12 frames.
The expected bytes are the oracle's stitch of the frames converted by tests/yuv10_ref.py's numpy (the in rule:
v8 = min(255, (v10 + 2) >> 2), the 4:2:2 layouts then averaged with rounding up); the pictures are made once as 10-bit
4:2:2 planes, so one oracle stitch serves the four layouts."""
import json
import math

import numpy as np
import pytest

import oracle_py as O
import yuv10_ref as R10
from yuv10_ref import LAYOUTS, VALUES, shape10, in_rule

pytestmark = pytest.mark.gpu

FILL = 0x5A


def padded(p, pad):
    """The byte plane inside an array whose pitch is its width + pad."""
    a = np.full((p.shape[0], p.shape[1] + pad), 0xC3, np.uint8)
    a[:, :p.shape[1]] = p
    return a[:, :p.shape[1]]


def host_planes(fmt, frame, w, h, pad=6):
    """The plane tuple push() takes for the layout, cut from the whole frame (bytes): Y and the U,V plane, or Y, U, V."""
    if not R10.planar(fmt):
        return (padded(frame[:h], pad), padded(frame[h:], pad))
    return (padded(frame[:h], pad), padded(frame[h:, :w], pad), padded(frame[h:, w:], pad + 2 if pad else 0))


@pytest.fixture(scope="module")
def ox(product_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    assert hasattr(product_lib, "PIX_P010"), "OCTVR_PIX_P010 is missing"
    return product_lib


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


def pictures(t, seed):
    from octvr_amd import synthetic
    return [R10.noise_picture(synthetic.smooth_yuv_frame(w, h, seed + i), w, h, seed + 50 + i, edges=i == 0)
            for i, (w, h) in enumerate(t["sizes"])]


_CASE = {}


def case():
    """Five picture sets of rigA (more than the pipeline's slots), the converted frames and the oracle's stitches."""
    if not _CASE:
        t = golden("rigA")
        pics = [pictures(t, 100 * f) for f in range(5)]
        frames = [[R10.frame8(p) for p in s] for s in pics]
        _CASE.update(t=t, pics=pics, frames=frames, want=[oracle(t, fr, enable_gain=True) for fr in frames])
    return _CASE


def laid(fmt, c, f):
    """Picture set f as whole frames of the layout (random ignored bits); the rule gives the oracle's frames."""
    frames = [R10.laid_out(fmt, p, 2000 + 10 * f + i) for i, p in enumerate(c["pics"][f])]
    for p, f8, (w, h) in zip(frames, c["frames"][f], c["t"]["sizes"]):
        assert np.array_equal(in_rule(fmt, p, w, h), f8), "the layouts carry one picture"
    return frames


def planes_of(fmt, c, f, pad=6):
    return [host_planes(fmt, p, w, h, pad) for p, (w, h) in zip(laid(fmt, c, f), c["t"]["sizes"])]


def host_out(W, H, fmt, pad=4):
    y = np.full((H, W + pad), FILL, np.uint8)[:, :W]
    if fmt == "nv12":
        return (y, np.full((H // 2, W + pad), FILL, np.uint8)[:, :W])
    return (y, np.full((H // 2, W // 2 + pad), FILL, np.uint8)[:, :W // 2], np.full((H // 2, W // 2 + pad), FILL, np.uint8)[:, :W // 2])


def check_host(out, want, W, H, fmt, what):
    assert np.array_equal(out[0], want[:H]), (what, "Y")
    u, v = want[H:, :W // 2], want[H:, W // 2:]
    if fmt == "nv12":
        assert np.array_equal(out[1][:, 0::2], u) and np.array_equal(out[1][:, 1::2], v), (what, "UV")
    else:
        assert np.array_equal(out[1], u) and np.array_equal(out[2], v), (what, "U, V")
    for p in out:
        assert (p.base[:, p.shape[1]:] == FILL).all(), (what, "bytes past a plane's width were written")


@pytest.mark.parametrize("fmt", LAYOUTS)
@pytest.mark.parametrize("out_fmt", ["yuv420p", "nv12"])
def test_gpu_async_yuv10_push_more_frames_than_slots(ox, out_fmt, fmt):
    """Five frames through push with padded pitches, the first output registered, the others not."""
    c = case()
    t = c["t"]
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([template(ox, t)], t["sizes"], (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])
    am.set_pixel_formats(fmt, out_fmt)
    assert am.pixel_formats == (fmt, out_fmt)
    assert am.info()["pixel_formats"] == [VALUES[fmt], int(out_fmt == "nv12")]
    outs = [host_out(W, H, out_fmt) for _ in range(5)]
    am.register_output(outs[0])
    planes = [planes_of(fmt, c, f) for f in range(5)]
    assert all(p.strides[0] > p.shape[1] for tri in planes[0] for p in tri)
    for f in range(3):
        am.push(planes[f], outs[f])
    assert am.pending() == 3
    for f in range(3, 5):  # every slot again
        assert am.pop() is outs[f - 3]
        am.push(planes[f], outs[f])
    for f in range(2, 5):
        assert am.pop() is outs[f]
    for f in range(5):
        check_host(outs[f], c["want"][f], W, H, out_fmt, (fmt, out_fmt, f))
    am.unregister_output(outs[0])
    am.close()


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_async_yuv10_uint16_planes(ox, fmt):
    """push takes planes of 16-bit words as uint16 arrays too."""
    c = case()
    t = c["t"]
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([template(ox, t)], t["sizes"], (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])
    am.set_pixel_formats(fmt, "yuv420p")
    out = host_out(W, H, "yuv420p")
    am.push([tuple(np.ascontiguousarray(p).view(np.uint16) for p in tri) for tri in planes_of(fmt, c, 1, 0)], out)
    am.pop()
    check_host(out, c["want"][1], W, H, "yuv420p", fmt)
    am.close()


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_async_yuv10_push_device_two_regions(ox, fmt):
    """Two mappers over the same inputs (one conversion for both), side by side in the merged frame; host planes
    and device frames (windows with pitch + 6, 2 bytes past a 16-byte boundary)."""
    import torch
    c = case()
    t = c["t"]
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([template(ox, t), template(ox, t)], t["sizes"], (2 * W, H), [0, 0], [0, 0],
                             [(0.0, 0.0, 0.5, 1.0), (0.5, 0.0, 0.5, 1.0)])
    am.set_pixel_formats(fmt, "yuv420p")
    want = c["want"][0]
    merged = np.empty((H * 3 // 2, 2 * W), np.uint8)  # "Y over [U|V]" of the 2 W wide frame
    merged[:H, :W], merged[:H, W:] = want[:H], want[:H]
    merged[H:, :W // 2], merged[H:, W // 2:W] = want[H:, :W // 2], want[H:, :W // 2]
    merged[H:, W:W + W // 2], merged[H:, W + W // 2:] = want[H:, W // 2:], want[H:, W // 2:]
    out = host_out(2 * W, H, "yuv420p")
    am.push(planes_of(fmt, c, 0), out)
    dout = torch.full((H * 3 // 2, 2 * W), FILL, dtype=torch.uint8, device="cuda")
    dev = []
    for p in laid(fmt, c, 0):
        rows, cols = p.shape
        buf = torch.full(((rows + 1) * (cols + 6) + 32,), FILL, dtype=torch.uint8, device="cuda")
        off = (-buf.data_ptr()) % 16 + 2
        d = buf[off:off + rows * (cols + 6)].view(rows, cols + 6)[:, :cols]
        d.copy_(torch.from_numpy(p))
        dev.append(d)
    torch.cuda.synchronize()
    am.push_device(dev, dout)
    am.pop()
    check_host(out, merged, 2 * W, H, "yuv420p", "host")
    am.pop()
    assert np.array_equal(dout.cpu().numpy(), merged)
    with pytest.raises(ValueError):  # an 8-bit-shaped tensor is not a frame of the layout
        am.push_device([torch.zeros((h * 3 // 2, w), dtype=torch.uint8, device="cuda") for w, h in t["sizes"]], dout)
    odd = [d for d in dev]
    odd[0] = torch.zeros((dev[0].shape[0], dev[0].shape[1] + 1), dtype=torch.uint8, device="cuda")[:, 1:]
    with pytest.raises(ox.OctvrError):  # an odd base address
        am.push_device(odd, dout)
    assert am.pending() == 0
    am.close()


_RING = {}


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_async_yuv10_byte_path(ox, fmt):
    """324-wide inputs (w % 8 == 4): every group takes the per-sample path, the last group of a row is partial and the
    composite has wide (gathered) tiles.  The device frames hold a pattern outside the footprint, so a used byte
    that was not uploaded shows as a mismatch."""
    from octvr_amd import synthetic
    n, in_w, in_h, W, H = 5, 324, 240, 512, 256
    if not _RING:
        rig = synthetic.fisheye_rig(in_w, in_h, [2 * math.pi * k / n for k in range(n)], [0.35 * (-1) ** k for k in range(n)])
        mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
        t = dict(W=W, H=H, n=n, sizes=[(in_w, in_h)] * n, rois=[], maps1=[], maps2=[], masks=[], seams=None)
        for i in range(n):
            roi, m1, m2, mk, _ = mt.input(i)
            t["rois"].append(roi); t["maps1"].append(m1); t["maps2"].append(m2); t["masks"].append(mk)
        pics = [pictures(t, 4500 + 10 * f) for f in range(2)]
        frames = [[R10.frame8(p) for p in s] for s in pics]
        _RING.update(mt=mt, t=t, pics=pics, frames=frames, want=[oracle(t, fr, enable_gain=True) for fr in frames])
    c = _RING
    am = ox.AsyncMultiMapper([c["mt"]], c["t"]["sizes"], (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])
    am.set_pixel_formats(fmt, "nv12")
    outs = [host_out(W, H, "nv12") for _ in range(2)]
    for f in range(2):
        am.push(planes_of(fmt, c, f), outs[f])
    for f in range(2):
        am.pop()
        check_host(outs[f], c["want"][f], W, H, "nv12", (fmt, f))
    am.close()


def test_gpu_async_yuv10_format_switches_rebuild_the_table(ox):
    """8-bit 4:2:2 -> 10-bit 4:2:0 -> 10-bit 4:2:2 -> 8-bit 4:2:2 -> planar on one pipeline: the packed offsets are each
    format's own (4, 6, 8 and 4 bytes per pixel of a piece's row)."""
    c = case()
    t = c["t"]
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([template(ox, t)], t["sizes"], (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])

    def nv16_planes(f):  # the 8-bit frames by the 8-bit out rule: every chroma row twice
        out = []
        for f8, (w, h) in zip(c["frames"][f], t["sizes"]):
            uv = np.empty((h, w), np.uint8)
            uv[:, 0::2] = np.repeat(f8[h:, :w // 2], 2, axis=0)
            uv[:, 1::2] = np.repeat(f8[h:, w // 2:], 2, axis=0)
            out.append((np.ascontiguousarray(f8[:h]), uv))
        return out
    steps = [("nv16", 0), ("yuv420p10", 1), ("p010", 2), ("p210", 3), ("yuv422p10", 4), ("nv16", 1), ("p010", 0)]
    for fmt, f in steps:
        am.set_pixel_formats(fmt, "yuv420p")
        assert am.pixel_formats == (fmt, "yuv420p")
        out = host_out(W, H, "yuv420p")
        am.push(nv16_planes(f) if fmt == "nv16" else planes_of(fmt, c, f), out)
        am.pop()
        check_host(out, c["want"][f], W, H, "yuv420p", (fmt, f))
    am.set_pixel_formats("yuv420p", "yuv420p")
    out = host_out(W, H, "yuv420p")
    am.push([(fr[:h, :w], fr[h:, :w // 2], fr[h:, w // 2:]) for fr, (w, h) in zip(c["frames"][2], t["sizes"])], out)
    am.pop()
    check_host(out, c["want"][2], W, H, "yuv420p", "planar after the 10-bit formats")
    am.close()


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_async_yuv10_errors(ox, fmt):
    c = case()
    t = c["t"]
    W, H = t["W"], t["H"]
    val = VALUES[fmt]
    am = ox.AsyncMultiMapper([template(ox, t)], t["sizes"], (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])
    lib = ox.lib()
    E_INVALID, E_UNSUPPORTED = -1, lib.octvr_async_set_pixel_formats(am._h, 0, 16)
    assert E_UNSUPPORTED not in (0, E_INVALID)
    am.set_pixel_formats("nv12", "nv12")
    assert lib.octvr_async_set_pixel_formats(am._h, 0, val) == E_UNSUPPORTED
    assert lib.octvr_async_set_pixel_formats(am._h, val, val) == E_UNSUPPORTED
    with pytest.raises(ox.OctvrError) as e:
        am.set_pixel_formats("yuv420p", fmt)
    assert e.value.code == E_UNSUPPORTED and "output" in str(e.value)
    assert am.pixel_formats == ("nv12", "nv12"), "a rejected call changes nothing"
    for bad in (2, 7, -1, 15, 20):
        assert lib.octvr_async_set_pixel_formats(am._h, bad, 0) == E_INVALID
        assert lib.octvr_async_set_pixel_formats(am._h, val, bad) == E_INVALID
    assert am.pixel_formats == ("nv12", "nv12")
    am.set_pixel_formats(fmt, "yuv420p")
    out = host_out(W, H, "yuv420p")
    good = planes_of(fmt, c, 0, 0)
    for k in range(len(good[0])):  # each plane of the layout narrower than required, or at an odd pitch
        for cut in (2, 1):
            bad_planes = [tuple(np.ascontiguousarray(p[:, :-cut]) if j == k else p for j, p in enumerate(tri)) for tri in good]
            with pytest.raises(ox.OctvrError):
                am.push(bad_planes, out)
    assert am.pending() == 0
    am.push(good, out)
    with pytest.raises(ox.OctvrError):  # a format change with a frame pending is refused
        am.set_pixel_formats("nv12", "yuv420p")
    am.pop()
    check_host(out, c["want"][0], W, H, "yuv420p", "after the refused calls")
    am.close()


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_async_yuv10_debug_pack_runs(ox, fmt):
    """octvr_debug_pack_runs for the layout: a run is its two luma rows, then its chroma row(s) in the layout's order,
    6 or 8 bytes per pixel of the run (the last group of a 330 wide row is 2 pixels)."""
    w, h = 330, 8
    rng = np.random.RandomState(31)
    crows = h if R10.is422(fmt) else h // 2
    frame = R10.lay_out(fmt, rng.randint(0, 1024, (h, w)), rng.randint(0, 1024, (crows, w // 2)),
                        rng.randint(0, 1024, (crows, w // 2)), seed=3)
    runs = [(0, 1, 3, 2), (0, 3, 40, 2), (0, 0, 0, 42)]
    packed, sizes = ox.debug_pack_runs([(w, h)], runs, [host_planes(fmt, frame, w, h)], fmt)
    want = []
    for _, rp, g0, ng in runs:
        x0, x1 = 8 * g0, min(8 * (g0 + ng), w)
        want += [frame[r, 2 * x0:2 * x1] for r in (2 * rp, 2 * rp + 1)]
        for r in ((2 * rp, 2 * rp + 1) if R10.is422(fmt) else (rp,)):
            if R10.planar(fmt):
                want += [frame[h + r, x0:x1], frame[h + r, w + x0:w + x1]]
            else:
                want.append(frame[h + r, 2 * x0:2 * x1])
    assert np.array_equal(packed, np.concatenate(want))
    bpp = 8 if R10.is422(fmt) else 6
    assert sizes.tolist() == [bpp * (min(8 * (g0 + ng), w) - 8 * g0) for _, _, g0, ng in runs]
