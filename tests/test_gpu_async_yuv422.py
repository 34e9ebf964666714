"""YUYV, planar YUV422P and NV16 inputs of the AsyncMultiMapper pipeline (octvr_async_set_pixel_formats with
OCTVR_PIX_YUYV422 / _YUV422P / _NV16 as the input format): push packs and uploads the footprint runs of the host
planes, push_device converts the caller's device frames, and the mappers stitch the pipeline's 4:2:0 frames.  The
expected bytes are the oracle's stitch of the frames converted by this file's own numpy (the input rule: chroma
rows averaged with rounding up, luma copied); the pictures are made as (Y, U, V) planes, so one oracle stitch
serves the three layouts."""
import copy
import json

import numpy as np
import pytest

import oracle_py as O

pytestmark = pytest.mark.gpu

FILL = 0x5A
LAYOUTS = ["yuyv422", "yuv422p", "nv16"]
VALUES = {"yuyv422": 17, "yuv422p": 18, "nv16": 19}


def in_rule(y, u, v):
    """in rule on the 4:2:2 planes -> "Y over [U|V]"."""
    h, w = y.shape
    f = np.empty((h * 3 // 2, w), np.uint8)
    f[:h] = y
    u, v = u.astype(np.int32), v.astype(np.int32)
    f[h:, :w // 2] = (u[0::2] + u[1::2] + 1) >> 1
    f[h:, w // 2:] = (v[0::2] + v[1::2] + 1) >> 1
    return f


def noise_yuv(w, h, seed):
    from octvr_amd import synthetic
    c = np.random.RandomState(seed).randint(0, 256, (h, w), dtype=np.int64).astype(np.uint8)
    return synthetic.smooth_yuv_frame(w, h, seed)[:h, :w].copy(), c[:, :w // 2].copy(), c[:, w // 2:].copy()


def padded(p, pad):
    """The plane inside an array whose pitch is its width + pad."""
    a = np.full((p.shape[0], p.shape[1] + pad), 0xC3, np.uint8)
    a[:, :p.shape[1]] = p
    return a[:, :p.shape[1]]


def host_planes(fmt, y, u, v, pad=6):
    """The plane tuple push() takes for the layout."""
    h, w = y.shape
    if fmt == "yuyv422":
        p = np.empty((h, 2 * w), np.uint8)
        p[:, 0::2], p[:, 1::4], p[:, 3::4] = y, u, v
        return (padded(p, pad),)
    if fmt == "yuv422p":
        return (padded(y, pad), padded(u, pad // 2), padded(v, pad // 2 + 1))
    uv = np.empty((h, w), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = u, v
    return (padded(y, pad), padded(uv, pad))


def frame(fmt, y, u, v):
    """The whole frame of the layout, as push_device (and the Mapper) takes it."""
    h, w = y.shape
    if fmt == "yuyv422":
        return np.ascontiguousarray(host_planes(fmt, y, u, v, 0)[0])
    p = np.empty((2 * h, w), np.uint8)
    p[:h] = y
    if fmt == "yuv422p":
        p[h:, :w // 2], p[h:, w // 2:] = u, v
    else:
        p[h:, 0::2], p[h:, 1::2] = u, v
    return p


@pytest.fixture(scope="module")
def ox(product_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    assert hasattr(product_lib, "PIX_YUYV422"), "OCTVR_PIX_YUYV422 is missing"
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


_CASE = {}


def case():
    """Four picture sets of rigA as (Y, U, V) planes, the converted frames and the oracle's planar stitches."""
    if not _CASE:
        t = golden("rigA")
        yuv = [[noise_yuv(w, h, 100 * f + i) for i, (w, h) in enumerate(t["sizes"])] for f in range(4)]
        frames = [[in_rule(*p) for p in s] for s in yuv]
        _CASE.update(t=t, yuv=yuv, frames=frames, want=[oracle(t, fr, enable_gain=True) for fr in frames])
    return _CASE


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
def test_gpu_async_yuv422_push_three_pending(ox, out_fmt, fmt):
    c = case()
    t = c["t"]
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([template(ox, t)], t["sizes"], (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])
    am.set_pixel_formats(fmt, out_fmt)
    assert am.pixel_formats == (fmt, out_fmt)
    assert am.info()["pixel_formats"] == [VALUES[fmt], int(out_fmt == "nv12")]
    outs = [host_out(W, H, out_fmt) for _ in range(3)]
    for f in range(3):
        am.push([host_planes(fmt, *p) for p in c["yuv"][f]], outs[f])
    assert am.pending() == 3
    for f in range(3):
        assert am.pop() is outs[f]
        check_host(outs[f], c["want"][f], W, H, out_fmt, (fmt, out_fmt, f))
    am.close()


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_async_yuv422_push_device_behind_ready_and_mixed(ox, fmt):
    """Device frames written on a side stream, the stitch behind their `ready` event; then host and device
    frames mixed on the same pipeline."""
    import torch
    c = case()
    t = c["t"]
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([template(ox, t)], t["sizes"], (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])
    am.set_pixel_formats(fmt, "yuv420p")
    side = torch.cuda.Stream()
    whole = [[frame(fmt, *p) for p in s] for s in c["yuv"]]
    staged = [[torch.from_numpy(p).pin_memory() for p in s] for s in whole]
    dev = [[torch.empty((p.shape[0], p.shape[1] + 6), dtype=torch.uint8, device="cuda")[:, :p.shape[1]] for p in s]
           for s in whole]
    douts = [torch.full((H * 3 // 2, W), FILL, dtype=torch.uint8, device="cuda") for _ in range(4)]
    houts = {1: host_out(W, H, "yuv420p"), 3: host_out(W, H, "yuv420p")}
    torch.cuda.synchronize()
    for f in range(4):
        if f in houts:  # mixed: a host frame between the device frames
            am.push([host_planes(fmt, *p) for p in c["yuv"][f]], houts[f])
            continue
        ev = torch.cuda.Event()
        with torch.cuda.stream(side):
            for d, s in zip(dev[f], staged[f]):
                d.copy_(s, non_blocking=True)
            ev.record(side)
        am.push_device(dev[f], douts[f], ready=ev)
    for f in range(4):
        got = am.pop()
        if f in houts:
            assert got is houts[f]
            check_host(houts[f], c["want"][f], W, H, "yuv420p", (fmt, f))
        else:
            assert got is douts[f]
            assert np.array_equal(douts[f].cpu().numpy(), c["want"][f]), (fmt, f)
    with pytest.raises(ValueError):  # a 4:2:0-shaped tensor is not a frame of the layout
        am.push_device([torch.zeros((h * 3 // 2, w), dtype=torch.uint8, device="cuda") for w, h in t["sizes"]], douts[0])
    am.close()


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_async_yuv422_two_regions(ox, fmt):
    """Two mappers over the same inputs (one conversion for both), side by side in the merged frame; host planes
    and device frames."""
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
    am.push([host_planes(fmt, *p) for p in c["yuv"][0]], out)
    dout = torch.full((H * 3 // 2, 2 * W), FILL, dtype=torch.uint8, device="cuda")
    am.push_device([torch.from_numpy(frame(fmt, *p)).cuda() for p in c["yuv"][0]], dout)
    am.pop()
    check_host(out, merged, 2 * W, H, "yuv420p", "host")
    am.pop()
    assert np.array_equal(dout.cpu().numpy(), merged)
    am.close()


_OVERLAY = {}


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_async_yuv422_overlay_rig(ox, fmt):
    import camera_rigs as R
    import overlay_ref as OR
    rig = copy.deepcopy(R.mask_rigs()["overlay_include"])
    W, H = 512, 256
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
    sizes = [(640, 360)] * len(rig["inputs"]) + [(192, 128)]
    if not _OVERLAY:
        yuv = [noise_yuv(w, h, 60 + i) for i, (w, h) in enumerate(sizes)]
        frames = [in_rule(*p) for p in yuv]
        _OVERLAY.update(yuv=yuv, want=OR.expected(OR.prepare(mt, 0), frames, sizes, blend=0, enable_gain=True)[0])
    am = ox.AsyncMultiMapper([mt], sizes, (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])
    am.set_pixel_formats(fmt, "yuv420p")
    out = host_out(W, H, "yuv420p")
    am.push([host_planes(fmt, *p) for p in _OVERLAY["yuv"]], out)
    am.pop()
    check_host(out, _OVERLAY["want"], W, H, "yuv420p", "overlay")
    am.close()


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_async_yuv422_errors(ox, fmt):
    c = case()
    t = c["t"]
    W, H = t["W"], t["H"]
    val = VALUES[fmt]
    am = ox.AsyncMultiMapper([template(ox, t)], t["sizes"], (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])
    lib = ox.lib()
    E_INVALID, E_UNSUPPORTED = -1, lib.octvr_async_set_pixel_formats(am._h, 0, 16)
    assert E_UNSUPPORTED not in (0, E_INVALID), "UYVY as the pipeline's output format stays unsupported, not invalid"
    assert lib.octvr_async_set_pixel_formats(am._h, 0, val) == E_UNSUPPORTED
    assert lib.octvr_async_set_pixel_formats(am._h, val, val) == E_UNSUPPORTED
    with pytest.raises(ox.OctvrError) as e:
        am.set_pixel_formats("yuv420p", fmt)
    assert e.value.code == E_UNSUPPORTED and "output" in str(e.value)
    for bad in (2, 7, -1):
        assert lib.octvr_async_set_pixel_formats(am._h, bad, 0) == E_INVALID
        assert lib.octvr_async_set_pixel_formats(am._h, val, bad) == E_INVALID
    assert am.pixel_formats == ("yuv420p", "yuv420p"), "a rejected call changes nothing"
    am.set_pixel_formats(fmt, "yuv420p")
    out = host_out(W, H, "yuv420p")
    good = [host_planes(fmt, *p, pad=0) for p in c["yuv"][0]]
    for k in range(len(good[0])):  # each plane of the layout narrower than required
        bad_planes = [tuple(np.ascontiguousarray(p[:, :-2]) if j == k else p for j, p in enumerate(tri)) for tri in good]
        with pytest.raises(ox.OctvrError):
            am.push(bad_planes, out)
    assert am.pending() == 0
    am.push(good, out)
    with pytest.raises(ox.OctvrError):  # a format change with a frame pending is refused
        am.set_pixel_formats("nv12", "yuv420p")
    assert am.pixel_formats == (fmt, "yuv420p")
    am.pop()
    check_host(out, c["want"][0], W, H, "yuv420p", "after the refused calls")
    am.set_pixel_formats("yuv420p", "yuv420p")  # and back: planar planes again
    f = c["frames"][1]
    out = host_out(W, H, "yuv420p")
    am.push([(fr[:h, :w], fr[h:, :w // 2], fr[h:, w // 2:]) for fr, (w, h) in zip(f, t["sizes"])], out)
    am.pop()
    check_host(out, c["want"][1], W, H, "yuv420p", "planar after 4:2:2")
    am.close()


@pytest.mark.parametrize("fmt", LAYOUTS)
def test_gpu_async_yuv422_debug_pack_runs(ox, fmt):
    """octvr_debug_pack_runs for the layout: a run is its two luma rows, then its two chroma rows in the layout's
    order, 4 bytes per pixel of the run (the last group of a 330 wide row is 2 pixels)."""
    w, h = 330, 8
    y, u, v = noise_yuv(w, h, 31)
    runs = [(0, 1, 3, 2), (0, 3, 40, 2), (0, 0, 0, 42)]
    packed, sizes = ox.debug_pack_runs([(w, h)], runs, [host_planes(fmt, y, u, v)], fmt)
    want = []
    for _, rp, g0, ng in runs:
        x0, x1 = 8 * g0, min(8 * (g0 + ng), w)
        rows = (2 * rp, 2 * rp + 1)
        if fmt == "yuyv422":
            whole = frame(fmt, y, u, v)
            want += [whole[r, 2 * x0:2 * x1] for r in rows]
            continue
        want += [y[r, x0:x1] for r in rows]
        for r in rows:
            if fmt == "yuv422p":
                want += [u[r, x0 // 2:x1 // 2], v[r, x0 // 2:x1 // 2]]
            else:
                uv = np.empty(w, np.uint8)
                uv[0::2], uv[1::2] = u[r], v[r]
                want.append(uv[x0:x1])
    assert np.array_equal(packed, np.concatenate(want))
    assert sizes.tolist() == [4 * (min(8 * (g0 + ng), w) - 8 * g0) for _, _, g0, ng in runs]
