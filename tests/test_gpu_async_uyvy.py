"""Packed UYVY 4:2:2 inputs of the AsyncMultiMapper pipeline (octvr_async_set_pixel_formats with
OCTVR_PIX_UYVY422 as the input format): push packs and uploads the footprint runs of the packed rows, push_device
converts the caller's device frames, and the mappers stitch the pipeline's 4:2:0 frames.  The expected bytes are
the oracle's stitch of the frames converted by this file's own numpy (the input rule: chroma rows averaged with
rounding up, luma copied)."""
import copy
import json

import numpy as np
import pytest

import oracle_py as O

pytestmark = pytest.mark.gpu

FILL = 0x5A


def unpack_rule(p, w, h):
    f = np.empty((h * 3 // 2, w), np.uint8)
    f[:h] = p[:, 1:2 * w:2]
    u = p[:, 0:2 * w:4].astype(np.int32)
    v = p[:, 2:2 * w:4].astype(np.int32)
    f[h:, :w // 2] = (u[0::2] + u[1::2] + 1) >> 1
    f[h:, w // 2:] = (v[0::2] + v[1::2] + 1) >> 1
    return f


def noise_packed(w, h, seed):
    from octvr_amd import synthetic
    p = np.empty((h, 2 * w), np.uint8)
    p[:, 1::2] = synthetic.smooth_yuv_frame(w, h, seed)[:h, :w]
    p[:, 0::2] = np.random.RandomState(seed).randint(0, 256, (h, w), dtype=np.int64).astype(np.uint8)
    return p


@pytest.fixture(scope="module")
def ox(product_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    assert hasattr(product_lib, "PIX_UYVY422"), "OCTVR_PIX_UYVY422 is missing"
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
    """Four packed frame sets of rigA, the converted frames and the oracle's planar stitches."""
    if not _CASE:
        t = golden("rigA")
        packed = [[noise_packed(w, h, 100 * f + i) for i, (w, h) in enumerate(t["sizes"])] for f in range(4)]
        frames = [[unpack_rule(p, w, h) for p, (w, h) in zip(s, t["sizes"])] for s in packed]
        _CASE.update(t=t, packed=packed, frames=frames, want=[oracle(t, fr, enable_gain=True) for fr in frames])
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


def padded(p, pad=6):
    """The packed plane inside an array of pitch 2 W + pad."""
    a = np.full((p.shape[0], p.shape[1] + pad), 0xC3, np.uint8)
    a[:, :p.shape[1]] = p
    return a[:, :p.shape[1]]


@pytest.mark.parametrize("out_fmt", ["yuv420p", "nv12"])
def test_gpu_async_uyvy_push_three_pending(ox, out_fmt):
    c = case()
    t = c["t"]
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([template(ox, t)], t["sizes"], (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])
    am.set_pixel_formats("uyvy422", out_fmt)
    assert am.pixel_formats == ("uyvy422", out_fmt)
    assert am.info()["pixel_formats"] == [16, int(out_fmt == "nv12")]
    outs = [host_out(W, H, out_fmt) for _ in range(3)]
    for f in range(3):
        am.push([(padded(p),) for p in c["packed"][f]], outs[f])
    assert am.pending() == 3
    for f in range(3):
        assert am.pop() is outs[f]
        check_host(outs[f], c["want"][f], W, H, out_fmt, (out_fmt, f))
    am.close()


def test_gpu_async_uyvy_push_device_behind_ready_and_mixed(ox):
    """Device frames written on a side stream, the stitch behind their `ready` event; then host and device
    frames mixed on the same pipeline."""
    import torch
    c = case()
    t = c["t"]
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([template(ox, t)], t["sizes"], (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])
    am.set_pixel_formats("uyvy422", "yuv420p")
    side = torch.cuda.Stream()
    staged = [[torch.from_numpy(p).pin_memory() for p in s] for s in c["packed"]]
    dev = [[torch.empty((p.shape[0], p.shape[1] + 6), dtype=torch.uint8, device="cuda")[:, :p.shape[1]] for p in s]
           for s in c["packed"]]
    douts = [torch.full((H * 3 // 2, W), FILL, dtype=torch.uint8, device="cuda") for _ in range(4)]
    houts = {1: host_out(W, H, "yuv420p"), 3: host_out(W, H, "yuv420p")}
    torch.cuda.synchronize()
    for f in range(4):
        if f in houts:  # mixed: a host frame between the device frames
            am.push([(p,) for p in c["packed"][f]], houts[f])
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
            check_host(houts[f], c["want"][f], W, H, "yuv420p", f)
        else:
            assert got is douts[f]
            assert np.array_equal(douts[f].cpu().numpy(), c["want"][f]), f
    with pytest.raises(ValueError):  # a 4:2:0-shaped tensor is not a packed frame
        am.push_device([torch.zeros((h * 3 // 2, w), dtype=torch.uint8, device="cuda") for w, h in t["sizes"]], douts[0])
    am.close()


def test_gpu_async_uyvy_two_regions(ox):
    """Two mappers over the same packed inputs (one conversion for both), side by side in the merged frame; host
    planes and device frames."""
    import torch
    c = case()
    t = c["t"]
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([template(ox, t), template(ox, t)], t["sizes"], (2 * W, H), [0, 0], [0, 0],
                             [(0.0, 0.0, 0.5, 1.0), (0.5, 0.0, 0.5, 1.0)])
    am.set_pixel_formats("uyvy422", "yuv420p")
    want = c["want"][0]
    merged = np.empty((H * 3 // 2, 2 * W), np.uint8)  # "Y over [U|V]" of the 2 W wide frame
    merged[:H, :W], merged[:H, W:] = want[:H], want[:H]
    merged[H:, :W // 2], merged[H:, W // 2:W] = want[H:, :W // 2], want[H:, :W // 2]
    merged[H:, W:W + W // 2], merged[H:, W + W // 2:] = want[H:, W // 2:], want[H:, W // 2:]
    out = host_out(2 * W, H, "yuv420p")
    am.push([(p,) for p in c["packed"][0]], out)
    dout = torch.full((H * 3 // 2, 2 * W), FILL, dtype=torch.uint8, device="cuda")
    am.push_device([torch.from_numpy(p).cuda() for p in c["packed"][0]], dout)
    am.pop()
    check_host(out, merged, 2 * W, H, "yuv420p", "host")
    am.pop()
    assert np.array_equal(dout.cpu().numpy(), merged)
    am.close()


def test_gpu_async_uyvy_overlay_rig(ox):
    import camera_rigs as R
    import overlay_ref as OR
    rig = copy.deepcopy(R.mask_rigs()["overlay_include"])
    W, H = 512, 256
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
    tt = OR.prepare(mt, 0)
    sizes = [(640, 360)] * len(rig["inputs"]) + [(192, 128)]
    packed = [noise_packed(w, h, 60 + i) for i, (w, h) in enumerate(sizes)]
    frames = [unpack_rule(p, w, h) for p, (w, h) in zip(packed, sizes)]
    want = OR.expected(tt, frames, sizes, blend=0, enable_gain=True)[0]
    am = ox.AsyncMultiMapper([mt], sizes, (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])
    am.set_pixel_formats("uyvy422", "yuv420p")
    out = host_out(W, H, "yuv420p")
    am.push([(p,) for p in packed], out)
    am.pop()
    check_host(out, want, W, H, "yuv420p", "overlay")
    am.close()


def test_gpu_async_uyvy_errors(ox):
    c = case()
    t = c["t"]
    W, H = t["W"], t["H"]
    am = ox.AsyncMultiMapper([template(ox, t)], t["sizes"], (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)])
    lib = ox.lib()
    E_INVALID, E_UNSUPPORTED = -1, lib.octvr_async_set_pixel_formats(am._h, 0, 16)
    assert E_UNSUPPORTED not in (0, E_INVALID), "UYVY as the pipeline's output format is unsupported, not invalid"
    with pytest.raises(ox.OctvrError) as e:
        am.set_pixel_formats("yuv420p", "uyvy422")
    assert e.value.code == E_UNSUPPORTED and "output" in str(e.value)
    for bad in (2, 7, -1):
        assert lib.octvr_async_set_pixel_formats(am._h, bad, 0) == E_INVALID
        assert lib.octvr_async_set_pixel_formats(am._h, 16, bad) == E_INVALID
    assert am.pixel_formats == ("yuv420p", "yuv420p"), "a rejected call changes nothing"
    am.set_pixel_formats("uyvy422", "yuv420p")
    out = host_out(W, H, "yuv420p")
    with pytest.raises(ox.OctvrError):  # a plane narrower than 2 W
        am.push([(np.ascontiguousarray(p[:, :-2]),) for p in c["packed"][0]], out)
    am.push([(p,) for p in c["packed"][0]], out)
    with pytest.raises(ox.OctvrError):  # a format change with a frame pending is refused
        am.set_pixel_formats("nv12", "yuv420p")
    assert am.pixel_formats == ("uyvy422", "yuv420p")
    am.pop()
    check_host(out, c["want"][0], W, H, "yuv420p", "after the refused calls")
    am.set_pixel_formats("yuv420p", "yuv420p")  # and back: planar planes again
    f = c["frames"][1]
    out = host_out(W, H, "yuv420p")
    am.push([(fr[:h, :w], fr[h:, :w // 2], fr[h:, w // 2:]) for fr, (w, h) in zip(f, t["sizes"])], out)
    am.pop()
    check_host(out, c["want"][1], W, H, "yuv420p", "planar after UYVY")
    am.close()
