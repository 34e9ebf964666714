"""The blend = 0 composite with 8-byte quad records (kernels.hpp kItemPacked): items whose every quad qualifies are
stored as one record per lane quad and half, the others keep their 4-byte entries, and the composite's
instance for such a LUT branches per item.  Whatever the entry format, every output and every estimated gain
must equal the oracle's Mapper::stitch bit for bit: with the records on by default, packed wherever an item
qualifies (OCTVR_ENTRY_QUAD=1: also rigs with few qualifying items, whose unpacked items then run beside the
packed ones) and forced off (OCTVR_ENTRY_QUAD=0), with 1, 2 and 4 frames per launch, planar and NV12 frames,
estimated and caller gains."""
import json
import math

import numpy as np
import pytest

import oracle_py as O

pytestmark = pytest.mark.gpu

MODES = {"default": None, "packed": "1", "entries32": "0"}


def to_nv12(f, w, h):
    """"Y over [U|V]" -> NV12 (this file's own numpy, never the library's helpers)."""
    m = np.empty((h * 3 // 2, w), np.uint8)
    m[:h] = f[:h, :w]
    m[h:, 0::2] = f[h:, :w // 2]
    m[h:, 1::2] = f[h:, w // 2:w]
    return m


@pytest.fixture(scope="module")
def ox(product_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return product_lib


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_RIGS = {}


def rig_case(ox, name):
    """The rig's template arrays, its frames and the oracle's results, computed once and shared by the modes."""
    if name in _RIGS:
        return _RIGS[name]
    from octvr_amd import synthetic
    if name == "oversampled":
        # two 160x120 fisheyes -> 512x256: magnification below 1 away from the seams and the poles
        rig = synthetic.fisheye_rig(160, 120, [0.0, math.pi], [0.35, -0.35])
        W, H, n = 512, 256, 2
        sizes = [(160, 120)] * n
        mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
        rois, maps1, maps2, masks = [], [], [], []
        for i in range(n):
            roi, m1, m2, mk, _ = mt.input(i)
            rois.append(roi); maps1.append(m1); maps2.append(m2); masks.append(mk)
    else:
        rig, z = O.load_rig(name)
        W, H = (int(v) for v in z["out_size"])
        n = len(z["rois"])
        sizes = [(rig["inputs"][i]["options"]["width"], rig["inputs"][i]["options"]["height"]) for i in range(n)]
        rois = z["rois"].tolist()
        maps1 = [z[f"map1_{i}"] for i in range(n)]
        maps2 = [z[f"map2_{i}"] for i in range(n)]
        masks = [z[f"mask_{i}"] for i in range(n)]
    frames = [[synthetic.smooth_yuv_frame(w, h, 5100 + 11 * f + i) for i, (w, h) in enumerate(sizes)] for f in range(4)]
    given = [[0.8 + 0.05 * ((f + 2 * i) % 7) for i in range(n)] for f in range(4)]
    want_est, want_giv = [], []
    for f in range(4):
        want_est.append(O.stitch_frame(frames[f], sizes, rois, maps1, maps2, masks, W, H, enable_gain=True, gains=None,
                                       threads=8))
        want_giv.append(O.stitch_frame(frames[f], sizes, rois, maps1, maps2, masks, W, H, enable_gain=True,
                                       gains=given[f], threads=8)[0])
    _RIGS[name] = dict(W=W, H=H, n=n, sizes=sizes, rois=rois, maps1=maps1, maps2=maps2, masks=masks, frames=frames,
                       given=given, want_est=want_est, want_giv=want_giv)
    return _RIGS[name]


def make_mapper(ox, t, monkeypatch, mode):
    monkeypatch.delenv("OCTVR_ENTRY32", raising=False)
    if MODES[mode] is None:
        monkeypatch.delenv("OCTVR_ENTRY_QUAD", raising=False)
    else:
        monkeypatch.setenv("OCTVR_ENTRY_QUAD", MODES[mode])
    mt = ox.MapperTemplate.from_arrays(t["W"], t["H"], t["rois"], t["maps1"], t["maps2"], t["masks"])
    m = ox.Mapper(mt, t["sizes"], blend=0, enable_gain=True)  # the format is fixed here, at creation
    return mt, m


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["rigA", "rigB", "rigC", "rigD", "oversampled"])
def test_gpu_entry_pack_vs_oracle(ox, monkeypatch, name, mode):
    import torch
    t = rig_case(ox, name)
    W, H, sizes = t["W"], t["H"], t["sizes"]
    mt, m = make_mapper(ox, t, monkeypatch, mode)
    info = m.info()
    packable = ox.debug_tiled_lut_info(mt, sizes)["items_packable"]
    assert info["items_packable"] == packable
    if mode == "entries32":
        assert info["items_packed"] == 0
    elif mode == "packed":
        assert info["items_packed"] == packable
    else:  # by default only where more than half of the items qualify
        assert info["items_packed"] == (packable if 2 * packable > sum(info["items_by_chunks"].values()) else 0)
    m.set_frames_in_flight(4)
    for fmt in ("yuv420p", "nv12"):
        m.set_pixel_formats(fmt, fmt)
        dev = [[_cuda(to_nv12(x, w, h) if fmt == "nv12" else x) for x, (w, h) in zip(fr, sizes)] for fr in t["frames"]]
        for nb, given in ((1, False), (1, True), (2, False), (4, True)):
            outs = [torch.zeros((H * 3 // 2, W), dtype=torch.uint8, device="cuda") for _ in range(nb)]
            gains = t["given"][:nb] if given else None
            if nb == 1:
                m.stitch(dev[0], outs[0], gains=gains[0] if given else None)
            else:
                m.stitch_batch(dev[:nb], outs, gains=gains)
            g_last = np.array(m.gains())
            torch.cuda.synchronize()
            for f in range(nb):
                want = t["want_giv"][f] if given else t["want_est"][f][0]
                if fmt == "nv12":
                    want = to_nv12(want, W, H)
                got = outs[f].cpu().numpy()
                assert np.array_equal(got, want), (name, mode, fmt, nb, given, f, int((got != want).sum()))
            if not given:
                np.testing.assert_array_equal(g_last, np.array(t["want_est"][nb - 1][1]))


def test_gpu_entry_pack_both_forms_in_one_launch(ox, monkeypatch):
    """The oversampled rig holds packed and unpacked items by default (both decode forms and the per-item branch
    run in one launch), and golden rigA holds packed items next to its seam items."""
    for name in ("oversampled", "rigA"):
        t = rig_case(ox, name)
        _, m = make_mapper(ox, t, monkeypatch, "default")
        info = m.info()
        staged = sum(info["items_by_chunks"].values())
        assert 0 < info["items_packed"] < staged, (name, info["items_packed"], staged)
        # the traffic model charges a packed item 2 bytes per pixel instead of 4
        lut_b, _ = m.traffic_parts()
        _, m32 = make_mapper(ox, t, monkeypatch, "entries32")
        lut32, _ = m32.traffic_parts()
        assert lut32 - lut_b == 2.0 * 128 * 16 * info["items_packed"]
