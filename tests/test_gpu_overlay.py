"""Mapper over templates with overlays (camera N + k = overlay k's live frame), bit-exact against
tests/overlay_ref.py: blend 0 (the overlays are the tail of the composite LUT), multi-band and feather
(overlay_apply_kernel onto the result frame), with gain, vignette, NV12, the texture mode, scaled output,
preview, frames in flight and batches.  Output 512 x 256, inputs 640 x 360, overlay frames of other sizes."""
import copy
import json

import numpy as np
import pytest

import camera_rigs as R
import oracle_py as O
import overlay_ref as OR

pytestmark = pytest.mark.gpu

W, H = 512, 256
FF = {"width": 640, "height": 360, "hfov": 3.4906585, "center_dx": 0.0, "center_dy": 0.0,
      "radial": [0.0, 0.0, 0.0], "crop": {"rect": [140, 500, 0, 360], "is_circular": True}}


def _fisheye(yaw, pitch=0.0, **more):
    return {"type": "fullframe_fisheye",
            "options": dict(FF, rotation={"roll": 0.0, "yaw": yaw, "pitch": pitch}, **more)}


def _overlay(yaw, pitch, pts, **more):
    return _fisheye(yaw, pitch, exclude_masks=[],
                    include_masks=[{"type": "polygonal", "args": [float(v) + 0.25 for v in pts]}], **more)


def rig_one():
    return copy.deepcopy(R.mask_rigs()["overlay_include"])


def rig_two():
    """A second overlay over the first one's."""
    rig = rig_one()
    rig["overlays"].append(_overlay(1.25, 0.1, [260, 100, 420, 140, 380, 300, 240, 260]))
    return rig


def rig_wide():
    """Four inputs a quarter radian apart (crescents of four winners inside one tile) and an overlay on them."""
    return {"output": {"type": "equirectangular", "options": {"rotation": {"roll": 0.0, "yaw": 0.1, "pitch": 0.05}}},
            "inputs": [_fisheye(0.25 * k) for k in range(4)],
            "overlays": [_overlay(1.0, 0.0, [280, 120, 380, 140, 370, 240, 290, 230])]}


def _sizes(rig, ov_sizes=((192, 128), (96, 160))):
    return [(640, 360)] * len(rig["inputs"]) + list(ov_sizes[:len(rig.get("overlays", []))])


def _frames(sizes, seed):
    return [O.rand_img(w, h * 3 // 2, 1, seed + i) for i, (w, h) in enumerate(sizes)]


def _winners(t):
    """Per output pixel the winning camera of the whole chain (-1: none) and how many overlays claim it."""
    win = -np.ones((H, W), np.int64)
    claims = np.zeros((H, W), np.int64)
    for i, (roi, m) in enumerate(zip(t["rois"], t["masks"])):
        x, y, w, h = roi
        on = np.asarray(m) != 0
        win[y:y + h, x:x + w][on] = i
        if i >= t["n"]:
            claims[y:y + h, x:x + w][on] += 1
    return win, claims


def _vig(rig, sizes):
    out = []
    for c, (w, h) in zip(rig["inputs"] + rig.get("overlays", []), sizes):
        v = O.vignette_map(c["options"])
        out.append(None if v is None else O.resize_linear_cuda_f32(v, w, h))
    return out if any(v is not None for v in out) else None


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    d = got != want
    assert got.shape == want.shape and not d.any(), (what, int(d.sum()), np.argwhere(d)[:5].tolist())


def _stitch(ox, rig, blend=0, enable_gain=True, scale=None, preview=None, remap="remap", fmts=("yuv420p", "yuv420p"),
            seed=40, mt=None):
    """One stitch of `rig` through the product and through overlay_ref; returns (mapper, template arrays)."""
    import torch
    mt = mt or ox.MapperTemplate.from_json(json.dumps(rig), W, H)
    t = OR.prepare(mt, blend)
    sizes = _sizes(rig)
    frames = _frames(sizes, seed)
    vig = _vig(rig, sizes)
    m = ox.Mapper(mt, sizes, blend=blend, enable_gain=enable_gain, scale_output=scale or (0, 0), remap=remap)
    want = OR.expected(t, frames, sizes, blend=blend, enable_gain=enable_gain, vig=vig, scale=scale, preview=preview,
                       remap_tex=remap == "texture")
    ow, oh = scale or (W, H)
    for fi, fo in ([fmts] if isinstance(fmts[0], str) else fmts):
        m.set_pixel_formats(fi, fo)
        dev = [torch.from_numpy(ox.nv12_from_yuv420p(f, w, h) if fi == "nv12" else f).cuda()
               for f, (w, h) in zip(frames, sizes)]
        out = torch.zeros((oh * 3 // 2, ow), dtype=torch.uint8, device="cuda")
        pv = torch.zeros((preview[1], preview[0], 3), dtype=torch.uint8, device="cuda") if preview else None
        m.stitch(dev, out, preview=pv)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        _same(ox.yuv420p_from_nv12(got, ow, oh) if fo == "nv12" else got, want[0], (fi, fo))
        if preview:
            _same(pv.cpu().numpy(), want[2], "preview")
        g = np.asarray(m.gains(), np.float64)
        assert len(g) == t["n"]
        _same(g.view(np.int64), np.asarray(want[1], np.float64).view(np.int64), "gains")
    return m, t


def test_gpu_overlay_blend0_gain(product_lib):
    """The overlay_include rig, blend 0, gain on: the output, and gains equal to the oracle's over the N inputs."""
    m, t = _stitch(product_lib, rig_one())
    info = m.info()
    assert info["inputs"] == 2 and info["overlays"] == 1 and info["gain"] == 1
    assert m.traffic_bytes() > 0


def test_gpu_include_mask_gains_without_overlays(product_lib):
    """No overlays: a rig whose include masks clear other inputs' masks over in-image pixels
    (include_arbitration).  The feed reads the warped pixel there whatever the mask says, so the gain plan must
    keep those samples: gains and output equal the oracle's."""
    rig = copy.deepcopy(R.mask_rigs()["include_arbitration"])
    m, t = _stitch(product_lib, rig)
    assert t["k"] == 0 and m.info()["gain"] == 1
    cleared = sum(int(((np.asarray(mk) == 0) & (m1 >= 0) & (m1 < 1) & (m2 >= 0) & (m2 < 1)).sum())
                  for mk, m1, m2 in zip(t["masks"], t["map1"], t["map2"]))
    assert cleared > 0, "the rig has no masked-out pixel with an in-image map value"


def test_gpu_overlay_two_overlapping(product_lib):
    """Two overlays that overlap each other, cross an item boundary (x a multiple of 128, y of 16) and leave
    partly covered chroma quads."""
    ox = product_lib
    rig = rig_two()
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
    t = OR.prepare(mt)
    win, claims = _winners(t)
    ov = win >= t["n"]
    q = ov.reshape(H // 2, 2, W // 2, 2).sum(axis=(1, 3))
    assert ((q > 0) & (q < 4)).any(), "no partly covered chroma quad"
    assert (claims > 1).any(), "no pixel claimed by both overlays"
    on = claims > 0
    assert (on[:, 127] & on[:, 128]).any() and (on[15] & on[16]).any(), "no item boundary crossed"
    assert (win == t["n"]).any() and (win == t["n"] + 1).any(), "an overlay wins nothing"
    _stitch(ox, rig, mt=mt)


def test_gpu_overlay_wide_tile(product_lib):
    """Four overlapping inputs plus an overlay inside one 128 x 8 tile: a wide tile holds overlay pixels."""
    ox = product_lib
    rig = rig_wide()
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
    t = OR.prepare(mt)
    win, _ = _winners(t)
    wide = 0
    for ty in range(H // 8):
        for tx in range(W // 128):
            u = set(np.unique(win[ty * 8:ty * 8 + 8, tx * 128:tx * 128 + 128]).tolist()) - {-1}
            wide += len(u) > 4 and any(c >= t["n"] for c in u)
    assert wide > 0, "no tile with five winners, the overlay among them"
    m, _ = _stitch(ox, rig, mt=mt)
    assert m.info()["wide_tiles"] >= wide


def test_gpu_overlay_vignette(product_lib):
    rig = rig_one()
    rig["overlays"][0]["options"]["vignette"] = [1.1, -0.35, 0.12, -0.04]
    rig["inputs"][1]["options"]["vignette"] = [1.0, -0.3, 0.1, -0.03]
    _stitch(product_lib, rig)


def test_gpu_overlay_single_input(product_lib):
    """N = 1 with an overlay: gain and blend are off whatever was asked for (mapper.cpp:78-82)."""
    rig = rig_one()
    del rig["inputs"][1]
    m, t = _stitch(product_lib, rig, blend=5, enable_gain=True)
    assert m.info()["blend"] == 0 and m.info()["gain"] == 0 and m.gains() == [1.0]


def test_gpu_overlay_dat_round_trip(product_lib, tmp_path):
    ox = product_lib
    rig = rig_two()
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
    p = tmp_path / "ov.dat"
    mt.dump(str(p))
    back = ox.MapperTemplate.load(str(p))
    assert back.num_overlays == 2
    _stitch(ox, rig, mt=back)


def test_gpu_overlay_nv12_pairs(product_lib):
    """All four format pairs on one mapper, overlay frames included."""
    _stitch(product_lib, rig_two(), fmts=[(a, b) for a in ("yuv420p", "nv12") for b in ("yuv420p", "nv12")])


def test_gpu_overlay_texture_mode(product_lib):
    _stitch(product_lib, rig_one(), remap="texture")


def test_gpu_overlay_scaled_preview_blend0(product_lib):
    """Scaled output 384 x 192 and a preview of 200 x 100 (an odd split), from the patched result."""
    _stitch(product_lib, rig_two(), scale=(384, 192), preview=(200, 100))
    _stitch(product_lib, rig_one(), preview=(200, 100))


def test_gpu_overlay_inflight_and_batch(product_lib):
    """Blend 0: three frames in flight on their own streams, and a batch of two; every frame has its own overlay
    frame and its own expected output."""
    import torch
    ox = product_lib
    rig = rig_one()
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
    t = OR.prepare(mt)
    sizes = _sizes(rig)
    sets = [_frames(sizes, 500 + 10 * f) for f in range(3)]
    want = [OR.expected(t, fr, sizes) for fr in sets]
    m = ox.Mapper(mt, sizes, blend=0, enable_gain=True)
    m.set_frames_in_flight(3)
    dev = [[torch.from_numpy(a).cuda() for a in fr] for fr in sets]
    outs = [torch.zeros((H * 3 // 2, W), dtype=torch.uint8, device="cuda") for _ in range(3)]
    streams = [torch.cuda.Stream() for _ in range(3)]
    torch.cuda.synchronize()
    for f in range(3):
        m.stitch(dev[f], outs[f], stream=streams[f])
    torch.cuda.synchronize()
    for f in range(3):
        _same(outs[f].cpu().numpy(), want[f][0], ("in flight", f))
    for o in outs:
        o.zero_()
    m.stitch_batch(dev[:2], outs[:2])
    torch.cuda.synchronize()
    for f in range(2):
        _same(outs[f].cpu().numpy(), want[f][0], ("batch", f))
    _same(np.asarray(m.gains()).view(np.int64), np.asarray(want[1][1]).view(np.int64), "gains of the last frame")


@pytest.mark.parametrize("blend", [5, -4])
@pytest.mark.parametrize("two", [False, True])
def test_gpu_overlay_blended(product_lib, blend, two):
    """Multi-band (5) and feather (-4) with one and two overlays: overlay_apply_kernel after the blend; planar
    and NV12 output, NV12 input."""
    ox = product_lib
    m, t = _stitch(ox, rig_two() if two else rig_one(), blend=blend,
                   fmts=[("yuv420p", "yuv420p"), ("yuv420p", "nv12"), ("nv12", "yuv420p")])
    info = m.info()
    assert info["blend"] == blend and info["overlays"] == (2 if two else 1)
    assert info["overlay_groups"] > 0 and info["overlay_groups"] % 32 == 0
    _, claims = _winners(t)
    assert info["overlay_px"] == int((claims > 0).sum())
    with pytest.raises(ox.OctvrError) as e:
        m.set_frames_in_flight(2)
    assert e.value.code == ox.E_UNSUPPORTED


@pytest.mark.parametrize("blend", [5, -4])
def test_gpu_overlay_blended_scaled_preview(product_lib, blend):
    _stitch(product_lib, rig_two(), blend=blend, scale=(384, 192), preview=(200, 100))


def test_gpu_overlay_blended_texture_vignette(product_lib):
    rig = rig_one()
    rig["overlays"][0]["options"]["vignette"] = [1.1, -0.35, 0.12, -0.04]
    _stitch(product_lib, rig, blend=5, remap="texture")


def test_gpu_overlay_errors(product_lib):
    import torch
    ox = product_lib
    rig = rig_one()
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
    sizes = _sizes(rig)
    for bad, word in ((sizes[:2], "overlay"), (sizes + [(64, 64)], "overlay"), (sizes[:2] + [(191, 128)], "even")):
        with pytest.raises(ox.OctvrError) as e:
            ox.Mapper(mt, bad, blend=0, enable_gain=True)
        assert e.value.code == ox.E_INVALID and word in str(e.value), bad
    m = ox.Mapper(mt, sizes, blend=0, enable_gain=True)
    dev = [torch.from_numpy(f).cuda() for f in _frames(sizes, 7)]
    out = torch.zeros((H * 3 // 2, W), dtype=torch.uint8, device="cuda")
    with pytest.raises(ox.OctvrError) as e:
        m.stitch(dev, out, gains=[1.0] * 3)  # n_gains = N + K
    assert e.value.code == ox.E_INVALID
    m.stitch(dev, out, gains=[1.0, 1.1])
    torch.cuda.synchronize()
