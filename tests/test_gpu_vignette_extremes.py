"""Vignette correction at the edges of its arithmetic (multiply(rgba, vignette) = MulOpSpecial_c4 with
saturate_cast<uchar>, cudaarithm/src/cuda/mul_mat.cu:198-214; the map resized by cuda::resize INTER_LINEAR,
mapper.cpp:108-112): gains that make every second value an exact tie, that clamp, vanish, turn negative, infinite
or NaN, and steep maps in which a neighbouring pixel's gain gives another byte — through the composite's staging
(dword and byte-wise), the direct gathers (wide tiles, the gain feed's per-tap path, the prepared preview), the
multi-band remap and the feather blend, for cameras of several sizes and the composite instances no other vignette
test selects.

Every case is bit-exact against oracle_py.stitch_frame(..., vig=...): the output frame, the estimated gains and
the preview where there is one.  Frames are random bytes (oracle_py.rand_img) throughout: every channel value
occurs, YUV -> RGB itself saturates, and the estimated gains still differ between cameras (asserted), so no case
needed smooth frames.  The counts that show a case reaches its edge come from the oracle and numpy
(tests/vignette_cases.py), never from the product.

The composite instance of each case (launch_tiled_vd, composite.hip; `dw` = every frame base, pitch and width
8-aligned) is named in the case's docstring; Mapper.info() gives the staged / gathered tile split at blend 0."""
import numpy as np
import pytest

import vignette_cases as VC

pytestmark = pytest.mark.gpu

MIN_COUNT = 1000  # of the edge a family is for, over the rig's footprint
MIN_CHANGED = 0.1  # of the output's pixels, between the oracle with and without the vignette


@pytest.fixture(scope="module")
def ox(product_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return product_lib


def _cuda(frames):
    import torch
    return [torch.from_numpy(np.array(f)).cuda() for f in frames]  # a copy: the cached frames are read-only


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    d = got != want
    assert got.shape == want.shape and not d.any(), (what, int(d.sum()), np.argwhere(d)[:5].tolist())


def _same_gains(m, want, what):
    _same(np.asarray(m.gains(), np.float64).view(np.int64), np.asarray(want, np.float64).view(np.int64), (what, "gains"))


def _family(ox, name):
    return VC.template(ox, name, VC.rig_with(VC.FAMILIES[name]))


def _check_reach(key, t, frames, blend, ref, **kw):
    """What every case asserts of its expectation: the vignette changes a tenth of the output, and the estimated
    gains are finite and differ between cameras."""
    plain = VC.want((key, "plain"), t, frames, blend, vig=False, **kw)
    assert VC.changed_fraction(ref[0], plain[0], t["H"]) >= MIN_CHANGED, key
    g = np.asarray(ref[1])
    assert np.isfinite(g).all() and g.max() - g.min() > 0.05, (key, g)


def _stitch_slots(ox, t, frame_sets, blend, dev_sets=None, **kw):
    """One mapper with len(frame_sets) frames in flight: set k stitched on stream k into its own output.
    Returns (mapper, outputs)."""
    import torch
    k = len(frame_sets)
    m = ox.Mapper(t["mt"], t["sizes"], blend=blend, enable_gain=True, **kw)
    m.set_frames_in_flight(k)
    dev = dev_sets or [_cuda(fr) for fr in frame_sets]
    outs = [torch.zeros((t["H"] * 3 // 2, t["W"]), dtype=torch.uint8, device="cuda") for _ in range(k)]
    streams = [torch.cuda.Stream() for _ in range(k)]
    torch.cuda.synchronize()
    for j in range(k):
        m.stitch(dev[j], outs[j], stream=streams[j])
    torch.cuda.synchronize()
    return m, outs


# ---- 1. the constant maps are the values the families are named for --------------------------------------
def test_gpu_vignette_constant_maps_exact():
    for name, value in VC.CONSTANT.items():
        assert VC.constant_gain(getattr(VC, name.upper())) == value, name


# ---- 2. gain families -------------------------------------------------------------------------------------
@pytest.mark.parametrize("inflight", [1, 3])
@pytest.mark.parametrize("blend", [0, 16, -5])
@pytest.mark.parametrize("family", ["ties", "saturation", "pole"])
def test_gpu_vignette_family(ox, family, blend, inflight):
    """Aligned planar frames: planar <DWORD_STAGE = true, VIG = true>, MODE 0 at blend 0 (144 staged items, no
    wide tile), MODE 1 (the multi-band remap, which the feather blend shares) otherwise.  One frame in flight:
    the full gain feed; three (distinct frame sets, one per slot and stream): the lean feed's per-tap gathers."""
    t = _family(ox, family)
    sizes = tuple(t["sizes"])
    sets = [VC.random_frames(sizes, 4100 + 50 * k) for k in range(inflight)]
    refs = [VC.want((family, k), t, fr, blend) for k, fr in enumerate(sets)]
    c = VC.counts(t, sets[0])
    if family == "ties":
        assert c["ties"] >= MIN_COUNT, c
    elif family == "saturation":
        assert c["clamped"] >= MIN_COUNT, c
    else:
        assert c["odd_gains"] >= MIN_COUNT, c
        # in the resized maps themselves: negative gains past the pole, infinities and 0 * inf = NaN of the resize
        g = np.concatenate([v.reshape(-1) for v in t["vig"] if v is not None])
        assert (g < 0).sum() >= MIN_COUNT and np.isinf(g).sum() >= MIN_COUNT and np.isnan(g).sum() >= MIN_COUNT
    _check_reach(family, t, sets[0], blend, refs[0])
    m, outs = _stitch_slots(ox, t, sets, blend)
    if blend == 0:
        info = m.info()
        assert info["staged_bytes"] > 0 and info["wide_tiles"] == 0, info
    for k, (out, ref) in enumerate(zip(outs, refs)):
        _same(out.cpu().numpy(), ref[0], (family, blend, "slot", k))
    _same_gains(m, refs[-1][1], (family, blend, inflight))


# ---- 3. the map resized to cameras of several sizes -------------------------------------------------------
@pytest.mark.parametrize("blend", [0, 16])
def test_gpu_vignette_map_resize(ox, blend):
    """Steep maps on cameras of 192 x 108 (shrink), 64 x 36 (strong shrink), 520 x 300 (enlarged, width a
    multiple of 8) and 512 x 512 (1:1).  Planar <true, true>; at blend 0 the 512-wide camera's boxes exceed 256
    source columns, so its tiles are gathered by stitch_wide_kernel and the rest are staged."""
    t = VC.template(ox, "resize", VC.rig_with(VC.RESIZE_OPTIONS, VC.RESIZE_SIZES))
    base, _ = VC.oracle_vig(t["rig"])
    one = VC.RESIZE_SIZES.index((512, 512))
    assert np.array_equal(t["vig"][one].view(np.int32), base[one].view(np.int32)), "the 1:1 resize is not a copy"
    frames = VC.random_frames(tuple(t["sizes"]), 4300)
    ref = VC.want("resize", t, frames, blend)
    assert VC.neighbour_changes(t, frames) >= MIN_COUNT
    assert all(VC.footprint(t, i).sum() >= MIN_COUNT for i in range(len(t["sizes"])))
    _check_reach("resize", t, frames, blend, ref)
    m, outs = _stitch_slots(ox, t, [frames], blend)
    if blend == 0:
        info = m.info()
        assert info["wide_tiles"] > 0 and info["staged_bytes"] > 0, info
    _same(outs[0].cpu().numpy(), ref[0], ("resize", blend))
    _same_gains(m, ref[1], ("resize", blend))


# ---- 4. composite instances -------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", [0, 16, -5])
def test_gpu_vignette_unaligned_planar(ox, blend):
    """Frames at base % 8 == 2 with pitch w + 2: planar <DWORD_STAGE = false, VIG = true> (byte-wise staging with
    the float4 gain loads), MODE 0 and MODE 1.  The ties rig: same expectation as the aligned case."""
    t = _family(ox, "ties")
    frames = VC.random_frames(tuple(t["sizes"]), 4100)
    ref = VC.want(("ties", 0), t, frames, blend)
    assert VC.counts(t, frames)["ties"] >= MIN_COUNT and VC.neighbour_changes(t, frames) >= MIN_COUNT
    _check_reach("ties", t, frames, blend, ref)
    dev = VC.unaligned(frames, t["sizes"])
    for v, (w, h) in zip(dev, t["sizes"]):
        assert v.data_ptr() % 8 == 2 and v.stride(0) == w + 2
    m, outs = _stitch_slots(ox, t, [frames], blend, dev_sets=[dev])
    assert m.pixel_formats == ("yuv420p", "yuv420p")
    _same(outs[0].cpu().numpy(), ref[0], ("unaligned", blend))
    _same_gains(m, ref[1], ("unaligned", blend))


def test_gpu_vignette_unaligned_texture(ox):
    """The same unaligned frames with remap="texture", blend 0: stitch_tiled_tex_kernel <false, 0, true> for the
    staged items (140 of rigB's) and the gathers with clamped texture taps for the tiles on the image edges."""
    t = _family(ox, "ties")
    frames = VC.random_frames(tuple(t["sizes"]), 4100)
    ref = VC.want(("ties", 0, "tex"), t, frames, 0, remap_tex=True)
    assert (ref[0] != VC.want(("ties", 0), t, frames, 0)[0]).any()  # another sampling than the default's
    _check_reach("ties", t, frames, 0, ref, remap_tex=True)
    m, outs = _stitch_slots(ox, t, [frames], 0, dev_sets=[VC.unaligned(frames, t["sizes"])], remap="texture")
    info = m.info()
    assert info["wide_tiles"] > 0 and info["staged_bytes"] > 0, info
    _same(outs[0].cpu().numpy(), ref[0], "unaligned texture")
    _same_gains(m, ref[1], "unaligned texture")


def test_gpu_vignette_batch_of_four(ox):
    """stitch_batch of four distinct frame sets: planar <true, true> with LG = 2 (four frames in one launch), each
    frame with its own lean gain feed."""
    import torch
    t = _family(ox, "ties")
    sizes = tuple(t["sizes"])
    sets = [VC.random_frames(sizes, 4100 + 50 * k) for k in range(4)]
    refs = [VC.want(("ties", k), t, fr, 0) for k, fr in enumerate(sets)]
    m = ox.Mapper(t["mt"], t["sizes"], blend=0, enable_gain=True)
    m.set_frames_in_flight(4)
    outs = [torch.zeros((t["H"] * 3 // 2, t["W"]), dtype=torch.uint8, device="cuda") for _ in range(4)]
    m.stitch_batch([_cuda(fr) for fr in sets], outs)
    torch.cuda.synchronize()
    for k in range(4):
        assert k == 0 or (refs[k][0] != refs[0][0]).any()
        _same(outs[k].cpu().numpy(), refs[k][0], ("batch", k))
    _same_gains(m, refs[3][1], "batch")


@pytest.mark.parametrize("blend,inflight", [(0, 1), (16, 1), (0, 2), (16, 2)])
def test_gpu_vignette_width_196(ox, blend, inflight):
    """A vignetted camera 196 pixels wide (196 % 8 == 4) beside 192-wide ones with and without a vignette: every
    tile that shows it is gathered (stitch_wide_kernel with f.vig, rows of gains that are not 16-byte aligned),
    the others are staged by planar <false, true> (a width off 8 clears `dw` for the launch) with float4 gains,
    and the gain feed gathers that camera's vignette per tap."""
    t = VC.template(ox, "w196", VC.rig_with(VC.W196_OPTIONS, VC.W196_SIZES))
    wide_cam = VC.W196_SIZES.index((196, 108))
    assert t["vig"][wide_cam] is not None and t["vig"][wide_cam].shape == (108, 196)
    sizes = tuple(t["sizes"])
    sets = [VC.random_frames(sizes, 4400 + 50 * k) for k in range(inflight)]
    refs = [VC.want(("w196", k), t, fr, blend) for k, fr in enumerate(sets)]
    c = VC.counts(t, sets[0])
    assert c["ties"] >= MIN_COUNT and VC.neighbour_changes(t, sets[0]) >= MIN_COUNT, c
    _check_reach("w196", t, sets[0], blend, refs[0])
    info = ox.Mapper(t["mt"], t["sizes"], blend=0, enable_gain=True).info()
    assert info["wide_tiles"] > 0 and info["staged_bytes"] > 0, info  # gathered and staged tiles in one composite
    m, outs = _stitch_slots(ox, t, sets, blend)
    for k, (out, ref) in enumerate(zip(outs, refs)):
        _same(out.cpu().numpy(), ref[0], ("w196", blend, "slot", k))
    _same_gains(m, refs[-1][1], ("w196", blend, inflight))


def test_gpu_vignette_prepared_preview(ox):
    """prepare_preview at an odd width, the saturation family: preview_gather_kernel's taps (gather_taps_frame with
    f.vig) see clamped, vanished and black values; the output is the family case's."""
    import torch
    t = _family(ox, "saturation")
    preview = (301, 151)
    frames = VC.random_frames(tuple(t["sizes"]), 4100)
    ref = VC.want(("saturation", 0, "preview"), t, frames, 0, preview=preview)
    assert VC.counts(t, frames)["clamped"] >= MIN_COUNT
    _check_reach("saturation", t, frames, 0, ref)
    _same(ref[0], VC.want(("saturation", 0), t, frames, 0)[0], "the oracle's output with and without a preview")
    plain = VC.want(("saturation", "plain", "preview"), t, frames, 0, vig=False, preview=preview)
    assert (ref[2] != plain[2]).any(axis=2).mean() >= MIN_CHANGED
    m = ox.Mapper(t["mt"], t["sizes"], blend=0, enable_gain=True)
    m.prepare_preview(*preview)
    assert m.info()["preview_prepared"] == list(preview)
    out = torch.zeros((t["H"] * 3 // 2, t["W"]), dtype=torch.uint8, device="cuda")
    pv = torch.full((preview[1], preview[0], 3), 0x5A, dtype=torch.uint8, device="cuda")
    m.stitch(_cuda(frames), out, preview=pv)
    torch.cuda.synchronize()
    _same(out.cpu().numpy(), ref[0], "output")
    _same(pv.cpu().numpy(), ref[2], "preview")
    _same_gains(m, ref[1], "preview")


@pytest.mark.parametrize("blend", [0, 16])
def test_gpu_vignette_scaled_output(ox, blend):
    """scale_output = (384, 192), the saturation family: the composite writes the RGBA result frame (planar <true,
    true> with the RGBA output) and the resize reads clamped values."""
    import torch
    t = _family(ox, "saturation")
    scale = (384, 192)
    frames = VC.random_frames(tuple(t["sizes"]), 4100)
    ref = VC.want(("saturation", 0, "scaled"), t, frames, blend, scale=scale)
    plain = VC.want(("saturation", "plain", "scaled"), t, frames, blend, vig=False, scale=scale)
    assert VC.counts(t, frames)["clamped"] >= MIN_COUNT
    assert VC.changed_fraction(ref[0], plain[0], scale[1]) >= MIN_CHANGED
    m = ox.Mapper(t["mt"], t["sizes"], blend=blend, enable_gain=True, scale_output=scale)
    assert m.info()["scaled_out"] == list(scale)
    out = torch.zeros((scale[1] * 3 // 2, scale[0]), dtype=torch.uint8, device="cuda")
    m.stitch(_cuda(frames), out)
    torch.cuda.synchronize()
    _same(out.cpu().numpy(), ref[0], ("scaled", blend))
    _same_gains(m, ref[1], ("scaled", blend))
