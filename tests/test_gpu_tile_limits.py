"""The tiled composite on the cases of tests/tile_limit_cases.py: items with more than kGroupFirst = 4 staging chunks
(the overflow loop of stitch_tiled_body and its grp1 table), two to four slots that start before and among the
overflow chunks (stage_slot's search), black groups past the image's edge, packed and unpacked large items in one
launch, boxes 256 pixels wide, LDS at kTileLdsBytes, and the steps from staged to gathered tiles beside them.
tests/test_tile_limits_host.py proves on the CPU that each case reaches its path; here each test first repeats the
key figures from the mapper's own LUT (Mapper.info()) and then compares every byte of the output (Y and both chroma
planes; outputs start as 0x5A) and every estimated gain with the oracle's Mapper::stitch, with no tolerance.  The
frames are random bytes, so every staged group has its own content and a misplaced or missing group changes bytes;
the estimated gains are compared on smooth frames with overlapping masks (tile_limit_cases.overlapped: the same LUT)."""
import numpy as np
import pytest

import oracle_py as O
import tile_limit_cases as T
import vignette_cases as V

pytestmark = pytest.mark.gpu

MODES = {"default": None, "packed": "1", "entries32": "0"}  # OCTVR_ENTRY_QUAD, as tests/test_gpu_entry_pack.py
STAT_KEYS = ("wide_tiles", "items_by_slots", "max_chunks", "max_lds_bytes", "max_stride", "grp1_chunks", "items_overflow",
             "items_late_slot", "items_early_slot", "items_packable", "items_by_chunks", "black_groups", "grp1_black_groups")
NOISE, SMOOTH = 9100, 5100


@pytest.fixture(scope="module")
def ox(product_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return product_lib


def to_nv12(f, w, h):
    """"Y over [U|V]" -> NV12 (this file's own numpy, never the library's helpers)."""
    m = np.empty((h * 3 // 2, w), np.uint8)
    m[:h] = f[:h, :w]
    m[h:, 0::2] = f[h:, :w // 2]
    m[h:, 1::2] = f[h:, w // 2:w]
    return m


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the cached frames are read-only


def _out(c, n=1):
    import torch
    return [torch.full((c.H * 3 // 2, c.W), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(n)]


def make_mapper(ox, c, monkeypatch, mode="default", blend=0, remap="remap", seams=None, entry32=False, vig=None):
    """The case's mapper, its entry format fixed at creation by the environment; vig: {camera: gain map}."""
    if entry32:
        monkeypatch.setenv("OCTVR_ENTRY32", "1")
    else:
        monkeypatch.delenv("OCTVR_ENTRY32", raising=False)
    if MODES[mode] is None:
        monkeypatch.delenv("OCTVR_ENTRY_QUAD", raising=False)
    else:
        monkeypatch.setenv("OCTVR_ENTRY_QUAD", MODES[mode])
    mt = T.template(ox, c, seams)
    for i, g in (vig or {}).items():
        mt.set_vignette(i, g)
    return ox.Mapper(mt, list(c.sizes), blend=blend, enable_gain=True, remap=remap)


def check_lut(ox, c, m, mode="default", remap="remap"):
    """The mapper's own blend = 0 LUT has the figures the host test proved for the case."""
    info, host = m.info(), T.lut_info(ox, c, remap)
    info["items"] = sum(info["items_by_slots"])  # staged items ("tiles" counts the jobs, staged or gathered)
    assert info["items"] == host["items"] and info["tiles"] == 8
    for k in STAT_KEYS:
        assert info[k] == host[k], (c.key, k, info[k], host[k])
    packable, items = host["items_packable"], host["items"]
    if mode == "entries32" or remap == "texture":
        assert info["items_packed"] == 0
    elif mode == "packed":
        assert info["items_packed"] == packable
    else:  # by default only where more than half of the items qualify
        assert info["items_packed"] == (packable if 2 * packable > items else 0)
    return info


def same(got, want, what):
    got = got.cpu().numpy()
    d = got != want
    assert not d.any(), (what, int(d.sum()), np.argwhere(d)[:5].tolist())


def run_blend0(ox, c, m, fmts=("yuv420p", "nv12"), remap_tex=False, vig=None):
    """Noise and smooth frames, caller and estimated gains, in each of the frame layouts, against the oracle's stitch
    of case c (the masks of c decide whether the estimated gains depend on the frames)."""
    import torch
    n = len(c.sizes)
    kw = dict(remap_tex=True) if remap_tex else {}
    if vig is not None:
        kw["vig"] = vig
    for fmt in fmts:
        m.set_pixel_formats(fmt, fmt)
        conv = (lambda f, w, h: to_nv12(f, w, h)) if fmt == "nv12" else (lambda f, w, h: f)
        for kind, frames in (("noise", T.noise_frames(c.sizes, NOISE)), ("smooth", T.smooth_frames(c.sizes, SMOOTH))):
            dev = [_cuda(conv(f, w, h)) for f, (w, h) in zip(frames, c.sizes)]
            for given in (True, False):
                gains = T.given_gains(n) if given else None
                want, g = T.want(c, frames, enable_gain=True, gains=gains, **kw)
                out = _out(c)[0]
                m.stitch(dev, out, gains=gains)
                g_got = np.array(m.gains())
                torch.cuda.synchronize()
                same(out, conv(want, c.W, c.H), (c.key, fmt, kind, given))
                if not given:
                    np.testing.assert_array_equal(g_got, np.array(g))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", T.ALL_NAMES)
def test_gpu_tile_limits_blend0(ox, monkeypatch, name, mode):
    """Every case, planar and NV12 frames in and out, caller and estimated gains, with the quad records on by
    default, forced on and forced off."""
    c = T.case(ox, name)
    m = make_mapper(ox, c, monkeypatch, mode)
    info = check_lut(ox, c, m, mode)
    if name in ("cams2_10", "cams4_10") and mode != "entries32":  # packed and large
        assert info["items_packed"] == info["items"] == 8 and info["max_chunks"] > T.K_GROUP_FIRST
    if name == "mixed" and mode == "packed":  # packed small items beside unpacked large ones, alternating per band
        assert 0 < info["items_packed"] < info["items"] and 0 < info["items_overflow"] < info["items"]
    run_blend0(ox, c, m)
    if len(c.sizes) > 1:  # gains that depend on the frames
        o = T.overlapped(c)
        mo = make_mapper(ox, o, monkeypatch, mode)
        check_lut(ox, c, mo, mode)
        run_blend0(ox, o, mo)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["cams4_115", "mixed", "tall2_115"])
def test_gpu_tile_limits_batches(ox, monkeypatch, name, mode):
    """1, 2 and 4 distinct frames per launch (the unit index item << nf_log2 | frame on the overflow path): caller
    gains with the case's masks, estimated gains with the overlapping ones."""
    import torch
    base = T.case(ox, name)
    for c, given in ((base, True), (T.overlapped(base), False)):
        m = make_mapper(ox, c, monkeypatch, mode)
        check_lut(ox, base, m, mode)
        m.set_frames_in_flight(4)
        n = len(c.sizes)
        frames = [T.noise_frames(c.sizes, NOISE + 16 * f) if given else T.smooth_frames(c.sizes, SMOOTH + 16 * f)
                  for f in range(4)]
        dev = [[_cuda(x) for x in fr] for fr in frames]
        wants = [T.want(c, frames[f], enable_gain=True,
                        gains=T.given_gains(n, f) if given else None) for f in range(4)]
        for nb in (1, 2, 4):
            outs = _out(c, nb)
            m.stitch_batch(dev[:nb], outs, gains=[T.given_gains(n, f) for f in range(nb)] if given else None)
            g_last = np.array(m.gains())
            torch.cuda.synchronize()
            for f in range(nb):
                same(outs[f], wants[f][0], (c.key, mode, nb, f))
            if not given:
                np.testing.assert_array_equal(g_last, np.array(wants[nb - 1][1]))


@pytest.mark.parametrize("name", ["one_cam_13", "cams3_115"])
def test_gpu_tile_limits_three_in_flight(ox, monkeypatch, name):
    """Three frames in flight on three streams, twice over (every slot is reused): distinct frames, estimated gains."""
    import torch
    base = T.case(ox, name)
    c = T.overlapped(base) if len(base.sizes) > 1 else base
    m = make_mapper(ox, c, monkeypatch)
    check_lut(ox, base, m)
    m.set_frames_in_flight(3)
    streams = [torch.cuda.Stream() for _ in range(3)]
    frames = [T.noise_frames(c.sizes, NOISE + 16 * f) if f % 2 else T.smooth_frames(c.sizes, SMOOTH + 16 * f) for f in range(6)]
    dev = [[_cuda(x) for x in fr] for fr in frames]
    outs = _out(c, 6)
    torch.cuda.synchronize()
    for f in range(6):
        m.stitch(dev[f], outs[f], stream=streams[f % 3])
    g_last = np.array(m.gains())
    torch.cuda.synchronize()
    for f in range(6):
        want, g = T.want(c, frames[f], enable_gain=True, gains=None)
        same(outs[f], want, (c.key, f))
    np.testing.assert_array_equal(g_last, np.array(g))


@pytest.mark.parametrize("name", ["cams4_115", "cams4_10"])
def test_gpu_tile_limits_vignette(ox, monkeypatch, name):
    """Cameras 1 and 3 with a vignette table (the VIG instances: eight gains per staged group, in overflow chunks
    too) beside cameras 0 and 2 without one; cams4_10: the same on packed items."""
    base = T.case(ox, name)
    maps = {1: O.vignette_map(V.STEEP), 3: O.vignette_map(V.ONE_AND_HALF)}
    for c in (base, T.overlapped(base)):
        vig = [O.resize_linear_cuda_f32(maps[i], w, h) if i in maps else None for i, (w, h) in enumerate(c.sizes)]
        m = make_mapper(ox, c, monkeypatch, vig=maps)
        check_lut(ox, base, m)
        run_blend0(ox, c, m, vig=vig)
    # the tables change the result: the comparison above is not one of two unvignetted stitches
    frames = T.noise_frames(base.sizes, NOISE)
    plain = T.want(base, frames, enable_gain=True, gains=T.given_gains(4))[0]
    assert (T.want(base, frames, enable_gain=True, gains=T.given_gains(4), vig=vig)[0] != plain).any()


@pytest.mark.parametrize("name", ["one_cam_13", "cams4_115", "edge"])
def test_gpu_tile_limits_texture(ox, monkeypatch, name):
    """The texture sampling convention (16-bit fraction codes, the f32 filter instance) on overflow items; border
    cells take the gather path beside them."""
    base = T.case(ox, name)
    host = T.lut_info(ox, base, "texture")
    assert host["tex"] == 1 and host["max_chunks"] > T.K_GROUP_FIRST
    for c in ((base, T.overlapped(base)) if len(base.sizes) > 1 else (base,)):
        m = make_mapper(ox, c, monkeypatch, remap="texture")
        check_lut(ox, base, m, remap="texture")
        run_blend0(ox, c, m, remap_tex=True)


BLEND_CASES = ["cams2_115", "cams4_10", "edge", "edge2", "cams2_115_full"]


@pytest.mark.parametrize("blend,entry32", [(4, False), (4, True), (-3, False)])
@pytest.mark.parametrize("name", BLEND_CASES)
def test_gpu_tile_limits_blends(ox, monkeypatch, name, blend, entry32):
    """Multi-band (4 bands) and feather (-3) with create_masks seams: the MODE 1 remap stages each camera's whole map
    with the same code.  Masks with zeros give entries that carry "no gain", which keep the LUT at 32 bits;
    cams2_115_full (full masks) holds 24-bit entries in its overflow chunks unless OCTVR_ENTRY32 is set.  Its seams
    are all 255 and all 0, so at blend 4 every level-0 sub-tile is deep: the remap writes the whole result and no
    level has blend work (an empty work list, which once ran the blend over every tile instead of none).  A single
    input disables the blend (as in the reference): edge runs the copy chain here; edge2 has black groups past the
    right and bottom edge in the remap's overflow chunks."""
    import torch
    c = T.case(ox, name)
    n = len(c.sizes)
    seams = T.seams(c)
    m = make_mapper(ox, c, monkeypatch, blend=blend, seams=list(seams), entry32=entry32)
    info = m.info()
    if n == 1:
        assert info["blend"] == 0
        check_lut(ox, c, m)
    else:
        assert info["blend"] == blend and info["remap_items"] > 0
        assert info["remap_lut"]["max_chunks"] > T.K_GROUP_FIRST and info["remap_lut"]["grp1_chunks"] > 0
        assert info["remap_entry_bits"] == (24 if name == "cams2_115_full" and not entry32 else 32)
        assert (info["remap_lut"]["grp1_black_groups"] > 0) == (name == "edge2")
    if name == "cams2_115_full" and blend > 0:
        assert info["remap_result_subtiles"] == 4 * 8 * 2  # every 32 x 8 sub-tile of the 256 x 64 frame
        assert [lv["blend_subtiles"] for lv in info["level_tiles"]] == [0] * (info["bands"] + 1)
    for kind, frames in (("noise", T.noise_frames(c.sizes, NOISE)), ("smooth", T.smooth_frames(c.sizes, SMOOTH))):
        dev = [_cuda(f) for f in frames]
        for given in (True, False):
            gains = T.given_gains(n) if given else None
            want, g = T.want(c, frames, enable_gain=True, gains=gains,
                             blend=blend, seams=list(seams))
            out = _out(c)[0]
            m.stitch(dev, out, gains=gains)
            g_got = np.array(m.gains())
            torch.cuda.synchronize()
            same(out, want, (name, blend, entry32, kind, given))
            if not given:
                np.testing.assert_array_equal(g_got, np.array(g))


@pytest.mark.parametrize("staged,over", [("wide_box", "wide_box_over"), ("lds_edge", "lds_over"), ("cams4_10", "cams5")])
def test_gpu_tile_limits_boundary_pairs(ox, monkeypatch, staged, over):
    """One step apart across a limit of build_tiled_lut (box width 256, kTileLdsBytes, four slots): the staged side
    stages every tile, the other side gathers some, and both equal the oracle."""
    a, b = T.case(ox, staged), T.case(ox, over)
    ma, mb = make_mapper(ox, a, monkeypatch), make_mapper(ox, b, monkeypatch)
    ia, ib = check_lut(ox, a, ma), check_lut(ox, b, mb)
    assert ia["wide_tiles"] == 0 and ia["items"] == 8 and ib["wide_tiles"] > 0
    if staged == "wide_box":
        assert ia["max_stride"] >= 256
    if staged == "lds_edge":
        assert ia["max_lds_bytes"] >= T.K_TILE_LDS_BYTES - 1024
    run_blend0(ox, a, ma, fmts=("yuv420p",))
    run_blend0(ox, b, mb, fmts=("yuv420p",))
