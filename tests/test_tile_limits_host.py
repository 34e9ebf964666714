"""The cases of tests/tile_limit_cases.py on the CPU (no GPU): octvr_debug_tiled_lut_info builds each case's blend = 0
tiled LUT exactly as octvr_mapper_create does, and its statistics (tiling.cpp: items_by_slots, max_chunks,
max_lds_bytes, max_stride, grp1_chunks, items_overflow, items_late_slot, items_early_slot) show that the case reaches
the staging path it is named for.  tests/test_gpu_tile_limits.py stitches the same cases against the oracle and
repeats the key figures from the mapper's own LUT; the oracle-side properties at the end check the reference side
on its own."""
import numpy as np
import pytest

import oracle_py as O
import tile_limit_cases as T

OVERFLOW = ("one_cam_13", "cams2_10", "cams3_10", "cams4_10", "cams2_115", "cams3_115", "cams4_115", "tall2_10", "tall4_10",
            "tall2_115", "edge", "edge2", "mixed", "wide_box", "lds_edge", "lds_over")
TEXTURE = ("one_cam_13", "cams4_115", "edge")


def check_case(name, info):
    """The properties of case `name`'s LUT statistics, in either sampling convention."""
    assert sum(info["items_by_slots"]) == info["items"] == sum(info["items_by_chunks"].values())
    assert info["items_late_slot"] <= info["items"] and info["items_early_slot"] <= info["items_overflow"] <= info["items"]
    assert info["max_lds_bytes"] <= T.K_TILE_LDS_BYTES and info["max_stride"] <= 256 + 28
    if name in OVERFLOW:
        assert info["max_chunks"] > T.K_GROUP_FIRST and info["grp1_chunks"] > 0 and info["items_overflow"] > 0
        assert info["grp1_entries"] == 64 * info["grp1_chunks"]
    if name == "one_cam_13":
        assert info["items"] > 0 and info["items_by_slots"][1] == info["items"]
    if name.startswith("cams2_") or name.startswith("tall2_"):
        assert info["items_by_slots"][2] > 0
    if name.startswith("cams3_"):
        assert info["items_by_slots"][3] > 0
    if name.startswith("cams4_") or name.startswith("tall4_"):
        assert info["items_by_slots"][4] > 0
    if name == "cams5":
        assert info["items"] == 0 and info["wide_tiles"] == 16
    if name == "tall2_115":
        assert info["items"] > 0 and info["wide_tiles"] > 0
    if name == "mixed":
        assert 0 < info["items_packable"] < info["items"]
        # items of exactly kGroupFirst chunks (the whole of grp0, nothing of grp1) beside items with overflow chunks
        assert 0 < info["items_overflow"] < info["items"]
        assert info["items_by_chunks"]["4"] == info["items"] - info["items_overflow"]
    if name in ("cams2_10", "cams4_10"):  # packed and large
        assert info["items_packable"] == info["items"] > 0 and info["max_chunks"] > T.K_GROUP_FIRST
    if name == "wide_box":
        assert info["max_stride"] >= 256 and info["wide_tiles"] == 0
    if name == "wide_box_over":
        assert info["wide_tiles"] > 0
    if name == "lds_edge":
        assert info["wide_tiles"] == 0 and info["items"] == 8
        assert T.K_TILE_LDS_BYTES - 1024 <= info["max_lds_bytes"] <= T.K_TILE_LDS_BYTES
    if name == "lds_over":
        assert info["wide_tiles"] > 0
    if name in ("edge", "edge2") and not info["tex"]:  # (texture convention: border cells are gathered, never staged)
        # staged groups past the image's right or bottom edge (kStageBlack), some of them in overflow chunks
        assert info["items"] > 0 and info["black_groups"] >= info["grp1_black_groups"] > 0
    else:
        assert info["black_groups"] == 0 and info["grp1_black_groups"] == 0
    if name == "edge2":
        assert info["items_by_slots"][2] == info["items"] and info["items_late_slot"] > 0


@pytest.mark.parametrize("name", T.ALL_NAMES)
def test_case_reaches_its_path(product_lib, name):
    ox = product_lib
    info = T.lut_info(ox, T.case(ox, name))
    assert info["tex"] == 0
    if name not in ("cams5", "tall2_115", "wide_box_over", "lds_over"):
        assert info["wide_tiles"] == 0 and info["items"] == 8
    check_case(name, info)


@pytest.mark.parametrize("name", TEXTURE)
def test_case_reaches_its_path_texture(product_lib, name):
    """The texture convention stages from one more tap column and row, and border cells go to the gather path."""
    ox = product_lib
    c = T.case(ox, name)
    base, info = T.lut_info(ox, c), T.lut_info(ox, c, remap="texture")
    assert info["tex"] == 1 and info["items"] > 0 and info["items_packable"] == 0
    assert info["wide_tiles"] >= base["wide_tiles"]
    assert info["items"] + info["wide_tiles"] // 2 == 8
    if name == "edge":
        assert info["wide_tiles"] > 0
    check_case(name, info)


def test_slot_paths_covered(product_lib):
    """Over the case list: a slot past the first that starts among the overflow chunks (found by stage_slot's search,
    its groups padded inside grp1) in a two-, a three- and a four-slot case, and one that starts before them in an
    item that has overflow chunks (the map word for its first chunk, the search for the rest)."""
    ox = product_lib
    late, early = set(), 0
    for name in T.ALL_NAMES:
        info = T.lut_info(ox, T.case(ox, name))
        if info["items_late_slot"] > 0:
            late |= {k for k in (2, 3, 4) if info["items_by_slots"][k] == info["items"]}
        early += info["items_early_slot"]
    assert late == {2, 3, 4} and early > 0


def test_lds_pair_is_one_step_apart(product_lib):
    ox = product_lib
    a, b = T.lds_pair(ox)
    assert a.cams[0].sx < b.cams[0].sx <= a.cams[0].sx + 1.0 / 64 + 1e-12
    assert a.cams[0].sy == b.cams[0].sy == T.LDS_SY


def test_wide_box_is_the_last_width(product_lib):
    """Restated from the maps: every tile of wide_box has a box of exactly 256 pixels (first tap column rounded down to
    8, the column after the last tap rounded up to 8; in tile column 0 the last tap sits in box column 255), and
    wide_box_over's are 264 wide."""
    ox = product_lib
    widths = {}
    for name in ("wide_box", "wide_box_over"):
        c = T.case(ox, name)
        sx = np.rint((c.m1[0] * np.float32(c.sizes[0][0])) * np.float32(32)).astype(np.int64) >> 5
        tiles = [sx[:, 128 * tx:128 * (tx + 1)] for tx in range(2)]
        widths[name] = [((int(t.max()) + 1 + 1 + 7) & ~7) - (int(t.min()) & ~7) for t in tiles]
        if name == "wide_box":
            assert int(tiles[0].max()) + 1 - (int(tiles[0].min()) & ~7) == 255
    assert widths == {"wide_box": [256, 256], "wide_box_over": [264, 264]}
    assert T.lut_info(ox, T.case(ox, "wide_box"))["max_stride"] <= 256 + 28


@pytest.mark.parametrize("name", ["cams2_10", "cams3_115", "cams4_115", "tall2_115", "mixed"])
def test_overlapped_masks_keep_the_lut(product_lib, name):
    """The overlapping masks of the estimated-gain comparisons give the same tiled LUT as the partition, and gains that
    depend on the frames (the partition's are all 1: no two cameras share a pixel)."""
    ox = product_lib
    c = T.case(ox, name)
    o = T.overlapped(c)
    assert T.lut_info(ox, o) == T.lut_info(ox, c)
    frames = T.smooth_frames(c.sizes, 5100)
    assert list(T.want(c, frames, enable_gain=True, gains=None)[1]) == [1.0] * len(c.sizes)
    g = np.asarray(T.want(o, frames, enable_gain=True, gains=None)[1])
    assert (g != 1.0).all() and np.isfinite(g).all()


# ---- the oracle's side, on its own ----

def test_oracle_edge_is_black_beyond_the_image(product_lib):
    """edge: the oracle's stitch is black (Y 0, U = V = 128) exactly where every tap lies outside the image, from
    output column 246 and row 53 on, and not black in the pixels before them."""
    ox = product_lib
    c = T.case(ox, "edge")
    out, _ = T.want(c, T.noise_frames(c.sizes, 9100), enable_gain=True, gains=[1.0])
    black = T.black_region(c)
    assert black[:, 246:].all() and black[53:].all() and not black[:53, :246].any()
    Y, UV = out[:c.H], out[c.H:]
    assert (Y[black] == 0).all() and (UV[27:] == 128).all() and (UV[:, 123:128] == 128).all() and (UV[:, 251:] == 128).all()
    # the last staged column group and row: pixels of noise, none of them black
    assert (Y[:53, 238:246] != 0).all() and (Y[52, :246] != 0).all()


def test_oracle_edge2_is_black_beyond_both_images(product_lib):
    """edge2: the same for two cameras, each black in its own column blocks where its taps leave its image."""
    ox = product_lib
    c = T.case(ox, "edge2")
    out, _ = T.want(c, T.noise_frames(c.sizes, 9100), enable_gain=True, gains=[1.0, 1.0])
    black = np.zeros((c.H, c.W), bool)
    for i in range(2):
        black |= T.black_region(c, i) & (c.mk[i] != 0)
    assert black[56:].all() and black[:, 248:].all() and not black[:54, :240].any()
    Y = out[:c.H]
    assert (Y[black] == 0).all() and (Y[:54, :240] != 0).all()


def test_set_vignette_sets_and_removes(product_lib):
    """MapperTemplate.set_vignette: the map comes back bit for bit, None removes it, other inputs are untouched."""
    ox = product_lib
    mt = T.template(ox, T.case(ox, "cams2_10"))
    g = np.linspace(0.5, 1.5, 12, dtype=np.float32).reshape(3, 4)
    assert mt.vignette(0) is None and mt.vignette(1) is None
    mt.set_vignette(1, g)
    assert mt.vignette(0) is None and np.array_equal(mt.vignette(1), g)
    mt.set_vignette(1, None)
    assert mt.vignette(1) is None
    with pytest.raises(ox.OctvrError):
        mt.set_vignette(2, g)


def test_oracle_copy_chain_is_per_camera(product_lib):
    """cams2_10 with every gain 1: in camera c's column blocks the oracle's stitch equals its stitch of camera c
    alone (the blocks are 64 columns wide, so no chroma sample straddles two cameras)."""
    ox = product_lib
    c = T.case(ox, "cams2_10")
    frames = T.noise_frames(c.sizes, 9100)
    both, _ = T.want(c, frames, enable_gain=True, gains=[1.0, 1.0])
    for i in range(2):
        alone, _ = O.stitch_frame([frames[i]], [c.sizes[i]], [list(c.rois[i])], [c.m1[i]], [c.m2[i]], [c.mk[i]], c.W, c.H,
                                  enable_gain=True, gains=[1.0])
        own = c.mk[i] != 0
        assert np.array_equal(both[:c.H][own], alone[:c.H][own])
        cown = own[::2, ::2]
        for plane in (slice(0, c.W // 2), slice(c.W // 2, c.W)):
            assert np.array_equal(both[c.H:, plane][cown], alone[c.H:, plane][cown])
        assert (alone[:c.H][~own] == 0).all() and (both[:c.H][own] != 0).any()
