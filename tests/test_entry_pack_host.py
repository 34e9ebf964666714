"""The blend = 0 composite's 8-byte quad records on the CPU (no GPU): octvr_debug_entry_pack packs quads of four
4-byte tiled entries (opencv-octvr_amd/csrc/kernels.hpp quad_pack, what TiledLutDev::upload stores for a
kItemPacked item) and decodes each record back with the arithmetic the kernel's decode runs (quad_unpack: the
flag masks, the dot-product multipliers, the fxy views).  A quad qualifies when it is all black, or has one
slot, no black or "no gain" pixel and tap origins within {0, 1} x {0, 1} of a common base."""
import itertools

import numpy as np
import pytest


def entry(off_dw, fxy, slot, nogain=0):
    """kernels.hpp tiled_entry: bit 0 "no gain", 3-12 fxy, 13-26 the tap's LDS byte offset, 30-31 the slot."""
    return np.uint32(nogain | (fxy & 1023) << 3 | (off_dw * 4) << 13 | slot << 30)


def quad(base, S, deltas, fxy=(0, 0, 0, 0), slot=0):
    return [entry(base + dx + dy * S, f, slot) for (dx, dy), f in zip(deltas, fxy)]


ALL_DELTAS = list(itertools.product([(0, 0), (1, 0), (0, 1), (1, 1)], repeat=4))  # 256 (dx, dy) combinations


@pytest.mark.parametrize("S", [8, 100, 284])  # the smallest stride, a bank-padded one, the largest (256 + 28)
def test_pack_roundtrip(product_lib, S):
    ox = product_lib
    rng = np.random.default_rng(S)
    quads = []
    # every (dx, dy) combination of the four pixels, with random fraction codes, over every slot
    for k, d in enumerate(ALL_DELTAS):
        quads.append(quad(4 + k, S, d, rng.integers(0, 1024, 4), k & 3))
    # every fraction code in every pixel position
    for f in range(1024):
        quads.append(quad(40, S, ALL_DELTAS[f & 255], [(f + 257 * p) & 1023 for p in range(4)], f & 3))
    # the largest base offset: the last tap (base + S + 1) is the last dword of the 12-bit field's range
    top = 4095 - S - 1
    for d in ALL_DELTAS[::17]:
        quads.append(quad(top, S, d, (1023, 0, 511, 31), 3))
    quads.append([np.uint32(0)] * 4)  # all black
    e = np.array(quads, np.uint32)
    ok, rec, un = ox.debug_entry_pack(e, S)
    assert ok.all()
    assert np.array_equal(un, e)
    assert rec[-1] == 0  # black is the all-zero record ...
    assert (rec[:-1] != 0).all()  # ... and nothing else is
    # the base is the quad's minimum origin in each axis, also where no pixel sits on it ((1, 0) and (0, 1))
    k = ALL_DELTAS.index(((1, 0), (0, 1), (1, 0), (0, 1)))
    assert (int(rec[k]) >> 36) & 0xFFF == 4 + k


def test_pack_rejects(product_lib):
    ox = product_lib
    S = 64
    good = quad(100, S, [(0, 0), (1, 0), (0, 1), (1, 1)], (1, 2, 3, 4), 2)
    two_slots = list(good)
    two_slots[3] = entry(100 + S + 1, 4, 1)
    black_mix = list(good)
    black_mix[1] = np.uint32(0)
    delta2_x = [entry(100, 1, 2), entry(102, 2, 2), entry(100 + S, 3, 2), entry(101 + S, 4, 2)]
    delta2_y = [entry(100, 1, 2), entry(101, 2, 2), entry(100 + 2 * S, 3, 2), entry(101 + S, 4, 2)]
    # pixel 0 one column right of the others' minimum and pixel 3 two columns left of pixel 0: a delta of -1
    # before the minimum is taken, 2 after
    neg = [entry(101, 1, 2), entry(100, 2, 2), entry(101 + S, 3, 2), entry(99 + S, 4, 2)]
    # a negative delta alone (pixel 0 right of the rest) is no reason to reject: the base is the minimum
    neg_ok = [entry(101, 1, 2), entry(100, 2, 2), entry(101 + S, 3, 2), entry(100 + S, 4, 2)]
    nogain = list(good)
    nogain[2] = entry(100 + S, 3, 2, nogain=1)
    e = np.array([good, two_slots, black_mix, delta2_x, delta2_y, neg, neg_ok, nogain], np.uint32)
    ok, rec, un = ox.debug_entry_pack(e, S)
    assert ok.tolist() == [True, False, False, False, False, False, True, False]
    assert (rec[~ok] == 0).all()
    assert np.array_equal(un[ok], e[ok])
    # a stride that is no multiple of 4 dwords cannot carry the record's multipliers
    ok, _, _ = ox.debug_entry_pack(np.array([good], np.uint32), 66)
    assert not ok.any()


@pytest.mark.parametrize("name", ["rigA", "rigB", "rigC", "rigD"])
def test_packable_items_counted(product_lib, name):
    """The tiler's count of items every quad of which qualifies (octvr_debug_tiled_lut_info)."""
    import oracle_py as O
    ox = product_lib
    rig, z = O.load_rig(name)
    W, H = (int(v) for v in z["out_size"])
    n = len(z["rois"])
    mt = ox.MapperTemplate.from_arrays(W, H, z["rois"].tolist(), [z[f"map1_{i}"] for i in range(n)],
                                       [z[f"map2_{i}"] for i in range(n)], [z[f"mask_{i}"] for i in range(n)])
    sizes = [(c["options"]["width"], c["options"]["height"]) for c in rig["inputs"]]
    info = ox.debug_tiled_lut_info(mt, sizes)
    assert 0 <= info["items_packable"] <= info["items"]
    assert ox.debug_tiled_lut_info(mt, sizes, remap="texture")["items_packable"] == 0
