"""The configurations of tests/test_gpu_fastmapper_layouts.py on the CPU (no GPU): the host index audit
(octvr_debug_fastmapper_audit, the replay of every index fast_y_kernel / fast_uv_kernel derive) without a
violation on each of them, in both entry formats and with every input pitch pad the GPU tests use, and the
conditions those tests rest on, which are properties of the oracle's output alone: the accumulator wraps, whole
runs stay uncovered, the 100 x 50 planes end in partial runs.

The audit replays addresses relative to the frame's base, so a base that is not 4-byte aligned is outside it: the
kernels form the same offsets whatever the base, and what the hardware does with the resulting unaligned 8-byte
loads is covered by the GPU tests only (test_gpu_fastmapper_layouts.py, the misaligned inputs)."""
import json

import numpy as np
import pytest

import fastmapper_cases as FC


def _audit(ox, c, wide, pad):
    ok, rep = ox.debug_fastmapper_audit(FC.template(ox, c), list(c.sizes), wide=wide, pitch_pad=pad)
    assert ok, (c.key, wide, pad, json.dumps(rep))
    for plane in ("y", "uv"):
        p = rep[plane]
        assert p["violations"] == 0, (c.key, wide, pad, plane, p["first"])
        assert p["live_slots"] == p["blocks"]
        assert p["slot_loads"] == 4 * p["groups"]
        if wide:
            assert p["compact"] == 0 and p["interior_slots"] == 0
    return rep


def _runs(c):
    return (c.W * c.H + 255) // 256, ((c.W // 2) * (c.H // 2) + 255) // 256


@pytest.mark.parametrize("wide", [False, True], ids=["compact", "wide"])
@pytest.mark.parametrize("pad", FC.IN_PADS)
def test_audit_layouts(product_lib, pad, wide):
    """The edge-tap template at every input pitch the GPU tests use: w + {0, 1, 2, 3, 8, 64} (rows that start at
    every residue mod 4, the end-of-frame clamp at a pitch that is not a multiple of 4)."""
    c = FC.layouts()
    rep = _audit(product_lib, c, wide, pad)
    assert (rep["y"]["runs"], rep["uv"]["runs"]) == _runs(c)
    assert rep["y"]["blocks"] == 2 * rep["y"]["runs"] and rep["y"]["taps_in_image"] > 0


@pytest.mark.parametrize("wide", [False, True], ids=["compact", "wide"])
@pytest.mark.parametrize("ncam", [1, 3])
@pytest.mark.parametrize("shape", FC.TINY_SHAPES, ids=lambda s: "%dx%d" % s)
def test_audit_tiny(product_lib, shape, ncam, wide):
    """Outputs below one run and ragged last runs; sources down to 4 x 2 and 2 x 2 (the latter only with a pitch
    of 4 or more: the audit reports a 6-byte frame as a violation, the stitch refuses it)."""
    ox = product_lib
    c = FC.tiny(shape[0], shape[1], ncam)
    for pad in (2, 3, 8):  # one pad for every camera here; the GPU test pads the 2 x 2 source alone
        rep = _audit(ox, c, wide, pad)
        assert (rep["y"]["runs"], rep["uv"]["runs"]) == _runs(c)
        assert rep["y"]["blocks"] == ncam * rep["y"]["runs"]
    if (2, 2) in c.sizes:
        ok, rep = ox.debug_fastmapper_audit(FC.template(ox, c), list(c.sizes), wide=wide, pitch_pad=0)
        assert not ok and "frame under 8 bytes" in rep["y"]["first"], rep
    else:
        _audit(ox, c, wide, 0)


def test_tails_100x50():
    """100 x 50: the last luma run holds 136 pixels, the last chroma run 226, and a chroma run of 256 pixels in
    rows of 50 spans more than five rows (the row-step loop after the scalar division runs up to six times)."""
    assert 100 * 50 == 19 * 256 + 136
    assert 50 * 25 == 4 * 256 + 226
    assert 256 > 5 * 50
    assert 258 * 2 == 2 * 256 + 4 and 256 - 258 == -2 and 254 * 6 == 5 * 256 + 244


@pytest.mark.parametrize("wide", [False, True], ids=["compact", "wide"])
@pytest.mark.parametrize("all_zero", [False, True], ids=["partial", "all_zero"])
def test_audit_and_oracle_uncovered(product_lib, all_zero, wide):
    """Runs without a camera: the run table holds a zero mask for them (no group, no block) and the oracle's
    output is 0 over at least one whole run of each plane; with every mask zero neither plane has a block."""
    c = FC.uncovered(all_zero)
    rep = _audit(product_lib, c, wide, 3)
    _, out = FC.want(c, 31)
    luma, chroma = out[:c.H].ravel(), out[c.H:].reshape(c.H // 2, c.W // 2, 2)
    if all_zero:
        assert rep["y"]["blocks"] == 0 and rep["uv"]["blocks"] == 0 and rep["y"]["groups"] == 0
        assert not out.any()
        return
    # weights are zero up to five pixels past a mask's edge: luma rows 0..28, chroma rows 0..13
    assert rep["y"]["groups"] < rep["y"]["runs"] and rep["uv"]["groups"] < rep["uv"]["runs"]
    assert rep["y"]["groups"] > 0 and rep["uv"]["groups"] > 0
    assert not luma[:9 * 256].any() and not chroma.reshape(-1, 2)[:2 * 256].any()
    assert luma.any() and chroma.any()


@pytest.mark.parametrize("wide", [False, True], ids=["compact", "wide"])
@pytest.mark.parametrize("n", FC.MANY_N)
def test_audit_many_cameras(product_lib, n, wide):
    """Up to 32 cameras: every camera has weight in every run, so a run has ceil(n / 4) groups and the last
    group's dead slots reload its first block."""
    c = FC.many(n)
    for pad in (0, 3):
        rep = _audit(product_lib, c, wide, pad)
        for plane in ("y", "uv"):
            assert rep[plane]["blocks"] == n * rep[plane]["runs"]
            assert rep[plane]["groups"] == (n + 3) // 4 * rep[plane]["runs"]
            assert rep[plane]["max_block"] == rep[plane]["blocks"] - 1


@pytest.mark.parametrize("n", FC.WRAP_N)
def test_oracle_wraps(product_lib, n):
    """The wrap construction does wrap in the oracle: white frames, constant maps; at least one luma pixel and one
    chroma byte at 4 or below (a kernel that saturated its sum would write 255 there), and no pixel in between:
    the n weights are each rounded once (luma) or twice (the halved chroma weights), so their sum s lies within
    n of 255 and the pixel is s (no wrap) or about s - 257 (wrapped)."""
    c = FC.wrap(n)
    _audit(product_lib, c, False, 0)
    _, out = FC.want(c, None)
    luma, chroma = FC.wrapped_counts(c, out)
    print("wrap n=%d: %d luma pixels, %d chroma bytes <= 4" % (n, luma, chroma))
    assert luma >= 1 and chroma >= 1
    assert ((out <= n) | (out >= 254 - n)).all()
    assert (out >= 254 - n).any()


@pytest.mark.parametrize("kind", FC.INTERIOR_KINDS)
def test_audit_interior_boundary(product_lib, kind):
    """The interior flag at its boundary x1 <= pw - 2, y1 <= ph - 3, x0, y0 >= 0: set for run 0 when its largest
    tap is exactly (w - 2, h - 3), clear when one pixel moves to w - 1, to h - 2 or to -1; run 1 is an edge block
    in every case.  The chroma plane's flags follow from the averaged maps (expected_interior_blocks)."""
    c = FC.interior(kind)
    exp = FC.expected_interior_blocks(c)
    assert exp["y"] == (1 if kind == "A" else 0)
    for pad in (0, 1, 64):
        rep = _audit(product_lib, c, False, pad)
        assert rep["y"]["runs"] == 2 and rep["y"]["blocks"] == 2 and rep["uv"]["runs"] == 1
        assert rep["y"]["interior_slots"] == exp["y"], (kind, rep)
        assert rep["uv"]["interior_slots"] == exp["uv"], (kind, rep)
    _audit(product_lib, c, True, 0)


def test_audit_interior_mixed_group(product_lib):
    """An interior and an edge block in one group of four, the fifth camera alone in the second group."""
    c = FC.interior_group()
    exp = FC.expected_interior_blocks(c)
    assert exp["y"] == 4
    rep = _audit(product_lib, c, False, 0)
    assert rep["y"]["runs"] == 2 and rep["y"]["groups"] == 4 and rep["y"]["blocks"] == 10
    assert rep["y"]["interior_slots"] == 4
    assert rep["uv"]["groups"] == 2 and rep["uv"]["interior_slots"] == exp["uv"]
    _audit(product_lib, c, True, 0)


@pytest.mark.parametrize("wide", [False, True], ids=["compact", "wide"])
def test_audit_nonfinite_maps(product_lib, wide):
    """NaN, +-inf, +-1e9 and the taps 32767 / -32768 under a non-zero weight: blocks span the whole s16 range, so
    the luma plane keeps the 8-byte entries whatever format is asked for, and no address leaves its frame."""
    c = FC.nonfinite()
    for m in c.m1 + c.m2:
        assert np.isnan(m).any() and np.isposinf(m).any() and np.isneginf(m).any()
    for pad in (0, 1, 2, 3):
        rep = _audit(product_lib, c, wide, pad)
        assert rep["y"]["compact"] == 0
