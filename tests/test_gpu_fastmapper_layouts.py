"""vr::FastMapper::stitch_nv12 and its batch on caller-made data (the configurations of fastmapper_cases.py):
frame layouts the caller chooses (input pitches above the width and off every alignment, input and output
bases off 4-byte alignment, output pitches above the width), outputs below one run and with ragged last runs,
runs without any camera, up to 32 cameras per frame, the u16 accumulator wrap, the boundary of the interior
flag, non-finite map values, and two streams at once.

Every case is bit-exact against the oracle (oracle_py.fastmapper_nv12, which gets contiguous copies of the
frames).  Every output allocation is prefilled with 0xA5: the W x 3H/2 window must equal the oracle and every
other byte (the padding between W and the pitch, the guard rows before and after, the bytes in front of an
offset base) must still be 0xA5, so a run or plane that wrote nothing shows as 0xA5 where the oracle has 0.
Input allocations hold random bytes outside the frame's own columns.  tests/test_fastmapper_layouts_host.py
audits the same configurations on the host and checks the oracle-side conditions."""
import numpy as np
import pytest

import fastmapper_cases as FC

pytestmark = pytest.mark.gpu

CANARY = 0xA5
FORMATS = pytest.mark.parametrize("wide", [False, True], ids=["compact", "wide"])


def _dev_frame(frame, pad=0, off=0, seed=0):
    """`frame` on the device at pitch w + pad, its base `off` bytes into a fresh allocation: a view into a
    (rows + 1) x pitch tensor of random bytes (one spare row, so pitch * rows bytes from the base stay inside)."""
    import torch
    rows, w = frame.shape
    pitch = w + pad
    rng = np.random.default_rng(9000 + seed)
    wide = torch.from_numpy(rng.integers(0, 256, ((rows + 1) * pitch,), dtype=np.uint8)).cuda()
    assert wide.data_ptr() % 4 == 0 and off < pitch
    v = wide[off:off + rows * pitch].view(rows, pitch)[:, :w]
    v.copy_(torch.from_numpy(np.array(frame)))
    assert v.stride(0) == pitch and v.data_ptr() % 4 == off % 4
    return v


class _Out:
    """A W x 3H/2 output window at pitch W + pad, `off` bytes past `guard` rows, in an allocation of 0xA5."""

    def __init__(self, W, H, pad=0, off=0, guard=2):
        import torch
        self.W, self.rows, self.pitch = W, H * 3 // 2, W + pad
        self.start = guard * self.pitch + off
        self.buf = torch.full(((self.rows + 2 * guard) * self.pitch + 4,), CANARY, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 4 == 0
        self.t = self.buf[self.start:self.start + self.rows * self.pitch].view(self.rows, self.pitch)[:, :W]

    def check(self, want, tag=None):
        host = self.buf.cpu().numpy()
        idx = self.start + np.arange(self.rows)[:, None] * self.pitch + np.arange(self.W)[None, :]
        got = host[idx]
        d = got != want
        assert not d.any(), (tag, int(d.sum()), np.argwhere(d)[:5].tolist(), got[d][:5].tolist(), want[d][:5].tolist())
        outside = np.ones(host.size, bool)
        outside[idx.ravel()] = False
        hit = outside & (host != CANARY)
        assert not hit.any(), (tag, "bytes written outside the output window", np.flatnonzero(hit)[:8].tolist())

    def untouched(self):
        return bool((self.buf == CANARY).all().item())


def _mapper(ox, c, wide, monkeypatch):
    monkeypatch.setenv("OCTVR_FAST_WIDE", "1" if wide else "0")
    return ox.FastMapper(FC.template(ox, c), list(c.sizes))


def _stitch_check(fm, c, seed, in_pads=None, in_offs=None, out_pad=0, out_off=0, tag=None):
    import torch
    frames, want = FC.want(c, seed)
    n = len(frames)
    in_pads, in_offs = in_pads or [0] * n, in_offs or [0] * n
    ins = [_dev_frame(f, in_pads[i], in_offs[i], i) for i, f in enumerate(frames)]
    out = _Out(c.W, c.H, out_pad, out_off)
    fm.stitch_nv12(ins, out.t)
    torch.cuda.synchronize()
    out.check(want, tag)


def _batch_check(fm, c, seeds, layout=None, out_pad=0, out_offs=None):
    """One batch launch of len(seeds) frames: frame f's inputs at layout(f, i) = (pad, off), its output at
    out_offs[f]; every frame against the oracle's stitch of that frame."""
    import torch
    nb, n = len(seeds), len(c.sizes)
    layout = layout or (lambda f, i: (0, 0))
    sets = []
    for f, seed in enumerate(seeds):
        frames, _ = FC.want(c, seed)
        sets.append([_dev_frame(x, *layout(f, i), seed=31 * f + i) for i, x in enumerate(frames)])
    outs = [_Out(c.W, c.H, out_pad, (out_offs or [0] * nb)[f]) for f in range(nb)]
    fm.stitch_nv12_batch(sets, [o.t for o in outs])
    torch.cuda.synchronize()
    for f, seed in enumerate(seeds):
        outs[f].check(FC.want(c, seed)[1], ("frame", f))


# ---- frame layouts ---------------------------------------------------------------------------------------
# (input pads, input base offsets, output pad, output base offset); inputs 40 x 24 and 42 x 26
_LAYOUTS = (
    [((p, p), (0, 0), 0, 0) for p in FC.IN_PADS[1:]] +       # input pitch w + {1, 2, 3, 8, 64}
    [((k, k), (k, k), 0, 0) for k in (1, 2, 3)] +            # input base at 1, 2, 3 mod 4
    [((0, 0), (0, 0), p, 0) for p in (2, 32)] +              # output pitch W + {2, 32}
    [((0, 0), (0, 0), 4, k) for k in (1, 3)] +               # output base at 1, 3 mod 4
    [((3, 8), (1, 2), 2, 3), ((64, 1), (3, 0), 32, 1), ((2, 3), (2, 3), 2, 1)]  # all at once, per camera
)


@FORMATS
@pytest.mark.parametrize("lay", _LAYOUTS, ids=lambda l: "in%s@%s_out%d@%d" % ("-".join(map(str, l[0])), "-".join(map(str, l[1])), l[2], l[3]))
def test_layouts_single(product_lib, lay, wide, monkeypatch):
    """Two cameras with taps on and past every edge of both planes; the row loads start at `xa * bpp & ~3` from
    the base, so every residue of the pitch and of the base moves them against the dword grid."""
    c = FC.layouts()
    fm = _mapper(product_lib, c, wide, monkeypatch)
    _stitch_check(fm, c, 300, list(lay[0]), list(lay[1]), lay[2], lay[3])


@FORMATS
@pytest.mark.parametrize("nb", [2, 4])
def test_layouts_batch(product_lib, nb, wide, monkeypatch):
    """The batch launch with another pitch and base for every frame and camera (the kernels read each frame's
    table entry at f << cam_lg), outputs at pitch W + 2 from bases at 0..3 mod 4."""
    c = FC.layouts()
    fm = _mapper(product_lib, c, wide, monkeypatch)
    pads = (1, 2, 3, 8, 64, 0, 5, 7)
    _batch_check(fm, c, [310 + f for f in range(nb)],
                 layout=lambda f, i: (pads[2 * f + i], (f + 2 * i + 1) % 4),
                 out_pad=2, out_offs=[(3 * f + 1) % 4 for f in range(nb)])


# ---- tiny and ragged outputs -----------------------------------------------------------------------------
@FORMATS
@pytest.mark.parametrize("ncam", [1, 3])
@pytest.mark.parametrize("shape", FC.TINY_SHAPES, ids=lambda s: "%dx%d" % s)
def test_tiny_and_ragged_outputs(product_lib, shape, ncam, wide, monkeypatch):
    """Outputs from 2 x 2 (four lanes of the luma run, one of the chroma run) to 100 x 50 (luma tail
    of 136 lanes, chroma tail of 226, chroma runs over more than five rows), 258 x 2 and 254 x 6 (runs that end
    inside a row); sources down to 4 x 2 and 2 x 2 at pitch 4 (a 12-byte frame: the chroma row's load is
    clamped to size - 8 = 4 and its taps are bytes 4 and 5 of the load)."""
    c = FC.tiny(shape[0], shape[1], ncam)
    fm = _mapper(product_lib, c, wide, monkeypatch)
    _stitch_check(fm, c, 320, in_pads=FC.tiny_pads(c), out_pad=3, out_off=1)


def test_source_below_8_bytes_is_refused(product_lib, monkeypatch):
    """A contiguous 2 x 2 NV12 frame is 6 bytes, below the 8-byte row loads: refused with OCTVR_E_INVALID before
    anything is launched (the output keeps its prefill); the same FastMapper then stitches the padded frame."""
    import torch
    ox = product_lib
    c = FC.tiny(2, 2, 1)
    assert c.sizes == ((2, 2),)
    fm = _mapper(ox, c, False, monkeypatch)
    frames, _ = FC.want(c, 320)
    out = _Out(c.W, c.H)
    with pytest.raises(ox.OctvrError) as err:
        fm.stitch_nv12([torch.from_numpy(np.array(frames[0])).cuda()], out.t)
    assert err.value.code == ox.E_INVALID
    assert ox.lib().octvr_last_error().decode() == "input frame below 8 bytes"
    torch.cuda.synchronize()
    assert out.untouched()
    _stitch_check(fm, c, 320, in_pads=[2])


# ---- uncovered output ------------------------------------------------------------------------------------
@FORMATS
@pytest.mark.parametrize("all_zero", [False, True], ids=["partial", "all_zero"])
def test_uncovered_runs_are_written_zero(product_lib, all_zero, wide, monkeypatch):
    """Runs whose camera mask is 0, and planes without any block (nblk == 0, the arrays hold one dummy block):
    the kernels still write 0 there, over the 0xA5 prefill."""
    c = FC.uncovered(all_zero)
    fm = _mapper(product_lib, c, wide, monkeypatch)
    _stitch_check(fm, c, 31, in_pads=[1, 2], out_pad=2)
    _batch_check(fm, c, [31, 32], out_pad=2)


# ---- many cameras ----------------------------------------------------------------------------------------
@FORMATS
@pytest.mark.parametrize("n", FC.MANY_N)
def test_many_cameras_single(product_lib, n, wide, monkeypatch):
    """Camera bits up to 31 and up to eight groups of four, the last one with dead slots (n = 7, 9, 17)."""
    c = FC.many(n)
    fm = _mapper(product_lib, c, wide, monkeypatch)
    _stitch_check(fm, c, 400, in_pads=[i % 4 for i in range(n)], in_offs=[i % 4 for i in range(n)])


@FORMATS
@pytest.mark.parametrize("nb,n", [(4, 16), (2, 17), (2, 32)])
def test_many_cameras_batch(product_lib, nb, n, wide, monkeypatch):
    """The frame tables to their last entry: 16 cameras per frame at f << 4 in a batch of 4, 32 at f << 5 in a
    batch of 2; a kernel reading the wrong table entry takes another frame's (different) pixels."""
    c = FC.many(n)
    fm = _mapper(product_lib, c, wide, monkeypatch)
    _batch_check(fm, c, [400 + 50 * f for f in range(nb)], layout=lambda f, i: ((f + i) % 4, (f + i) % 4))


def test_batch_refusals(product_lib, monkeypatch):
    """4 x 17 cameras (a 4-frame batch holds 16 per frame) and a batch of 3 are refused with OCTVR_E_INVALID
    before any launch: the outputs keep their prefill, and the next valid call is exact."""
    import torch
    ox = product_lib
    c = FC.many(17)
    fm = _mapper(ox, c, False, monkeypatch)
    for nb in (4, 3):
        sets = [[_dev_frame(x) for x in FC.want(c, 400 + 50 * f)[0]] for f in range(nb)]
        outs = [_Out(c.W, c.H) for _ in range(nb)]
        with pytest.raises(ox.OctvrError) as err:
            fm.stitch_nv12_batch(sets, [o.t for o in outs])
        assert err.value.code == ox.E_INVALID, nb
        torch.cuda.synchronize()
        assert all(o.untouched() for o in outs), nb
    _batch_check(fm, c, [400, 450])
    _stitch_check(fm, c, 400)


# ---- accumulator wrap ------------------------------------------------------------------------------------
def _wrap_want(c):
    _, want = FC.want(c, None)
    luma, chroma = FC.wrapped_counts(c, want)
    assert luma >= 1 and chroma >= 1, (luma, chroma)  # a condition on the oracle: the construction wraps
    return want


@FORMATS
@pytest.mark.parametrize("n", FC.WRAP_N)
def test_accumulator_wraps(product_lib, n, wide, monkeypatch):
    """White frames under weights that sum past 257: the reference's u16 accumulators wrap and the pixel comes
    out at 1..4; the kernel's 32-bit sum must be masked to 16 bits, not saturated."""
    c = FC.wrap(n)
    _wrap_want(c)
    fm = _mapper(product_lib, c, wide, monkeypatch)
    _stitch_check(fm, c, None)


def test_accumulator_wraps_batch(product_lib, monkeypatch):
    """The same per frame of a batch of 2 at 32 cameras: one white frame set, one random."""
    c = FC.wrap(32)
    _wrap_want(c)
    fm = _mapper(product_lib, c, False, monkeypatch)
    _batch_check(fm, c, [None, 500])


# ---- interior boundary -----------------------------------------------------------------------------------
def _audit(ox, c):
    ok, rep = ox.debug_fastmapper_audit(FC.template(ox, c), list(c.sizes))
    assert ok, rep
    return rep


@pytest.mark.parametrize("kind", FC.INTERIOR_KINDS)
def test_interior_boundary(product_lib, kind, monkeypatch):
    """Run 0's largest tap at exactly (w - 2, h - 3) takes the interior path (no clamps, no masks): its last
    8-byte loads end inside the plane; one tap further in x, in y or at -1 it must take the general path.  The
    host audit says which path each run takes before the kernels run; the chroma plane's flag follows from the
    averaged maps and is whatever the maps give."""
    ox = product_lib
    c = FC.interior(kind)
    exp = FC.expected_interior_blocks(c)
    rep = _audit(ox, c)
    assert rep["y"]["interior_slots"] == (1 if kind == "A" else 0), rep
    assert rep["uv"]["interior_slots"] == exp["uv"], rep
    fm = _mapper(ox, c, False, monkeypatch)
    _stitch_check(fm, c, 600, in_pads=[1], in_offs=[1])
    _batch_check(fm, c, [600, 601], layout=lambda f, i: (3 * f, 0))


def test_interior_and_edge_block_in_one_group(product_lib, monkeypatch):
    """Five cameras: run 0's first group holds three interior blocks and an edge block and must take the general
    path for all four; the fifth camera, alone in the second group, takes the interior path."""
    ox = product_lib
    c = FC.interior_group()
    rep = _audit(ox, c)
    assert rep["y"]["groups"] == 4 and rep["y"]["blocks"] == 10 and rep["y"]["interior_slots"] == 4, rep
    assert rep["uv"]["interior_slots"] == FC.expected_interior_blocks(c)["uv"], rep
    fm = _mapper(ox, c, False, monkeypatch)
    _stitch_check(fm, c, 610)
    _batch_check(fm, c, [610, 611, 612, 613])


# ---- non-finite maps -------------------------------------------------------------------------------------
@FORMATS
def test_nonfinite_and_huge_maps(product_lib, wide, monkeypatch):
    """NaN, +-inf, +-1e9 and the taps 32767 / -32768 under full weight: the taps are outside every image and add
    0, the luma plane falls back to the 8-byte entries in either setting."""
    ox = product_lib
    c = FC.nonfinite()
    ok, rep = ox.debug_fastmapper_audit(FC.template(ox, c), list(c.sizes), wide=wide)
    assert ok and rep["y"]["compact"] == 0, rep
    fm = _mapper(ox, c, wide, monkeypatch)
    _stitch_check(fm, c, 700, in_pads=[1, 3], in_offs=[1, 2], out_pad=2)
    assert FC.want(c, 700)[1].any()


# ---- two streams -----------------------------------------------------------------------------------------
def test_two_streams_one_mapper(product_lib, monkeypatch):
    """One FastMapper, two streams, two frame sets and two outputs issued back to back (the FastMapper keeps no
    per-call device state): both outputs exact."""
    import torch
    c = FC.many(9)
    fm = _mapper(product_lib, c, False, monkeypatch)
    seeds = (400, 450)
    ins = [[_dev_frame(x, i % 4, i % 4, i) for i, x in enumerate(FC.want(c, s)[0])] for s in seeds]
    outs = [_Out(c.W, c.H, 2, k) for k in (1, 2)]
    torch.cuda.synchronize()  # the uploads and prefills ran on the current stream
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for k in range(2):
        fm.stitch_nv12(ins[k], outs[k].t, stream=streams[k])
    for s in streams:
        s.synchronize()
    for k in range(2):
        outs[k].check(FC.want(c, seeds[k])[1], ("stream", k))
