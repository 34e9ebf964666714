"""The merged frame of an AsyncMultiMapper pipeline in a converted output layout (octvr_async_set_output_format), in
numpy and independent of the library and of its Python helpers: the eight out rules applied to an 8-bit
"Y over [U|V]" stitch, and where a region's bytes land in the merged frame and in its host planes.

A frame of a layout is a 2-D uint8 array (rows, bytes per row):
  uyvy422 / yuyv422   h rows of 2w bytes, U0 Y0 V0 Y1 / Y0 U0 Y1 V0; both rows of a row pair carry its chroma row
  yuv422p / nv16      h rows of Y, then h chroma rows ([U | V] halves / U,V pairs), each 4:2:0 chroma row twice
  p010 / p210         rows of w little-endian words, v8 << 8: Y, then h/2 / h rows of U,V pairs
  yuv420p10 / yuv422p10   rows of w words, v8 << 2: Y, then h/2 / h rows of [U | V] halves
The 10-bit four can be checked against yuv10_ref.out_rule (tests/test_async_out_host.py does)."""
import numpy as np

LAYOUTS = ["uyvy422", "yuyv422", "yuv422p", "nv16", "p010", "yuv420p10", "p210", "yuv422p10"]
VALUES = {"uyvy422": 16, "yuyv422": 17, "yuv422p": 18, "nv16": 19, "p010": 32, "yuv420p10": 33, "p210": 34,
          "yuv422p10": 35}
PACKED = ("uyvy422", "yuyv422")
PAIRS = ("nv16", "p010", "p210")
HALVES = ("yuv422p", "yuv420p10", "yuv422p10")
FILL = 0x5A


def sample_bytes(fmt):
    return 2 if fmt in ("p010", "yuv420p10", "p210", "yuv422p10") else 1


def chroma_rows(fmt):
    """Chroma rows per row pair."""
    return 1 if fmt in ("p010", "yuv420p10") else 2


def frame_dims(fmt, w, h):
    """(rows, bytes per row) of a w x h frame."""
    if fmt in PACKED:
        return h, 2 * w
    return h + chroma_rows(fmt) * (h // 2), sample_bytes(fmt) * w


def _words(a, shift):
    """8-bit values as little-endian 16-bit words v8 << shift, as bytes."""
    return np.ascontiguousarray((a.astype(np.uint16) << shift).astype("<u2")).view(np.uint8)


def out_rule(fmt, f, w, h):
    """The frame of the layout from the 8-bit "Y over [U|V]" frame f (3h/2 rows, w columns)."""
    y, u, v = f[:h, :w], f[h:h * 3 // 2, :w // 2], f[h:h * 3 // 2, w // 2:w]
    if chroma_rows(fmt) == 2:  # each chroma row of the 4:2:0 frame on both rows of its pair
        u, v = np.repeat(u, 2, axis=0), np.repeat(v, 2, axis=0)
    if fmt in PACKED:
        p = np.empty((h, 2 * w), np.uint8)
        luma, cu, cv = (1, 0, 2) if fmt == "uyvy422" else (0, 1, 3)
        p[:, luma::2], p[:, cu::4], p[:, cv::4] = y, u, v
        return p
    c = np.empty((u.shape[0], w), np.uint8)
    if fmt in HALVES:
        c[:, :w // 2], c[:, w // 2:] = u, v
    else:
        c[:, 0::2], c[:, 1::2] = u, v
    p = np.vstack([y, c])
    if sample_bytes(fmt) == 1:
        return p
    return _words(p, 8 if fmt in ("p010", "p210") else 2)


def merged_frame(fmt, OW, OH, regions, fill=FILL):
    """The merged OW x OH frame of the layout: `fill`, then each region (x, y, stitch) — stitch the region's own
    8-bit "Y over [U|V]" frame of rw x rh — put where the layout has it:
      packed  rows [y, y + rh), bytes [2x, 2x + 2rw)
      pairs   luma rows [y, y + rh), bytes [S x, S (x + rw)); chroma rows OH + cr y / 2 + [0, cr rh / 2), the same bytes
      halves  luma as pairs; the same chroma rows, U at bytes [S x / 2, S (x + rw) / 2), V at S OW / 2 plus the same"""
    rows, nbytes = frame_dims(fmt, OW, OH)
    m = np.full((rows, nbytes), fill, np.uint8)
    S, cr = sample_bytes(fmt), chroma_rows(fmt)
    for x, y, stitch in regions:
        rw, rh = stitch.shape[1], stitch.shape[0] * 2 // 3
        assert x % 2 == 0 and y % 2 == 0, "a region of a converted layout starts at even x and y"
        r = out_rule(fmt, stitch, rw, rh)
        if fmt in PACKED:
            m[y:y + rh, 2 * x:2 * (x + rw)] = r
            continue
        m[y:y + rh, S * x:S * (x + rw)] = r[:rh]
        c0, cn = OH + cr * y // 2, cr * rh // 2
        if fmt in PAIRS:
            m[c0:c0 + cn, S * x:S * (x + rw)] = r[rh:]
        else:
            m[c0:c0 + cn, S * x // 2:S * (x + rw) // 2] = r[rh:, :S * rw // 2]
            m[c0:c0 + cn, S * OW // 2 + S * x // 2:S * OW // 2 + S * (x + rw) // 2] = r[rh:, S * rw // 2:]
    return m


def plane_dims(fmt, OW, OH):
    """[(rows, bytes per row)] of the host planes: one packed plane; Y and the U,V plane; or Y, U and V."""
    rows, nbytes = frame_dims(fmt, OW, OH)
    if fmt in PACKED:
        return [(rows, nbytes)]
    if fmt in PAIRS:
        return [(OH, nbytes), (rows - OH, nbytes)]
    return [(OH, nbytes), (rows - OH, nbytes // 2), (rows - OH, nbytes // 2)]


def planes_of(fmt, frame, OW, OH):
    """The host planes of a whole frame, as views."""
    if fmt in PACKED:
        return (frame,)
    if fmt in PAIRS:
        return (frame[:OH], frame[OH:])
    half = frame.shape[1] // 2
    return (frame[:OH], frame[OH:, :half], frame[OH:, half:])


def new_planes(fmt, OW, OH, pad=6, fill=FILL):
    """Host planes full of `fill`, each inside an array whose pitch is its row + pad (+ 2 for the third plane)."""
    out = []
    for k, (rows, nbytes) in enumerate(plane_dims(fmt, OW, OH)):
        out.append(np.full((rows, nbytes + pad + (2 if k == 2 and pad else 0)), fill, np.uint8)[:, :nbytes])
    return tuple(out)


def check_planes(got, want_frame, fmt, OW, OH, what, fill=FILL):
    """Every plane equals its part of the expected frame (regions and untouched fill alike), and the bytes between a
    plane's row and its pitch still hold the fill."""
    want = planes_of(fmt, want_frame, OW, OH)
    assert len(got) == len(want), (what, len(got))
    for k, (g, w) in enumerate(zip(got, want)):
        g8 = g.view(np.uint8) if g.dtype != np.uint8 else g
        d = g8 != w
        assert not d.any(), (what, "plane %d" % k, int(d.sum()), np.argwhere(d)[:6].tolist())
        base = g8.base if g8.base is not None and g8.base.ndim == 2 else g8
        assert (base[:, g8.shape[1]:] == fill).all(), (what, "plane %d: bytes past the row were written" % k)
