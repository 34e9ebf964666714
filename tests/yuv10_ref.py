"""The 10-bit layouts (OCTVR_PIX_P010 / _YUV420P10 / _P210 / _YUV422P10) and their two conversion rules in numpy, for the
tests of the 10-bit paths — written out here, independent of the library and of its Python helpers:
  in   v8 = min(255, (v10 + 2) >> 2) per sample (v10: bits 15..6 of a "p010" / "p210" word, bits 9..0 of a planar one,
       the other 6 bits ignored); the 4:2:2 layouts then average the narrowed chroma rows, (a + b + 1) >> 1
  out  v10 = v8 << 2 (the ignored bits 0), the 4:2:2 layouts with chroma row r on rows 2r and 2r + 1
A picture is (Y, U, V) of 10-bit values (int32): Y h x w, U and V of h chroma rows x w / 2 (4:2:2).  picture420 derives
the 4:2:0 picture whose 8-bit frame is the same, so one oracle stitch serves the four layouts; every test checks that
claim on its own frames (laid)."""
import numpy as np

LAYOUTS = ["p010", "yuv420p10", "p210", "yuv422p10"]
VALUES = {"p010": 32, "yuv420p10": 33, "p210": 34, "yuv422p10": 35}
EDGE = [1023, 1022, 1021, 1020, 6, 5, 3, 2, 1, 0]
PAIRS = [(3, 6), (1023, 1021), (2, 1), (1, 2)]


def is422(fmt):
    return fmt in ("p210", "yuv422p10")


def planar(fmt):
    return fmt in ("yuv420p10", "yuv422p10")


def shape10(fmt, w, h):
    """(rows, byte columns)."""
    return (2 * h if is422(fmt) else h * 3 // 2, 2 * w)


def narrow(v10):
    return np.minimum(255, (np.asarray(v10, np.int32) + 2) >> 2)


def lay_out(fmt, y, u, v, seed=None):
    """The frame of the layout as bytes (rows, 2w) from 10-bit planes (U, V: h rows for 4:2:2, h / 2 for 4:2:0);
    the 6 ignored bits of every word random with a seed, else 0."""
    h, w = y.shape
    rows = shape10(fmt, w, h)[0]
    assert u.shape == v.shape == (rows - h, w // 2)
    p = np.empty((rows, w), np.int32)
    p[:h] = y
    if planar(fmt):
        p[h:, :w // 2], p[h:, w // 2:] = u, v
    else:
        p[h:, 0::2], p[h:, 1::2] = u, v
    assert p.min() >= 0 and p.max() <= 1023
    junk = np.random.RandomState(seed).randint(0, 64, p.shape) if seed is not None else np.zeros_like(p)
    words = (p | junk << 10) if planar(fmt) else (p << 6 | junk)
    return np.ascontiguousarray(words.astype("<u2")).view(np.uint8)


def planes10(fmt, frame, w, h):
    """(Y, U, V) 10-bit values of a frame given as bytes (columns past 2w dropped)."""
    words = np.ascontiguousarray(frame[:, :2 * w]).view("<u2").astype(np.int32)
    v10 = words & 0x3FF if planar(fmt) else words >> 6
    c = v10[h:]
    if planar(fmt):
        return v10[:h], c[:, :w // 2], c[:, w // 2:]
    return v10[:h], c[:, 0::2], c[:, 1::2]


def in_rule(fmt, frame, w, h):
    """in rule: the layout's bytes -> the 8-bit "Y over [U|V]" frame."""
    y, u, v = (narrow(p) for p in planes10(fmt, frame, w, h))
    if is422(fmt):
        u, v = (u[0::2] + u[1::2] + 1) >> 1, (v[0::2] + v[1::2] + 1) >> 1
    f = np.empty((h * 3 // 2, w), np.uint8)
    f[:h], f[h:, :w // 2], f[h:, w // 2:] = y, u, v
    return f


def out_rule(fmt, f, w, h):
    """out rule: the 8-bit "Y over [U|V]" frame -> the layout's bytes."""
    u, v = f[h:, :w // 2].astype(np.int32) << 2, f[h:, w // 2:w].astype(np.int32) << 2
    if is422(fmt):
        u, v = np.repeat(u, 2, axis=0), np.repeat(v, 2, axis=0)
    return lay_out(fmt, f[:h, :w].astype(np.int32) << 2, u, v)


def from8(p8, rng):
    """10-bit values that narrow to p8: 4 v8 + d with d in -2 .. 1."""
    return np.clip(4 * p8.astype(np.int32) + rng.randint(-2, 2, p8.shape), 0, 1023)


def noise_picture(luma8, w, h, seed, edges=False):
    """A 4:2:2 10-bit picture: luma that narrows to luma8 (h x w), noise chroma.  With `edges`, rows from h / 4 on carry
    the edge values 1023 .. 0, rows alternating 1023 and 0 in neighbouring samples (both phases) in luma and — on both
    rows of a chroma row pair — in chroma, and the chroma row pairs (3, 6), (1023, 1021), (2, 1), (1, 2)."""
    rng = np.random.RandomState(seed)
    y = from8(luma8[:h, :w], rng)
    u, v = rng.randint(0, 1024, (h, w // 2)), rng.randint(0, 1024, (h, w // 2))
    if edges:
        r0 = h // 4 & ~1
        x = np.arange(w)
        pats = [np.array(EDGE)[x % 10], np.where(x & 1, 0, 1023), np.where(x & 1, 1023, 0)]
        for k, pat in enumerate(pats):
            y[r0 + k] = pat
            y[r0 + 3 + k] = np.roll(pat, 3)
            for c, roll in ((u, 0), (v, 1)):  # the same row on both rows of the pair: a 4:2:0 picture carries it as is
                c[r0 + 2 * k] = c[r0 + 2 * k + 1] = np.roll(pat, roll)[:w // 2]
        for k, (a, b) in enumerate(PAIRS):
            u[r0 + 8 + 2 * k], u[r0 + 9 + 2 * k] = a, b
            v[r0 + 8 + 2 * k], v[r0 + 9 + 2 * k] = PAIRS[(k + 1) % 4]
    return y, u, v


def picture420(y, u, v, seed):
    """The 4:2:0 picture with the 4:2:2 picture's 8-bit frame: a chroma row pair of equal rows as it is (the edge
    rows), any other as 10-bit values that narrow to the pair's 8-bit average."""
    rng = np.random.RandomState(seed)
    out = []
    for c in (u, v):
        a, b = c[0::2], c[1::2]
        c2 = from8((narrow(a) + narrow(b) + 1) >> 1, rng)
        equal = (a == b).all(axis=1)
        c2[equal] = a[equal]
        out.append(c2)
    return y, out[0], out[1]


def laid_out(fmt, pic, seed):
    """The 4:2:2 picture `pic` as a frame of fmt with random ignored bits (the 4:2:0 layouts through picture420)."""
    return lay_out(fmt, *(pic if is422(fmt) else picture420(*pic, seed=seed + 1)), seed=seed)


def frame8(pic):
    """The 8-bit "Y over [U|V]" frame of the 4:2:2 picture by the in rule."""
    h, w = pic[0].shape
    return in_rule("yuv422p10", lay_out("yuv422p10", *pic), w, h)
