"""v210 (OCTVR_PIX_V210 = 48) and its two conversion rules in numpy, for the tests of the v210 paths — written out from
the format's definition, independent of the library and of its Python helpers.

A w x h frame (w, h even) is h rows of 16-byte blocks of four little-endian 32-bit words; a word carries three 10-bit
components in bits 9..0, 19..10 and 29..20.  Block b holds pixels 6b .. 6b + 5:
    word 0 = Cb0 | Y0 << 10 | Cr0 << 20        word 1 = Y1 | Cb1 << 10 | Y2 << 20
    word 2 = Cr1 | Y3 << 10 | Cb2 << 20        word 3 = Y4 | Cr2 << 10 | Y5 << 20
Cb_k, Cr_k belonging to the pixel pair 6b + 2k, 6b + 2k + 1.  row_bytes(w) = 128 ceil(w / 48).  Bits 31..30, the
components of pixels >= w and the blocks past the last pixel are ignored on input and 0 on output.
  in   v8 = min(255, (v10 + 2) >> 2) per component, each chroma row narrowed, then chroma row r =
       (c8[2r] + c8[2r + 1] + 1) >> 1; luma copied
  out  v10 = v8 << 2, chroma row r on rows 2r and 2r + 1
A picture is (Y, U, V) of 10-bit values: Y h x w, U and V h x w / 2 (4:2:2)."""
import numpy as np

VALUE = 48

# (word, shift) of luma Y_i (i = 0..5) and of Cb_k, Cr_k (k = 0..2) in a block
Y_AT = [(0, 10), (1, 0), (1, 20), (2, 10), (3, 0), (3, 20)]
CB_AT = [(0, 0), (1, 10), (2, 20)]
CR_AT = [(0, 20), (2, 0), (3, 10)]


def row_bytes(w):
    return 128 * ((w + 47) // 48)


def shape(w, h):
    """(rows, byte columns)."""
    return (h, row_bytes(w))


def narrow(v10):
    return np.minimum(255, (np.asarray(v10, np.int64) + 2) >> 2)


def lay_out(y, u, v, seed=None):
    """The frame as bytes (h, row_bytes(w)) from 10-bit planes.  With a seed, bits 31..30 of every word, the absent
    components of the last block with pixels and the padding blocks are random; else 0."""
    y, u, v = (np.asarray(p, np.int64) for p in (y, u, v))
    h, w = y.shape
    assert w % 2 == 0 and h % 2 == 0 and u.shape == v.shape == (h, w // 2)
    assert min(y.min(), u.min(), v.min()) >= 0 and max(y.max(), u.max(), v.max()) <= 1023
    nb = row_bytes(w) // 16
    rng = np.random.RandomState(seed)
    if seed is not None:  # everything random first, the real components then replace their fields
        words = rng.randint(0, 1 << 32, (h, nb, 4), dtype=np.int64)
    else:
        words = np.zeros((h, nb, 4), np.int64)

    def put(plane, at, step):
        # sample j of the plane's rows belongs to block j // step, place j % step
        for k, (word, sh) in enumerate(at):
            cols = plane[:, k::step]
            n = cols.shape[1]
            field = words[:, :n, word]
            words[:, :n, word] = (field & ~(0x3FF << sh)) | (cols << sh)

    put(y, Y_AT, 6)
    put(u, CB_AT, 3)
    put(v, CR_AT, 3)
    return np.ascontiguousarray(words.reshape(h, nb * 4).astype("<u4")).view(np.uint8)


def planes10(frame, w, h):
    """(Y, U, V) 10-bit values of a frame given as bytes (columns past row_bytes(w) dropped)."""
    nb = row_bytes(w) // 16
    words = np.ascontiguousarray(frame[:h, :16 * nb]).view("<u4").astype(np.int64).reshape(h, nb, 4)

    def get(at, n):
        out = np.empty((h, nb * len(at)), np.int64)
        for k, (word, sh) in enumerate(at):
            out[:, k::len(at)] = (words[:, :, word] >> sh) & 0x3FF
        return out[:, :n]

    return get(Y_AT, w), get(CB_AT, w // 2), get(CR_AT, w // 2)


def in_rule(frame, w, h):
    """in rule: v210 bytes -> the 8-bit "Y over [U|V]" frame."""
    y, u, v = (narrow(p) for p in planes10(frame, w, h))
    u, v = (u[0::2] + u[1::2] + 1) >> 1, (v[0::2] + v[1::2] + 1) >> 1
    f = np.empty((h * 3 // 2, w), np.uint8)
    f[:h], f[h:, :w // 2], f[h:, w // 2:] = y, u, v
    return f


def out_rule(f, w, h):
    """out rule: the 8-bit "Y over [U|V]" frame -> v210 bytes (every ignored bit, absent component and padding
    block 0)."""
    f = np.asarray(f)
    u = np.repeat(f[h:h * 3 // 2, :w // 2].astype(np.int64) << 2, 2, axis=0)
    v = np.repeat(f[h:h * 3 // 2, w // 2:w].astype(np.int64) << 2, 2, axis=0)
    return lay_out(f[:h, :w].astype(np.int64) << 2, u, v)


def ignored_mask(w, h):
    """Bytes (h, row_bytes(w)) with the bits set that the format ignores on input."""
    ones = np.full((h, w), 1023), np.full((h, w // 2), 1023), np.full((h, w // 2), 1023)
    return ~lay_out(*ones)
