"""tests/v210_ref.py, the numpy statement of v210 the GPU tests compare against, checked on its own: out-then-in is the
identity, its out rule carries P210's components (tests/yuv10_ref.py), and a hand-written block is its four words."""
import numpy as np
import pytest

import v210_ref as V
import yuv10_ref as R10


@pytest.mark.parametrize("w", [96, 146, 148, 150, 256])
def test_v210_ref_out_then_in_is_the_identity(w):
    h = 6
    f = np.random.RandomState(w).randint(0, 256, (h * 3 // 2, w)).astype(np.uint8)
    frame = V.out_rule(f, w, h)
    assert frame.shape == V.shape(w, h) == (h, 128 * -(-w // 48)) and frame.dtype == np.uint8
    assert (V.in_rule(frame, w, h) == f).all()
    # ... and with every ignored bit, absent component and padding block random
    y, u, v = V.planes10(frame, w, h)
    junk = V.lay_out(y, u, v, seed=5)
    assert (junk != frame).any() and ((junk ^ frame) & ~V.ignored_mask(w, h) == 0).all()
    assert (V.in_rule(junk, w, h) == f).all()
    if w % 48:
        assert (frame[:, 16 * -(-w // 6):] == 0).all(), "the padding blocks are 0"


@pytest.mark.parametrize("w", [96, 146, 148, 150, 256])
def test_v210_ref_out_rule_carries_p210s_components(w):
    h = 4
    f = np.random.RandomState(w + 1).randint(0, 256, (h * 3 // 2, w)).astype(np.uint8)
    y, u, v = V.planes10(V.out_rule(f, w, h), w, h)
    py, pu, pv = R10.planes10("p210", R10.out_rule("p210", f, w, h), w, h)
    assert (y == py).all() and (u == pu).all() and (v == pv).all()
    # and the in rules agree on a noisy 10-bit picture
    rng = np.random.RandomState(w + 2)
    pic = rng.randint(0, 1024, (h, w)), rng.randint(0, 1024, (h, w // 2)), rng.randint(0, 1024, (h, w // 2))
    assert (V.in_rule(V.lay_out(*pic, seed=3), w, h) == R10.in_rule("p210", R10.lay_out("p210", *pic), w, h)).all()


def test_v210_ref_a_hand_written_block():
    y = np.array([[100, 101, 102, 103, 104, 105]] * 2)
    cb = np.array([[200, 201, 202]] * 2)
    cr = np.array([[300, 301, 302]] * 2)
    words = V.lay_out(y, cb, cr).view("<u4")
    assert words.shape == (2, 32)
    expect = [200 | 100 << 10 | 300 << 20, 101 | 201 << 10 | 102 << 20, 301 | 103 << 10 | 202 << 20,
              104 | 302 << 10 | 105 << 20]
    assert words[0, :4].tolist() == expect and words[1, :4].tolist() == expect
    assert (words[:, 4:] == 0).all()
    # the rule's own example: 10-bit 3 and 6 narrow to 1 and 2 and average to 2; 1023 and 1021 to 255
    got = V.in_rule(V.lay_out(np.zeros((2, 2), int), np.array([[3], [6]]), np.array([[1023], [1021]])), 2, 2)
    assert got[2].tolist() == [2, 255]
    assert V.narrow([1023, 1022, 1021, 1020, 6, 5, 3, 2, 1, 0]).tolist() == [255, 255, 255, 255, 2, 1, 1, 1, 0, 0]
