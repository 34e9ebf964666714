"""The numpy layout helpers octvr_amd.nv12_from_yuv420p / yuv420p_from_nv12 ("Y over [U|V]" <-> NV12), against
this file's own permutation.  No GPU."""
import numpy as np
import pytest

import oracle_py as O


@pytest.fixture(scope="module")
def ox(product_lib):
    return product_lib


def _perm(f, w, h):
    m = np.empty((h * 3 // 2, w), np.uint8)
    m[:h] = f[:h]
    m[h:, 0::2] = f[h:, :w // 2]
    m[h:, 1::2] = f[h:, w // 2:]
    return m


def test_nv12_helpers_match_permutation(ox):
    w, h = 34, 18
    f = O.rand_img(w, h * 3 // 2, 1, 991)  # pitch = width
    nv = ox.nv12_from_yuv420p(f, w, h)
    assert nv.shape == (h * 3 // 2, w) and nv.dtype == np.uint8
    assert np.array_equal(nv, _perm(f, w, h))
    assert np.array_equal(nv[:h], f[:h])
    # every chroma byte is distinct enough to show a mis-pairing: U of column pair k at byte 2k, V at 2k + 1
    assert nv[h, 0] == f[h, 0] and nv[h, 1] == f[h, w // 2] and nv[h + 3, 6] == f[h + 3, 3] and nv[h + 3, 7] == f[h + 3, w // 2 + 3]
    back = ox.yuv420p_from_nv12(_perm(f, w, h), w, h)
    assert np.array_equal(back, f)


def test_nv12_helpers_round_trip(ox):
    w, h = 34, 18
    f = O.rand_img(w, h * 3 // 2, 1, 992)
    assert np.array_equal(ox.yuv420p_from_nv12(ox.nv12_from_yuv420p(f, w, h), w, h), f)
    assert np.array_equal(ox.nv12_from_yuv420p(ox.yuv420p_from_nv12(f, w, h), w, h), f)
    g = f.copy()
    ox.nv12_from_yuv420p(g, w, h)
    assert np.array_equal(g, f), "the input is left unchanged"


@pytest.mark.parametrize("w,h", [(33, 18), (34, 17), (0, 18), (34, 0)])
def test_nv12_helpers_reject_odd_sizes(ox, w, h):
    f = np.zeros((27, 34), np.uint8)
    with pytest.raises(ValueError):
        ox.nv12_from_yuv420p(f, w, h)
    with pytest.raises(ValueError):
        ox.yuv420p_from_nv12(f, w, h)


def test_nv12_helpers_reject_bad_shape(ox):
    with pytest.raises(ValueError):
        ox.nv12_from_yuv420p(np.zeros((26, 34), np.uint8), 34, 18)  # not 3h/2 rows
    with pytest.raises(ValueError):
        ox.yuv420p_from_nv12(np.zeros((27, 32), np.uint8), 34, 18)  # narrower than w
