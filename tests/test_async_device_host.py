"""Host-side checks of AsyncMultiMapper.push_device (no GPU): the entry point exists and refuses NULL without
touching a device, the Python and C++ wrappers carry it, and octvr_async_create's region rule holds for the
1036 x 512 halves tests/test_gpu_async_device.py merges."""
import ctypes as C
import os

import oracle_py as O
import test_gpu_async as G


def test_push_device_refuses_null(product_lib):
    ox = product_lib
    lib = ox.lib()
    assert hasattr(lib, "octvr_async_push_device"), "octvr_async_push_device is missing"
    assert lib.octvr_async_push_device(None, None, None, None, 0, None) == ox.E_INVALID
    assert b"NULL" in lib.octvr_last_error()
    assert callable(getattr(ox.AsyncMultiMapper, "push_device", None))


def test_push_device_declared_for_c_and_cpp():
    inc = os.path.join(O.ROOT, "include")
    assert "int octvr_async_push_device(octvr_async* async, const uint8_t* const* in_dev, const size_t* in_pitch," in \
        open(os.path.join(inc, "octvr_hip.h")).read()
    hpp = open(os.path.join(inc, "octvr.hpp")).read()
    assert hpp.count("void push_device(const std::vector<const uint8_t*>& in, const std::vector<size_t>& in_pitch") == 2


def test_region_rule_holds_for_1036x512():
    """Even sizes, c.w = r.w / 2 and c.h = r.h / 2 for the left and right half of 1036 x 512, and the alignments
    the merge test relies on: r.x = r.w = 518 = 6 (mod 16), c.x = c.w = 259, odd."""
    for k, reg in enumerate([(0.0, 0.0, 0.5, 1.0), (0.5, 0.0, 0.5, 1.0)]):
        r = G._rect_mul_size(reg, 1036, 512)
        c = G._rect_mul_size(reg, 518, 256)
        assert r == (518 * k, 0, 518, 512) and c == (259 * k, 0, 259, 256)
        assert r[2] % 2 == 0 and r[3] % 2 == 0 and c[2] == r[2] // 2 and c[3] == r[3] // 2
    assert 518 % 16 == 6 and 259 % 2 == 1
