"""Host-side checks of the AsyncMultiMapper's converted output layouts (octvr_async_set_output_format; no GPU):
the entry point exists and refuses NULL without touching a device, both headers declare it, the Python method
exists; the arithmetic merge_pack_kernel runs (csrc/async_host.hpp build_merge_pack_table, merge_pack_item,
region_rects; csrc/frame_layout.hpp pack_item_at, pack_lane) in tests/cpp/async_merge_pack_check.cpp, a stand-alone
program compiled with -fsanitize=address,undefined and run directly; and tests/async_out_ref.py, the numpy the GPU
tests expect bytes from, against yuv10_ref.out_rule and against hand-written frames."""
import os
import subprocess

import numpy as np

import async_out_ref as R
import oracle_py as O
import test_gpu_async as G
import yuv10_ref as R10


def test_set_output_format_refuses_null(product_lib):
    ox = product_lib
    lib = ox.lib()
    assert hasattr(lib, "octvr_async_set_output_format"), "octvr_async_set_output_format is missing"
    assert lib.octvr_async_set_output_format(None, ox.PIX_UYVY422) == ox.E_INVALID
    assert b"NULL" in lib.octvr_last_error()
    assert lib.octvr_async_set_output_format(None, ox.PIX_NV12) == ox.E_INVALID
    assert callable(getattr(ox.AsyncMultiMapper, "set_output_format", None))


def test_set_output_format_declared_for_c_and_cpp():
    inc = os.path.join(O.ROOT, "include")
    assert "int octvr_async_set_output_format(octvr_async* async, int out_format);" in \
        open(os.path.join(inc, "octvr_hip.h")).read()
    hpp = open(os.path.join(inc, "octvr.hpp")).read()
    assert hpp.count("void set_output_format(int out_format)") == 2


def test_plane_shapes_match_the_reference_numpy(product_lib):
    ox = product_lib
    for fmt in R.LAYOUTS:
        assert ox.plane_shapes(fmt, 1036, 512) == R.plane_dims(fmt, 1036, 512), fmt
        assert ox.frame_shape(fmt, 1036, 512) == R.frame_dims(fmt, 1036, 512), fmt
        assert ox._pix_value(fmt) == R.VALUES[fmt]


def test_async_merge_pack_check_runs_clean():
    lib_dir = os.path.join(O.ROOT, "opencv-octvr_amd")
    subprocess.check_call(["make", "-s", "-C", lib_dir, "lib/async_merge_pack_check"])
    r = subprocess.run([os.path.join(lib_dir, "lib", "async_merge_pack_check")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out
    assert "async_merge_pack_check: ok" in out


def test_out_rules_of_the_10_bit_layouts_equal_yuv10_ref():
    w, h = 12, 6
    f = np.random.RandomState(5).randint(0, 256, (h * 3 // 2, w)).astype(np.uint8)
    f[0, :2] = (255, 0)
    for fmt in R10.LAYOUTS:
        assert np.array_equal(R.out_rule(fmt, f, w, h), R10.out_rule(fmt, f, w, h)), fmt


def test_out_rules_by_hand():
    """A 4 x 2 picture: Y = 1..8, U = (20, 21), V = (30, 31)."""
    f = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [20, 21, 30, 31]], np.uint8)
    assert R.out_rule("uyvy422", f, 4, 2).tolist() == [[20, 1, 30, 2, 21, 3, 31, 4], [20, 5, 30, 6, 21, 7, 31, 8]]
    assert R.out_rule("yuyv422", f, 4, 2).tolist() == [[1, 20, 2, 30, 3, 21, 4, 31], [5, 20, 6, 30, 7, 21, 8, 31]]
    assert R.out_rule("yuv422p", f, 4, 2).tolist() == [[1, 2, 3, 4], [5, 6, 7, 8], [20, 21, 30, 31], [20, 21, 30, 31]]
    assert R.out_rule("nv16", f, 4, 2).tolist() == [[1, 2, 3, 4], [5, 6, 7, 8], [20, 30, 21, 31], [20, 30, 21, 31]]
    assert R.out_rule("p010", f, 4, 2).tolist() == [[0, 1, 0, 2, 0, 3, 0, 4], [0, 5, 0, 6, 0, 7, 0, 8],
                                                    [0, 20, 0, 30, 0, 21, 0, 31]]
    assert R.out_rule("yuv420p10", f, 4, 2)[2].tolist() == [80, 0, 84, 0, 120, 0, 124, 0]


def test_region_placement_by_hand():
    """A 2 x 2 region at (2, 2) of an 8 x 4 frame, in one layout of each kind."""
    s = np.array([[1, 2], [3, 4], [9, 7]], np.uint8)  # Y rows, then [U | V]
    m = R.merged_frame("uyvy422", 8, 4, [(2, 2, s)])
    want = np.full((4, 16), R.FILL, np.uint8)
    want[2, 4:8], want[3, 4:8] = [9, 1, 7, 2], [9, 3, 7, 4]
    assert np.array_equal(m, want)
    m = R.merged_frame("nv16", 8, 4, [(2, 2, s)])
    want = np.full((8, 8), R.FILL, np.uint8)
    want[2, 2:4], want[3, 2:4], want[6, 2:4], want[7, 2:4] = [1, 2], [3, 4], [9, 7], [9, 7]
    assert np.array_equal(m, want)
    m = R.merged_frame("yuv420p10", 8, 4, [(2, 2, s)])
    want = np.full((6, 16), R.FILL, np.uint8)
    want[2, 4:8], want[3, 4:8] = [4, 0, 8, 0], [12, 0, 16, 0]
    want[5, 2:4], want[5, 10:12] = [36, 0], [28, 0]
    assert np.array_equal(m, want)
    assert [p.shape for p in R.planes_of("yuv420p10", m, 8, 4)] == [(4, 16), (2, 8), (2, 8)]


def test_odd_origin_region_passes_creation_rule():
    """x = 3 / 512 with half the width: creation accepts it (r.w even, c.w == r.w / 2) although r.x is odd and c.x is
    not its half — the region tests/test_gpu_async_out.py sees refused for UYVY."""
    reg = (3 / 512, 0.0, 0.5, 1.0)
    r, c = G._rect_mul_size(reg, 512, 256), G._rect_mul_size(reg, 256, 128)
    assert r[0] == 3 and r[2] % 2 == 0 and r[3] % 2 == 0 and c[2] == r[2] // 2 and c[3] == r[3] // 2
    assert r[0] % 2 == 1
