"""octvr_mapper_stitch_tensor without a GPU: the symbol, its declarations and wrappers, its NULL refusals, and
the tensor kernels' index arithmetic (opencv-octvr_amd/csrc/tensor_out_index.hpp) through
tests/cpp/tensor_out_check.cpp, a stand-alone program compiled with -fsanitize=address,undefined: every base
alignment 0..15, widths 1..40 and around the segment sizes, each element of the three windows stored exactly once
and nothing outside them, wide stores aligned."""
import ctypes as C
import os
import re
import subprocess

import oracle_py as O

ROOT = O.ROOT


def test_tensor_symbol_and_constants(product_lib):
    ox = product_lib
    assert hasattr(ox.lib(), "octvr_mapper_stitch_tensor")
    assert (ox.TENSOR_U8, ox.TENSOR_F16, ox.TENSOR_F32) == (0, 1, 2)
    assert callable(ox.Mapper.stitch_tensor)
    hdr = open(os.path.join(ROOT, "include", "octvr_hip.h")).read()
    assert re.search(r"enum\s*\{\s*OCTVR_TENSOR_U8 = 0,\s*OCTVR_TENSOR_F16 = 1,\s*OCTVR_TENSOR_F32 = 2\s*\}", hdr)
    assert re.search(r"^int octvr_mapper_stitch_tensor\(octvr_mapper\*", hdr, re.M)
    assert "typedef struct octvr_tensor_out" in hdr
    hpp = open(os.path.join(ROOT, "include", "octvr.hpp")).read()
    assert "struct TensorOut" in hpp and re.search(r"void stitch_tensor\(", hpp)


def test_tensor_struct_matches_the_header(product_lib):
    """ctypes lays TensorOut out as a C compiler lays out octvr_tensor_out (LP64)."""
    T = product_lib.TensorOut
    assert [(n, getattr(T, n).offset) for n, _ in T._fields_] == [
        ("dev", 0), ("w", 8), ("h", 12), ("dtype", 16), ("bgr", 20), ("row_stride", 24), ("plane_stride", 32),
        ("scale", 40), ("bias", 52)]
    assert C.sizeof(T) == 64


def test_tensor_refuses_null_without_a_device(product_lib):
    ox = product_lib
    f = ox.lib().octvr_mapper_stitch_tensor
    t = ox.TensorOut(None, 8, 8, ox.TENSOR_U8, 0, 8, 64, (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0))
    assert f(None, None, None, None, 0, None, None, 0, None) == ox.E_INVALID
    assert f(None, None, None, None, 0, C.byref(t), None, 0, None) == ox.E_INVALID  # dev NULL
    t.dev = 4096
    assert f(None, None, None, None, 0, C.byref(t), None, 0, None) == ox.E_INVALID  # mapper NULL
    assert ox.lib().octvr_last_error()


def test_tensor_out_check_runs_clean():
    lib_dir = os.path.join(ROOT, "opencv-octvr_amd")
    subprocess.check_call(["make", "-s", "-C", lib_dir, "lib/tensor_out_check"])
    r = subprocess.run([os.path.join(lib_dir, "lib", "tensor_out_check")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out
    assert "tensor_out_check ok" in out
