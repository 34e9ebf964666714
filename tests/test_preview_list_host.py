"""The tap-list builder of preview_gather_kernel (opencv-octvr_amd/csrc/preview_list.hpp) on the CPU: builds
tests/cpp/preview_list_check.cpp, a stand-alone program compiled with -fsanitize=address,undefined, and runs it —
the coordinate table against a per-pixel loop (down-scale, identity, up-scale, odd sizes), the padding, the last
row and column clamps, and every listed entry being the LUT's own."""
import os
import subprocess

import oracle_py as O

ROOT = O.ROOT


def test_preview_list_check_runs_clean():
    lib_dir = os.path.join(ROOT, "opencv-octvr_amd")
    subprocess.check_call(["make", "-s", "-C", lib_dir, "lib/preview_list_check"])
    r = subprocess.run([os.path.join(lib_dir, "lib", "preview_list_check")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out
    assert "preview_list_check: ok" in out
