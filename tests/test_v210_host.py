"""v210's arithmetic (opencv-octvr_amd/csrc/v210_layout.hpp: the work items and lane bodies of v210_unpack_kernel and
v210_pack_kernel; frame_layout.hpp: its frame shape, run table and run packing) on the CPU: builds
tests/cpp/v210_check.cpp, a stand-alone program compiled with -fsanitize=address,undefined, and runs it — every unpack
and pack item of widths 48, 96, 146, 148, 150, 190 and 256, heights 2 and 6, pitches row_bytes and row_bytes + 4, bases
0 and 4 (mod 16), from the caller's frame and from the packed upload, runs starting at each of the three group phases,
against exactly sized heap blocks and a per-sample restatement of the format."""
import os
import subprocess

import oracle_py as O

ROOT = O.ROOT


def test_v210_check_runs_clean():
    lib_dir = os.path.join(ROOT, "opencv-octvr_amd")
    subprocess.check_call(["make", "-s", "-C", lib_dir, "lib/v210_check"])
    r = subprocess.run([os.path.join(lib_dir, "lib", "v210_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=300)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out
    assert "v210_check ok" in out
