"""The arithmetic of the packed UYVY conversions (opencv-octvr_amd/csrc/uyvy_host.hpp: the work items of
uyvy_unpack_kernel and uyvy_pack_kernel, the run packing of the pipeline's copy-in) on the CPU: builds
tests/cpp/uyvy_runs_check.cpp, a stand-alone program compiled with -fsanitize=address,undefined, and runs it —
every work item of widths 8k .. 8k + 6, pitches 2 W and 2 W + 6 and base alignments 0-15 against exactly sized
heap blocks: every footprint byte written once with the right value, nothing else written, nothing read outside."""
import os
import subprocess

import oracle_py as O

ROOT = O.ROOT


def test_uyvy_runs_check_runs_clean():
    lib_dir = os.path.join(ROOT, "opencv-octvr_amd")
    subprocess.check_call(["make", "-s", "-C", lib_dir, "lib/uyvy_runs_check"])
    r = subprocess.run([os.path.join(lib_dir, "lib", "uyvy_runs_check")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out
    assert "uyvy_runs_check ok" in out
