"""The arithmetic of the YUYV / YUV422P / NV16 conversions (opencv-octvr_amd/csrc/yuv422_host.hpp: the lane bodies of
yuv422_unpack_kernel and yuv422_pack_kernel, the run packing of the pipeline's copy-in) on the CPU: builds
tests/cpp/yuv422_check.cpp, a stand-alone program compiled with -fsanitize=address,undefined, and runs it — for
each layout every work item of widths 8k .. 8k + 6, pitches minimal and minimal + 6 and base alignments 0-15
against exactly sized heap blocks: every footprint byte written once with the right value, nothing else written,
nothing read outside."""
import os
import subprocess

import oracle_py as O

ROOT = O.ROOT


def test_yuv422_check_runs_clean():
    lib_dir = os.path.join(ROOT, "opencv-octvr_amd")
    subprocess.check_call(["make", "-s", "-C", lib_dir, "lib/yuv422_check"])
    r = subprocess.run([os.path.join(lib_dir, "lib", "yuv422_check")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out
    assert "yuv422_check ok" in out
