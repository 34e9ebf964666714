"""The arithmetic of the 10-bit conversions (opencv-octvr_amd/csrc/yuv10_host.hpp: the lane bodies of
yuv10_unpack_kernel and yuv10_pack_kernel, the run packing of the pipeline's copy-in, the format's own run table) on
the CPU: builds tests/cpp/yuv10_check.cpp, a stand-alone program compiled with -fsanitize=address,undefined, and
runs it — for P010, YUV420P10, P210 and YUV422P10 every work item of widths 8k .. 8k + 6, 328, 330 and 332, pitches
minimal and minimal + 6 and every 2-byte base alignment within 16 against exactly sized heap blocks: every footprint
byte written once with the rule's value, nothing else written, nothing read outside, every vector store aligned,
out-then-in the identity.  The programs of the 8-bit 4:2:2 conversions still build and pass: their run table is
shared."""
import os
import subprocess

import pytest

import oracle_py as O

ROOT = O.ROOT


def _run(name):
    lib_dir = os.path.join(ROOT, "opencv-octvr_amd")
    subprocess.check_call(["make", "-s", "-C", lib_dir, "lib/" + name])
    r = subprocess.run([os.path.join(lib_dir, "lib", name)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out
    assert name + " ok" in out


def test_yuv10_check_runs_clean():
    _run("yuv10_check")


@pytest.mark.parametrize("name", ["uyvy_runs_check", "yuv422_check"])
def test_yuv10_leaves_the_422_checks_passing(name):
    _run(name)
