"""The multi-band / feather plan (opencv-octvr_amd/csrc/multiband_plan.hpp: rectangles, level-0 weights, block activity,
pixel owners, pyrUp tap tables, sub-tile kinds, required blocks, work lists, down items and remap jobs) on the CPU: builds
tests/cpp/multiband_plan_check.cpp, a stand-alone program compiled with -fsanitize=address,undefined, and runs it — two to
four cameras on outputs from 256 x 64 to 512 x 128 (partition seams at 1, 2 and 3 bands, graded seams, a grid origin above 0
with the crop cutting deep sub-tiles, camera origins off the 8-pixel block grid, one camera alone, feather with odd ROIs),
each multi-band rig with no knob, with no_deep and with no_remap_result, every rule restated pixel by pixel from up_taps
and the weights."""
import os
import subprocess

import oracle_py as O

ROOT = O.ROOT


def test_multiband_plan_check_runs_clean():
    lib_dir = os.path.join(ROOT, "opencv-octvr_amd")
    subprocess.check_call(["make", "-s", "-C", lib_dir, "lib/multiband_plan_check"])
    r = subprocess.run([os.path.join(lib_dir, "lib", "multiband_plan_check")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out
    assert out.rstrip().endswith("multiband_plan_check ok"), out
