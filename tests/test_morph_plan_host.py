"""The morph's per-camera plan (opencv-octvr_amd/csrc/morph_plan.hpp: cv::Subdiv2D triangles, warpAffine matrices, the
int16 owner raster over csrc/fill_poly.hpp) on the CPU: builds tests/cpp/morph_plan_check.cpp, a stand-alone program
compiled with -fsanitize=address,undefined, and runs it — destination corners off every side of the raster, triangles
wholly outside, rasters one pixel wide or high, duplicate and collinear vertices, singular destination triangles; the
owner map against the last triangle whose full-raster fill covers each pixel."""
import os
import subprocess

import oracle_py as O

ROOT = O.ROOT


def test_morph_plan_check_runs_clean():
    lib_dir = os.path.join(ROOT, "opencv-octvr_amd")
    subprocess.check_call(["make", "-s", "-C", lib_dir, "lib/morph_plan_check"])
    r = subprocess.run([os.path.join(lib_dir, "lib", "morph_plan_check")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out
    assert out.rstrip().endswith("morph_plan_check ok"), out
