#!/usr/bin/env python3
"""The multi-band plan of two builds of the library, side by side: the multi-band keys of Mapper.info() (bands, the
rectangles, the remap's counts, traffic_parts, level_tiles) on the rigs of tests/test_gpu_blend_geometry.py and
tests/test_gpu_blend_seams.py, the benchmark's multi-band configuration (C3) and the golden rigs A-D, at blend 3, 5, 9 and
a feather blend, the multi-band blends also with OCTVR_MB_NO_DEEP and with OCTVR_MB_NO_REMAP_RESULT set; and the time
multiband_create takes on the benchmark's configuration.

  python scripts/mb_plan_ab.py --parent PARENT.so [--new NEW.so] [--out profiles/mb_plan_ab.jsonl]

Every run is a fresh child process under its own `timeout` (OCTVR_HIP_LIB selects the library); the first failure or
difference ends the script.  The creation time is Mapper(...) on a built template, five fresh processes per library,
parent and new alternating; the new median may exceed the parent's by no more than the parent's max - min."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opencv-octvr_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

KEYS = ["bands", "align_result_roi", "grid_roi", "full_cover", "crop", "traffic_parts", "level_tiles"]
BLENDS = [3, 5, 9, -3]
KNOBS = [None, "OCTVR_MB_NO_DEEP", "OCTVR_MB_NO_REMAP_RESULT"]
GOLDEN = ["rigA", "rigB", "rigC", "rigD"]


def mb_keys(info):
    return {k: v for k, v in info.items() if k in KEYS or k.startswith("remap_")}


def rigs(ox):
    """(name, template, input sizes) of every rig."""
    import oracle_py as O
    import test_gpu_blend_geometry as G
    import test_gpu_blend_seams as S
    from octvr_amd import synthetic
    for name in sorted(G.GEOMETRIES):
        t = G.make_rig(name)
        yield "geometry/" + name, G.template(ox, t), t["sizes"]
    for name in S.GEOS:
        for family in S.FAMILIES:
            t = S.seam_rig(name, family)
            yield "seams/" + t["name"], S.template(ox, t), t["sizes"]
    for name in GOLDEN:
        with open(os.path.join(ROOT, "tests", "golden", name + ".json")) as f:
            text = f.read()
        rig = json.loads(text)
        W, H = (int(v) for v in O.load_rig(name)[1]["out_size"])
        mt = ox.MapperTemplate.from_json(text, W, H, device=0)
        mt.create_masks(0)
        yield "golden/" + name, mt, [(c["options"]["width"], c["options"]["height"]) for c in rig["inputs"]]
    rig, W, H, sizes = synthetic.CONFIGS["C3"]()
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H, use_roi=True, device=0)
    mt.create_masks(0)
    yield "bench/C3", mt, sizes


def child_info():
    """One JSON object: rig -> blend -> knob -> the multi-band keys of info() (or the error a create raised)."""
    import octvr_amd as ox
    out = {}
    for name, mt, sizes in rigs(ox):
        for blend in BLENDS:
            for knob in KNOBS if blend > 0 else [None]:
                for k in KNOBS[1:]:
                    os.environ.pop(k, None)
                if knob:
                    os.environ[knob] = "1"
                try:
                    got = mb_keys(ox.Mapper(mt, sizes, blend=blend, enable_gain=True, device=0).info())
                except ox.OctvrError as e:  # a rig too small for the bands: both libraries must say the same
                    got = {"error": str(e)}
                out.setdefault(name, {}).setdefault(str(blend), {})[knob or "default"] = got
    print(json.dumps({"lib": lib_sha(ox), "info": out}))


def child_create():
    """One JSON object: seconds of Mapper(...) for the benchmark's multi-band configuration, on a built template."""
    import torch
    import octvr_amd as ox
    from octvr_amd import synthetic
    rig, W, H, sizes = synthetic.CONFIGS["C3"]()
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H, use_roi=True, device=0)
    mt.create_masks(0)
    torch.cuda.synchronize(0)
    t0 = time.perf_counter()
    m = ox.Mapper(mt, sizes, blend=synthetic.BLEND["C3"], enable_gain=synthetic.GAIN["C3"], device=0)
    torch.cuda.synchronize(0)
    dt = time.perf_counter() - t0
    print(json.dumps({"lib": lib_sha(ox), "create_s": dt, "bands": m.info()["bands"]}))


def lib_sha(ox):
    with open(ox.LIB_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def run_child(what, lib, limit):
    env = dict(os.environ)
    for k in ["OCTVR_HIP_LIB"] + KNOBS[1:]:
        env.pop(k, None)
    if lib:
        env["OCTVR_HIP_LIB"] = os.path.abspath(lib)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", what]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE)
    if r.returncode != 0:
        raise SystemExit("mb_plan_ab: the %s child of %s ended with %d" % (what, lib or "the tree's library", r.returncode))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the parent commit's liboctvr_hip.so")
    ap.add_argument("--new", default=None, help="this commit's (default: the tree's)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per child")
    args = ap.parse_args()
    if args.child:
        return child_info() if args.child == "info" else child_create()
    if not args.parent:
        ap.error("--parent is required")

    a, b = run_child("info", args.parent, args.timeout), run_child("info", args.new, args.timeout)
    cases, diffs = 0, []
    for rig in a["info"]:
        for blend in a["info"][rig]:
            for knob, want in a["info"][rig][blend].items():
                cases += 1
                if b["info"].get(rig, {}).get(blend, {}).get(knob) != want:
                    diffs.append("%s blend %s %s" % (rig, blend, knob))
    lines = [{"metric": "mb_plan_info_equal", "parent_lib": a["lib"], "new_lib": b["lib"], "rigs": len(a["info"]),
              "cases": cases, "errors_both": sum(1 for r in a["info"].values() for c in r.values() for v in c.values() if "error" in v),
              "equal": not diffs and a["info"].keys() == b["info"].keys(), "different": diffs[:20]}]
    print(json.dumps(lines[0]), flush=True)
    if not lines[0]["equal"]:
        raise SystemExit("mb_plan_ab: info() differs between the libraries")

    t = {"parent": [], "new": []}
    for _ in range(5):
        t["parent"].append(run_child("create", args.parent, 180)["create_s"])
        t["new"].append(run_child("create", args.new, 180)["create_s"])
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = max(t["parent"]) - min(t["parent"])
    lines.append({"metric": "mb_create_seconds_C3", "parent_s": [round(v, 4) for v in t["parent"]],
                  "new_s": [round(v, 4) for v in t["new"]], "parent_median_s": round(med["parent"], 4),
                  "new_median_s": round(med["new"], 4), "parent_spread_s": round(spread, 4),
                  "within_spread": med["new"] <= med["parent"] + spread,
                  "how": "Mapper(...) on a built template with masks, one creation per fresh process, parent and new alternating"})
    print(json.dumps(lines[1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")
    if not lines[1]["within_spread"]:
        raise SystemExit("mb_plan_ab: creation is slower than the parent's by more than its spread")


if __name__ == "__main__":
    main()
