#!/usr/bin/env python3
"""AsyncMultiMapper.push_device (device frames in and out) on the C2 rig against the host path and against
the bare mapper, and the host path against the parent commit's library; one JSON line per timed run.  Every
run is a fresh child process (OCTVR_HIP_LIB selects the library), 3 frames in flight as in bench.async_e2e.

  python scripts/async_device_ab.py --against PARENT_LIB [--frames N] [--out FILE]
      1. host path (scripts/async_nv12_ab.py's planar pipeline with registered outputs), this library
         against PARENT_LIB, three pairs in each order; the summary says whether this library's median lies
         inside the parent's own min-max;
      2. in the same job: PARENT_LIB's Mapper.stitch with one frame in flight (the pipeline serialises its
         stitches on one compute stream, so this is its ceiling), this library's push_device on the same single
         full-frame region (stitched in place, no merge), and push_device with two template-size regions stacked
         into a W x 2H frame (one merge launch per frame), three runs each; the summary gives the ratios.
  python scripts/async_device_ab.py --child KIND      (what --against starts: host, mapper, device, stacked)
      `--child stacked` under a kernel trace gives merge_regions_kernel's time per frame; the bytes it moves
      are in the run's JSON line ("merge_bytes": read + written).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import async_nv12_ab as base  # noqa: E402  (setup, Pipe, emit; puts the repository on sys.path)

ROOT = base.ROOT


def device_frames(frames):
    import numpy as np
    import torch
    return [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames]


def child(args):
    import torch
    ox, mt, sizes, W, H, frames = base.setup()
    n = args.frames
    rec = {"kind": args.child, "frames": n}
    if args.child == "host":
        p = base.Pipe(ox, mt, sizes, W, H, frames, "yuv420p")
        rec.update(p.timed(n))
        p.am.close()
    elif args.child == "mapper":
        m = ox.Mapper(mt, sizes, blend=0, enable_gain=True, device=0)
        ins = ox.Mapper.frame_refs(device_frames(frames))
        out = torch.empty((H * 3 // 2, W), dtype=torch.uint8, device="cuda")
        for _ in range(4):
            m.stitch(ins, out)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):  # one frame in flight
            m.stitch(ins, out)
            torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rec.update(mp_s=round(n * W * H / 1e6 / dt, 1), ms_per_frame=round(dt * 1e3 / n, 3))
    else:
        stacked = args.child == "stacked"
        OH = 2 * H if stacked else H
        k = 2 if stacked else 1
        regions = [(0.0, 0.0, 1.0, 0.5), (0.0, 0.5, 1.0, 0.5)] if stacked else [(0.0, 0.0, 1.0, 1.0)]
        am = ox.AsyncMultiMapper([mt] * k, sizes, (W, OH), [0] * k, [0] * k, regions, device=0)
        ins = device_frames(frames)
        outs = [torch.empty((OH * 3 // 2, W), dtype=torch.uint8, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()

        def run(count):
            for f in range(count):
                am.push_device(ins, outs[f % 4])
                if am.pending() >= 3:
                    am.pop()
            while am.pending():
                am.pop()

        run(4)
        t0 = time.perf_counter()
        run(n)
        dt = time.perf_counter() - t0
        info = am.info()
        am.close()
        rec.update(mp_s=round(n * W * OH / 1e6 / dt, 1), ms_per_frame=round(dt * 1e3 / n, 3), out=[W, OH],
                   merge_launches=info["merge_launches"], device_frames=info["device_frames"],
                   merge_bytes=2 * W * OH * 3 // 2 if stacked else 0)
    print("RESULT " + json.dumps(rec), flush=True)


def run_child(kind, lib, frames):
    env = dict(os.environ, OCTVR_HIP_LIB=lib)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--frames", str(frames)], env=env,
                         capture_output=True, text=True, timeout=300)
    if out.returncode != 0:
        sys.exit("child %s failed (%d): %s" % (kind, out.returncode, out.stderr[-2000:]))
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def against(args):
    libs = {"this": os.path.join(ROOT, "opencv-octvr_amd", "lib", "liboctvr_hip.so"), "parent": os.path.abspath(args.against)}
    res = {"this": [], "parent": []}
    for order in [("this", "parent")] * 3 + [("parent", "this")] * 3:
        for lab in order:
            r = run_child("host", libs[lab], args.frames)
            r.update(lib=lab, first=order[0])
            res[lab].append(r["mp_s"])
            base.emit(r, args.out)
    med = statistics.median(res["this"])
    base.emit({"kind": "host_vs_parent_summary", "this": spread(res["this"]), "parent": spread(res["parent"]),
               "this_median_inside_parent_min_max": min(res["parent"]) <= med <= max(res["parent"])}, args.out)
    runs = {"mapper": [], "device": [], "stacked": []}
    for _ in range(3):
        for kind in runs:
            r = run_child(kind, libs["parent" if kind == "mapper" else "this"], args.frames)
            r["lib"] = "parent" if kind == "mapper" else "this"
            runs[kind].append(r["mp_s"])
            base.emit(r, args.out)
    host, ceil, dev = statistics.median(res["parent"]), statistics.median(runs["mapper"]), statistics.median(runs["device"])
    base.emit({"kind": "device_summary", "parent_host_path_mp_s": host, "parent_mapper_one_in_flight_mp_s": ceil,
               "push_device_mp_s": spread(runs["device"]), "push_device_stacked_mp_s": spread(runs["stacked"]),
               "push_device_over_host_path": round(dev / host, 2), "push_device_over_mapper": round(dev / ceil, 3)}, args.out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--out")
    ap.add_argument("--against")
    ap.add_argument("--child", choices=["host", "mapper", "device", "stacked"])
    a = ap.parse_args()
    if a.child:
        child(a)
    elif a.against:
        against(a)
    else:
        ap.error("--against PARENT_LIB or --child KIND")
