#!/usr/bin/env python3
"""AsyncMultiMapper end to end on the C2 rig with NV12 host planes against planar ones, registered outputs,
3 frames in flight (the shape of bench.async_e2e), one JSON line per timed run:

  python scripts/async_nv12_ab.py [--frames N] [--out FILE]
      formats: one planar/planar and one NV12/NV12 pipeline on the loaded library, timed alternately, three
      pairs planar-first and three NV12-first; the frames' NV12 form is prepared before the timed region.
      Then once the host conversion an NV12 user pays without the feature: numpy de-interleave of the six
      inputs plus interleave of the output, per frame.
  python scripts/async_nv12_ab.py --against PARENT_LIB [--frames N] [--out FILE]
      planar only, this tree's library against PARENT_LIB (a liboctvr_hip.so of the parent commit): one fresh
      child process per run (OCTVR_HIP_LIB selects the library), three pairs in each order; the last line
      says whether this library's median lies inside the parent's own min-max.
  python scripts/async_nv12_ab.py --child LABEL      (what --against starts)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "opencv-octvr_amd"))


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def interleave(u, v):
    import numpy as np
    uv = np.empty((u.shape[0], 2 * u.shape[1]), np.uint8)
    uv[:, 0::2] = u
    uv[:, 1::2] = v
    return uv


class Pipe:
    """One C2 pipeline in one format with its input planes and a registered ring of four outputs."""

    def __init__(self, ox, mt, sizes, W, H, frames_np, fmt):
        import numpy as np
        self.am = ox.AsyncMultiMapper([mt], sizes, (W, H), [0], [0], [(0.0, 0.0, 1.0, 1.0)], device=0)
        self.fmt = fmt
        planar = [(f[:h], f[h:, :w // 2], f[h:, w // 2:]) for f, (w, h) in zip(frames_np, sizes)]
        if fmt == "nv12":
            self.am.set_pixel_formats("nv12", "nv12")
            self.ins = [(y, interleave(u, v)) for y, u, v in planar]
            # an NV12 output frame is one allocation: Y rows, then U,V rows
            bufs = [np.empty((H * 3 // 2, W), np.uint8) for _ in range(4)]
            self.outs = [(b[:H], b[H:]) for b in bufs]
        else:
            self.ins = planar
            self.outs = [(np.empty((H, W), np.uint8), np.empty((H // 2, W // 2), np.uint8),
                          np.empty((H // 2, W // 2), np.uint8)) for _ in range(4)]
        for o in self.outs:
            self.am.register_output(o)
        self.px = W * H
        self.run(4)  # warm-up: pinned buffers, first touch

    def run(self, n):
        am = self.am
        for k in range(n):
            am.push(self.ins, self.outs[k % 4])
            if am.pending() >= 3:
                am.pop()
        while am.pending():
            am.pop()

    def timed(self, n):
        t0 = time.perf_counter()
        self.run(n)
        dt = time.perf_counter() - t0
        return {"fmt": self.fmt, "frames": n, "mp_s": round(n * self.px / 1e6 / dt, 1), "ms_per_frame": round(dt * 1e3 / n, 3)}


def setup():
    import bench
    import octvr_amd as ox
    from octvr_amd import synthetic
    rig, W, H, sizes = synthetic.CONFIGS["C2"]()
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H, use_roi=True, device=0)
    frames = [synthetic.yuv_frame(w, h, bench.frame_seed(0, 0, i)) for i, (w, h) in enumerate(sizes)]
    return ox, mt, sizes, W, H, frames


def host_conversion(sizes, W, H, frames_np, reps=9):
    """ms per frame of what an NV12 integrator does on the host around a planar-only pipeline."""
    import numpy as np
    nv = [(f[:h].copy(), interleave(f[h:, :w // 2], f[h:, w // 2:])) for f, (w, h) in zip(frames_np, sizes)]
    u_out = np.zeros((H // 2, W // 2), np.uint8)
    v_out = np.zeros((H // 2, W // 2), np.uint8)
    uv_out = np.empty((H // 2, W), np.uint8)
    us = [np.empty((h // 2, w // 2), np.uint8) for w, h in sizes]
    vs = [np.empty((h // 2, w // 2), np.uint8) for w, h in sizes]
    t_in, t_out = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        for (y, uv), u, v in zip(nv, us, vs):
            u[:] = uv[:, 0::2]
            v[:] = uv[:, 1::2]
        t1 = time.perf_counter()
        uv_out[:, 0::2] = u_out
        uv_out[:, 1::2] = v_out
        t2 = time.perf_counter()
        t_in.append((t1 - t0) * 1e3)
        t_out.append((t2 - t1) * 1e3)
    return {"kind": "host_conversion", "deinterleave_inputs_ms": round(statistics.median(t_in), 3),
            "interleave_output_ms": round(statistics.median(t_out), 3),
            "total_ms_per_frame": round(statistics.median(t_in) + statistics.median(t_out), 3), "reps": reps}


def formats(args):
    ox, mt, sizes, W, H, frames = setup()
    pipes = {f: Pipe(ox, mt, sizes, W, H, frames, f) for f in ("yuv420p", "nv12")}
    info = pipes["nv12"].am.info()
    emit({"kind": "setup", "rig": "C2", "out": [W, H], "packed_bytes": info["packed_bytes"], "runs": info["runs"],
          "output_bytes": info["output_bytes"]}, args.out)
    res = {"yuv420p": [], "nv12": []}
    for order in [("yuv420p", "nv12")] * 3 + [("nv12", "yuv420p")] * 3:
        for f in order:
            r = pipes[f].timed(args.frames)
            r.update(kind="formats", first=order[0])
            res[f].append(r["mp_s"])
            emit(r, args.out)
    for p in pipes.values():
        p.am.close()
    emit({"kind": "formats_summary",
          **{f: {"median": statistics.median(v), "min": min(v), "max": max(v)} for f, v in res.items()},
          "nv12_over_planar": round(statistics.median(res["nv12"]) / statistics.median(res["yuv420p"]), 4)}, args.out)
    emit(host_conversion(sizes, W, H, frames), args.out)


def child(args):
    ox, mt, sizes, W, H, frames = setup()
    p = Pipe(ox, mt, sizes, W, H, frames, "yuv420p")
    r = p.timed(args.frames)
    p.am.close()
    r.update(kind="planar_vs_parent", lib=args.child)
    print("RESULT " + json.dumps(r), flush=True)


def against(args):
    libs = {"this": os.path.join(ROOT, "opencv-octvr_amd", "lib", "liboctvr_hip.so"), "parent": os.path.abspath(args.against)}
    res = {"this": [], "parent": []}
    for order in [("this", "parent")] * 3 + [("parent", "this")] * 3:
        for lab in order:
            env = dict(os.environ, OCTVR_HIP_LIB=libs[lab])
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lab, "--frames", str(args.frames)],
                                 env=env, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                sys.exit("child %s failed (%d): %s" % (lab, out.returncode, out.stderr[-2000:]))
            r = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            r["first"] = order[0]
            res[lab].append(r["mp_s"])
            emit(r, args.out)
    med = statistics.median(res["this"])
    emit({"kind": "planar_vs_parent_summary", "this": {"median": med, "min": min(res["this"]), "max": max(res["this"])},
          "parent": {"median": statistics.median(res["parent"]), "min": min(res["parent"]), "max": max(res["parent"])},
          "this_median_inside_parent_min_max": min(res["parent"]) <= med <= max(res["parent"])}, args.out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--out")
    ap.add_argument("--against")
    ap.add_argument("--child")
    a = ap.parse_args()
    child(a) if a.child else against(a) if a.against else formats(a)
