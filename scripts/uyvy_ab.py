#!/usr/bin/env python3
"""What packed UYVY 4:2:2 frames cost on the C2 rig (BASELINE.json configs[1]): the bench's frame sets stitched
planar in / planar out, NV12 in / NV12 out, UYVY in, UYVY out and both, at one and at three frames in flight,
interleaved, `--rounds` times each (default 3), `--steps` timed steps (default 300) after a preroll.  bench.py
has no format switch and is not changed; this reuses its helpers.

Per run one JSON line on stdout (and appended to --out): wall us per step and the stitch's event us per launch
(octvr_mapper_kernel_busy; with a UYVY side the events bracket the conversion launches and the gain feed too,
without one the composite alone, so event us of the two kinds do not subtract).  At the end one line per
conversion kernel: its time as the difference of the median wall us per step at one frame in flight — one
stream, the device never idle — between the run with the conversion and the NV12 run without it (the feed and
the composite between them are the same NV12 instances), and its bytes / time from octvr_mapper_info's
uyvy_in_bytes / uyvy_out_bytes plus the 4:2:0 bytes of the other side.  Before the runs, the full-size parity: UYVY in and out equals the planar stitch of the same pixels
rearranged by the two rules (torch, on the device).

  python scripts/uyvy_ab.py [--rounds 3] [--steps 300] [--out profiles/uyvy_ab.jsonl]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opencv-octvr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CONFIGS = [("yuv420p", "yuv420p"), ("nv12", "nv12"), ("uyvy422", "nv12"), ("nv12", "uyvy422"), ("uyvy422", "uyvy422")]


def to_nv12(t, w, h):
    out = t.clone()
    out[h:, 0::2] = t[h:, :w // 2]
    out[h:, 1::2] = t[h:, w // 2:]
    return out


def to_uyvy(t, w, h):
    """"Y over [U|V]" -> packed UYVY by the output rule (every chroma row on two packed rows), on the device."""
    import torch
    out = torch.empty((h, 2 * w), dtype=torch.uint8, device=t.device)
    out[:, 1::2] = t[:h, :w]
    out[:, 0::4] = t[h:, :w // 2].repeat_interleave(2, dim=0)
    out[:, 2::4] = t[h:, w // 2:w].repeat_interleave(2, dim=0)
    return out


def kernel_lines(lines, W, H):
    """One line per conversion kernel from the runs' lines (the first of which is the parity line)."""
    info = lines[0]

    def med(fi, fo):
        return statistics.median(d["us_per_step"] for d in lines
                                 if d.get("metric") == "uyvy_ab_C2" and d["frames_in_flight"] == 1 and (d["in"], d["out"]) == (fi, fo))

    out = []
    for name, with_, moved in (("uyvy_unpack_kernel", ("uyvy422", "nv12"), info["uyvy_in_bytes"] + info["footprint_bytes"]),
                               ("uyvy_pack_kernel", ("nv12", "uyvy422"), 1.5 * W * H + info["uyvy_out_bytes"])):
        us = med(*with_) - med("nv12", "nv12")
        out.append({"metric": "uyvy_kernel_C2", "kernel": name, "us": round(us, 2), "bytes": int(moved),
                    "tb_per_s": round(moved / us / 1e6, 3) if us > 0 else None,
                    "how": "median wall us per step at one frame in flight, with the conversion minus NV12 in / NV12 out"})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--preroll", type=float, default=0.5)
    ap.add_argument("--frame-sets", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import bench
    import octvr_amd as ox
    from octvr_amd import synthetic

    dev = 0
    torch.cuda.set_device(dev)
    rig, W, H, sizes = synthetic.CONFIGS["C2"]()
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H, use_roi=True, device=dev)
    m = ox.Mapper(mt, sizes, blend=0, enable_gain=True, device=dev)
    nsets = max(3, args.frame_sets)
    base = [torch.from_numpy(synthetic.yuv_frame(w, h, bench.frame_seed(0, 0, i))).to(f"cuda:{dev}")
            for i, (w, h) in enumerate(sizes)]
    planar = [base] + [bench.derive_set(base, [bench.frame_seed(0, j, i) for i in range(len(sizes))])
                       for j in range(1, nsets)]
    conv = {"yuv420p": lambda t, w, h: t, "nv12": to_nv12, "uyvy422": to_uyvy}
    sets = {k: [[f(t, w, h) for t, (w, h) in zip(fs, sizes)] for fs in planar] for k, f in conv.items()}
    refs = {k: [ox.Mapper.frame_refs(fs) for fs in v] for k, v in sets.items()}
    outs = {k: [torch.empty(ox.frame_shape(k, W, H), dtype=torch.uint8, device=f"cuda:{dev}") for _ in range(3)]
            for k in conv}
    streams = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(dev) for _ in range(2)]
    raw = [ctypes.c_void_p(st.cuda_stream) for st in streams]
    sha = bench.lib_sha256()

    def sync():
        torch.cuda.synchronize(dev)

    m.set_pixel_formats("yuv420p", "yuv420p")
    m.stitch(sets["yuv420p"][1], outs["yuv420p"][0])
    sync()
    g_planar = m.gains()
    m.set_pixel_formats("uyvy422", "uyvy422")
    m.stitch(sets["uyvy422"][1], outs["uyvy422"][0])
    sync()
    parity = bool(torch.equal(outs["uyvy422"][0], to_uyvy(outs["yuv420p"][0], W, H))) and m.gains() == g_planar
    info = m.info()
    lines = [{"metric": "uyvy_parity_C2", "equal": parity, "uyvy_runs": info["uyvy_runs"],
              "uyvy_in_bytes": info["uyvy_in_bytes"], "uyvy_out_bytes": info["uyvy_out_bytes"],
              "footprint_bytes": info["footprint_bytes"], "so_sha256": sha}]
    print(json.dumps(lines[0]), flush=True)
    if not parity:
        raise SystemExit("uyvy_ab: the UYVY output differs from the rearranged planar output")

    def run(fmt, inflight, rnd):
        m.set_frames_in_flight(inflight)
        m.set_pixel_formats(*fmt)
        r, o = refs[fmt[0]], outs[fmt[1]]

        def step(k):
            j = k % inflight
            m.stitch(r[k % nsets], o[j], stream=raw[j])

        for k in range(max(inflight, nsets) + args.warmup):
            step(k)
        sync()
        n_pre = bench.preroll(step, args.preroll, sync)
        m.kernel_time()
        m.set_timing(1)
        elapsed = bench.timed_region(step, args.steps, sync)
        m.set_timing(False)
        span_ms, busy_ms, launches = m.kernel_busy()
        return {"metric": "uyvy_ab_C2", "in": fmt[0], "out": fmt[1], "round": rnd, "steps": args.steps,
                "frames_in_flight": inflight, "preroll": {"s": args.preroll, "steps": n_pre},
                "us_per_step": round(elapsed * 1e6 / args.steps, 2),
                "event_us": round(span_ms * 1e3 / max(launches, 1), 2),
                "event_busy_us": round(busy_ms * 1e3 / max(launches, 1), 2), "launches": launches, "so_sha256": sha}

    for rnd in range(args.rounds):
        for inflight in (1, 3):
            for fmt in CONFIGS:
                d = run(fmt, inflight, rnd)
                lines.append(d)
                print(json.dumps(d), flush=True)

    for d in kernel_lines(lines, W, H):
        lines.append(d)
        print(json.dumps(d), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
