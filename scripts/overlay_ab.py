#!/usr/bin/env python3
"""What an overlay costs on the C2 rig (BASELINE.json configs[1]): the rig stitched without and with a nadir
overlay — a 1024 x 1024 pinhole frame looking straight down, half field of view 20 degrees (28 in the corners),
so equirect latitudes below about -70 (-62 in the corners) — interleaved, `--pairs` times each (default 3).

  blend0   blend 0, 3 frames in flight on 3 streams: the overlay is one more camera of the composite LUT,
           no extra pass is expected.
  c3       the C3 blend (multi-band, blend 16), one frame in flight, three variants:
             plain    no overlay, the blend writes YUV itself;
             result   no overlay, but stitched through the RGBA result frame (a 16 x 8 preview forces that
                      path; its own resize kernel is a few workgroups);
             overlay  the overlay: result-frame path plus overlay_apply_kernel (same preview).
           The stitch's HIP events (octvr_mapper_set_timing) bracket the whole sequence, so
           overlay - result is overlay_apply_kernel's own duration and result - plain the price of the
           result-frame path.

Per run one JSON line on stdout (and appended to --out): us per step (wall), the events' us per stitch, the
library's sha256.  bench.py is not changed; this reuses its helpers.

  python scripts/overlay_ab.py [--pairs 3] [--steps 300] [--out profiles/overlay_ab.jsonl]"""
import argparse
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opencv-octvr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

OV_SIZE = (1024, 1024)
PREVIEW = (16, 8)


def nadir_overlay():
    """A pinhole camera looking straight down (roll -pi/2 of the rig's frame)."""
    f = 512.0 / math.tan(math.radians(20.0))
    return {"type": "pinhole", "options": {"width": OV_SIZE[0], "height": OV_SIZE[1], "fx": f, "fy": f, "cx": 511.5,
                                           "cy": 511.5, "rotation": {"roll": -math.pi / 2, "yaw": 0.0, "pitch": 0.0}}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--preroll", type=float, default=0.3)
    ap.add_argument("--modes", default="blend0,c3")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import bench
    import octvr_amd as ox
    from octvr_amd import synthetic

    dev = 0
    torch.cuda.set_device(dev)
    rig, W, H, sizes = synthetic.CONFIGS["C2"]()
    with_ov = dict(rig, overlays=[nadir_overlay()])
    sha = bench.lib_sha256()
    frames = [torch.from_numpy(synthetic.yuv_frame(w, h, bench.frame_seed(0, 0, i))).to(f"cuda:{dev}")
              for i, (w, h) in enumerate(sizes + [OV_SIZE])]
    lines = []

    def sync():
        torch.cuda.synchronize(dev)

    def emit(d):
        d["so_sha256"] = sha
        lines.append(d)
        print(json.dumps(d), flush=True)

    def make(r, blend, inflight):
        mt = ox.MapperTemplate.from_json(json.dumps(r), W, H, use_roi=True, device=dev)
        k = mt.num_overlays
        if blend:
            mt.create_masks(dev)
        m = ox.Mapper(mt, sizes + [OV_SIZE] * k, blend=blend, enable_gain=True, device=dev)
        if inflight > 1:
            m.set_frames_in_flight(inflight)
        return m, ox.Mapper.frame_refs(frames[:len(sizes) + k])

    def run(m, refs, inflight, preview):
        outs = [torch.empty((H * 3 // 2, W), dtype=torch.uint8, device=f"cuda:{dev}") for _ in range(inflight)]
        streams = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(dev) for _ in range(inflight - 1)]
        raw = [ctypes.c_void_p(st.cuda_stream) for st in streams]
        pv = torch.empty((PREVIEW[1], PREVIEW[0], 3), dtype=torch.uint8, device=f"cuda:{dev}") if preview else None

        def step(k):
            j = k % inflight
            m.stitch(refs, outs[j], stream=raw[j], preview=pv)

        for k in range(inflight + args.warmup):
            step(k)
        sync()
        n_pre = bench.preroll(step, args.preroll, sync)
        m.kernel_time()
        m.set_timing(1)
        elapsed = bench.timed_region(step, args.steps, sync)
        m.set_timing(False)
        span_ms, busy_ms, launches = m.kernel_busy()
        return {"steps": args.steps, "frames_in_flight": inflight, "preroll_steps": n_pre,
                "us_per_step": round(elapsed * 1e6 / args.steps, 2),
                "events_us_per_stitch": round(span_ms * 1e3 / max(launches, 1), 2),
                "events_busy_us_per_stitch": round(busy_ms * 1e3 / max(launches, 1), 2)}

    modes = args.modes.split(",")
    if "blend0" in modes:
        plain, overlay = make(rig, 0, 3), make(with_ov, 0, 3)
        info = overlay[0].info()
        emit({"metric": "overlay_ab_info", "mode": "blend0", "overlays": info["overlays"], "wide_tiles": info["wide_tiles"],
              "traffic_plain": plain[0].traffic_bytes(), "traffic_overlay": overlay[0].traffic_bytes()})
        for pair in range(args.pairs):
            for name, (m, refs) in (("plain", plain), ("overlay", overlay)):
                emit(dict(run(m, refs, 3, False), metric="overlay_ab", mode="blend0", variant=name, pair=pair))
        del plain, overlay
    if "c3" in modes:
        plain, overlay = make(rig, 16, 1), make(with_ov, 16, 1)
        info = overlay[0].info()
        emit({"metric": "overlay_ab_info", "mode": "c3", "overlays": info["overlays"],
              "overlay_groups": info["overlay_groups"], "overlay_px": info["overlay_px"],
              "traffic_plain": plain[0].traffic_bytes(), "traffic_overlay": overlay[0].traffic_bytes()})
        for pair in range(args.pairs):
            for name, (m, refs), pv in (("plain", plain, False), ("result", plain, True), ("overlay", overlay, True)):
                emit(dict(run(m, refs, 1, pv), metric="overlay_ab", mode="c3", variant=name, pair=pair))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
