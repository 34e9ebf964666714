#!/usr/bin/env python3
"""What a preview costs a blend-0 mapper on the C2 rig (BASELINE.json configs[1]) with a 1280 x 640 preview:
the parent commit's library, which stitches every preview through the RGBA result frame with one frame in
flight, against this library with the preview prepared (octvr_mapper_prepare_preview: the plain composite plus
preview_gather_kernel), one and three frames in flight.  Every run is a fresh child process (OCTVR_HIP_LIB
selects the library), the two libraries interleaved, `--rounds` times each (default 3).

  python scripts/preview_ab.py --against PARENT_LIB [--rounds 3] [--steps 300] [--out profiles/preview_ab.jsonl]
  python scripts/preview_ab.py --child    (what --against starts, once per library and round)

A child runs, on one mapper and the same frames, after a preroll:
  plain      no preview, 1 and 3 frames in flight: the composite alone;
  result     a preview of a size that is not prepared: the result-frame path (one frame in flight; the only
             preview path of a library without octvr_mapper_prepare_preview);
  prepared   the prepared preview, 1 and 3 frames in flight (this library only).
Per run one JSON line: wall us per step, the stitch's HIP events' us per stitch (octvr_mapper_set_timing: they
bracket the composite alone without a preview, the composite and the preview kernel(s) with one), the library's
sha256.  prepared - plain is the gather kernel's term; the summary line gives the medians.  bench.py is not
changed; this reuses its helpers."""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opencv-octvr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PREVIEW = (1280, 640)


def child(args):
    import torch
    import bench
    import octvr_amd as ox
    from octvr_amd import synthetic

    dev = 0
    torch.cuda.set_device(dev)
    rig, W, H, sizes = synthetic.CONFIGS["C2"]()
    with open(ox.LIB_PATH, "rb") as f:  # the library this child loaded (OCTVR_HIP_LIB or the tree's)
        sha = hashlib.sha256(f.read()).hexdigest()
    frames = [torch.from_numpy(synthetic.yuv_frame(w, h, bench.frame_seed(0, 0, i))).to(f"cuda:{dev}")
              for i, (w, h) in enumerate(sizes)]
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H, use_roi=True, device=dev)
    m = ox.Mapper(mt, sizes, blend=0, enable_gain=True, device=dev)
    refs = ox.Mapper.frame_refs(frames)
    can_prepare = hasattr(ox.lib(), "octvr_mapper_prepare_preview")

    def sync():
        torch.cuda.synchronize(dev)

    def run(variant, inflight):
        m.set_frames_in_flight(inflight)
        outs = [torch.empty((H * 3 // 2, W), dtype=torch.uint8, device=f"cuda:{dev}") for _ in range(inflight)]
        streams = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(dev) for _ in range(inflight - 1)]
        raw = [ctypes.c_void_p(st.cuda_stream) for st in streams]
        pvs = [torch.empty((PREVIEW[1], PREVIEW[0], 3), dtype=torch.uint8, device=f"cuda:{dev}")
               for _ in range(inflight)] if variant != "plain" else [None] * inflight

        def step(k):
            j = k % inflight
            m.stitch(refs, outs[j], stream=raw[j], preview=pvs[j])

        for k in range(inflight + args.warmup):
            step(k)
        sync()
        n_pre = bench.preroll(step, args.preroll, sync)
        m.kernel_time()
        m.set_timing(1)
        elapsed = bench.timed_region(step, args.steps, sync)
        m.set_timing(False)
        span_ms, busy_ms, launches = m.kernel_busy()
        d = {"metric": "preview_ab", "config": "C2", "preview": list(PREVIEW), "lib": args.tag, "variant": variant,
             "round": args.round, "steps": args.steps, "frames_in_flight": inflight, "preroll_steps": n_pre,
             "us_per_step": round(elapsed * 1e6 / args.steps, 2),
             "events_us_per_stitch": round(span_ms * 1e3 / max(launches, 1), 2),
             "events_busy_us_per_stitch": round(busy_ms * 1e3 / max(launches, 1), 2), "so_sha256": sha}
        if can_prepare:
            d["preview_prepared"] = m.info()["preview_prepared"]
        print(json.dumps(d), flush=True)

    run("plain", 1)
    run("plain", 3)
    run("result", 1)  # nothing prepared yet: the result-frame path in either library
    if can_prepare:
        m.prepare_preview(*PREVIEW)
        run("prepared", 1)
        run("prepared", 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", default=None, help="the parent commit's liboctvr_hip.so")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tag", default="this")
    ap.add_argument("--round", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--preroll", type=float, default=0.3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.against or not os.path.exists(args.against):
        sys.exit("--against PARENT_LIB: the parent commit's liboctvr_hip.so")
    lines = []
    for rnd in range(args.rounds):
        for tag, lib in (("parent", os.path.abspath(args.against)), ("this", None)):
            env = dict(os.environ)
            env.pop("OCTVR_HIP_LIB", None)
            if lib:
                env["OCTVR_HIP_LIB"] = lib
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tag", tag, "--round", str(rnd), "--steps",
                   str(args.steps), "--warmup", str(args.warmup), "--preroll", str(args.preroll)]
            # a fresh child per library and round; a child that fails or runs over ends the whole comparison
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=args.timeout)
            sys.stdout.write(r.stdout.decode())
            sys.stdout.flush()
            if r.returncode != 0:
                sys.exit("child %s (round %d) exited with %d" % (tag, rnd, r.returncode))
            lines += [json.loads(l) for l in r.stdout.decode().splitlines() if l.startswith("{")]

    def med(lib, variant, inflight, key):
        v = [d[key] for d in lines if d["lib"] == lib and d["variant"] == variant and d["frames_in_flight"] == inflight]
        return round(statistics.median(v), 2) if v else None

    summary = {"metric": "preview_ab_summary", "config": "C2", "preview": list(PREVIEW), "rounds": args.rounds,
               "steps": args.steps}
    for lib, variant, k in (("parent", "plain", 1), ("parent", "plain", 3), ("parent", "result", 1), ("this", "plain", 1),
                            ("this", "plain", 3), ("this", "result", 1), ("this", "prepared", 1), ("this", "prepared", 3)):
        summary["%s_%s_%d" % (lib, variant, k)] = {"us_per_step": med(lib, variant, k, "us_per_step"),
                                                   "events_us_per_stitch": med(lib, variant, k, "events_us_per_stitch")}
    a, b = summary["this_prepared_1"]["events_us_per_stitch"], summary["this_plain_1"]["events_us_per_stitch"]
    summary["gather_term_events_us"] = round(a - b, 2) if a is not None and b is not None else None
    print(json.dumps(summary), flush=True)
    lines.append(summary)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
