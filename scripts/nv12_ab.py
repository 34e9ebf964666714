#!/usr/bin/env python3
"""NV12 against planar on the C2 rig (BASELINE.json configs[1]): the bench's workload — its frame sets
(bench.frame_seed / derive_set, 8 sets), 3 frames in flight on 3 streams, 0.5 s of preroll, 1,000 timed steps
— stitched planar in / planar out and NV12 in / NV12 out, interleaved, `--pairs` times each (default 3).
bench.py has no format switch and is not changed; this reuses its helpers.

Per run one JSON line on stdout (and appended to --out): us per step (wall), the composite's busy time per
launch (octvr_mapper_kernel_busy: the union of the launches' intervals), MP/s, and the library's sha256.
Before the runs, the full-size parity: the NV12/NV12 output of one C2 frame equals the planar output with the
chroma bytes rearranged (torch, on the device).

  python scripts/nv12_ab.py [--pairs 3] [--steps 1000] [--out profiles/nv12_ab_C2.jsonl]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opencv-octvr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def to_nv12(t, w, h):
    """"Y over [U|V]" -> NV12 on the device."""
    import torch
    out = t.clone()
    out[h:, 0::2] = t[h:, :w // 2]
    out[h:, 1::2] = t[h:, w // 2:]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--preroll", type=float, default=0.5)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--frame-sets", type=int, default=8)
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
    inflight = args.inflight
    m.set_frames_in_flight(inflight)
    nsets = max(inflight, args.frame_sets)
    base = [torch.from_numpy(synthetic.yuv_frame(w, h, bench.frame_seed(0, 0, i))).to(f"cuda:{dev}")
            for i, (w, h) in enumerate(sizes)]
    planar = [base] + [bench.derive_set(base, [bench.frame_seed(0, j, i) for i in range(len(sizes))])
                       for j in range(1, nsets)]
    sets = {"yuv420p": planar,
            "nv12": [[to_nv12(t, w, h) for t, (w, h) in zip(fs, sizes)] for fs in planar]}
    outs = [torch.empty((H * 3 // 2, W), dtype=torch.uint8, device=f"cuda:{dev}") for _ in range(inflight)]
    streams = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(dev) for _ in range(inflight - 1)]
    raw = [ctypes.c_void_p(st.cuda_stream) for st in streams]
    refs = {k: [ox.Mapper.frame_refs(fs) for fs in v] for k, v in sets.items()}
    sha = bench.lib_sha256()

    def sync():
        torch.cuda.synchronize(dev)

    # full-size parity, once: NV12 in / NV12 out = the planar stitch with the chroma bytes rearranged
    a, b = outs[0], outs[1]
    m.set_pixel_formats("yuv420p", "yuv420p")
    m.stitch(sets["yuv420p"][1], a)
    sync()
    g_planar = m.gains()
    m.set_pixel_formats("nv12", "nv12")
    m.stitch(sets["nv12"][1], b)
    sync()
    parity = bool(torch.equal(b, to_nv12(a, W, H))) and m.gains() == g_planar
    lines = [{"metric": "nv12_parity_C2", "equal": parity, "so_sha256": sha}]
    print(json.dumps(lines[0]), flush=True)
    if not parity:
        raise SystemExit("nv12_ab: the NV12/NV12 output differs from the permuted planar output")

    def run(fmt, pair):
        m.set_pixel_formats(fmt, fmt)
        r = refs[fmt]

        def step(k):
            j = k % inflight
            m.stitch(r[k % nsets], outs[j], stream=raw[j])

        for j in range(max(inflight, nsets)):
            step(j)
        sync()
        for k in range(args.warmup):
            step(k)
        sync()
        n_pre = bench.preroll(step, args.preroll, sync)
        m.kernel_time()
        m.set_timing(1)
        elapsed = bench.timed_region(step, args.steps, sync)
        m.set_timing(False)
        span_ms, busy_ms, launches = m.kernel_busy()
        return {"metric": "nv12_ab_C2", "format": fmt, "pair": pair, "steps": args.steps, "frames_in_flight": inflight,
                "preroll": {"s": args.preroll, "steps": n_pre}, "us_per_step": round(elapsed * 1e6 / args.steps, 2),
                "composite_busy_us": round(busy_ms * 1e3 / max(launches, 1), 2),
                "composite_span_us": round(span_ms * 1e3 / max(launches, 1), 2), "launches": launches,
                "mp_per_s": round(W * H * args.steps / elapsed / 1e6, 1), "so_sha256": sha}

    for pair in range(args.pairs):
        for fmt in ("yuv420p", "nv12"):
            d = run(fmt, pair)
            lines.append(d)
            print(json.dumps(d), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
