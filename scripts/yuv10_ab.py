#!/usr/bin/env python3
"""What the 10-bit layouts cost on the C2 rig (BASELINE.json configs[1]): the bench's frame sets stitched with each of
"uyvy422" (the 8-bit yardstick: uyvy.hip's kernels), "p010", "yuv420p10", "p210" and "yuv422p10" on both sides, the
formats interleaved, `--rounds` times `--steps` stitches each at one frame in flight.  Per format it prints one JSON
line with the stitch's own HIP-event times (octvr_mapper_set_timing: the events bracket the unpack, the stitch and the
pack) in three configurations — format in and out, in only, out only — and the planar stitch timed the same way,
so unpack = in-only - planar and pack = out-only - planar (medians), next to the bytes the conversions move
(octvr_mapper_info).  Before the runs, the full-size parity of every layout: in and out equals the planar stitch of
the same pixels rearranged by the two rules (torch, on the device).  --out appends the lines to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opencv-octvr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

FORMATS = ["uyvy422", "p010", "yuv420p10", "p210", "yuv422p10"]


def to_format(fmt, t, w, h):
    """"Y over [U|V]" -> layout fmt by the output rule, on the device (bytes)."""
    import torch
    u, v = t[h:, :w // 2], t[h:, w // 2:w]
    if fmt == "uyvy422":
        out = torch.empty((h, 2 * w), dtype=torch.uint8, device=t.device)
        out[:, 1::2] = t[:h, :w]
        out[:, 0::4] = u.repeat_interleave(2, dim=0)
        out[:, 2::4] = v.repeat_interleave(2, dim=0)
        return out
    c422, planar = fmt in ("p210", "yuv422p10"), fmt in ("yuv420p10", "yuv422p10")
    if c422:
        u, v = u.repeat_interleave(2, dim=0), v.repeat_interleave(2, dim=0)
    words = torch.empty((2 * h if c422 else h * 3 // 2, w), dtype=torch.int16, device=t.device)
    words[:h] = t[:h, :w].to(torch.int16)
    if planar:
        words[h:, :w // 2], words[h:, w // 2:] = u.to(torch.int16), v.to(torch.int16)
    else:
        words[h:, 0::2], words[h:, 1::2] = u.to(torch.int16), v.to(torch.int16)
    return (words << (2 if planar else 8)).view(torch.uint8)  # little-endian words as bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
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
    sets = {k: [[to_format(k, t, w, h) for t, (w, h) in zip(fs, sizes)] for fs in planar] for k in FORMATS}
    sets["yuv420p"] = planar
    outs = {k: torch.empty(ox.frame_shape(k, W, H), dtype=torch.uint8, device=f"cuda:{dev}") for k in FORMATS + ["yuv420p"]}
    ref = outs["yuv420p"]

    m.stitch(planar[1], ref)
    torch.cuda.synchronize(dev)
    g_planar = m.gains()
    info = {"metric": "yuv10_parity_C2", "so_sha256": bench.lib_sha256(), "footprint_bytes": m.info()["footprint_bytes"],
            "out_420_bytes": W * H * 3 // 2}
    moved = {}
    for k in FORMATS:
        m.set_pixel_formats(k, k)
        m.stitch(sets[k][1], outs[k])
        torch.cuda.synchronize(dev)
        ok = bool(torch.equal(outs[k], to_format(k, ref, W, H))) and m.gains() == g_planar
        i = m.info()
        pre = "uyvy" if k == "uyvy422" else "yuv10"
        info["equal_" + k] = ok
        moved[k] = (i[pre + "_in_bytes"] + info["footprint_bytes"], i[pre + "_out_bytes"] + info["out_420_bytes"])
        if not ok:
            raise SystemExit("yuv10_ab: the %s output differs from the rearranged planar output" % k)
    lines = [info]
    print(json.dumps(info), flush=True)

    configs = [("both", lambda k: (k, k)), ("in", lambda k: (k, "yuv420p")), ("out", lambda k: ("yuv420p", k))]
    times = {}
    m.set_timing(1)
    for rnd in range(args.rounds):
        for k in ["yuv420p"] + FORMATS:
            for name, pair in (configs if k != "yuv420p" else [("both", lambda k: (k, k))]):
                fi, fo = pair(k)
                m.set_pixel_formats(fi, fo)
                for s in range(5):  # warm-up, read and dropped
                    m.stitch(sets[fi][s % nsets], outs[fo])
                m.kernel_time()
                for s in range(args.steps):
                    m.stitch(sets[fi][s % nsets], outs[fo])
                ms, launches = m.kernel_time()
                assert launches == args.steps
                times.setdefault((k, name), []).append(ms / launches)
    m.set_timing(0)
    med = {key: statistics.median(v) * 1e3 for key, v in times.items()}  # us: the median round's mean
    base_us = med[("yuv420p", "both")]
    for k in FORMATS:
        unpack, pack = med[(k, "in")] - base_us, med[(k, "out")] - base_us
        d = {"metric": "yuv10_kernel_C2", "format": k, "rounds": len(times[(k, "in")]), "steps": args.steps, "planar_us": round(base_us, 2),
             "in_us": round(med[(k, "in")], 2), "out_us": round(med[(k, "out")], 2), "both_us": round(med[(k, "both")], 2),
             "unpack_us": round(unpack, 2), "pack_us": round(pack, 2), "unpack_bytes": int(moved[k][0]),
             "pack_bytes": int(moved[k][1]), "unpack_tb_per_s": round(moved[k][0] / max(unpack, 1e-3) / 1e6, 3),
             "pack_tb_per_s": round(moved[k][1] / max(pack, 1e-3) / 1e6, 3),
             "how": "HIP events of the stitch (set_timing, kernel_time), mean per round, median round; conversion = format side - planar"}
        lines.append(d)
        print(json.dumps(d), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
