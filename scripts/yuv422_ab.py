#!/usr/bin/env python3
"""What the 4:2:2 capture layouts cost on the C2 rig (BASELINE.json configs[1]): the bench's frame sets stitched
with each of "uyvy422" (the yardstick: uyvy.hip's kernels), "yuyv422", "yuv422p" and "nv16" on both sides, the
formats interleaved, `--rounds` times `--steps` stitches each at one frame in flight.  Meant to run under a
kernel trace of its own,

  rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python scripts/yuv422_ab.py

and then, without a GPU, `python scripts/yuv422_ab.py --summarize DIR [--out profiles/yuv422_ab.jsonl]` reads the
trace and prints one JSON line per conversion kernel: launches, median and mean us, the bytes it moves (the 4:2:2
bytes of octvr_mapper_info plus the 4:2:0 bytes of the other side) and bytes / median time.  Before the runs, the
full-size parity of every layout: in and out equals the planar stitch of the same pixels rearranged by the two
rules (torch, on the device).  The run itself prints one line with those byte counts and writes it to the
--info file, which --summarize reads."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opencv-octvr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

FORMATS = ["uyvy422", "yuyv422", "yuv422p", "nv16"]
KERNELS = {"uyvy422": ("uyvy_unpack_kernel", "uyvy_pack_kernel"),
           "yuyv422": ("yuv422_unpack_kernel<0>", "yuv422_pack_kernel<0>"),
           "yuv422p": ("yuv422_unpack_kernel<1>", "yuv422_pack_kernel<1>"),
           "nv16": ("yuv422_unpack_kernel<2>", "yuv422_pack_kernel<2>")}


def to_422(fmt, t, w, h):
    """"Y over [U|V]" -> layout fmt by the output rule (every chroma row on two rows), on the device."""
    import torch
    u = t[h:, :w // 2].repeat_interleave(2, dim=0)
    v = t[h:, w // 2:w].repeat_interleave(2, dim=0)
    if fmt in ("uyvy422", "yuyv422"):
        out = torch.empty((h, 2 * w), dtype=torch.uint8, device=t.device)
        y0 = 1 if fmt == "uyvy422" else 0
        out[:, y0::2] = t[:h, :w]
        out[:, 1 - y0::4] = u
        out[:, 3 - y0::4] = v
        return out
    out = torch.empty((2 * h, w), dtype=torch.uint8, device=t.device)
    out[:h] = t[:h, :w]
    if fmt == "yuv422p":
        out[h:, :w // 2], out[h:, w // 2:] = u, v
    else:
        out[h:, 0::2], out[h:, 1::2] = u, v
    return out


def summarize(trace_dir, info, out):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no kernel trace under " + trace_dir)
    spans = {}
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name") or row.get("Name") or ""
                spans.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    lines = []
    for fmt in FORMATS:
        for kind, key in zip(("unpack", "pack"), KERNELS[fmt]):
            mangled = key.replace("<", "ILi").replace(">", "EEE")  # a trace that keeps the mangled names
            us = [v for name, vs in spans.items() if key in name.replace(" ", "") or mangled in name for v in vs]
            if not us:
                continue
            med = statistics.median(us)
            moved = info["in_bytes"] + info["footprint_bytes"] if kind == "unpack" else info["out_bytes"] + info["out_420_bytes"]
            lines.append({"metric": "yuv422_kernel_C2", "format": fmt, "kernel": key, "kind": kind, "launches": len(us),
                          "median_us": round(med, 2), "mean_us": round(statistics.fmean(us), 2),
                          "p10_us": round(sorted(us)[len(us) // 10], 2), "p90_us": round(sorted(us)[len(us) * 9 // 10], 2),
                          "bytes": int(moved), "tb_per_s": round(moved / med / 1e6, 3),
                          "how": "rocprofv3 --kernel-trace, end - start per launch, one frame in flight"})
    for d in lines:
        print(json.dumps(d))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(json.dumps(dict(info, metric="yuv422_parity_C2")) + "\n")
            for d in lines:
                f.write(json.dumps(d) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--frame-sets", type=int, default=4)
    ap.add_argument("--info", default=None, help="write the run's info line here")
    ap.add_argument("--summarize", metavar="DIR", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarize:
        with open(args.info) as f:
            info = json.load(f)
        return summarize(args.summarize, info, args.out)

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
    sets = {k: [[to_422(k, t, w, h) for t, (w, h) in zip(fs, sizes)] for fs in planar] for k in FORMATS}
    outs = {k: torch.empty(ox.frame_shape(k, W, H), dtype=torch.uint8, device=f"cuda:{dev}") for k in FORMATS}
    ref = torch.empty((H * 3 // 2, W), dtype=torch.uint8, device=f"cuda:{dev}")

    m.stitch(planar[1], ref)
    torch.cuda.synchronize(dev)
    g_planar = m.gains()
    info = {"so_sha256": bench.lib_sha256(), "footprint_bytes": m.info()["footprint_bytes"], "out_420_bytes": W * H * 3 // 2}
    for k in FORMATS:
        m.set_pixel_formats(k, k)
        m.stitch(sets[k][1], outs[k])
        torch.cuda.synchronize(dev)
        ok = bool(torch.equal(outs[k], to_422(k, ref, W, H))) and m.gains() == g_planar
        i = m.info()
        pre = "uyvy" if k == "uyvy422" else "yuv422"
        info["equal_" + k] = ok
        info["in_bytes"], info["out_bytes"], info["runs"] = i[pre + "_in_bytes"], i[pre + "_out_bytes"], i[pre + "_runs"]
        if not ok:
            raise SystemExit("yuv422_ab: the %s output differs from the rearranged planar output" % k)
    print(json.dumps(info), flush=True)
    if args.info:
        os.makedirs(os.path.dirname(os.path.abspath(args.info)), exist_ok=True)
        with open(args.info, "w") as f:
            json.dump(info, f)
    for rnd in range(args.rounds):
        for k in FORMATS:
            m.set_pixel_formats(k, k)
            for s in range(args.steps):
                m.stitch(sets[k][s % nsets], outs[k])
            torch.cuda.synchronize(dev)


if __name__ == "__main__":
    main()
