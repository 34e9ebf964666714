#!/usr/bin/env python3
"""What the converted capture layouts cost on the C2 rig (BASELINE.json configs[1]): the bench's frame sets stitched
with each of "uyvy422", "yuyv422", "yuv422p", "nv16", "p010", "yuv420p10", "p210" and "yuv422p10" (frame_layout.hip's
kernels), the formats interleaved, `--rounds` times `--steps` stitches each at one frame in flight.  Per format it
prints one JSON line with the stitch's own HIP-event times (octvr_mapper_set_timing: the events bracket the unpack, the
stitch and the pack) in three configurations — format in and out, in only, out only — and the planar stitch timed the
same way, so unpack = in-only - planar and pack = out-only - planar (medians), next to the bytes the conversions move
(octvr_mapper_info).  Before the runs, the full-size parity of every layout: in and out equals the planar stitch of
the same pixels rearranged by the two rules (torch, on the device).  --out appends the lines to a file.
--formats restricts the run to some of the layouts."""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opencv-octvr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

FORMATS = ["uyvy422", "yuyv422", "yuv422p", "nv16", "p010", "yuv420p10", "p210", "yuv422p10"]
# the prefix of a format's octvr_mapper_info keys
INFO_PREFIX = {"uyvy422": "uyvy", "yuyv422": "yuv422", "yuv422p": "yuv422", "nv16": "yuv422", "p010": "yuv10", "yuv420p10": "yuv10",
               "p210": "yuv10", "yuv422p10": "yuv10"}


def to_format(fmt, t, w, h):
    """"Y over [U|V]" -> layout fmt by the output rule (a 4:2:2 layout carries every chroma row on two rows; a 10-bit
    sample is the byte << 2 in its word's bits 9..0 or 15..6), on the device (bytes)."""
    import torch
    u, v = t[h:, :w // 2], t[h:, w // 2:w]
    if fmt not in ("p010", "yuv420p10"):
        u, v = u.repeat_interleave(2, dim=0), v.repeat_interleave(2, dim=0)
    if fmt in ("uyvy422", "yuyv422"):
        out = torch.empty((h, 2 * w), dtype=torch.uint8, device=t.device)
        y0 = 1 if fmt == "uyvy422" else 0
        out[:, y0::2] = t[:h, :w]
        out[:, 1 - y0::4] = u
        out[:, 3 - y0::4] = v
        return out
    out = torch.empty((h + u.shape[0], w), dtype=torch.uint8, device=t.device)
    out[:h] = t[:h, :w]
    if fmt in ("yuv422p", "yuv420p10", "yuv422p10"):
        out[h:, :w // 2], out[h:, w // 2:] = u, v
    else:
        out[h:, 0::2], out[h:, 1::2] = u, v
    if fmt in ("yuv422p", "nv16"):
        return out
    return (out.to(torch.int16) << (2 if fmt in ("yuv420p10", "yuv422p10") else 8)).view(torch.uint8)  # little-endian words


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--frame-sets", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--formats", default=",".join(FORMATS))
    args = ap.parse_args()

    formats = [k for k in FORMATS if k in args.formats.split(",")]
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
    sets = {k: [[to_format(k, t, w, h) for t, (w, h) in zip(fs, sizes)] for fs in planar] for k in formats}
    sets["yuv420p"] = planar
    outs = {k: torch.empty(ox.frame_shape(k, W, H), dtype=torch.uint8, device=f"cuda:{dev}") for k in formats + ["yuv420p"]}
    ref = outs["yuv420p"]

    m.stitch(planar[1], ref)
    torch.cuda.synchronize(dev)
    g_planar = m.gains()
    with open(ox.LIB_PATH, "rb") as f:  # the library in use (OCTVR_HIP_LIB selects another build for an A/B)
        so_sha256 = hashlib.sha256(f.read()).hexdigest()
    info = {"metric": "layout_parity_C2", "so_sha256": so_sha256, "footprint_bytes": m.info()["footprint_bytes"],
            "out_420_bytes": W * H * 3 // 2}
    moved = {}
    for k in formats:
        m.set_pixel_formats(k, k)
        m.stitch(sets[k][1], outs[k])
        torch.cuda.synchronize(dev)
        ok = bool(torch.equal(outs[k], to_format(k, ref, W, H))) and m.gains() == g_planar
        i = m.info()
        pre = INFO_PREFIX[k]
        info["equal_" + k] = ok
        moved[k] = (i[pre + "_in_bytes"] + info["footprint_bytes"], i[pre + "_out_bytes"] + info["out_420_bytes"])
        if not ok:
            raise SystemExit("layout_ab: the %s output differs from the rearranged planar output" % k)
    lines = [info]
    print(json.dumps(info), flush=True)

    configs = [("both", lambda k: (k, k)), ("in", lambda k: (k, "yuv420p")), ("out", lambda k: ("yuv420p", k))]
    times = {}
    m.set_timing(1)
    for rnd in range(args.rounds):
        for k in ["yuv420p"] + formats:
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
    for k in formats:
        unpack, pack = med[(k, "in")] - base_us, med[(k, "out")] - base_us
        d = {"metric": "layout_kernel_C2", "format": k, "rounds": len(times[(k, "in")]), "steps": args.steps, "planar_us": round(base_us, 2),
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
