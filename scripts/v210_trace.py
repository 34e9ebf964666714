#!/usr/bin/env python3
"""v210's two kernels beside P210's, for one kernel trace: a Mapper on the C2 rig (6 x 3840 x 2160 in, 7680 x 3840 out)
stitching with P210 on both sides and with v210 on both sides.  Run it under

  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/v210_trace.py [--frames N]

and read v210_unpack_kernel / v210_pack_kernel and layout_unpack_kernel / layout_pack_kernel (P210's template argument)
from DIR's kernel_stats.csv (scripts/collect_profiles.py).  The frames are random bytes: every bit pattern is a frame
of either layout, and neither conversion's time depends on the values.  Prints one JSON line with the algorithmic bytes
per frame of each kernel (the unpack's from octvr_mapper_info)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import async_nv12_ab as base  # noqa: E402  (setup; puts the repository on sys.path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    a = ap.parse_args()
    import torch
    ox, mt, sizes, W, H, _ = base.setup()
    rec = {"out": [W, H], "frames": a.frames, "bytes_per_frame": {}}
    g = torch.Generator(device="cuda").manual_seed(210)
    for fmt, key in (("p210", "yuv10"), ("v210", "v210")):
        ins = [torch.randint(0, 256, ox.frame_shape(fmt, w, h), dtype=torch.uint8, device="cuda", generator=g) for w, h in sizes]
        m = ox.Mapper(mt, sizes, blend=0, enable_gain=True, device=0)
        m.set_pixel_formats(fmt, fmt)
        out = torch.empty(ox.frame_shape(fmt, W, H), dtype=torch.uint8, device="cuda")
        for _ in range(a.frames):
            m.stitch(ins, out)
            torch.cuda.synchronize()
        info = m.info()
        rec["bytes_per_frame"][fmt] = {"unpack_in": info[key + "_in_bytes"], "unpack_out": info["footprint_bytes"],
                                       "pack_in": W * H * 3 // 2, "pack_out": info[key + "_out_bytes"]}
        m.close()
    print("RESULT " + json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
