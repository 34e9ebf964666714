#!/usr/bin/env python3
"""The kernels behind a merged 7680 x 3840 frame in a converted layout, for one kernel trace: merge_pack_kernel (one
pass: the mappers' NV12 region frames -> the merged frame of the layout) against the two-pass alternative,
merge_regions_kernel (a native-output pipeline's merge) plus layout_pack_kernel (a Mapper writing the same layout from
its own NV12 frame).  Run it under

  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/async_out_trace.py [--frames N]

and read the kernels' average times from DIR's kernel_stats.csv (scripts/collect_profiles.py); merge_pack_kernel and
layout_pack_kernel appear once per layout (their template argument), merge_regions_kernel once.  The C2 rig's template
in two regions, the top and the bottom half of 7680 x 3840 (a single whole-frame region of a native-output pipeline is
stitched in place, with no merge to time), device frames in and out, UYVY and P210.  Prints one JSON line with the
algorithmic bytes per frame of each kernel."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import async_nv12_ab as base  # noqa: E402  (setup; puts the repository on sys.path)

TOP_BOTTOM = [(0.0, 0.0, 1.0, 0.5), (0.0, 0.5, 1.0, 0.5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    a = ap.parse_args()
    import numpy as np
    import torch
    ox, mt, sizes, W, H, frames = base.setup()
    ins = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames]
    rec = {"out": [W, H], "frames": a.frames, "bytes_per_frame": {"merge_regions_kernel": 2 * W * H * 3 // 2}}

    def pipeline(out_fmt):
        am = ox.AsyncMultiMapper([mt, mt], sizes, (W, H), [0, 0], [0, 0], TOP_BOTTOM, device=0)
        am.set_output_format(out_fmt)
        out = torch.empty(ox.frame_shape(out_fmt, W, H), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for _ in range(a.frames):
            am.push_device(ins, out)
            am.pop()
        info = am.info()
        am.close()
        return info

    info = pipeline("nv12")
    assert info["merge_launches"] == a.frames, info
    for fmt in ("uyvy422", "p210"):
        info = pipeline(fmt)
        assert info["merge_pack_launches"] == a.frames and info["merge_launches"] == 0, info
        rows, nbytes = ox.frame_shape(fmt, W, H)
        rec["bytes_per_frame"]["merge_pack_kernel<%s>" % fmt] = W * H * 3 // 2 + rows * nbytes
        rec["bytes_per_frame"]["layout_pack_kernel<%s>" % fmt] = W * H * 3 // 2 + rows * nbytes
        m = ox.Mapper(mt, sizes, blend=0, enable_gain=True, device=0)
        m.set_pixel_formats("yuv420p", fmt)
        out = torch.empty((rows, nbytes), dtype=torch.uint8, device="cuda")
        for _ in range(a.frames):
            m.stitch(ins, out)
            torch.cuda.synchronize()
        m.close()
    print("RESULT " + json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
