#!/usr/bin/env python3
"""What a model's input tensor costs on the C2 rig (6 x 4K into 7680 x 3840, blend 0, gains estimated): the two
paths of Mapper.stitch_tensor against the route a caller had before it, stitch() with a preview and then permute,
.to(float16) and the multiply-add in torch.  A measurement, not a gate.

  python scripts/tensor_out_bench.py [--calls 200] [--warmup 30] [--out profiles/tensor_out.jsonl]

Lines, all in one process, in this order, the whole order run twice (pass 0 and 1):
  a      stitch_tensor: an ImageNet-normalised f16 tensor at template size, the YUV frame given (result-frame path,
         one frame in flight);
  c_a    today's route to the same tensor: stitch(preview = template size), then torch;
  b      stitch_tensor: a prepared 1024 x 512 f16 tensor, output=None, three frames in flight on three streams
         (gathered path: the gain feed and the gather, no composite);
  c_b    today's route to that tensor: stitch(prepared 1024 x 512 preview) with its YUV frame, three frames in
         flight, then torch on the same streams.
A timed call is one round of as many stitches as there are frames in flight, ended by a device synchronise; its
time is divided by that number.  After the warm-up, `--calls` rounds are timed and the median is reported, with the
bytes each route moves per frame as computed from the shapes (bytes_model, device bytes read + written):
  result frame   4 W H written by the composite, read once per resize (YUV, tensor or preview);
  yuv            1.5 W H written;  tensor: 3 w h e written (e = 2 for f16);  preview: 3 w h written;
  torch          permute + convert: 3 w h read, 6 w h written; multiply: 6 + 6; add: 6 + 6  (33 w h in all);
  gathered       the tap list, 32 w h read, and the source bytes under its taps (not modelled: at most the
                 mapper's footprint, octvr_mapper_info "footprint_bytes"); composite: octvr_mapper_traffic."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opencv-octvr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SMALL = (1024, 512)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_out.jsonl"))
    args = ap.parse_args()
    if args.calls < 200:
        sys.exit("--calls: at least 200 timed calls per line")

    import torch
    import bench
    import octvr_amd as ox
    from octvr_amd import synthetic

    if not torch.cuda.is_available():
        sys.exit("tensor_out_bench needs the GPU: nothing is measured without one")
    dev = 0
    torch.cuda.set_device(dev)
    cuda = f"cuda:{dev}"
    rig, W, H, sizes = synthetic.CONFIGS["C2"]()
    frames = [torch.from_numpy(synthetic.yuv_frame(w, h, bench.frame_seed(0, 0, i))).to(cuda) for i, (w, h) in enumerate(sizes)]
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H, use_roi=True, device=dev)
    m = ox.Mapper(mt, sizes, blend=0, enable_gain=True, device=dev)
    refs = ox.Mapper.frame_refs(frames)
    scale = [1.0 / (255.0 * s) for s in STD]
    bias = [-mu / s for mu, s in zip(MEAN, STD)]
    sc16 = torch.tensor(scale, dtype=torch.float16, device=cuda).view(3, 1, 1)
    bi16 = torch.tensor(bias, dtype=torch.float16, device=cuda).view(3, 1, 1)
    composite = m.traffic_bytes()

    def measure(step, inflight):
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize(dev)
        t = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize(dev)
            t.append((time.perf_counter() - t0) * 1e6 / inflight)
        return {"us_per_call_median": round(statistics.median(t), 2), "us_per_call_min": round(min(t), 2),
                "us_per_call_p90": round(sorted(t)[int(0.9 * len(t))], 2)}

    def line_a():
        m.prepare_preview(0, 0)
        m.set_frames_in_flight(1)
        out = torch.empty((H * 3 // 2, W), dtype=torch.uint8, device=cuda)
        ten = torch.empty((3, H, W), dtype=torch.float16, device=cuda)
        r = measure(lambda: m.stitch_tensor(refs, ten, output=out, scale=scale, bias=bias), 1)
        r["bytes_model"] = {"result_frame": 4 * W * H * 3, "yuv": 1.5 * W * H, "tensor": 6 * W * H}
        return r, (W, H), 1

    def line_c_a():
        m.prepare_preview(0, 0)
        m.set_frames_in_flight(1)
        out = torch.empty((H * 3 // 2, W), dtype=torch.uint8, device=cuda)
        pv = torch.empty((H, W, 3), dtype=torch.uint8, device=cuda)

        def step():
            m.stitch(refs, out, preview=pv)
            return pv.permute(2, 0, 1).to(torch.float16) * sc16 + bi16

        r = measure(step, 1)
        r["bytes_model"] = {"result_frame": 4 * W * H * 3, "yuv": 1.5 * W * H, "preview": 3 * W * H, "torch": 33 * W * H}
        return r, (W, H), 1

    def streams3():
        st = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(dev) for _ in range(2)]
        return st, [ctypes.c_void_p(s.cuda_stream) for s in st]

    def line_b():
        m.set_frames_in_flight(1)
        m.prepare_preview(*SMALL)
        m.set_frames_in_flight(3)
        st, raw = streams3()
        tens = [torch.empty((3, SMALL[1], SMALL[0]), dtype=torch.float16, device=cuda) for _ in st]

        def step():
            for j in range(3):
                m.stitch_tensor(refs, tens[j], stream=raw[j], scale=scale, bias=bias)

        r = measure(step, 3)
        px = SMALL[0] * SMALL[1]
        r["bytes_model"] = {"tap_list": 32 * px, "tensor": 6 * px, "sources_at_most": m.info()["footprint_bytes"]}
        return r, SMALL, 3

    def line_c_b():
        m.set_frames_in_flight(1)
        m.prepare_preview(*SMALL)
        m.set_frames_in_flight(3)
        st, raw = streams3()
        outs = [torch.empty((H * 3 // 2, W), dtype=torch.uint8, device=cuda) for _ in st]
        pvs = [torch.empty((SMALL[1], SMALL[0], 3), dtype=torch.uint8, device=cuda) for _ in st]

        def step():
            for j in range(3):
                m.stitch(refs, outs[j], stream=raw[j], preview=pvs[j])
                with torch.cuda.stream(st[j]):
                    pvs[j].permute(2, 0, 1).to(torch.float16) * sc16 + bi16

        r = measure(step, 3)
        px = SMALL[0] * SMALL[1]
        r["bytes_model"] = {"composite": composite, "tap_list": 32 * px, "preview": 3 * px, "torch": 33 * px,
                            "sources_at_most": m.info()["footprint_bytes"]}
        return r, SMALL, 3

    lines = []
    for rnd in range(2):
        for name, fn in (("a", line_a), ("c_a", line_c_a), ("b", line_b), ("c_b", line_c_b)):
            r, size, inflight = fn()
            d = {"metric": "tensor_out", "config": "C2", "line": name, "pass": rnd, "tensor": list(size), "dtype": "f16",
                 "frames_in_flight": inflight, "timed_calls": args.calls, "warmup": args.warmup}
            d.update(r)
            print(json.dumps(d), flush=True)
            lines.append(d)
    info = m.info()
    lines.append({"metric": "tensor_out_counters", "tensor_resized": info["tensor_resized"],
                  "tensor_gathered": info["tensor_gathered"], "tensor_no_composite": info["tensor_no_composite"]})
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
