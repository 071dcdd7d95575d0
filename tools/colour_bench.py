"""Cost of lft_colour_merge (GPU box).  Prints one JSON line: per shape, the median milliseconds of one `colour.merge` call (HIP
events around each call after a warm-up), the byte contract -- the centre views' raw LR RGB read once, sr_y read once, the output
written once -- and the GB/s these bytes give.  Shapes: 5 x 5 views of 108 x 156 LR pixels at 4x (uint8 in, uint8 and fp32 out),
and 9 x 9 views of 128 x 128 at 2x.

  python tools/colour_bench.py [--reps 50] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from lft_amd import colour  # noqa: E402

SHAPES = [(5, 108, 156, 4, torch.uint8, torch.uint8), (5, 108, 156, 4, torch.uint8, torch.float32),
          (5, 108, 156, 4, torch.float32, torch.uint8), (9, 128, 128, 2, torch.uint8, torch.uint8)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device="cpu").manual_seed(0)
    rows = []
    for A, H, W, s, cls, out_cls in SHAPES:
        lf = torch.rand(A, A, H, W, 3, generator=gen)
        lf = ((lf * 255).round().to(torch.uint8) if cls == torch.uint8 else lf.to(cls)).to(dev)
        sr_y = torch.rand(A * s * H, A * s * W, generator=gen).to(dev)
        for _ in range(args.warmup):
            out = colour.merge(lf, sr_y, A, s, out_cls)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(args.reps):
            e0.record()
            colour.merge(lf, sr_y, A, s, out_cls)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = statistics.median(ms)
        nbytes = lf.numel() * lf.element_size() + sr_y.numel() * 4 + out.numel() * out.element_size()
        rows.append({"A": A, "lr": [H, W], "s": s, "in": str(cls).split(".")[-1], "out": str(out_cls).split(".")[-1],
                     "ms": round(med, 4), "ms_spread": [round(min(ms), 4), round(max(ms), 4)], "bytes": nbytes,
                     "GBps": round(nbytes / (med * 1e-3) / 1e9, 1)})
    print(json.dumps({"bench": "colour_merge", "device": torch.cuda.get_device_name(0), "reps": args.reps, "cases": rows}))


if __name__ == "__main__":
    main()
