"""Cost of a focal stack (GPU box).  Prints one JSON line.

Workload: 5 x 5 views of 512 x 512 x 3 uint8 (the 4x output of a 128 x 128 scene), 16 slopes from -2 to 2, full aperture, uint8 out.
  * ``cubic_ms``: one `refocus.refocus` call (one k_refocus launch), and the rate on the contract bytes
    D * (A^2*H*W*C + H*W*C): every slope reads the views once and writes its slice once.
  * ``linear_ms`` against ``torch_linear_ms``: the same stack with interp="linear", and a composition of stock torch ops that
    computes it -- per slope and view one F.grid_sample (bilinear, border padding, align_corners) of the fp32 view, accumulated
    with the aperture weight; its sampling grids and the fp32 views are made outside the timed region.  The two are timed in the
    same process, alternating, in `--rounds` rounds (HIP events around `--reps` / `--torch_reps` calls after a warm-up);
    ``kernel_faster_in_every_round`` is the condition the design rests on.  ``max_abs_diff_linear`` compares their results.

  python tools/refocus_bench.py [--rounds 3] [--reps 200] [--torch_reps 30] [--warmup 3] [--out profiles/refocus_bench.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from lft_amd import refocus  # noqa: E402

A, H, W, C, D = 5, 512, 512, 3, 16


def torch_grids(slopes, dev):
    """Per (slope, view) the normalised sampling grid [1, H, W, 2] of the position (y + d*(u-uc), x + d*(v-uc))."""
    uc = (A - 1) / 2
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    return [[torch.stack(((xs + d * (v - uc)) * (2 / (W - 1)) - 1, (ys + d * (u - uc)) * (2 / (H - 1)) - 1), dim=-1)[None].float()
             for u in range(A) for v in range(A)] for d in slopes]


def torch_linear_stack(planes, grids, weights):
    """planes: [A*A, C, H, W] fp32 -> [D, C, H, W]: D * A^2 resampling ops, each with a full-size temporary."""
    out = []
    for g in grids:
        acc = torch.zeros_like(planes[0:1])
        for n in range(A * A):
            acc.add_(F.grid_sample(planes[n:n + 1], g[n], mode="bilinear", padding_mode="border", align_corners=True), alpha=weights[n])
        out.append(acc)
    return torch.cat(out)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--torch_reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    slopes = [float(x) for x in np.linspace(-2.0, 2.0, D)]
    lf = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (A, A, H, W, C)).astype(np.uint8)).to(dev)
    planes = (lf.float() / 255).permute(0, 1, 4, 2, 3).reshape(A * A, C, H, W).contiguous()
    grids = torch_grids(slopes, dev)
    weights = [1.0 / (A * A)] * (A * A)

    def cubic():
        return refocus.refocus(lf, slopes, interp="cubic")

    def linear():
        return refocus.refocus(lf, slopes, interp="linear")

    def composed():
        return torch_linear_stack(planes, grids, weights)

    for _ in range(args.warmup):
        cubic(), linear(), composed()
    ours = refocus.refocus(lf, slopes, interp="linear", out_dtype=torch.float32)
    diff = float((ours.permute(0, 3, 1, 2) - composed()).abs().max())
    torch.cuda.synchronize()
    rounds = []
    for _ in range(args.rounds):
        rounds.append({"cubic_ms": round(timed(cubic, args.reps), 4), "linear_ms": round(timed(linear, args.reps), 4),
                       "torch_linear_ms": round(timed(composed, args.torch_reps), 4)})
    nbytes = D * (A * A * H * W * C + H * W * C)
    best = min(r["cubic_ms"] for r in rounds)
    line = json.dumps({"bench": "refocus", "device": torch.cuda.get_device_name(0), "A": A, "view": [H, W, C], "in": "uint8", "out": "uint8",
                       "D": D, "aperture": "full", "reps": args.reps, "torch_reps": args.torch_reps, "rounds": rounds,
                       "cubic_ms_best": best, "contract_bytes": nbytes, "cubic_GBps": round(nbytes / (best * 1e-3) / 1e9, 1),
                       "torch_ops_per_stack": D * A * A, "max_abs_diff_linear": diff,
                       "kernel_faster_in_every_round": all(r["linear_ms"] < r["torch_linear_ms"] for r in rounds)})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
