"""Refinement of a disparity map (lft_amd.refine): what each of its three kernels costs beside the plane sweep.  GPU box.

    python tools/refine_bench.py [--size 512 --slopes=-2:2:33 --reps 40 --inner 10]

One JSON line, for 5x5 views of --size squared pixels with 3 channels (a noisy two-layer scene, tests/disparity_util.two_layer) and
33 slopes: event-timed milliseconds per call of lft_disp_check with 4 ("cross") and 24 ("all") views, of lft_disp_fill (reach 32, the
check's mask), of lft_disp_wmedian at r = 3 and r = 7 (the centre view as the guide, sigma 0.1, the check's mask), and of the plain
sweep ``disparity.disparity`` in the same run.  Every variant is warmed up, then the variants alternate inside every repetition;
a figure is the time between two events recorded round --inner calls of one variant, divided by --inner, so it can hold host enqueue
gaps: an upper bound of the kernel's time, not a kernel trace.  Medians and minima of --reps.  "ratio_to_sweep" is a median over the
sweep's median in the same run: only such within-run ratios compare between machines.  "bytes" is each kernel's contract -- the
check reads the map and every view map once and writes three bytes per pixel; the fill and the median read the map, the mask and
(the median) the guide once and write a float and a byte per pixel -- and "hbm_peak_share" that contract over the best time over
the specified 8.0 TB/s.  The median is bound by LDS reads and integer work, not by memory: its share says how far."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lft_amd import disparity as Dm, refine as R  # noqa: E402
from lft_amd.refocus import parse_slopes  # noqa: E402

HBM_PEAK = 8.0e12                                                       # bytes per second, the MI355X's specified peak


def scene(size: int) -> np.ndarray:
    """fp32 views [5, 5, size, size, 3]: the two-layer scene with a foreground square in the middle, a little noise, three channels."""
    import disparity_util as DU
    q = size // 4
    L, _ = DU.two_layer(5, size, size, box=(q, size - q, q, size - q))
    L = L * np.array([1.0, 0.8, 0.6], np.float32)
    return (L + 0.02 * np.random.default_rng(7).standard_normal(L.shape)).astype(np.float32)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512, help="view height = width")
    ap.add_argument("--slopes", default="-2:2:33")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--inner", type=int, default=10, help="calls between the two events of one figure")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    A, H, W, C = 5, a.size, a.size, 3
    sl = parse_slopes(a.slopes)
    views = torch.from_numpy(scene(a.size)).to(dev)
    guide = R.quantise_guide(R.centre_view(views)).contiguous()
    tau = float(max(np.diff(sl)))
    with torch.no_grad():
        raw = Dm.disparity(views, sl).disparity
        pos = {4: R.view_positions(A, "cross"), 24: R.view_positions(A, "all")}
        dv = {n: R.disparity_views(views, sl, p) for n, p in pos.items()}
        valid = R.consistency(raw, dv[4], pos[4], reference=(2, 2), tau=tau).valid
        variants = {"sweep": lambda: Dm.disparity(views, sl),
                    "check_4": lambda: R.consistency(raw, dv[4], pos[4], reference=(2, 2), tau=tau),
                    "check_24": lambda: R.consistency(raw, dv[24], pos[24], reference=(2, 2), tau=tau),
                    "fill": lambda: R.fill(raw, valid, 32),
                    "wmedian_r3": lambda: R.weighted_median(raw, guide, 3, valid, 0.1),
                    "wmedian_r7": lambda: R.weighted_median(raw, guide, 7, valid, 0.1)}
        px = H * W
        contract = {"check_4": px * (4 + 4 * 4 + 3), "check_24": px * (4 + 4 * 24 + 3), "fill": px * (4 + 1 + 4 + 1),
                    "wmedian_r3": px * (4 + 1 + C + 4 + 1) + 2048, "wmedian_r7": px * (4 + 1 + C + 4 + 1) + 2048}
        ms = {name: [] for name in variants}
        for rep in range(a.reps + 5):                                   # five warm-up repetitions; the variants alternate inside every one
            for name, run in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    run()
                e1.record()
                e1.synchronize()
                if rep >= 5:
                    ms[name].append(e0.elapsed_time(e1) / a.inner)
    out = {"tool": "refine_bench", "config": f"{A}x{A} views of {H}x{W}x{C}, {len(sl)} slopes", "reps": a.reps, "inner": a.inner,
           "invalid_share": round(float((valid == 0).float().mean()), 4), "ms": {}, "ratio_to_sweep": {}, "bytes": contract, "hbm_peak_share": {}}
    for name, v in ms.items():
        out["ms"][name] = {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4)}
    for name in contract:
        out["ratio_to_sweep"][name] = round(out["ms"][name]["median"] / out["ms"]["sweep"]["median"], 3)
        out["hbm_peak_share"][name] = round(contract[name] / (out["ms"][name]["min"] * 1e-3) / HBM_PEAK, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
