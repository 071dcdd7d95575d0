"""Windowed blending of overlapping SR patches (lft_amd.scene, blend=): what it costs, and what it does to PSNR / SSIM.  GPU box.

    python tools/blend_bench.py [--size 96 --scenes 2 --epochs 20 --cost_size 512 --reps 40]

One JSON line.

"cost": event-timed milliseconds of ``integrate`` for a 5x5 scene of --cost_size squared LR pixels per view at 2x, patch 32, at
the strides 16 and 24: the crop (blend=None) and the hann blend, without and with a shear (random k in [-kmax, kmax] per patch),
all variants alternating inside every repetition; medians and minima of --reps.  Each figure is the time between two events
recorded from Python round one launch, so it can hold host enqueue gaps: an upper bound of the kernel's time, not a kernel trace.
"ratio_to_crop" is the blend's median over the crop's at the same stride in the same run: only such within-run ratios compare
between machines.  "bytes" is the contract -- the blend reads every SR patch element that lies inside a view once and writes every
scene element once, the crop reads and writes one element per scene element -- and "hbm_peak_share" that contract over the best
time over the specified 8.0 TB/s.

"quality": a small 5x5 2x network is trained the way tests/psnr_util.train_small_model does, then held-out scenes built by the same
formula go through ``evaluate.test_scene`` with the crop, the hann and the linear blend at the strides 16 and 24: the mean per-view
PSNR / SSIM of each, and the number of patches a scene is cut into."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lft_amd import evaluate, scene as S  # noqa: E402

HBM_PEAK = 8.0e12                                                       # bytes per second, the MI355X's specified peak
STRIDES = (16, 24)
PATCH = 32


def inside_elements(n: int, size: int, patch: int, stride: int) -> int:
    """Of the n patches along one axis of a view of `size` pixels, the pixels that lie inside the view (all sizes in SR pixels)."""
    bdr = (patch - stride) // 2
    return sum(max(0, min(size, k * stride - bdr + patch) - max(0, k * stride - bdr)) for k in range(n))


def cost(dev, A, s, size, reps):
    rng = np.random.default_rng(0)
    out = {"config": f"{A}x{A} views of {size}x{size} LR, {s}x, patch {PATCH}", "reps": reps, "per_stride": {}}
    variants, ms, facts = {}, {}, {}
    for stride in STRIDES:
        nu, nv = S.scene_counts(size, size, PATCH, stride)
        N, kmax = nu * nv, S.shear_limit(A, PATCH, stride)
        k = torch.from_numpy(rng.integers(-kmax, kmax + 1, N).astype(np.int32)).to(dev)
        srp = torch.rand((N, 1, A * PATCH * s, A * PATCH * s), device=dev)
        S.blend_window("hann", PATCH * s, dev)                          # on the device before anything is timed
        run = lambda srp=srp, stride=stride, **kw: S.integrate(srp, A, size, size, s, PATCH, stride, **kw)
        variants[f"crop_s{stride}"] = run
        variants[f"hann_s{stride}"] = lambda run=run: run(blend="hann")
        variants[f"crop_shear_s{stride}"] = lambda run=run, k=k: run(shear=k)
        variants[f"hann_shear_s{stride}"] = lambda run=run, k=k: run(shear=k, blend="hann")
        scene_el = (A * size * s) ** 2
        read_el = A * A * inside_elements(nu, size * s, PATCH * s, stride * s) * inside_elements(nv, size * s, PATCH * s, stride * s)
        facts[stride] = {"patches": N, "kmax": kmax, "bytes": {"crop": 8 * scene_el, "blend": 4 * (read_el + scene_el)}}
    ms = {name: [] for name in variants}
    for rep in range(reps + 5):                                         # the variants alternate inside every repetition
        for name, run in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            if rep >= 5:
                ms[name].append(e0.elapsed_time(e1))
    for stride in STRIDES:
        row = dict(facts[stride])
        for name in ("crop", "hann", "crop_shear", "hann_shear"):
            v = ms[f"{name}_s{stride}"]
            row[name + "_ms"] = {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4)}
        row["ratio_to_crop"] = {"hann": round(row["hann_ms"]["median"] / row["crop_ms"]["median"], 3),
                                "hann_shear": round(row["hann_shear_ms"]["median"] / row["crop_shear_ms"]["median"], 3)}
        row["hbm_peak_share"] = {"crop": round(row["bytes"]["crop"] / (row["crop_ms"]["min"] * 1e-3) / HBM_PEAK, 4),
                                 "hann": round(row["bytes"]["blend"] / (row["hann_ms"]["min"] * 1e-3) / HBM_PEAK, 4)}
        out["per_stride"][str(stride)] = row
    out["hann_s24_over_crop_s16_median"] = round(out["per_stride"]["24"]["hann_ms"]["median"] / out["per_stride"]["16"]["crop_ms"]["median"], 3)
    return out


def quality(dev, A, s, size, scenes, epochs):
    import psnr_util as PU
    from types import SimpleNamespace
    from model import LFT
    sd, hist = PU.train_small_model(dev, A, s, epochs=epochs)
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s), precision="fp32")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(dev).eval()
    held = PU.held_out_scenes(A, s, n=scenes, size=size)
    out = {"train_loss_first_last": [round(float(hist[0]), 5), round(float(hist[-1]), 5)], "scenes": scenes, "view_size_lr": size, "per_stride": {}}
    for stride in STRIDES:
        nu, nv = S.scene_counts(size, size, PATCH, stride)
        row = {"patches_per_scene": nu * nv}
        for name, blend in (("crop", None), ("hann", "hann"), ("linear", "linear")):
            res = [evaluate.test_scene(net, lr, hr, PATCH, stride, blend=blend)[:2] for lr, hr in held]
            row[name] = {"psnr_db": round(float(np.mean([r[0] for r in res])), 3), "ssim": round(float(np.mean([r[1] for r in res])), 5)}
        out["per_stride"][str(stride)] = row
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=96, help="LR view height = width of the held-out scenes")
    ap.add_argument("--scenes", type=int, default=2, help="held-out scenes")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--cost_size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--skip_quality", action="store_true", help="the cost alone")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    A, s = 5, 2
    with torch.no_grad():
        c = cost(dev, A, s, a.cost_size, a.reps)
    torch.cuda.empty_cache()
    print("blend_bench: cost measured" + ("" if a.skip_quality else ", training the small model"), file=sys.stderr, flush=True)
    q = None if a.skip_quality else quality(dev, A, s, a.size, a.scenes, a.epochs)
    print(json.dumps({"tool": "blend_bench", "cost": c, "quality": q}))


if __name__ == "__main__":
    main()
