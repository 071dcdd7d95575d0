"""Per-patch disparity compensation by integer shear (lft_amd.scene): what it does to the PSNR, and what it costs.  GPU box.

    python tools/shear_bench.py [--size 96 --scenes 2 --epochs 20 --cost_size 512 --reps 40]

One JSON line.

"effect": a small 5x5 2x network is trained the way tests/psnr_util.train_small_model does (scenes of lft_amd.trainer.SyntheticPatchSource,
|d| <= 0.75 LR pixels per view step), then held-out scenes built by the same formula at the LR disparities 0, 1, 2, 3 and -3 per view
step go through ``super_resolve_scene`` with shear=None, shear="auto" and the true k.  Per disparity: the mean per-view PSNR of the
three, and the share of patches where ``estimate_shear`` found the true k.  "auto_bits_equal_none_at_d0": at d = 0 auto gives k = 0 and
with it the bits of None.

"cost": event-timed milliseconds for a 5x5 scene of --cost_size squared LR pixels per view at 2x, patch 32 / stride 16: ``divide`` +
``integrate`` without and with a shear (random k in [-kmax, kmax] per patch), the two variants alternating in one loop, and
``estimate_shear`` alone; medians and minima of --reps.  Each figure is the time between two events recorded from Python round one
or two launches of about 0.1 ms, so it can hold host enqueue gaps: an upper bound of the kernels' time, not a kernel trace.  "bytes": the contract of the two gathers -- divide writes every patch element once
and reads the scene once from HBM (each scene element lands in (patch/stride)^2 patches, the repeats are the caches'), integrate reads
and writes one element per SR scene element, the sheared pair adds 4 bytes per patch -- and "hbm_peak_share" that contract over the
best time over the specified 8.0 TB/s."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lft_amd import scene as S  # noqa: E402

HBM_PEAK = 8.0e12                                                       # bytes per second, the MI355X's specified peak
DISPARITIES = (0, 1, 2, 3, -3)


def scene_at(d: int, A: int, s: int, size: int, seed: int):
    """(lr [A*size, A*size], hr [A*size*s, A*size*s]) by SyntheticPatchSource's formula at the LR disparity d per view step: the
    formula shifts view u by disp*u HR pixels against the image, which is the slope -disp in the disparity module's sign."""
    g = np.random.Generator(np.random.PCG64([seed, A, s, size]))
    P, disp, k = size * s, -d * s, 6
    yy, xx = np.meshgrid(np.arange(P, dtype=np.float32), np.arange(P, dtype=np.float32), indexing="ij")
    fy, fx = g.uniform(0.02, 0.25, k), g.uniform(0.02, 0.25, k)
    ph, am = g.uniform(0, 2 * np.pi, k), g.uniform(0.2, 1.0, k)
    hr = np.empty((A * P, A * P), dtype=np.float32)
    for u in range(A):
        for v in range(A):
            img = sum(am[j] * np.sin(2 * np.pi * (fy[j] * (yy + disp * u) + fx[j] * (xx + disp * v)) + ph[j]) for j in range(k))
            hr[u * P:(u + 1) * P, v * P:(v + 1) * P] = 0.5 + 0.5 * img / am.sum()
    hr_t = torch.from_numpy(hr)
    return hr_t.reshape(A, size, s, A, size, s).mean(dim=(2, 5)).reshape(A * size, A * size), hr_t


def view_psnr(sr: torch.Tensor, hr: torch.Tensor, A: int) -> float:
    """The mean over the views of 10 log10(1 / MSE), fp64."""
    H, W = hr.shape[0] // A, hr.shape[1] // A
    mse = ((sr.double() - hr.double()) ** 2).reshape(A, H, A, W).mean(dim=(1, 3))
    return float((10.0 * torch.log10(1.0 / mse)).mean())


def effect(dev, A, s, size, scenes, epochs):
    import psnr_util as PU
    from types import SimpleNamespace
    from model import LFT
    sd, hist = PU.train_small_model(dev, A, s, epochs=epochs)
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s), precision="fp32")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(dev).eval()
    out = {"train_loss_first_last": [round(float(hist[0]), 5), round(float(hist[-1]), 5)], "kmax": S.shear_limit(A), "per_disparity": {}}
    for d in DISPARITIES:
        psnr, found, patches, same = {"none": [], "auto": [], "true": []}, 0, 0, True
        for i in range(scenes):
            lr, hr = (t.to(dev) for t in scene_at(d, A, s, size, 100 + i))
            est = S.estimate_shear(S.divide(lr, A), A)
            found += int((est == d).sum())
            patches += est.numel()
            sr = {"none": S.super_resolve_scene(net, lr), "auto": S.super_resolve_scene(net, lr, shear="auto"), "true": S.super_resolve_scene(net, lr, shear=d)}
            for name, t in sr.items():
                psnr[name].append(view_psnr(t, hr, A))
            same = same and torch.equal(sr["auto"], sr["none"])
        out["per_disparity"][str(d)] = {"psnr_none_db": round(float(np.mean(psnr["none"])), 3), "psnr_auto_db": round(float(np.mean(psnr["auto"])), 3),
                                        "psnr_true_k_db": round(float(np.mean(psnr["true"])), 3), "auto_found_true_k_share": round(found / patches, 4),
                                        "patches": patches}
        if d == 0:
            out["auto_bits_equal_none_at_d0"] = bool(same)
    return out


def cost(dev, A, s, size, reps, patch=32, stride=16):
    rng = np.random.default_rng(0)
    sc = torch.from_numpy(rng.random((A * size, A * size), dtype=np.float32)).to(dev)
    nu, nv = S.scene_counts(size, size, patch, stride)
    N, kmax = nu * nv, S.shear_limit(A, patch, stride)
    k = torch.from_numpy(rng.integers(-kmax, kmax + 1, N).astype(np.int32)).to(dev)
    srp = torch.rand((N, 1, A * patch * s, A * patch * s), device=dev)
    patches = S.divide(sc, A, patch, stride)
    variants = {"plain_pair_ms": lambda: (S.divide(sc, A, patch, stride), S.integrate(srp, A, size, size, s, patch, stride)),
                "sheared_pair_ms": lambda: (S.divide(sc, A, patch, stride, k), S.integrate(srp, A, size, size, s, patch, stride, k)),
                "plain_divide_ms": lambda: S.divide(sc, A, patch, stride), "sheared_divide_ms": lambda: S.divide(sc, A, patch, stride, k),
                "plain_integrate_ms": lambda: S.integrate(srp, A, size, size, s, patch, stride),
                "sheared_integrate_ms": lambda: S.integrate(srp, A, size, size, s, patch, stride, k),
                "estimate_shear_ms": lambda: S.estimate_shear(patches, A, stride=stride)}
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
    out = {"config": f"{A}x{A} views of {size}x{size} LR, {s}x, patch {patch} stride {stride}, {N} patches, kmax {kmax}", "reps": reps}
    for name, v in ms.items():
        out[name] = {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4)}
    out["sheared_over_plain_pair_median"] = round(out["sheared_pair_ms"]["median"] / out["plain_pair_ms"]["median"], 3)
    div = 4 * (N * (A * patch) ** 2 + (A * size) ** 2)
    integ = 4 * 2 * (A * size * s) ** 2
    out["bytes"] = {"divide": div, "integrate": integ, "shear_array": 4 * N}
    for kind, extra in (("plain", 0), ("sheared", 4 * N)):
        out[f"{kind}_divide_hbm_peak_share"] = round((div + extra) / (out[f"{kind}_divide_ms"]["min"] * 1e-3) / HBM_PEAK, 4)
        out[f"{kind}_integrate_hbm_peak_share"] = round((integ + extra) / (out[f"{kind}_integrate_ms"]["min"] * 1e-3) / HBM_PEAK, 4)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=96, help="LR view height = width of the held-out scenes")
    ap.add_argument("--scenes", type=int, default=2, help="held-out scenes per disparity")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--cost_size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=40)
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    A, s = 5, 2
    with torch.no_grad():
        c = cost(dev, A, s, a.cost_size, a.reps)
    e = effect(dev, A, s, a.size, a.scenes, a.epochs)
    print(json.dumps({"tool": "shear_bench", "effect": e, "cost": c}))


if __name__ == "__main__":
    main()
