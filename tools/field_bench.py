"""Angular tiling of a U x V field (lft_amd.field): what the two gathers cost beside the per-window composition of the scene calls,
and what the tiled field does to the PSNR of the outer and of the centre views.  GPU box.

    python tools/field_bench.py [--size 64 --scenes 2 --epochs 20 --cost_size 512 --reps 20]

One JSON line.

"cost": event-timed milliseconds for 9x9 views of --cost_size squared LR pixels, A = 5, 2x, patch 32 / stride 16, at the angular
strides 4 and 2: ``field.divide``, ``field.integrate`` with the crop and with the hann blend (flat angular table), and in the same run
the composition of the pieces there were before: per window a torch slice into a sub-mosaic and ``scene.divide``; per window
``scene.integrate`` (crop / hann), accumulated into the field by torch and divided by the count.  All variants alternate inside every
repetition; medians and minima of --reps.  Each figure is the time between two events recorded from Python round the launches, so it
can hold host enqueue gaps: an upper bound of the kernels' time, not a kernel trace.  "ratio_to_composition" is the composition's
median over the field call's in the same run (above 1: the field call is faster).  "bytes" is the contract of the integrate -- every SR
patch element that shows a scene pixel read once, every field element written once -- and "hbm_peak_share" that contract over the best
time over the specified 8.0 TB/s.  "sr_patch_bytes" is what is live at once: mu*mv*N*(A*pz)^2*4.

"quality": a small 5x5 2x network is trained the way tests/psnr_util.train_small_model does, then held-out synthetic 9x9 scenes built
by the same formula go through ``field.super_resolve_field`` with angular flat / linear / hann at the angular strides 4 and 2.
"outer": the mean per-view PSNR of the 56 outer views, of the bicubic up-scaling of the same views (lft_amd.colour.bicubic_lf), and
the difference.  "centre": the mean per-view PSNR of the 25 centre views from the tiled field, from the single centre window
(``scene.super_resolve_scene``), the difference with its sign, and the least and the largest per-view difference.  The scenes are
trainer.SyntheticPatchSource's with 9 views per axis: view (p, q) is the base image shifted by disp*p, disp*q with one disp in
[-1.5, 1.5] per scene, so any 5x5 window of it has the disparity per view step the 5x5 model was trained on."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lft_amd import colour, field as F, scene as S  # noqa: E402

HBM_PEAK = 8.0e12                                                       # bytes per second, the MI355X's specified peak
ASTRIDES = (4, 2)
PATCH, STRIDE = 32, 16
U = V = 9


def inside_elements(n: int, size: int, patch: int, stride: int) -> int:
    """Of the n patches along one axis of a view of `size` pixels, the pixels that lie inside the view (all sizes in SR pixels)."""
    bdr = (patch - stride) // 2
    return sum(max(0, min(size, k * stride - bdr + patch) - max(0, k * stride - bdr)) for k in range(n))


def multiplicity(L: int, A: int, astride: int) -> list:
    o = F.origins(L, A, astride)
    return [sum(1 for x in o if x <= p < x + A) for p in range(L)]


def composed_divide(field, A, astride):
    h0, w0 = field.shape[0] // U, field.shape[1] // V
    views = field.reshape(U, h0, V, w0)
    return torch.cat([S.divide(views[ou:ou + A, :, ov:ov + A, :].reshape(A * h0, A * w0).contiguous(), A, PATCH, STRIDE)
                      for ou in F.origins(U, A, astride) for ov in F.origins(V, A, astride)], dim=0)


def composed_integrate(srp, A, astride, size, s, blend):
    H = size * s
    N = srp.shape[0] // (len(F.origins(U, A, astride)) * len(F.origins(V, A, astride)))
    acc = torch.zeros(U, H, V, H, device=srp.device)
    cnt = torch.zeros(U, 1, V, 1, device=srp.device)
    w = 0
    for ou in F.origins(U, A, astride):
        for ov in F.origins(V, A, astride):
            r = S.integrate(srp[w * N:(w + 1) * N], A, size, size, s, PATCH, STRIDE, blend=blend)
            acc[ou:ou + A, :, ov:ov + A, :] += r.reshape(A, H, A, H)
            cnt[ou:ou + A, :, ov:ov + A, :] += 1
            w += 1
    return (acc / cnt).reshape(U * H, V * H)


def cost(dev, A, s, size, reps):
    out = {"config": f"{U}x{V} views of {size}x{size} LR, A = {A}, {s}x, patch {PATCH} / stride {STRIDE}", "reps": reps, "per_astride": {}}
    field = torch.rand(U * size, V * size, device=dev)
    nu, nv = S.scene_counts(size, size, PATCH, STRIDE)
    pz, H = PATCH * s, size * s
    S.blend_window("hann", pz, dev)                                     # the tables are on the device before anything is timed
    F.angular_table("flat", A, dev)
    for astride in ASTRIDES:                                            # one stride's SR patches live at a time
        mu, mv = F.counts(U, V, A, astride)
        B = mu * mv * nu * nv
        srp = torch.rand((B, 1, A * pz, A * pz), device=dev)
        fi = lambda **kw: F.integrate(srp, U, V, A, size, size, s, PATCH, STRIDE, astride, **kw)
        variants = {"divide": lambda: F.divide(field, U, V, A, PATCH, STRIDE, astride),
                    "composed_divide": lambda: composed_divide(field, A, astride),
                    "integrate_crop": fi,
                    "composed_integrate_crop": lambda: composed_integrate(srp, A, astride, size, s, None),
                    "integrate_hann": lambda: fi(blend="hann"),
                    "composed_integrate_hann": lambda: composed_integrate(srp, A, astride, size, s, "hann")}
        # the composition computes what the field call computes: the cut to the bit, the crop to torch's division, the blend to the
        # rounding of a mean of means
        same = {"divide_equal": bool(torch.equal(variants["divide"](), variants["composed_divide"]()))}
        for n in ("integrate_crop", "integrate_hann"):
            same[n + "_max_abs_diff"] = float((variants[n]() - variants["composed_" + n]()).abs().max())
        ms = {name: [] for name in variants}
        for rep in range(reps + 3):                                     # the variants alternate inside every repetition
            for name, run in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                if rep >= 3:
                    ms[name].append(e0.elapsed_time(e1))
        field_el = U * V * H * H
        crop_read = sum(multiplicity(U, A, astride)) * sum(multiplicity(V, A, astride)) * H * H
        blend_read = mu * mv * A * A * inside_elements(nu, H, pz, STRIDE * s) * inside_elements(nv, H, pz, STRIDE * s)
        row = {"windows": mu * mv, "patches": B, "sr_patch_bytes": B * (A * pz) ** 2 * 4, "against_composition": same,
               "bytes": {"integrate_crop": 4 * (crop_read + field_el), "integrate_hann": 4 * (blend_read + field_el)}}
        for name, v in ms.items():
            row[name + "_ms"] = {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4)}
        row["ratio_to_composition"] = {n: round(row[f"composed_{n}_ms"]["median"] / row[f"{n}_ms"]["median"], 3) for n in ("divide", "integrate_crop", "integrate_hann")}
        row["hbm_peak_share"] = {n: round(row["bytes"][n] / (row[n + "_ms"]["min"] * 1e-3) / HBM_PEAK, 4) for n in ("integrate_crop", "integrate_hann")}
        out["per_astride"][str(astride)] = row
        del srp, variants, fi
        torch.cuda.empty_cache()
    return out


def quality(dev, A, s, size, scenes, epochs):
    import psnr_util as PU
    from types import SimpleNamespace
    from model import LFT
    sd, hist = PU.train_small_model(dev, A, s, epochs=epochs)
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s), precision="fp32")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(dev).eval()
    held = [(lr.to(dev), hr.to(dev)) for lr, hr in PU.held_out_scenes(U, s, n=scenes, size=size)]
    c0 = (U - A) // 2
    inner = np.zeros((U, V), bool)
    inner[c0:c0 + A, c0:c0 + A] = True
    bicubic, single = [], []
    for lr, hr in held:
        views = lr.reshape(U, size, V, size).permute(0, 2, 1, 3)
        rgb = views[..., None].expand(-1, -1, -1, -1, 3).contiguous()                  # grey views as an RGB field in [0, 1]
        up = colour.bicubic_lf(rgb, U, s, out_dtype=torch.float32)[..., 0]             # [U, V, sH, sW]
        bicubic.append(PU.view_psnrs(up.permute(0, 2, 1, 3).reshape(U * size * s, V * size * s), hr, U))
        centre = views[c0:c0 + A, c0:c0 + A].permute(0, 2, 1, 3).reshape(A * size, A * size).contiguous()
        hr_c = hr.reshape(U, size * s, V, size * s)[c0:c0 + A, :, c0:c0 + A, :].reshape(A * size * s, A * size * s)
        single.append(PU.view_psnrs(S.super_resolve_scene(net, centre, PATCH, STRIDE), hr_c, A))
    bicubic, single = np.mean(bicubic, axis=0), np.mean(single, axis=0)
    out = {"train_loss_first_last": [round(float(hist[0]), 5), round(float(hist[-1]), 5)], "scenes": scenes, "view_size_lr": size,
           "bicubic_outer_psnr_db": round(float(bicubic[~inner].mean()), 3), "single_centre_window_psnr_db": round(float(single.mean()), 3), "per_astride": {}}
    for astride in ASTRIDES:
        row = {"windows": int(np.prod(F.counts(U, V, A, astride)))}
        for angular in ("flat", "linear", "hann"):
            p = np.mean([PU.view_psnrs(F.super_resolve_field(net, lr, U, V, PATCH, STRIDE, astride=astride, angular=angular), hr, U) for lr, hr in held], axis=0)
            d = p[inner].reshape(A, A) - single
            row[angular] = {"outer": {"psnr_db": round(float(p[~inner].mean()), 3), "over_bicubic_db": round(float(p[~inner].mean() - bicubic[~inner].mean()), 3)},
                            "centre": {"psnr_db": round(float(p[inner].mean()), 3), "over_single_window_db": round(float(d.mean()), 3),
                                       "per_view_min_db": round(float(d.min()), 3), "per_view_max_db": round(float(d.max()), 3)}}
        out["per_astride"][str(astride)] = row
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64, help="LR view height = width of the held-out scenes")
    ap.add_argument("--scenes", type=int, default=2, help="held-out scenes")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--cost_size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip_quality", action="store_true", help="the cost alone")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    A, s = 5, 2
    with torch.no_grad():
        c = cost(dev, A, s, a.cost_size, a.reps)
    torch.cuda.empty_cache()
    print("field_bench: cost measured" + ("" if a.skip_quality else ", training the small model"), file=sys.stderr, flush=True)
    q = None if a.skip_quality else quality(dev, A, s, a.size, a.scenes, a.epochs)
    print(json.dumps({"tool": "field_bench", "cost": c, "quality": q}))


if __name__ == "__main__":
    main()
