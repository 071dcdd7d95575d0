"""Cost of a disparity map (GPU box).  Prints one JSON line.

Workload: 5 x 5 views of 512 x 512 x 3 uint8 (the 4x output of a 128 x 128 scene), 33 slopes from -2 to 2, linear, full aperture,
radius 2.
  * ``maps_ms``: one `disparity.disparity` call (k_sweep_cost + k_disparity_pick): disparity, confidence and index.
  * ``maps_aif_ms``: the same with the all-in-focus image (the sweep also writes its fp32 stack, the pick gathers from it).
  * ``torch_ms``: a composition of stock torch ops of the same definition up to the index -- per slope and view one F.grid_sample
    (bilinear, border padding, align_corners) of the fp32 view, accumulated into the two moments with the aperture weight;
    max(q - m^2, 0) summed over the channels; F.avg_pool2d on the replicate-padded volume; argmin.  Its sampling grids and the
    fp32 views are made outside the timed region.
The three are timed in the same process, alternating, in `--rounds` rounds (HIP events around `--reps` / `--torch_reps` calls after
a warm-up); ``kernels_faster_in_every_round`` is the condition the design rests on.  ``index_agreement`` is the share of pixels
where the two pick the same slope (their costs differ by fp32 rounding and the composition's fp32 grid coordinates).

  python tools/disparity_bench.py [--rounds 3] [--reps 200] [--torch_reps 10] [--warmup 3] [--out profiles/disparity_bench.txt]
  python tools/disparity_bench.py --regularize [--rounds 3] [--reps 200] [--warmup 3] [--out profiles/sgm_bench.txt]

  python tools/disparity_bench.py --occlusion [--rounds 3] [--reps 200] [--warmup 3] [--out profiles/occlusion_bench.txt]
  python tools/disparity_bench.py --subset_aif [--rounds 3] [--reps 200] [--warmup 3] [--out profiles/aif_subset_bench.txt]

--regularize times the semi-global aggregation of that workload's cost volume instead (``regularize_bench``).
--occlusion times the plain and the occlusion-aware sweep of that workload alternately instead (``occlusion_bench``).
--subset_aif times the occlusion-aware call with the all-in-focus image from all views, the same call with the image from the winning
subset, and that image's pass alone, alternately instead (``subset_aif_bench``)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from lft_amd import disparity  # noqa: E402
from refocus_bench import timed, torch_grids  # noqa: E402  (tools/refocus_bench.py: the same views, the same grids)

A, H, W, C, D, RADIUS = 5, 512, 512, 3, 33, 2


def torch_index(planes, grids, weights):
    """planes: [A*A, C, H, W] fp32 -> (index [H, W], E [D, H, W]): D * A^2 resampling ops, each with full-size temporaries."""
    vol = []
    for g in grids:
        m, q = torch.zeros_like(planes[0:1]), torch.zeros_like(planes[0:1])
        for n in range(A * A):
            s = F.grid_sample(planes[n:n + 1], g[n], mode="bilinear", padding_mode="border", align_corners=True)
            m.add_(s, alpha=weights[n])
            q.addcmul_(s, s, value=weights[n])
        vol.append((q - m * m).clamp_(min=0).sum(1))
    E = F.avg_pool2d(F.pad(torch.cat(vol)[None], (RADIUS,) * 4, mode="replicate"), 2 * RADIUS + 1, stride=1)[0]
    return E.argmin(0), E


HBM_PEAK = 8.0e12                                                       # bytes per second, the MI355X's specified peak


def regularize_bench(args, lf, slopes):
    """--regularize: one JSON line per path count.  ``sgm_ms`` is `disparity.regularize` alone (k_sgm_scan + k_sgm_pick) on the
    sweep's E, ``maps_ms`` the unchanged `disparity.disparity` at the same shape, alternating in the same rounds.  The byte
    contract follows the decomposition: every direction reads E once and writes its volume L_r once, the selection reads the R
    volumes once and writes three maps; ``hbm_peak_share`` is that contract over the best time over the specified 8.0 TB/s."""
    E = disparity.disparity(lf, slopes, interp="linear", radius=RADIUS, cost_volume=True).cost
    p1, p2 = disparity.penalties_from_cost(E)
    lines = []
    for paths in (8, 4):
        def sgm():
            return disparity.regularize(E, slopes, p1, p2, paths=paths)

        def maps():
            return disparity.disparity(lf, slopes, interp="linear", radius=RADIUS)

        for _ in range(args.warmup):
            sgm(), maps()
        torch.cuda.synchronize()
        rounds = [{"sgm_ms": round(timed(sgm, args.reps), 4), "maps_ms": round(timed(maps, args.reps), 4)} for _ in range(args.rounds)]
        best = min(r["sgm_ms"] for r in rounds)
        nbytes = 3 * paths * D * H * W * 4 + 3 * H * W * 4
        lines.append(json.dumps({"bench": "sgm", "device": torch.cuda.get_device_name(0), "A": A, "view": [H, W, C], "D": D, "paths": paths,
                                 "p1": p1, "p2": p2, "reps": args.reps, "rounds": rounds, "sgm_ms_best": best,
                                 "maps_ms_best": min(r["maps_ms"] for r in rounds), "contract_bytes": nbytes,
                                 "sgm_GBps": round(nbytes / (best * 1e-3) / 1e9, 1), "hbm_peak_share": round(nbytes / (best * 1e-3) / HBM_PEAK, 4)}))
    return lines


def occlusion_bench(args, lf, slopes):
    """--occlusion: one JSON line.  ``maps_ms`` is the unchanged `disparity.disparity` (k_sweep_cost + k_disparity_pick),
    ``halves_ms`` and ``quadrants_ms`` the same call with occlusion= (k_sweep_cost_occ + k_disparity_pick + k_occ_gather), the
    three alternating in the same rounds of one process.  The byte contract of the new sweep: the views are read once per slope, as
    for the plain one; V plus one byte per pixel and slope is written; the pick reads V and writes three maps; the gather reads
    the index and one byte per pixel and writes one.  ``subsets_per_view`` is the mean number of subsets a view belongs to: the
    accumulation is about 1 + that many times the plain one, on the same bytes read."""
    calls = {"maps_ms": lambda: disparity.disparity(lf, slopes, interp="linear", radius=RADIUS),
             "halves_ms": lambda: disparity.disparity(lf, slopes, interp="linear", radius=RADIUS, occlusion="halves"),
             "quadrants_ms": lambda: disparity.disparity(lf, slopes, interp="linear", radius=RADIUS, occlusion="quadrants")}
    for _ in range(args.warmup):
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    rounds = [{k: round(timed(f, args.reps), 4) for k, f in calls.items()} for _ in range(args.rounds)]
    best = {k: min(r[k] for r in rounds) for k in calls}
    read = D * A * A * H * W * C
    vol = D * H * W * 4
    nbytes = read + 2 * vol + 3 * H * W * 4
    nbytes_occ = nbytes + D * H * W + H * W * (4 + 1 + 1)
    per_view = {mode: float((disparity.subset_table(A, "full", None, mode)[0] != 0).sum()) / (A * A) for mode in ("halves", "quadrants")}
    return [json.dumps({"bench": "disparity_occlusion", "device": torch.cuda.get_device_name(0), "A": A, "view": [H, W, C], "in": "uint8", "D": D,
                        "interp": "linear", "radius": RADIUS, "aperture": "full", "margin": 2.0, "reps": args.reps, "rounds": rounds,
                        "maps_ms_best": best["maps_ms"], "halves_ms_best": best["halves_ms"], "quadrants_ms_best": best["quadrants_ms"],
                        "halves_over_plain": round(best["halves_ms"] / best["maps_ms"], 3), "quadrants_over_plain": round(best["quadrants_ms"] / best["maps_ms"], 3),
                        "subsets_per_view": per_view, "contract_bytes": nbytes, "contract_bytes_occlusion": nbytes_occ,
                        "maps_GBps": round(nbytes / (best["maps_ms"] * 1e-3) / 1e9, 1), "halves_GBps": round(nbytes_occ / (best["halves_ms"] * 1e-3) / 1e9, 1),
                        "quadrants_GBps": round(nbytes_occ / (best["quadrants_ms"] * 1e-3) / 1e9, 1)})]


def subset_aif_bench(args, lf, slopes):
    """--subset_aif: one JSON line.  ``aif_true_ms`` is `disparity.disparity(occlusion="halves", all_in_focus=True)` (k_sweep_cost_occ
    writing its fp32 stack + k_disparity_pick gathering from it + k_occ_gather), ``aif_subset_ms`` the same call with
    all_in_focus="subset" (the sweep without the stack, the pick, the gather, then k_aif_at), ``aif_at_ms`` `disparity.all_in_focus_at`
    alone on that call's index and subset; the three alternate in the same rounds of one process.  The workload's views are noise, so
    that index differs from pixel to pixel and nearly every wave of k_aif_at reads its records per lane: ``aif_at_uniform_ms`` is the
    same pass on a constant index and subset, where every wave reads them through a uniform address.  The byte contract of k_aif_at:
    the views read once, 4 + 1 bytes of maps in per pixel, the image out; ``aif_at_hbm_peak_share`` is that contract over the best
    time over the specified 8.0 TB/s.  ``stack_bytes_dropped`` is what the sweep no longer writes and the pick no longer reads from."""
    kw = dict(interp="linear", radius=RADIUS, occlusion="halves")
    res = disparity.disparity(lf, slopes, **kw)
    flat_index, flat_subset = torch.full_like(res.index, D // 2), torch.ones_like(res.subset)
    calls = {"aif_true_ms": lambda: disparity.disparity(lf, slopes, all_in_focus=True, **kw),
             "aif_subset_ms": lambda: disparity.disparity(lf, slopes, all_in_focus="subset", **kw),
             "aif_at_ms": lambda: disparity.all_in_focus_at(lf, slopes, res.index, res.subset, interp="linear", occlusion="halves"),
             "aif_at_uniform_ms": lambda: disparity.all_in_focus_at(lf, slopes, flat_index, flat_subset, interp="linear", occlusion="halves")}
    for _ in range(args.warmup):
        for f in calls.values():
            f()
    same = all(torch.equal(x, y) for x, y in zip(calls["aif_true_ms"]()[:3], calls["aif_subset_ms"]()[:3]))
    # a wave of k_aif_at is two rows of a 32-pixel-wide tile: the share of them with one (index, subset) pair
    pair = (res.index.long() * 8 + res.subset.long()).reshape(H // 2, 2, W // 32, 32).permute(0, 2, 1, 3).reshape(-1, 64)
    uniform = float((pair == pair[:, :1]).all(1).double().mean())
    torch.cuda.synchronize()
    rounds = [{k: round(timed(f, args.reps), 4) for k, f in calls.items()} for _ in range(args.rounds)]
    best = {k: min(r[k] for r in rounds) for k in calls}
    nbytes = A * A * H * W * C + H * W * (4 + 1) + H * W * C
    return [json.dumps({"bench": "disparity_subset_aif", "device": torch.cuda.get_device_name(0), "A": A, "view": [H, W, C], "in": "uint8", "out": "uint8", "D": D,
                        "interp": "linear", "radius": RADIUS, "aperture": "full", "occlusion": "halves", "margin": 2.0, "reps": args.reps, "rounds": rounds,
                        "aif_true_ms_best": best["aif_true_ms"], "aif_subset_ms_best": best["aif_subset_ms"], "aif_at_ms_best": best["aif_at_ms"],
                        "aif_at_uniform_ms_best": best["aif_at_uniform_ms"], "waves_uniform_share": round(uniform, 4),
                        "subset_over_true": round(best["aif_subset_ms"] / best["aif_true_ms"], 3),
                        "subset_faster_in_every_round": all(r["aif_subset_ms"] < r["aif_true_ms"] for r in rounds), "maps_bitwise_equal": same,
                        "subset_share_nonzero": round(float((res.subset != 0).double().mean()), 4),
                        "aif_at_contract_bytes": nbytes, "aif_at_GBps": round(nbytes / (best["aif_at_ms"] * 1e-3) / 1e9, 1),
                        "aif_at_hbm_peak_share": round(nbytes / (best["aif_at_ms"] * 1e-3) / HBM_PEAK, 4), "stack_bytes_dropped": D * H * W * C * 4})]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--regularize", action="store_true", help="time the semi-global aggregation beside the sweep instead (one line per path count)")
    ap.add_argument("--occlusion", action="store_true", help="time the plain and the occlusion-aware sweep alternately instead (one line)")
    ap.add_argument("--subset_aif", action="store_true", help="time the occlusion-aware call with either all-in-focus image and the subset image's pass alone (one line)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--torch_reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    slopes = [float(x) for x in np.linspace(-2.0, 2.0, D)]
    lf = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (A, A, H, W, C)).astype(np.uint8)).to(dev)
    if args.regularize or args.occlusion or args.subset_aif:
        lines = regularize_bench(args, lf, slopes) if args.regularize else occlusion_bench(args, lf, slopes) if args.occlusion else subset_aif_bench(args, lf, slopes)
        print("\n".join(lines))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    planes = (lf.float() / 255).permute(0, 1, 4, 2, 3).reshape(A * A, C, H, W).contiguous()
    grids = torch_grids(slopes, dev)
    weights = [1.0 / (A * A)] * (A * A)

    def maps():
        return disparity.disparity(lf, slopes, interp="linear", radius=RADIUS)

    def maps_aif():
        return disparity.disparity(lf, slopes, interp="linear", radius=RADIUS, all_in_focus=True)

    def composed():
        return torch_index(planes, grids, weights)

    for _ in range(args.warmup):
        maps(), maps_aif(), composed()
    ours = disparity.disparity(lf, slopes, interp="linear", radius=RADIUS, cost_volume=True)
    index, E = composed()
    agree = float((ours.index.long() == index).double().mean())
    diff = float((ours.cost - E).abs().max())
    torch.cuda.synchronize()
    rounds = []
    for _ in range(args.rounds):
        rounds.append({"maps_ms": round(timed(maps, args.reps), 4), "maps_aif_ms": round(timed(maps_aif, args.reps), 4),
                       "torch_ms": round(timed(composed, args.torch_reps), 4)})
    read = D * A * A * H * W * C                                          # every slope reads the views once, as bytes
    vol = D * H * W * 4                                                   # V: written by the sweep, read by the pick (halo apart)
    nbytes = read + 2 * vol + 3 * H * W * 4
    nbytes_aif = nbytes + D * H * W * C * 4 + H * W * C * 4 + H * W * C   # the stack written, one of D slices gathered, bytes out
    best, best_aif = min(r["maps_ms"] for r in rounds), min(r["maps_aif_ms"] for r in rounds)
    line = json.dumps({"bench": "disparity", "device": torch.cuda.get_device_name(0), "A": A, "view": [H, W, C], "in": "uint8", "D": D,
                       "interp": "linear", "radius": RADIUS, "aperture": "full", "reps": args.reps, "torch_reps": args.torch_reps,
                       "rounds": rounds, "maps_ms_best": best, "maps_aif_ms_best": best_aif, "contract_bytes": nbytes,
                       "contract_bytes_aif": nbytes_aif, "maps_GBps": round(nbytes / (best * 1e-3) / 1e9, 1),
                       "maps_aif_GBps": round(nbytes_aif / (best_aif * 1e-3) / 1e9, 1), "torch_ops_per_map": 3 * D * A * A + 4 * D + 4,
                       "index_agreement": agree, "max_abs_diff_cost": diff,
                       "kernels_faster_in_every_round": all(max(r["maps_ms"], r["maps_aif_ms"]) < r["torch_ms"] for r in rounds)})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
