"""Disparity map, confidence and all-in-focus image of one light field (GPU box): angular consistency as a number.

  python tools/disparity.py --lf scene.mat --angRes 5 --out_dir out/ --slopes=-2:2:33 --radius 2 [--aperture full|disk|gaussian]
                            [--interp nearest|linear|cubic] [--regularize [--p1 P1 --p2 P2] [--paths 4|8] [--edge_gain G]]
                            [--occlusion [halves|quadrants] [--margin B] [--min_views N] [--subset_aif]]
                            [--refine [--refine_views cross|corners|all] [--tau T] [--median_radius R] [--median_sigma S] [--median_iterations I]]
                            [--path_pre_pth LFT_5x5_4x.pth.tar --scale_factor 4 [--precision ..] [--self_ensemble ..]] [--bicubic]

The scene is a light-field .mat with the variable LF [U, V, H, W, C]; its centre angRes x angRes views are used.  Without
--path_pre_pth and --bicubic the raw views are swept.  With --path_pre_pth the light field first goes through
lft_amd.colour.super_resolve_lf; --bicubic does the same with colour.bicubic_lf and the prefix bicubic_ (--scale_factor says how
far).  Slopes are in pixels of the views being swept per view step, LO:HI:N or a comma list, strictly increasing.  Writes
<out_dir>/disparity.png (the slope range mapped to 0 .. 255, grey as RGB), confidence.png (0 .. 1 mapped to 0 .. 255, grey as RGB),
all_in_focus.png and disparity.npy (fp32 [H, W], slope units) from one lft_amd.disparity.disparity call.  With both
--path_pre_pth and --bicubic it prints one JSON line with lft_amd.disparity.disparity_error of the super-resolved views against
the bicubic ones: the mean absolute disparity difference over the pixels where the bicubic sweep is confident, and their share.
--regularize aggregates the cost volume along --paths paths before the selection (lft_amd.disparity.regularize): the penalties
default to lft_amd.disparity.penalties_from_cost of the winner-take-all sweep, and with --edge_gain the guide is the channel mean of
that sweep's all-in-focus image.  --occlusion scores every slope also by the variance of the views of each half (or quadrant) of the
aperture, so that the band round a foreground edge gets the background's slope (lft_amd.disparity.disparity(occlusion=)): a subset
wins where it is --margin times better than the whole aperture, subsets with fewer than --min_views views are dropped, and
<out_dir>/occlusion.png shows which subset set the cost at the chosen slope (0 black: all views agree; subset p as grey 63 p).
--subset_aif (it needs --occlusion) renders all_in_focus.png from the views of that subset and not from all of them
(lft_amd.disparity.disparity(all_in_focus="subset")): no ghost of the foreground in the band round a depth edge.
--refine refines the map after the selection (lft_amd.refine.refine): the maps swept at --refine_views other positions say which
pixels can be trusted (within --tau of each other, default the largest slope step), a weighted median of radius --median_radius
guided by the centre view (--median_sigma, in units of the full range per channel) smooths the map along the image's edges, and what
is left is filled from the farther neighbour.  It writes disparity_refined.png / .npy and valid.png (255 where the cross-view check
trusts the raw map) beside the other files, and prints one JSON line with the share of invalid pixels and of pixels the median
changed.  The sweeps at the other positions take --aperture, --interp, --radius, --regularize and --occlusion as the first does.
Without these flags the files keep their bytes."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lft_amd import colour, disparity, png, refine  # noqa: E402
from refocus import parse_slopes  # noqa: E402  (tools/refocus.py)
import super_resolve  # noqa: E402  (the loader of the scene and of the network)


def grey(x: torch.Tensor, lo: float, hi: float) -> np.ndarray:
    """fp32 [H, W] -> uint8 [H, W, 3]: lo .. hi mapped to 0 .. 255, rounded half to even, clipped."""
    g = ((x - lo) * (255.0 / (hi - lo)) if hi > lo else torch.zeros_like(x)).clamp(0, 255).round().to(torch.uint8)
    return g[..., None].expand(-1, -1, 3).contiguous().cpu().numpy()


def occlusion_arguments(args):
    """The `occlusion` dict of lft_amd.disparity.disparity for --occlusion, or None without it."""
    return dict(subsets=args.occlusion, margin=args.margin, min_views=args.min_views) if args.occlusion else None


def regularize_arguments(views, slopes, args, guided=True):
    """The `regularize` dict of lft_amd.disparity.disparity for --regularize, or None without it.  Penalties not given on the
    command line come from ``penalties_from_cost`` on the winner-take-all sweep's cost (this synchronises); with --edge_gain > 0 and
    `guided` the guide is the channel mean of that sweep's fp32 all-in-focus image."""
    if not args.regularize:
        return None
    want_guide = guided and args.edge_gain > 0
    wta = disparity.disparity(views, slopes, aperture=args.aperture, interp=args.interp, radius=args.radius, all_in_focus=want_guide,
                              aif_dtype=torch.float32, cost_volume=True, occlusion=occlusion_arguments(args))
    p1, p2 = disparity.penalties_from_cost(wta.cost)
    how = dict(p1=p1 if args.p1 is None else args.p1, p2=p2 if args.p2 is None else args.p2, paths=args.paths)
    if want_guide:
        how.update(guide=wta.all_in_focus.mean(-1), edge_gain=args.edge_gain)
    return how


def write_maps(out_dir, views, slopes, args, prefix=""):
    """views: [A, A, H, W, 3] on the GPU (uint8, or float32 in [0, 1]).  Returns the paths written."""
    r = disparity.disparity(views, slopes, aperture=args.aperture, interp=args.interp, radius=args.radius, all_in_focus="subset" if args.subset_aif else True,
                            aif_dtype=torch.uint8, regularize=regularize_arguments(views, slopes, args), occlusion=occlusion_arguments(args))
    paths = [os.path.join(out_dir, prefix + name) for name in ("disparity.png", "confidence.png", "all_in_focus.png", "disparity.npy")]
    png.write_png(paths[0], grey(r.disparity, min(slopes), max(slopes)))
    png.write_png(paths[1], grey(r.confidence, 0.0, 1.0))
    png.write_png(paths[2], r.all_in_focus.cpu().numpy())
    np.save(paths[3], r.disparity.cpu().numpy())
    if r.subset is not None:
        paths.append(os.path.join(out_dir, prefix + "occlusion.png"))
        png.write_png(paths[-1], (r.subset * 63)[..., None].expand(-1, -1, 3).contiguous().cpu().numpy())
    if args.refine:
        paths += write_refined(out_dir, views, slopes, args, prefix)
    return paths


def write_refined(out_dir, views, slopes, args, prefix=""):
    """--refine: disparity_refined.png / .npy and valid.png, and the JSON line.  Returns the paths written."""
    r = refine.refine(views, slopes, positions=args.refine_views, tau=args.tau, radius=args.median_radius, sigma=args.median_sigma,
                      iterations=args.median_iterations, sweep_radius=args.radius, aperture=args.aperture, interp=args.interp,
                      regularize=regularize_arguments(views, slopes, args), occlusion=occlusion_arguments(args))
    paths = [os.path.join(out_dir, prefix + name) for name in ("disparity_refined.png", "disparity_refined.npy", "valid.png")]
    png.write_png(paths[0], grey(r.disparity, min(slopes), max(slopes)))
    np.save(paths[1], r.disparity.cpu().numpy())
    png.write_png(paths[2], grey(r.valid.float(), 0.0, 1.0))
    changed = (r.disparity != r.raw.disparity) & (r.flags != 2)
    print(json.dumps({"refine": prefix + "disparity_refined", "views": args.refine_views, "invalid_share": float((r.valid == 0).float().mean()),
                      "median_changed_share": float(changed.float().mean()), "unfilled_share": float((r.flags == 2).float().mean())}))
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lf", required=True, help="light-field .mat (variable LF)")
    ap.add_argument("--angRes", type=int, default=5)
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--slopes", default="-2:2:33", help="LO:HI:N or a comma list, pixels per view step, strictly increasing")
    ap.add_argument("--radius", type=int, default=2, help="the cost is averaged over (2 radius + 1)^2 pixels, 0 .. 8")
    ap.add_argument("--aperture", default="full", choices=("full", "disk", "gaussian"))
    ap.add_argument("--interp", default="linear", choices=tuple(disparity.TAPS))
    ap.add_argument("--regularize", action="store_true", help="semi-global aggregation of the cost volume before the selection")
    ap.add_argument("--p1", type=float, default=None, help="penalty of a step of one slope (default: 0.1 x the mean cost)")
    ap.add_argument("--p2", type=float, default=None, help="penalty of a larger jump (default: the mean cost)")
    ap.add_argument("--paths", type=int, default=8, choices=(4, 8))
    ap.add_argument("--edge_gain", type=float, default=0.0, help="p2 falls by this times the step of the guide, not below p1")
    ap.add_argument("--occlusion", nargs="?", const="halves", default=None, choices=disparity.SUBSET_MODES,
                    help="occlusion-aware cost from partial apertures: the subsets of the views (default halves); also writes occlusion.png")
    ap.add_argument("--margin", type=float, default=2.0, help="a subset wins where it is this many times better than the whole aperture, >= 1")
    ap.add_argument("--min_views", type=int, default=2, help="subsets with fewer views of non-zero weight are dropped, >= 2")
    ap.add_argument("--subset_aif", action="store_true", help="all_in_focus.png from the views of the subset that set the cost (needs --occlusion)")
    ap.add_argument("--refine", action="store_true", help="cross-view check, guided weighted median and fill of the selected map; also writes disparity_refined.* and valid.png")
    ap.add_argument("--refine_views", default="cross", choices=refine.WHICH, help="the other positions whose maps the check compares with")
    ap.add_argument("--tau", type=float, default=None, help="two maps agree within this many slope units (default: the largest slope step)")
    ap.add_argument("--median_radius", type=int, default=3, help="the median's window is (2 R + 1)^2, 0 .. 7")
    ap.add_argument("--median_sigma", type=float, default=0.1, help="the guide's range weight falls by e per this share of the full range")
    ap.add_argument("--median_iterations", type=int, default=1)
    ap.add_argument("--min_confidence", type=float, default=0.5, help="pixels counted by the printed disparity_error")
    ap.add_argument("--path_pre_pth", default=None, help="checkpoint in the reference's format: sweep the super-resolved views")
    ap.add_argument("--scale_factor", type=int, default=4)
    ap.add_argument("--bicubic", action="store_true", help="sweep the bicubic baseline (prefix bicubic_)")
    ap.add_argument("--self_ensemble", default=None)
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16", "fp16"))
    ap.add_argument("--patch_size_for_test", type=int, default=32)
    ap.add_argument("--stride_for_test", type=int, default=16)
    args = ap.parse_args(argv)
    if args.subset_aif and not args.occlusion:
        ap.error("--subset_aif needs --occlusion")

    dev = torch.device("cuda", 0)
    slopes = parse_slopes(args.slopes)
    lf = super_resolve.load_field(args.lf, args.angRes, dev)
    os.makedirs(args.out_dir, exist_ok=True)
    paths = []
    sr = base = None
    if args.path_pre_pth:
        net = super_resolve.load_model(args, dev)
        sr = colour.super_resolve_lf(net, lf, args.patch_size_for_test, args.stride_for_test, ensemble=args.self_ensemble)
        paths += write_maps(args.out_dir, sr, slopes, args)
    if args.bicubic:
        base = colour.bicubic_lf(lf, args.angRes, args.scale_factor)
        paths += write_maps(args.out_dir, base, slopes, args, "bicubic_")
    if sr is None and base is None:
        raw = lf if lf.dtype in (torch.uint8, torch.float32) else lf.float()
        paths += write_maps(args.out_dir, raw, slopes, args)
    if sr is not None and base is not None:
        # one set of penalties for both sides: the bicubic (trusted) side's, and no guide
        err, share = disparity.disparity_error(sr, base, slopes, min_confidence=args.min_confidence, aperture=args.aperture,
                                               interp=args.interp, radius=args.radius, occlusion=occlusion_arguments(args), **({"regularize": regularize_arguments(base, slopes, args, guided=False)} if args.regularize else {}))
        print(json.dumps({"disparity_error": err, "confident_share": share, "min_confidence": args.min_confidence,
                          "against": "bicubic", "slopes": [min(slopes), max(slopes), len(slopes)], "radius": args.radius}))
    print(f"{args.out_dir}: {len(paths)} files, {len(slopes)} slopes from {min(slopes):g} to {max(slopes):g}")
    return paths


if __name__ == "__main__":
    main()
