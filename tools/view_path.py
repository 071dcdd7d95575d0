"""Views along a camera path, or the densified array of views, of one light field (GPU box): what the disparity map is for.

  python tools/view_path.py --lf scene.mat --angRes 5 --out_dir out/ --slopes=-2:2:33 --path circle|line|grid:<factor> --frames 24
                            [--radius 2] [--interp linear|cubic] [--blend quad|gaussian|nearest] [--visibility [TAU]]
                            [--path_pre_pth LFT_5x5_4x.pth.tar --scale_factor 4 [--precision ..] [--self_ensemble ..]] [--bicubic]

The scene is a light-field .mat with the variable LF [U, V, H, W, C]; its centre angRes x angRes views are used.  Without
--path_pre_pth and --bicubic the raw views are rendered.  With --path_pre_pth the light field first goes through
lft_amd.colour.super_resolve_lf; --bicubic does the same with colour.bicubic_lf and the prefix bicubic_.  The disparity map comes
from one lft_amd.disparity.disparity sweep of the views being rendered (slopes LO:HI:N or a comma list, pixels of those views per
view step), the views from one lft_amd.views.render call.  circle: --frames targets on the circle of radius (A-1)/2 about the
centre view; line: --frames targets from the left-most to the right-most view of the centre row; both write frame_<i>.png.
grid:<factor>: lft_amd.views.densify, written as view_<i>_<j>.png, i and j counting the factor * (A-1) + 1 positions a side.
With both --path_pre_pth and --bicubic it prints one JSON line with the leave-one-out PSNR (lft_amd.views.leave_one_out, mean
over the views) of the super-resolved and of the bicubic views: how well each field's other views predict a held-out one.
--visibility [TAU]: render with the per-view visibility test (lft_amd.views, "Visibility"), the per-view maps warped from the swept
one.  TAU defaults to the largest step between adjacent slopes of the sweep -- a choice, not a measurement: two surfaces the sweep
cannot tell apart do not occlude one another.  The JSON line then also carries the leave-one-out PSNR with the test
(leave_one_out_psnr_visible), beside the one without."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lft_amd import colour, disparity, png, views  # noqa: E402
from refocus import parse_slopes  # noqa: E402  (tools/refocus.py)
import super_resolve  # noqa: E402  (the loader of the scene and of the network)


def path_targets(kind: str, A: int, frames: int):
    """[(ut, vt)] of a circle or a line inside the grid of views."""
    uc = (A - 1) / 2
    if frames < 1:
        raise SystemExit("--frames must be positive")
    if kind == "circle":
        return [(uc + uc * math.sin(2 * math.pi * k / frames), uc + uc * math.cos(2 * math.pi * k / frames)) for k in range(frames)]
    if kind == "line":
        return [(float(A // 2), (A - 1) * k / max(frames - 1, 1)) for k in range(frames)]
    raise SystemExit(f"--path must be circle, line or grid:<factor>, got {kind!r}")


def visibility_of(args, slopes):
    """None, or the `visibility` argument of lft_amd.views.render for --visibility [TAU]."""
    if args.visibility is None:
        return None
    tau = max(np.diff(np.array(slopes, dtype=np.float64)), default=0.0) if args.visibility == "auto" else float(args.visibility)
    return dict(tau=float(tau))


def write_frames(out_dir, field, slopes, args, prefix=""):
    """field: [A, A, H, W, 3] on the GPU (uint8, or float32 in [0, 1]).  Returns the paths written."""
    A = int(field.shape[0])
    d_range = (min(slopes), max(slopes))
    dr = disparity.disparity(field, slopes, interp=args.interp, radius=args.radius).disparity
    kw = dict(blend=args.blend, interp=args.interp, out_dtype=torch.uint8, visibility=visibility_of(args, slopes))
    if args.path.startswith("grid:"):
        dense = views.densify(field, dr, int(args.path[5:]), d_range, **kw).cpu().numpy()
        named = [(f"view_{i}_{j}.png", dense[i, j]) for i in range(dense.shape[0]) for j in range(dense.shape[1])]
    else:
        got = views.render(field, dr, path_targets(args.path, A, args.frames), d_range, **kw).views.cpu().numpy()
        named = [(f"frame_{k}.png", got[k]) for k in range(got.shape[0])]
    paths = []
    for name, image in named:
        paths.append(os.path.join(out_dir, prefix + name))
        png.write_png(paths[-1], np.ascontiguousarray(image))
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lf", required=True, help="light-field .mat (variable LF)")
    ap.add_argument("--angRes", type=int, default=5)
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--slopes", default="-2:2:33", help="LO:HI:N or a comma list, pixels per view step, strictly increasing")
    ap.add_argument("--path", default="circle", help="circle, line or grid:<factor>")
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--radius", type=int, default=2, help="aggregation radius of the disparity sweep, 0 .. 8")
    ap.add_argument("--interp", default="linear", choices=tuple(views.TAPS))
    ap.add_argument("--blend", default="quad", choices=("quad", "gaussian", "nearest"))
    ap.add_argument("--visibility", nargs="?", const="auto", default=None, metavar="TAU",
                    help="per-view visibility test; TAU defaults to the largest step between adjacent slopes")
    ap.add_argument("--path_pre_pth", default=None, help="checkpoint in the reference's format: render the super-resolved views")
    ap.add_argument("--scale_factor", type=int, default=4)
    ap.add_argument("--bicubic", action="store_true", help="render the bicubic baseline (prefix bicubic_)")
    ap.add_argument("--self_ensemble", default=None)
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16", "fp16"))
    ap.add_argument("--patch_size_for_test", type=int, default=32)
    ap.add_argument("--stride_for_test", type=int, default=16)
    args = ap.parse_args(argv)

    dev = torch.device("cuda", 0)
    slopes = parse_slopes(args.slopes)
    lf = super_resolve.load_field(args.lf, args.angRes, dev)
    os.makedirs(args.out_dir, exist_ok=True)
    paths = []
    sr = base = None
    if args.path_pre_pth:
        net = super_resolve.load_model(args, dev)
        sr = colour.super_resolve_lf(net, lf, args.patch_size_for_test, args.stride_for_test, ensemble=args.self_ensemble)
        paths += write_frames(args.out_dir, sr, slopes, args)
    if args.bicubic:
        base = colour.bicubic_lf(lf, args.angRes, args.scale_factor)
        paths += write_frames(args.out_dir, base, slopes, args, "bicubic_")
    if sr is None and base is None:
        raw = lf if lf.dtype in (torch.uint8, torch.float32) else lf.float()
        paths += write_frames(args.out_dir, raw, slopes, args)
    if sr is not None and base is not None:
        loo = {name: views.leave_one_out(field, slopes, interp=args.interp, radius=args.radius) for name, field in (("sr", sr), ("bicubic", base))}
        rec = {"leave_one_out_psnr": {k: float(np.mean(v)) for k, v in loo.items()},
               "leave_one_out_psnr_min": {k: float(np.min(v)) for k, v in loo.items()}, "views": len(loo["sr"]),
               "slopes": [min(slopes), max(slopes), len(slopes)], "radius": args.radius, "interp": args.interp}
        vis = visibility_of(args, slopes)
        if vis is not None:
            seen = {name: views.leave_one_out(field, slopes, interp=args.interp, radius=args.radius, visibility=vis) for name, field in (("sr", sr), ("bicubic", base))}
            rec["leave_one_out_psnr_visible"] = {k: float(np.mean(v)) for k, v in seen.items()}
            rec["visibility_tau"] = vis["tau"]
        print(json.dumps(rec))
    print(f"{args.out_dir}: {len(paths)} files, path {args.path}")
    return paths


if __name__ == "__main__":
    main()
