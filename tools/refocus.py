"""Focal stack and EPI slices of one light field as PNG files (GPU box): what angular consistency is judged by.

  python tools/refocus.py --lf scene.mat --angRes 5 --out_dir out/ --slopes=-2:2:9 [--aperture full|disk|gaussian]
                          [--interp nearest|linear|cubic] [--epi_row R] [--epi_col C] [--epi_zoom 8]
                          [--path_pre_pth LFT_5x5_4x.pth.tar --scale_factor 4 [--precision ..] [--self_ensemble ..]] [--bicubic]

The scene is a light-field .mat with the variable LF [U, V, H, W, C]; its centre angRes x angRes views are used.  Without
--path_pre_pth and --bicubic the raw views are refocused.  With --path_pre_pth the light field first goes through
lft_amd.colour.super_resolve_lf (slopes are then in HR pixels per view step); --bicubic does the same with colour.bicubic_lf and
the prefix bicubic_, for a side-by-side comparison (--scale_factor says how far).  --slopes is LO:HI:N (N slopes from LO to HI) or
a comma list (written with = when it starts with a minus sign).  Writes <out_dir>/focus_<k>_<slope>.png per slope
(lft_amd.refocus.refocus, shift-and-add) and epi_h_<row>.png / epi_v_<col>.png, the horizontal and the vertical EPI through the
centre view (default: the middle row and column), every view's line repeated --epi_zoom times."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lft_amd import colour, png, refocus  # noqa: E402
import super_resolve  # noqa: E402  (the loader of the scene and of the network)


parse_slopes = refocus.parse_slopes      # LO:HI:N or a comma list; tools/disparity.py and tools/view_path.py take it from here


def write_stack(out_dir, views, slopes, args, prefix=""):
    """views: [A, A, H, W, 3] on the GPU (uint8, or float32 in [0, 1]).  Returns the paths written."""
    stack = refocus.refocus(views, slopes, aperture=args.aperture, interp=args.interp, out_dtype=torch.uint8).cpu().numpy()
    paths = []
    for k, d in enumerate(slopes):
        paths.append(os.path.join(out_dir, f"{prefix}focus_{k:02d}_{d:+.3f}.png"))
        png.write_png(paths[-1], stack[k])
    as_bytes = views if views.dtype == torch.uint8 else (views.clamp(0, 1) * 255).round().to(torch.uint8)
    for name, kw in ((f"epi_h_{args.epi_row if args.epi_row is not None else views.shape[2] // 2}", dict(row=args.epi_row)),
                     (f"epi_v_{args.epi_col if args.epi_col is not None else views.shape[3] // 2}",
                      dict(col=args.epi_col if args.epi_col is not None else views.shape[3] // 2))):
        e = refocus.epi(as_bytes, **kw).cpu().numpy()
        paths.append(os.path.join(out_dir, f"{prefix}{name}.png"))
        png.write_png(paths[-1], np.repeat(e, args.epi_zoom, axis=0))
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lf", required=True, help="light-field .mat (variable LF)")
    ap.add_argument("--angRes", type=int, default=5)
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--slopes", default="-2:2:9", help="LO:HI:N or a comma list, pixels per view step")
    ap.add_argument("--aperture", default="full", choices=("full", "disk", "gaussian"))
    ap.add_argument("--interp", default="cubic", choices=tuple(refocus.TAPS))
    ap.add_argument("--epi_row", type=int, default=None)
    ap.add_argument("--epi_col", type=int, default=None)
    ap.add_argument("--epi_zoom", type=int, default=8)
    ap.add_argument("--path_pre_pth", default=None, help="checkpoint in the reference's format: refocus the super-resolved views")
    ap.add_argument("--scale_factor", type=int, default=4)
    ap.add_argument("--bicubic", action="store_true", help="refocus the bicubic baseline (prefix bicubic_)")
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
    if args.path_pre_pth:
        net = super_resolve.load_model(args, dev)
        sr = colour.super_resolve_lf(net, lf, args.patch_size_for_test, args.stride_for_test, ensemble=args.self_ensemble)
        paths += write_stack(args.out_dir, sr, slopes, args)
    if args.bicubic:
        paths += write_stack(args.out_dir, colour.bicubic_lf(lf, args.angRes, args.scale_factor), slopes, args, "bicubic_")
    if not args.path_pre_pth and not args.bicubic:
        raw = lf if lf.dtype in (torch.uint8, torch.float32) else lf.float()
        paths += write_stack(args.out_dir, raw, slopes, args)
    print(f"{args.out_dir}: {len(paths)} PNG files, {len(slopes)} slopes from {min(slopes):g} to {max(slopes):g}")
    return paths


if __name__ == "__main__":
    main()
