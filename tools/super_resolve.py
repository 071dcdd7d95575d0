"""Super-resolve one raw RGB light field and write its views as PNG files (GPU box).

  python tools/super_resolve.py --angRes 5 --scale_factor 4 --path_pre_pth LFT_5x5_4x.pth.tar --lf scene.mat --out_dir out/
                                [--self_ensemble dihedral|flips|none] [--precision fp32|bf16|fp16] [--bicubic] [--mosaic] [--shear auto|K]
                                [--blend hann|linear|flat] [--views all [--angular_stride K] [--angular_window flat|linear|hann]]

The scene is a light-field .mat with the variable LF [U, V, H, W, C] (uint8, or single / double in [0, 1]); its centre angRes x angRes
views are the LOW-resolution input.  Writes <out_dir>/view_<u>_<v>.png, 8-bit RGB, one per view (lft_amd.colour.super_resolve_lf:
the network super-resolves the luma, the chroma is up-scaled bicubically).  --bicubic adds bicubic_<u>_<v>.png, the bicubic
up-scaling of every channel that comparison figures show beside the result; --mosaic adds mosaic.png (and bicubic_mosaic.png), the
whole array of views in one image.  --views all super-resolves every view of a square U x U file, not only the centre angRes x angRes:
angRes x angRes windows slide over the views, --angular_stride apart (default angRes), and where they overlap the results are averaged
with the weights of --angular_window (lft_amd.field); it writes view_<p>_<q>.png for every view of the file."""
import argparse
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from lft_amd import colour, field, png, prepare, scene, trainer  # noqa: E402


def write_views(out_dir: str, views: torch.Tensor, prefix: str, mosaic_name=None):
    """views: uint8 [A, A, H, W, 3] on any device.  Returns the paths written."""
    v = views.cpu().numpy()
    A = v.shape[0]
    paths = []
    for u in range(A):
        for w in range(A):
            paths.append(os.path.join(out_dir, f"{prefix}_{u}_{w}.png"))
            png.write_png(paths[-1], v[u, w])
    if mosaic_name:
        paths.append(os.path.join(out_dir, mosaic_name))
        png.write_png(paths[-1], v.transpose(0, 2, 1, 3, 4).reshape(A * v.shape[2], A * v.shape[3], 3))
    return paths


def load_model(args, dev):
    """The network of --angRes / --scale_factor / --precision with the weights of --path_pre_pth, on `dev`."""
    from model import LFT
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=args.angRes, scale_factor=args.scale_factor),
                        precision=args.precision).to(dev).eval()
    trainer.load_checkpoint(net, args.path_pre_pth)
    return net


def load_field(path: str, A: int, dev) -> torch.Tensor:
    """The centre A x A views of the light-field .mat at `path` on `dev`, in the stored class and memory order."""
    return prepare.to_device(prepare.load_lf(path), A, dev)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--angRes", type=int, default=5)
    ap.add_argument("--scale_factor", type=int, default=4)
    ap.add_argument("--path_pre_pth", required=True, help="checkpoint in the reference's format")
    ap.add_argument("--lf", required=True, help="light-field .mat (variable LF)")
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--self_ensemble", default=None, help="dihedral, flips or none (lft_amd.ensemble.MASKS); default: one pass")
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16", "fp16"))
    ap.add_argument("--bicubic", action="store_true", help="also write the bicubic baseline")
    ap.add_argument("--mosaic", action="store_true", help="also write the whole array of views as one PNG")
    ap.add_argument("--patch_size_for_test", type=int, default=32)
    ap.add_argument("--stride_for_test", type=int, default=16)
    ap.add_argument("--shear", default=None, help="auto, or a whole number of LR pixels per view step: per-patch disparity compensation")
    ap.add_argument("--blend", default=None, help="hann, linear or flat: blend the overlapping SR patches with this window (default: the central crop)")
    ap.add_argument("--views", default=None, choices=("centre", "all"), help="all: every view of the file (a square field), by angular tiling")
    ap.add_argument("--angular_stride", type=int, default=None, help="with --views all: the windows' stride in views, 1 .. angRes (default angRes)")
    ap.add_argument("--angular_window", default=None, help="with --views all: flat (the default), linear or hann weights over a window's views")
    args = ap.parse_args(argv)
    every = args.views == "all"
    if every:
        field.check_astride(args.angular_stride, args.angRes)
        field.parse_angular(args.angular_window or "flat")
    elif args.angular_stride is not None or args.angular_window is not None:
        raise scene.LftError("--angular_stride and --angular_window belong to --views all")
    shear = scene.parse_shear(args.shear)
    blend = scene.parse_blend(args.blend)
    if blend is not None:
        scene.check_blend(blend, args.angRes, args.patch_size_for_test, args.stride_for_test, args.scale_factor)
    if isinstance(shear, int):
        scene.check_shear_limit(shear, args.angRes, args.patch_size_for_test, args.stride_for_test)

    dev = torch.device("cuda", 0)
    net = load_model(args, dev)
    ang = args.angRes
    if every:                                           # the whole file, loaded once: its own view count takes the place of angRes from here on
        whole = prepare.load_lf(args.lf)
        if whole.ndim != 5 or whole.shape[0] != whole.shape[1]:
            raise scene.LftError(f"--views all: {args.lf} holds a light field of shape {tuple(whole.shape)}; the colour path takes a square field")
        ang = int(whole.shape[0])
        lf = prepare.to_device(whole, ang, dev)
    else:
        lf = load_field(args.lf, args.angRes, dev)
    os.makedirs(args.out_dir, exist_ok=True)
    more = dict(views="all", astride=args.angular_stride, angular=args.angular_window or "flat") if every else {}
    sr = colour.super_resolve_lf(net, lf, args.patch_size_for_test, args.stride_for_test, ensemble=args.self_ensemble, shear=shear,
                                 **({} if blend is None else {"blend": blend}), **more)
    paths = write_views(args.out_dir, sr, "view", "mosaic.png" if args.mosaic else None)
    if args.bicubic:
        paths += write_views(args.out_dir, colour.bicubic_lf(lf, ang, args.scale_factor), "bicubic",
                             "bicubic_mosaic.png" if args.mosaic else None)
    print(f"{args.out_dir}: {len(paths)} PNG files, views of {sr.shape[3]} x {sr.shape[2]}")
    return paths


if __name__ == "__main__":
    main()
