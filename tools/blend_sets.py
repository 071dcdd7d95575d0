#!/usr/bin/env python3
"""tools/test_sets.py with windowed blending of the overlapping SR patches: every scene of every test dataset under
``--path_for_test`` through LFdivide -> LFT -> the window-weighted mean of every SR patch pixel that shows a scene pixel, in
place of LFintegrate's central crop -> per-view PSNR / SSIM (lft_amd.evaluate.test_sets(..., blend=...)).
Option names are the reference's (option.py).

    python tools/blend_sets.py --angRes 5 --scale_factor 4 --use_pre_pth --path_pre_pth model.pth --blend hann --stride_for_test 24
    python -m torch.distributed.run --nproc-per-node 8 tools/blend_sets.py ...  (scenes of a dataset sharded over the ranks)

--blend: hann, linear or flat = the window over the SR patch (lft_amd.scene.window_table), none = the crop, i.e. what
tools/test_sets.py reports.  --stride_for_test: a larger stride runs fewer patches ((32/24)^2 = 2.25 times fewer at 24 than at 16);
patch - stride must be even.  A tiling the blend cannot take is refused before the device is opened."""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse(argv=None):
    """(args, blend): the options, and --blend as lft_amd.scene.super_resolve_scene takes it; needs no device."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--blend", default="hann", help="hann, linear, flat, or none")
    ap.add_argument("--angRes", type=int, default=5)
    ap.add_argument("--scale_factor", type=int, default=4)
    ap.add_argument("--model_name", default="LFT")
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--use_pre_pth", action="store_true")
    ap.add_argument("--path_pre_pth", default="./pth/LFT_5x5_4x_epoch_50_model.pth")
    ap.add_argument("--path_for_test", default="./data_for_test/")
    ap.add_argument("--patch_size_for_test", type=int, default=32)
    ap.add_argument("--stride_for_test", type=int, default=16)
    ap.add_argument("--num_workers", type=int, default=0)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "fp16", "bf16"])
    args = ap.parse_args(argv)
    from lft_amd import scene
    blend = scene.parse_blend(args.blend)
    if blend is not None:
        scene.check_blend(blend, args.angRes, args.patch_size_for_test, args.stride_for_test, args.scale_factor)
    return args, blend


def main(argv=None):
    args, blend = parse(argv)
    from lft_amd import dp, evaluate, trainer
    rank, local, world = dp.env_world()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=dev)
    MODEL = importlib.import_module("model." + args.model_name)
    args.lft_precision = args.precision
    net = MODEL.get_model(args).to(dev)
    if args.use_pre_pth:
        trainer.load_checkpoint(net, args.path_pre_pth)
    else:
        net.apply(MODEL.weights_init)
    return evaluate.test_sets(net, args, log=(print if rank == 0 else (lambda *_: None)), blend=blend)


if __name__ == "__main__":
    main()
