#!/usr/bin/env python3
"""tools/test_sets.py with per-patch disparity compensation: every scene of every test dataset under ``--path_for_test`` through
LFdivide with a whole-number shear per patch -> LFT -> LFintegrate against the shear -> per-view PSNR / SSIM
(lft_amd.evaluate.test_sets(..., shear=...)).  Option names are the reference's (option.py).

    python tools/shear_sets.py --angRes 5 --scale_factor 4 --use_pre_pth --path_pre_pth model.pth --shear auto
    python -m torch.distributed.run --nproc-per-node 8 tools/shear_sets.py ...  (scenes of a dataset sharded over the ranks)

--shear: auto = every patch's k from a plane sweep and a vote (lft_amd.scene.estimate_shear), K = one whole number of LR pixels per
view step for all patches (beyond lft_amd.scene.shear_limit it is refused before the device is opened), none = the plain cut, i.e.
what tools/test_sets.py reports."""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse(argv=None):
    """(args, shear): the options, and --shear as lft_amd.scene.super_resolve_scene takes it; needs no device."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--shear", default="auto", help="auto, none, or a whole number of LR pixels per view step")
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
    shear = None if args.shear == "none" else scene.parse_shear(args.shear)
    if isinstance(shear, int):
        scene.check_shear_limit(shear, args.angRes, args.patch_size_for_test, args.stride_for_test)
    return args, shear


def main(argv=None):
    args, shear = parse(argv)
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
    return evaluate.test_sets(net, args, log=(print if rank == 0 else (lambda *_: None)), shear=shear)


if __name__ == "__main__":
    main()
