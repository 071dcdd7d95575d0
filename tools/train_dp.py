"""One-process-per-GPU training launcher with the reference's option names (option.py) where they apply.

  python tools/train_dp.py --angRes 5 --scale_factor 2 --batch_size 8 --epoch 50 --data patches.npz --path_log ./log
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29500 tools/train_dp.py ...

--path_for_train DIR: the reference's own training tree (DIR/SR_AxA_sx/<dataset>/*.h5 with Lr_SAI_y / Hr_SAI_y, as
Generate_Data_for_Training.m writes it), read by lft_amd.h5lite (--data_name as in option.py).
--data: an .npz with arrays Lr_SAI_y [n, A*32, A*32] and Hr_SAI_y [n, A*32*s, A*32*s] (the two datasets of the
reference's training .h5 patches, stacked); --synthetic N instead makes N band-limited random light fields."""
import argparse, os, sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--angRes", type=int, default=5)
    ap.add_argument("--scale_factor", type=int, default=4)
    ap.add_argument("--model_name", default="LFT")
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--use_pre_pth", action="store_true")
    ap.add_argument("--path_pre_pth", default="./pth/LFT_5x5_4x_epoch_50_model.pth")
    ap.add_argument("--path_log", default="./log/")
    ap.add_argument("--batch_size", type=int, default=4, help="GLOBAL batch, as in the reference")
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--n_steps", type=int, default=15)
    ap.add_argument("--gamma", type=float, default=0.5)
    ap.add_argument("--decay_rate", type=float, default=0.0, help="Adam weight_decay, as the reference's option.py")
    ap.add_argument("--epoch", type=int, default=50)
    ap.add_argument("--data", default=None)
    ap.add_argument("--path_for_train", default=None, help="the reference's training tree (./data_for_train/): SR_AxA_sx/<dataset>/*.h5, read by lft_amd.h5lite")
    ap.add_argument("--data_name", default="ALL")
    ap.add_argument("--synthetic", type=int, default=0)
    ap.add_argument("--max_batches", type=int, default=0)
    ap.add_argument("--batch_metrics", action="store_true", help="per-batch PSNR / SSIM of train.py:121-124 (on the GPU) and the reference's epoch line")
    ap.add_argument("--gpu_augment", action="store_true", help="augment with one lft_dihedral_batch launch per tensor (same batches, bit for bit)")
    ap.add_argument("--max_grad_norm", type=float, default=None, help="clip the global gradient norm (as torch's clip_grad_norm_); implies --guard")
    ap.add_argument("--guard", action="store_true", help="guarded Adam step: a step with a NaN / inf gradient is skipped and reported, frozen tensors stay put")
    ap.add_argument("--ema_decay", type=float, default=None, help="keep an exponential moving average of the weights (e.g. 0.999); every epoch also writes ..._ema_model.pth")
    ap.add_argument("--no_ema_warmup", action="store_true", help="use --ema_decay from the first step instead of min(decay, (1 + t) / (10 + t))")
    ap.add_argument("--save_state", action="store_true", help="rewrite the training state file (moments, counters, EMA, history) after every epoch")
    ap.add_argument("--resume", default=None, metavar="auto|PATH", help="continue from a training state file; auto: the one in the checkpoint directory if there is one, else start fresh")
    ap.add_argument("--path_for_test", default=None, help="the reference's test tree: validate on it after every epoch (mean PSNR over the sets; the EMA weights with --ema_decay) and keep ..._best_model.pth")
    ap.add_argument("--loss", default="l1", choices=["l1", "mse", "charbonnier"], help="the penalty of the objective (lft_amd.loss.LFLoss); l1 alone is the reference's loss")
    ap.add_argument("--charbonnier_eps", type=float, default=1e-3)
    ap.add_argument("--pixel_weight", type=float, default=1.0, help="weight of the pixel term")
    ap.add_argument("--epi_weight", type=float, default=0.0, help="weight of the EPI-gradient term (the penalty on the gradients of the epipolar-plane images)")
    ap.add_argument("--ssim_weight", type=float, default=0.0, help="weight of the structural term 1 - SSIM (the mean over all views of the SSIM the epoch line reports)")
    ap.add_argument("--ssim_range", type=float, default=2.0, help="data range of that SSIM; 2 is what the epoch line and the tests report with")
    ap.add_argument("--focal_weight", type=float, default=0.0, help="weight of the focal-stack term: the penalty on the refocused difference SR - HR (lft_focal_loss)")
    ap.add_argument("--focal_slopes", default="-1:1:3", help="the slopes that term refocuses to: LO:HI:N or a comma list, HR pixels per view step")
    ap.add_argument("--focal_interp", default="linear", choices=["nearest", "linear", "cubic"], help="the interpolation of that refocus")
    args = ap.parse_args(argv)
    if args.resume and args.use_pre_pth:
        ap.error("--resume restores the weights of its own epoch: it cannot be combined with --use_pre_pth")
    return args


def loss_spec(args):
    """The spec for fit(loss=...), or None for the reference's L1 (which keeps the lft_l1_loss step)."""
    if args.loss == "l1" and args.pixel_weight == 1.0 and args.epi_weight == 0.0 and args.ssim_weight == 0.0 and args.focal_weight == 0.0:
        return None
    spec = {"penalty": args.loss, "eps": args.charbonnier_eps, "pixel_weight": args.pixel_weight, "epi_weight": args.epi_weight}
    if args.ssim_weight > 0.0:
        spec.update(ssim_weight=args.ssim_weight, ssim_range=args.ssim_range)
    if args.focal_weight > 0.0:
        from lft_amd.refocus import parse_slopes
        spec.update(focal_weight=args.focal_weight, focal_slopes=parse_slopes(args.focal_slopes), focal_interp=args.focal_interp)
    return spec


def checkpoint_dir(args) -> str:
    return os.path.join(args.path_log, "SR_%dx%d_%dx" % (args.angRes, args.angRes, args.scale_factor), args.model_name, "checkpoints")


def resolve_resume(args, log=print):
    """The state file to continue from, or None for a fresh start."""
    from lft_amd import trainer
    if not args.resume:
        return None
    if args.resume != "auto":
        return args.resume
    path = os.path.join(checkpoint_dir(args), trainer.training_state_name(args.model_name, args.angRes, args.scale_factor))
    if os.path.exists(path):
        return path
    log("--resume auto: no %s, starting fresh" % path)
    return None


def main():
    args = parse_args()
    import importlib
    from lft_amd import dp, trainer
    rank, local, world = dp.env_world()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=dev)
    MODEL = importlib.import_module("model." + args.model_name)          # reference train.py:31-33
    net = MODEL.get_model(args).to(dev)
    start = 0
    if args.use_pre_pth:
        start = trainer.load_checkpoint(net, args.path_pre_pth)
    else:
        net.apply(MODEL.weights_init)
    if args.path_for_train:
        from lft_amd import datasets
        src = datasets.H5PatchSource(args.path_for_train, args.angRes, args.scale_factor, args.data_name, cache=True)
    elif args.data:
        z = np.load(args.data)
        src = trainer.TensorPatchSource(torch.from_numpy(z["Lr_SAI_y"]), torch.from_numpy(z["Hr_SAI_y"]))
    else:
        src = trainer.SyntheticPatchSource(args.synthetic or 64, args.angRes, args.scale_factor, 32, seed=0)
    ckpt_dir = checkpoint_dir(args)
    # only rank 0 looks for the file: the others learn from it whether there is something to resume
    resume = resolve_resume(args) if rank == 0 else None
    if world > 1:
        box = [resume]
        dist.broadcast_object_list(box, src=0)
        resume = box[0]
    validate = None
    if args.path_for_test:
        from lft_amd import evaluate

        def validate(n):
            was_training = n.training
            res = evaluate.test_sets(n, args, log=lambda *_: None, sharded=False)   # rank 0 alone: no collective
            n.train(was_training)
            return float(np.mean([p for p, _ in res.values()]))
    trainer.fit(net, src, args.epoch, args.batch_size, lr=args.lr, n_steps=args.n_steps, gamma=args.gamma, start_epoch=start,
                ckpt_dir=ckpt_dir, model_name=args.model_name, max_batches_per_epoch=args.max_batches or None,
                decay_rate=args.decay_rate, batch_metrics=args.batch_metrics, gpu_augment=args.gpu_augment,
                max_grad_norm=args.max_grad_norm, guard=args.guard, ema_decay=args.ema_decay, ema_warmup=not args.no_ema_warmup,
                save_state=args.save_state, resume=resume, validate=validate,
                val_weights="ema" if args.ema_decay is not None else "live", loss=loss_spec(args))


if __name__ == "__main__":
    main()
