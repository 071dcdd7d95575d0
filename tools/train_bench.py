"""Training-step throughput (BASELINE configs[2]: LFT 5x5 angRes 2xSR training, Adam + gradient all-reduce), fp32.

  python tools/train_bench.py --batch 8 --steps 20 --warmup 5
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P tools/train_bench.py --gpus N ...

One process per GPU, each with its own --batch patches (weak scaling); a step = forward-with-tape, L1 loss + its
gradient, backward, ONE all-reduce of the flat gradient buffer (RCCL), fused Adam.  Same timing protocol as bench.py
(barrier + synchronize on both sides, max over ranks).  Prints one JSON line on rank 0.  --phases adds "adam_ms": the
event-timed milliseconds of the optimizer launches alone, as step() enqueues them (lft_adam_step or lft_adam_step_guarded, then
lft_ema_update with --ema_decay), the median over 50 groups of 10 updates.
--ema_decay D keeps the EMA of the weights (lft_ema_update after the Adam kernel); with --alternate R a second TrainStep WITHOUT the
EMA is built beside it and R rounds of --steps steps alternate between the two in this one process: "ms_per_step_rounds" then holds
both series, the only fair way to see a difference of this size.
--loss {l1,mse,charbonnier} / --epi_weight W: the step minimises an lft_amd.loss.LFLoss (lft_lf_loss in the place of lft_l1_loss), and
"loss_ms" holds the event-timed milliseconds of the loss launches alone -- lft_lf_loss and, alternating with it in this one process on
the same tensors, lft_l1_loss (medians over 50 calls each).
--ssim_weight W / --ssim_range R: the objective gains W * (1 - SSIM) (lft_ssim_loss right after lft_lf_loss, accumulating into the same
gradient); "loss_ms" then also times that call.
--focal_weight W / --focal_slopes=LO:HI:N / --focal_interp I: the objective gains W * F, the penalty on the focal stack of SR - HR
(lft_focal_loss after the other terms); "loss_ms" then also times that call, and with --alternate R a second TrainStep with the same
objective WITHOUT the focal term alternates with it ("ms_per_step_rounds": "focal" and "no_focal").  "loss_ms" gains
"lft_focal_loss_standalone": the call alone (not accumulating, with its gradient) on the step's tensors."""
import argparse, json, os, sys, time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_loss_launches(ts, hr, calls=50):
    """Median event-timed milliseconds of one lft_lf_loss call (the step's objective) and of one lft_l1_loss call on the same tensors,
    the two alternating."""
    from lft_amd import _lib
    from lft_amd.loss import focal_loss, lf_loss, ssim_loss
    sr, dout = ts.last_out, torch.empty_like(hr)
    n = sr.numel()
    scratch = ts._loss_scratch_for(hr)

    def run_lf():
        lf_loss(sr, hr, ts.A, ts.loss.penalty, ts.loss.eps, ts.loss.pixel_weight, ts.loss.epi_weight, dsr=dout, loss3=ts.last_loss_terms,
                scratch=scratch)

    def run_l1():
        _lib.enqueue("lft_l1_loss", hr.device, sr.data_ptr(), hr.data_ptr(), n, dout.data_ptr(), 1.0 / n, ts._scratch[1024:].data_ptr(),
                     ts._scratch.data_ptr())

    def run_ssim():
        ssim_loss(sr, hr, ts.A, ts.loss.ssim_range, ts.loss.ssim_weight, dsr=dout, accumulate=ts.loss.has_lf_terms(),
                  total=ts.last_loss_terms[0:1], ssim_out=ts.last_loss_terms[3:4], scratch=ts._ssim_scratch[tuple(hr.shape)])

    def run_focal(accumulate=True):
        focal_loss(sr, hr, ts.A, ts.loss.focal_slopes, ts.loss.focal_interp, "full", ts.loss.penalty, ts.loss.eps, ts.loss.focal_weight, dsr=dout,
                   accumulate=accumulate and (ts.loss.has_lf_terms() or ts.loss.ssim_weight > 0.0), total=ts.last_loss_terms[0:1],
                   focal_out=ts.last_loss_terms[4:5], scratch=ts._focal_scratch[tuple(hr.shape)])

    runs = [("lft_l1_loss", run_l1)] + ([("lft_lf_loss", run_lf)] if ts.loss.has_lf_terms() else [])
    if ts.loss.ssim_weight > 0.0:
        runs.append(("lft_ssim_loss", run_ssim))
    if ts.loss.focal_weight > 0.0:
        runs += [("lft_focal_loss", run_focal), ("lft_focal_loss_standalone", lambda: run_focal(False))]
    ms = {name: [] for name, _ in runs}
    for i in range(calls + 5):
        for name, run in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            if i >= 5:
                ms[name].append(e0.elapsed_time(e1))
    return {k: float(np.median(v)) for k, v in ms.items()}


def time_optimizer_launches(ts, groups=50, per=10):
    """Median event-timed milliseconds of one optimizer update of the step, on the step's own buffers (run after the timed steps:
    it moves the weights)."""
    from lft_amd import _lib, train as T
    dev = ts.flat_params.device

    def update():
        ts.t += 1
        if ts._guard is None:
            _lib.enqueue("lft_adam_step", dev, ts.flat_params.data_ptr(), ts.flat_grads.data_ptr(), ts.m.data_ptr(), ts.v.data_ptr(),
                         ts.flat_params.numel(), ts.lr, ts.betas[0], ts.betas[1], ts.eps, ts.t, 1.0, ts.weight_decay)
        else:
            T.adam_step_guarded(ts.flat_params, ts.flat_grads, ts.m, ts.v, ts._guard, ts.lr, ts.betas[0], ts.betas[1], ts.eps, 1.0,
                                ts.weight_decay, ts.max_grad_norm)
        if ts.ema is not None:
            T.ema_update(ts.ema, ts.flat_params, ts.ema_decay, ts.ema_warmup, ts.t, ts._guard)

    ms = []
    for i in range(groups + 5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per):
            update()
        e1.record()
        e1.synchronize()
        if i >= 5:
            ms.append(e0.elapsed_time(e1) / per)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8, help="LF patches per GPU per step")
    ap.add_argument("--ang", type=int, default=5)
    ap.add_argument("--lr", type=int, default=32)
    ap.add_argument("--scale", type=int, default=2, choices=[2, 4])
    ap.add_argument("--phases", action="store_true")
    ap.add_argument("--math", default="bf16x3", choices=["fp32", "bf16x3", "bf16x6"])
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--guard", action="store_true", help="the guarded Adam step (lft_adam_step_guarded, no clipping) in place of lft_adam_step")
    ap.add_argument("--ema_decay", type=float, default=None, help="keep an exponential moving average of the weights (lft_ema_update every step)")
    ap.add_argument("--alternate", type=int, default=0, metavar="R", help="with --ema_decay: R rounds alternating with an identical step that keeps no EMA")
    ap.add_argument("--loss", default=None, choices=["l1", "mse", "charbonnier"], help="penalty of an LFLoss objective; default: the reference's L1 step")
    ap.add_argument("--epi_weight", type=float, default=0.0, help="weight of the EPI-gradient term of --loss")
    ap.add_argument("--ssim_weight", type=float, default=0.0, help="weight of the structural term 1 - SSIM (lft_ssim_loss)")
    ap.add_argument("--ssim_range", type=float, default=2.0, help="data range of that SSIM; 2 is what fit and evaluate report with")
    ap.add_argument("--focal_weight", type=float, default=0.0, help="weight of the focal-stack term (lft_focal_loss)")
    ap.add_argument("--focal_slopes", default="-1:1:3", help="the slopes that term refocuses to: LO:HI:N or a comma list")
    ap.add_argument("--focal_interp", default="linear", choices=["nearest", "linear", "cubic"])
    args = ap.parse_args()
    if args.alternate and args.ema_decay is None and args.focal_weight == 0.0:
        ap.error("--alternate compares with and without the EMA or the focal term: it needs --ema_decay or --focal_weight")
    from lft_amd import dp, train as T
    from lft_amd.params import deterministic_state, synthetic_lr
    from model import LFT
    rank, local, world = dp.env_world()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=dev)
    A, S, H = args.ang, args.scale, args.lr

    def new_net():
        net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=S))
        net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, S, seed=1).items()})
        return net.to(dev).train()

    lr = torch.from_numpy(synthetic_lr(args.batch, A, H, H, seed=rank)).to(dev)
    hr = torch.from_numpy(np.random.Generator(np.random.PCG64([2, rank])).random((args.batch, 1, A * H * S, A * H * S), dtype=np.float32)).to(dev)
    spec = None if args.loss is None and args.ssim_weight == 0.0 else {"penalty": args.loss or "l1", "epi_weight": args.epi_weight}
    if args.ssim_weight > 0.0:
        spec.update(ssim_weight=args.ssim_weight, ssim_range=args.ssim_range)
    base_spec = spec                                     # the objective without the focal term: what --alternate compares with
    if args.focal_weight > 0.0:
        from lft_amd.refocus import parse_slopes
        spec = dict(spec or {"penalty": "l1"}, focal_weight=args.focal_weight, focal_slopes=parse_slopes(args.focal_slopes), focal_interp=args.focal_interp)
    ts = T.TrainStep(new_net(), lr=2e-4, math=args.math, graph=not args.no_graph, guard=args.guard, ema_decay=args.ema_decay, loss=spec)

    def sync():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    losses = []
    for _ in range(args.warmup):
        losses.append(ts.step(lr, hr))
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        losses.append(ts.step(lr, hr))
    sync()
    dt = dp.barrier_max_seconds(time.perf_counter() - t0, dev)
    rounds = None
    if args.alternate:
        with_name = "focal" if args.focal_weight > 0.0 else "ema"
        if args.focal_weight > 0.0:
            base = T.TrainStep(new_net(), lr=2e-4, math=args.math, graph=not args.no_graph, guard=args.guard, ema_decay=args.ema_decay, loss=base_spec)
        else:
            base = T.TrainStep(new_net(), lr=2e-4, math=args.math, graph=not args.no_graph, guard=args.guard)
        for _ in range(args.warmup):
            base.step(lr, hr)
        rounds = {with_name: [], "no_" + with_name: []}
        for _ in range(args.alternate):
            for name, step in (("no_" + with_name, base), (with_name, ts)):
                sync()
                t1 = time.perf_counter()
                for _ in range(args.steps):
                    step.step(lr, hr)
                sync()
                rounds[name].append(1e3 * dp.barrier_max_seconds(time.perf_counter() - t1, dev) / args.steps)
    loss_ms = None
    if ts.loss is not None:
        loss_ms = time_loss_launches(ts, hr)
    lv = [float(x) for x in losses]
    assert all(np.isfinite(lv)), lv
    if rank == 0:
        V = A * A
        flops_fwd = {2: 58.85e9, 4: 61.73e9}[S] * (H * H / 1024.0) * (V / 25.0)      # SURVEY 8d (approximate outside cfg shapes)
        out = {"metric": f"LF patches/sec training ({A}x{A} angRes, {H}x{H} LR, {S}xSR, fp32, Adam)", "value": args.batch * world * args.steps / dt,
               "unit": "patches/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
               "higher_is_better": True, "scaling": "weak", "dtype": "f32" if args.math == "fp32" else "f32 (split-bf16 products)", "data": "synthetic",
               "config": {"workload": f"LFT {A}x{A} angRes {S}xSR training step, batch={args.batch} per GPU, {H}x{H} LR patches",
                          "global_batch": args.batch * world, "parallelism": f"dp{world} (one flat-gradient all-reduce per step)"},
               "loss_first_last": [lv[0], lv[-1]],
               "tflops_algorithmic": 3 * flops_fwd * args.batch * world * args.steps / dt / 1e12,
               "tape_gib": T.tape_bytes(args.batch, A, H, H, S) / 2**30, "guard": bool(args.guard), "ema_decay": args.ema_decay}
        if rounds:
            out["ms_per_step_rounds"] = rounds
        if loss_ms:
            out["loss"] = ts.loss.spec()
            out["loss_ms"] = loss_ms
        if args.phases:
            out["adam_ms"] = time_optimizer_launches(ts)
        if args.guard:
            rep = ts.guard_report()
            out["guard_report"] = {k: rep[k] for k in ("grad_norm", "steps_applied", "steps_skipped", "steps_clipped")}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
