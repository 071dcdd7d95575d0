"""Worker of tests/test_gpu_resume.py::test_two_ranks_resume_with_only_rank_0_reading: torch.distributed.run starts 2 ranks that SHARE
cuda:0 (gloo backend), each with half of every 2-patch batch.  Guarded step with clipping and an EMA; the second batch holds a NaN in
rank 1's shard alone, so steps_applied != t when the state is saved.

  first  DIR : one TrainStep runs all four steps (the uninterrupted run); another, on fresh weights, runs two and rank 0 saves the
               model checkpoint and the training state into DIR.  Every rank saves the uninterrupted run's buffers.
  resume DIR : a new net (rank 1: OTHER weights) and a new TrainStep; the state is loaded with rank 1 pointed at a path that does not
               exist -- only rank 0 reads --, two more steps, every rank saves its buffers."""
import os, sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lft_amd import dp, trainer, train as T                           # noqa: E402
from lft_amd.params import deterministic_state, synthetic_lr          # noqa: E402
from model import LFT                                                  # noqa: E402

A, S, B, H, W = 2, 2, 2, 6, 6
KW = dict(lr=2e-4, max_grad_norm=0.05, ema_decay=0.9)


def new_net(seed=1):
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=S))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, S, seed=seed, flavor="stress").items()})
    return net.to("cuda:0").train()


def batches(rank, world):
    out = []
    for k in range(4):
        lr = torch.from_numpy(synthetic_lr(B, A, H, W, seed=k))
        hr = torch.from_numpy(np.random.Generator(np.random.PCG64(70 + k)).random((B, 1, A * H * S, A * W * S), dtype=np.float32))
        b, e = dp.shard_range(B, rank, world)
        lr, hr = lr[b:e].cuda(), hr[b:e].cuda()
        if k == 1 and rank == 1:
            lr[0, 0, 3, 4] = float("nan")
        out.append((lr, hr))
    return out


def record(ts):
    rep = ts.guard_report()
    return {"p": ts.flat_params.cpu().clone(), "m": ts.m.cpu().clone(), "v": ts.v.cpu().clone(), "ema": ts.ema.cpu().clone(), "t": ts.t,
            "counters": {k: rep[k] for k in ("steps_applied", "steps_skipped", "steps_clipped")}}


def run(mode, d):
    rank, _, world = dp.env_world()
    dist.init_process_group("gloo")
    data = batches(rank, world)
    state_path = os.path.join(d, trainer.training_state_name("LFT", A, S))
    if mode == "first":
        full = T.TrainStep(new_net(), **KW)
        for lr, hr in data:
            full.step(lr, hr)
        torch.save(record(full), os.path.join(d, f"full.rank{rank}"))
        half = T.TrainStep(new_net(), **KW)
        for lr, hr in data[:2]:
            half.step(lr, hr)
        if rank == 0:
            trainer.save_checkpoint(half.net, os.path.join(d, trainer.checkpoint_name("LFT", A, S, 1)), 1)
            trainer.save_training_state(state_path, half, 1, {"world": world})
    else:
        ts = T.TrainStep(new_net(seed=1 if rank == 0 else 2), **KW)
        got = trainer.load_training_state(state_path if rank == 0 else os.path.join(d, "not-on-this-rank", "state.pth"), ts, model_name="LFT")
        assert got["epoch"] == 1 and got["world"] == world, got
        for lr, hr in data[2:]:
            ts.step(lr, hr)
        torch.save(record(ts), os.path.join(d, f"resumed.rank{rank}"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    run(sys.argv[1], sys.argv[2])
