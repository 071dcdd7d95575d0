"""Worker of tests/test_gpu_guard_train.py::test_two_ranks_clip_and_skip_alike: torch.distributed.run starts 2 ranks that SHARE cuda:0
(gloo backend, flat gradients summed through the host), each with half of a 2-patch batch.  A first TrainStep (guard only) measures
the global gradient norm; a second one, on fresh weights, clips at half of it for one step and is then given a batch in which ONLY
rank 1's shard holds a NaN.  Every rank saves its weights after both steps and both reports."""
import os, sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lft_amd import dp, train as T                                     # noqa: E402
from lft_amd.params import deterministic_state, synthetic_lr          # noqa: E402
from model import LFT                                                  # noqa: E402

A, S, B, H, W = 2, 2, 2, 6, 6


def new_net():
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=S))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, S, seed=1, flavor="stress").items()})
    return net.to("cuda:0").train()


def run(out_path):
    rank, _, world = dp.env_world()
    dist.init_process_group("gloo")
    lr = torch.from_numpy(synthetic_lr(B, A, H, W, seed=0))
    hr = torch.from_numpy(np.random.Generator(np.random.PCG64(7)).random((B, 1, A * H * S, A * W * S), dtype=np.float32))
    b, e = dp.shard_range(B, rank, world)
    lr, hr = lr[b:e].cuda(), hr[b:e].cuda()
    probe = T.TrainStep(new_net(), lr=2e-4, guard=True)
    probe.step(lr, hr)
    norm = probe.guard_report()["grad_norm"]
    ts = T.TrainStep(new_net(), lr=2e-4, max_grad_norm=0.5 * norm)
    start = ts.flat_params.cpu().clone()
    ts.step(lr, hr)
    rec = {"norm": norm, "start": start, "clipped": ts.flat_params.cpu().clone(), "report_clipped": ts.guard_report()}
    bad = lr.clone()
    if rank == 1:
        bad[0, 0, 3, 4] = float("nan")
    ts.step(bad, hr)
    rec.update(skipped=ts.flat_params.cpu().clone(), report_skipped=ts.guard_report(), m=ts.m.cpu().clone(), v=ts.v.cpu().clone())
    torch.save(rec, f"{out_path}.rank{rank}")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    run(sys.argv[1])
