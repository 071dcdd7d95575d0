"""TrainStep(max_grad_norm=..., guard=True) end to end on the GPU: A2 / 2x / B2 / 6x6 views, seeded weights.

The backward pass is pinned elsewhere (tests/test_gpu_train.py); here the optimizer is isolated by feeding the reference model
(tests/guard_util.py: clip_grad_norm_ + torch.optim.Adam in fp64) OUR flat gradients, read back after each step -- the guarded update
never writes the gradient buffer, so what is read is what the update saw.  (The LayerNorm weights of the seeded state reach 1.5, where
half an ulp of p is 2.98e-4 of lr: the `p` figure of these steps is that rounding, just inside the 3.02e-4 gate by construction.)"""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import _lib
from lft_amd import train as T
from lft_amd.params import deterministic_state, param_table, synthetic_lr
from model import LFT

import gpu_util as G
import guard_util as U

pytestmark = pytest.mark.gpu

A, S, B, H, W = 2, 2, 2, 6, 6
NAMES = [n for n, _, _ in param_table(64, S)]


def new_net(freeze=None):
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=S))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, S, seed=1, flavor="stress").items()})
    net = net.to(G.DEV).train()
    if freeze:
        for name, p in net.named_parameters():
            if name.startswith(freeze):
                p.requires_grad_(False)
    return net


def batch():
    lr = torch.from_numpy(synthetic_lr(B, A, H, W, seed=0)).to(G.DEV)
    hr = torch.from_numpy(np.random.Generator(np.random.PCG64(7)).random((B, 1, A * H * S, A * W * S), dtype=np.float32)).to(G.DEV)
    return lr, hr


def poisoned(lr):
    bad = lr.clone()
    bad[0, 0, 3, 4] = float("nan")                                            # one NaN pixel, as a damaged .h5 patch would hold
    return bad


def state(ts):
    return [t.cpu().numpy().copy() for t in (ts.flat_params, ts.m, ts.v)]


def test_clipped_steps_match_the_reference_on_our_gradients():
    lr, hr = batch()
    probe = T.TrainStep(new_net(), lr=U.LR, guard=True)
    probe.step(lr, hr)
    norm = probe.guard_report()["grad_norm"]
    assert np.isfinite(norm) and norm > 0
    mx = U.F32(0.5 * norm)
    ts = T.TrainStep(new_net(), lr=U.LR, max_grad_norm=mx)
    assert ts.guard and ts.max_grad_norm == mx
    table = U.real_table(S)
    for k in (1, 2):
        p0, m0, v0 = state(ts)
        ts.step(lr, hr)
        g = ts.flat_grads.cpu().numpy().copy()
        ref, info = U.ref_guarded_step(p0, g, m0, v0, table, k, 0.0, mx, torch.float64, gscale=1.0)
        rep = ts.guard_report()
        print(f"step {k}: grad norm {rep['grad_norm']:.6g} (fp64 {info['norm']:.6g}), coef {rep['clip_coef']:.9g} (fp64 {info['coef']:.9g})")
        assert abs(rep["grad_norm"] - info["norm"]) <= 2.0 ** -23 * info["norm"]
        assert abs(rep["clip_coef"] - info["coef"]) <= 2.0 ** -23 * info["coef"] and rep["clip_coef"] < 1.0
        assert rep["steps_applied"] == k and rep["steps_clipped"] == k and rep["steps_skipped"] == 0 and not rep["skipped"]
        assert set(rep["param_norms"]) == set(NAMES)
        U.check_step([a.astype(np.float64) for a in state(ts)], ref, p0.astype(np.float64), f"TrainStep clipped step {k}")


def test_poisoned_batch_is_skipped_and_without_the_guard_destroys_the_weights():
    lr, hr = batch()
    ts = T.TrainStep(new_net(), lr=U.LR, guard=True)
    w0 = [t.clone() for t in (ts.flat_params, ts.m, ts.v)]
    loss = ts.step(poisoned(lr), hr)
    for t, t0 in zip((ts.flat_params, ts.m, ts.v), w0):
        assert torch.equal(t.view(torch.int32), t0.view(torch.int32)), "a skipped step changed the weights or the moments"
    rep = ts.guard_report()
    print(f"poisoned batch: loss {float(loss)}, report { {k: v for k, v in rep.items() if k != 'param_norms'} }")
    assert rep["skipped"] and rep["steps_skipped"] == 1 and rep["steps_applied"] == 0 and rep["nonfinite"] > 0
    assert rep["bad_parameter"] in NAMES
    ts.step(lr, hr)                                                           # the next clean batch trains ...
    rep = ts.guard_report()
    assert not rep["skipped"] and rep["steps_applied"] == 1 and rep["steps_skipped"] == 1 and rep["bad_parameter"] is None
    assert bool(torch.isfinite(ts.flat_params).all()) and not torch.equal(ts.flat_params, w0[0])
    fresh = T.TrainStep(new_net(), lr=U.LR, guard=True)                       # ... as step number 1: the bias corrections did not advance
    fresh.step(lr, hr)
    assert torch.equal(ts.flat_params, fresh.flat_params) and torch.equal(ts.m, fresh.m) and torch.equal(ts.v, fresh.v)
    # the behaviour being fixed: the same batch through the unguarded update
    plain = T.TrainStep(new_net(), lr=U.LR)
    plain.step(poisoned(lr), hr)
    assert not bool(torch.isfinite(plain.flat_params).all()), "without the guard a NaN batch was expected to reach the weights"


def test_frozen_parameters_do_not_move():
    lr, hr = batch()
    ts = T.TrainStep(new_net(freeze="altblock"), lr=U.LR, guard=True)
    w0 = ts.flat_params.clone()
    for _ in range(2):
        ts.step(lr, hr)
    rep = ts.guard_report()
    assert rep["steps_applied"] == 2
    off = 0
    for name, shape, _ in param_table(64, S):
        k = int(np.prod(shape))
        moved = not torch.equal(ts.flat_params[off:off + k], w0[off:off + k])
        assert moved == name.startswith(("conv_init", "upsampling")), (name, moved)
        if name.startswith("altblock"):
            assert not ts.m[off:off + k].any() and not ts.v[off:off + k].any() and rep["param_norms"][name] > 0
        off += k
    # the norm counts the trainable tensors only
    tr = np.sqrt(sum(v ** 2 for n, v in rep["param_norms"].items() if not n.startswith("altblock")))
    assert abs(rep["grad_norm"] - tr) <= 1e-5 * tr


def test_defaults_take_the_old_path(monkeypatch):
    lr, hr = batch()
    L = _lib.lib()
    calls = {}

    def counted(name):
        fn = getattr(L, name)

        def wrapper(*a):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a)
        return wrapper

    for name in _lib.GUARD_EXPORTS + ("lft_adam_step",):
        monkeypatch.setattr(L, name, counted(name))
    runs = []
    for _ in range(2):
        ts = T.TrainStep(new_net())
        assert not ts.guard and ts.max_grad_norm is None
        for _ in range(2):
            ts.step(lr, hr)
        runs.append(ts.flat_params.clone())
        with pytest.raises(_lib.LftError):
            ts.guard_report()
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
    assert calls == {"lft_adam_step": 4}, calls
    # an infinite or non-positive max_grad_norm is "no clipping" and does not switch the guard on by itself
    assert not T.TrainStep(new_net(), max_grad_norm=float("inf")).guard


def test_two_ranks_clip_and_skip_alike(tmp_path):
    """Two ranks sharing the one GPU (gloo): the decision is taken after the all-reduce, on the same buffer, so both replicas clip
    by the same coefficient, and a NaN in rank 1's shard alone makes BOTH skip."""
    worker = os.path.join(os.path.dirname(__file__), "dp_guard_worker.py")
    out = str(tmp_path / "guard.pt")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                    "--master-port", "29631", worker, out], check=True, env=env, timeout=300)
    a, b = torch.load(out + ".rank0"), torch.load(out + ".rank1")
    assert a["norm"] == b["norm"] and a["norm"] > 0
    assert torch.equal(a["clipped"].view(torch.int32), b["clipped"].view(torch.int32)) and not torch.equal(a["clipped"], a["start"])
    for r in (a, b):
        rc, rs = r["report_clipped"], r["report_skipped"]
        assert rc["steps_clipped"] == 1 and rc["steps_applied"] == 1 and rc["clip_coef"] < 1.0 and not rc["skipped"]
        assert torch.equal(r["skipped"].view(torch.int32), r["clipped"].view(torch.int32)), "a rank stepped on the poisoned batch"
        assert rs["skipped"] and rs["steps_skipped"] == 1 and rs["steps_applied"] == 1 and rs["bad_parameter"] is not None
        assert bool(torch.isfinite(r["m"]).all()) and bool(torch.isfinite(r["v"]).all())
    assert a["report_clipped"] == b["report_clipped"] and a["report_skipped"] == b["report_skipped"]
