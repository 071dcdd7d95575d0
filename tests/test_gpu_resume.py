"""Resuming a training run on the GPU: TrainStep.state_dict() / load_state_dict(), the EMA weights, trainer.fit(resume=...) and the
two-rank broadcast of a state only rank 0 reads.  A2 / 2x / B2 / 6x6 views, seeded "stress" weights (the shapes of
tests/dp_guard_worker.py).

What is asserted is bit equality: a run of six steps against three steps, a save through torch.save, a NEW net and a NEW TrainStep,
and three more steps.  The control continues from the weights alone -- the launcher's --use_pre_pth path -- and must NOT reproduce
the run: without it these tests could not see what they are for."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import train as T
from lft_amd import trainer
from lft_amd.params import deterministic_state, synthetic_lr
from model import LFT

import gpu_util as G

pytestmark = pytest.mark.gpu

A, S, B, H, W = 2, 2, 2, 6, 6
COUNTERS = ("steps_applied", "steps_skipped", "steps_clipped")
CASES = {
    "fp32-guard-clip-graph-nan": dict(kw=dict(math="fp32", max_grad_norm=0.05, graph=True), poison=1),
    "bf16x6-plain-graph": dict(kw=dict(math="bf16x6", graph=True), poison=None),
    "bf16x3-guard-eager": dict(kw=dict(math="bf16x3", guard=True, graph=False), poison=None),
}
EMA = dict(ema_decay=0.9, ema_warmup=True)


def new_net():
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=S))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, S, seed=1, flavor="stress").items()})
    return net.to(G.DEV).train()


def steps_of(poison):
    """Six steps over three distinct batches; `poison`: the index (in the first half) of a step whose batch holds one NaN pixel."""
    three = []
    for k in range(3):
        lr = torch.from_numpy(synthetic_lr(B, A, H, W, seed=k)).to(G.DEV)
        hr = torch.from_numpy(np.random.Generator(np.random.PCG64(70 + k)).random((B, 1, A * H * S, A * W * S), dtype=np.float32)).to(G.DEV)
        three.append((lr, hr))
    out = [three[i % 3] for i in range(6)]
    if poison is not None:
        bad = out[poison][0].clone()
        bad[0, 0, 3, 4] = float("nan")
        out[poison] = (bad, out[poison][1])
    return out


def snapshot(ts):
    snap = {k: getattr(ts, k).clone() for k in ("flat_params", "m", "v", "ema")}
    snap["t"] = ts.t
    if ts.guard:
        rep = ts.guard_report()
        snap.update({k: rep[k] for k in COUNTERS})
    return snap


def assert_same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{what}: {k} differs from the uninterrupted run"
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """runs(case), computed once per case: the uninterrupted six-step run, and the files (model checkpoint, state) after its first
    three steps -- written by a SEPARATE TrainStep that stopped there."""
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = build_runs(case, str(tmp_path_factory.mktemp("resume")))
        return cache[case]
    return get


def build_runs(case, d):
    c = CASES[case]
    steps = steps_of(c["poison"])
    full = T.TrainStep(new_net(), lr=2e-4, **c["kw"], **EMA)
    for lr, hr in steps:
        full.step(lr, hr)
    half = T.TrainStep(new_net(), lr=2e-4, **c["kw"], **EMA)
    for lr, hr in steps[:3]:
        half.step(lr, hr)
    trainer.save_checkpoint(half.net, os.path.join(d, "model.pth"), 0)
    torch.save(half.state_dict(), os.path.join(d, "state.pth"))
    return steps, snapshot(full), d, snapshot(half)


@pytest.mark.parametrize("case", list(CASES))
def test_resumed_run_equals_the_uninterrupted_one(case, runs):
    steps, full, d, half = runs(case)
    c = CASES[case]
    if c["poison"] is not None:                                               # the case exists for steps_applied != t
        assert half["t"] == 3 and half["steps_applied"] == 2 and half["steps_skipped"] == 1
        assert full["steps_clipped"] > 0, "max_grad_norm of this case does not clip: choose a smaller one"
    assert not torch.equal(full["ema"], full["flat_params"]) and not torch.equal(full["flat_params"], half["flat_params"])
    net = new_net()
    ts = T.TrainStep(net, lr=2e-4, **c["kw"], **EMA)
    trainer.load_checkpoint(net, os.path.join(d, "model.pth"))
    ts.load_state_dict(torch.load(os.path.join(d, "state.pth"), map_location="cpu"))
    assert_same(snapshot(ts), half, f"{case}, right after loading")
    for lr, hr in steps[3:]:
        ts.step(lr, hr)
    assert_same(snapshot(ts), full, case)


@pytest.mark.parametrize("case", list(CASES))
def test_control_weights_alone_do_not_reproduce_the_run(case, runs):
    steps, full, d, _ = runs(case)
    net = new_net()
    ts = T.TrainStep(net, lr=2e-4, **CASES[case]["kw"], **EMA)
    trainer.load_checkpoint(net, os.path.join(d, "model.pth"))                # today's --use_pre_pth: m = v = 0, t = 0
    for lr, hr in steps[3:]:
        ts.step(lr, hr)
    assert not torch.equal(ts.flat_params, full["flat_params"]), "continuing from the weights alone reproduced the run: the test sees nothing"
    assert not torch.equal(ts.m, full["m"]) and not torch.equal(ts.ema, full["ema"])


def test_loading_into_a_step_that_already_captured_its_graph(runs):
    case = "fp32-guard-clip-graph-nan"
    steps, full, d, half = runs(case)
    net = new_net()
    ts = T.TrainStep(net, lr=2e-4, **CASES[case]["kw"], **EMA)
    ts.step(*steps[0])                                                        # captures the graph, moves everything
    ts.step(*steps[1])                                                        # and a skipped step: counters to overwrite
    ptrs = [t.data_ptr() for t in (ts.flat_params, ts.m, ts.v, ts.ema, ts._guard)]
    graphs = dict(ts._graphs)
    trainer.load_checkpoint(net, os.path.join(d, "model.pth"))
    ts.load_state_dict(torch.load(os.path.join(d, "state.pth"), map_location="cpu"))
    assert [t.data_ptr() for t in (ts.flat_params, ts.m, ts.v, ts.ema, ts._guard)] == ptrs
    assert list(ts._graphs) == list(graphs) and all(ts._graphs[k] is graphs[k] for k in graphs)
    assert_same(snapshot(ts), half, "captured step, right after loading")
    for lr, hr in steps[3:]:
        ts.step(lr, hr)
    assert len(ts._graphs) == 1
    assert_same(snapshot(ts), full, "captured step")


def test_ema_weights_exchange_in_place_and_back(runs):
    steps, _, _, _ = runs("bf16x6-plain-graph")
    net = new_net()
    ts = T.TrainStep(net, lr=2e-4, math="bf16x6", **EMA)
    for lr, hr in steps[:3]:
        ts.step(lr, hr)
    lr = steps[0][0]
    p0, e0 = ts.flat_params.clone(), ts.ema.clone()
    ptrs = (ts.flat_params.data_ptr(), ts.ema.data_ptr(), [p.data_ptr() for p in ts.params])
    sd = ts.ema_state_dict()
    assert list(sd) == T.names(64, S) and all(not v.is_cuda for v in sd.values())
    assert [tuple(v.shape) for v in sd.values()] == [tuple(p.shape) for p in ts.params]
    assert torch.equal(torch.cat([v.reshape(-1) for v in sd.values()]), e0.cpu())
    other = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=S))
    other.load_state_dict(sd)                                                 # reference checkpoint form: loads as it is
    other = other.to(G.DEV).eval()
    with torch.no_grad():
        live = net(lr).clone()
        want = other(lr).clone()
        with ts.ema_weights() as averaged:
            assert averaged is net and net._packed is None
            assert torch.equal(ts.flat_params, e0) and torch.equal(ts.ema, p0)
            got = net(lr).clone()
        assert net._packed is None
        after = net(lr).clone()
    assert torch.equal(got, want), "inside ema_weights() the network did not run with the averaged weights"
    assert not torch.equal(got, live) and torch.equal(after, live)
    assert torch.equal(ts.flat_params.view(torch.int32), p0.view(torch.int32)) and torch.equal(ts.ema.view(torch.int32), e0.view(torch.int32))
    assert ptrs == (ts.flat_params.data_ptr(), ts.ema.data_ptr(), [p.data_ptr() for p in ts.params])
    with pytest.raises(RuntimeError):                                         # the exchange is undone when the block raises
        with ts.ema_weights():
            raise RuntimeError("validation failed")
    assert torch.equal(ts.flat_params, p0) and torch.equal(ts.ema, e0)
    plain = T.TrainStep(new_net(), lr=2e-4)                                   # no decay: nothing allocated, nothing to exchange
    assert plain.ema is None
    with pytest.raises(T._lib.LftError):
        plain.ema_state_dict()


def test_without_a_decay_step_launches_no_ema_kernel(monkeypatch, runs):
    steps, _, _, _ = runs("bf16x6-plain-graph")
    L = T._lib.lib()
    calls = []
    real = L.lft_ema_update
    monkeypatch.setattr(L, "lft_ema_update", lambda *a: calls.append(a) or real(*a))
    ts = T.TrainStep(new_net(), lr=2e-4)
    ts.step(*steps[0])
    assert calls == [] and ts.ema is None
    with_ema = T.TrainStep(new_net(), lr=2e-4, **EMA)
    with_ema.step(*steps[0])
    assert len(calls) == 1
    assert torch.equal(ts.flat_params, with_ema.flat_params), "keeping an average changed the weights"


def fit_kwargs(ckpt_dir, scores, seen):
    def validate(net):
        seen.append(net.state_dict()["conv_init0.0.weight"].detach().cpu().clone())
        return scores[len(seen) - 1]
    return dict(batch_size=2, lr=2e-4, n_steps=1, gamma=0.5, ckpt_dir=ckpt_dir, seed=3, use_augmentation=True, log=lambda *_: None,
                max_grad_norm=0.05, ema_decay=0.9, save_state=True, validate=validate, val_weights="ema")


def test_fit_resumed_at_an_epoch_boundary_equals_two_epochs_straight(tmp_path):
    src = trainer.SyntheticPatchSource(4, A, S, patch=6, seed=0)
    name = lambda d, f: os.path.join(str(tmp_path / d), f)
    # two epochs straight; the second epoch validates worse, so the best file is the first epoch's
    seen_a = []
    net_a = new_net()
    hist_a = trainer.fit(net_a, src, 2, **fit_kwargs(str(tmp_path / "a"), [1.0, 0.5], seen_a))
    best_a, guard_a = dict(trainer.fit.best), list(trainer.fit.last_guard)
    assert len(hist_a) == 2 and len(seen_a) == 2 and best_a == {"score": 1.0, "epoch": 1}
    assert trainer.step_lr(2e-4, 1, 1, 0.5) == 1e-4                           # the learning rate changes at the boundary
    # one epoch, then a resume of one more in a process that knows nothing but the files
    seen_b = []
    kw = fit_kwargs(str(tmp_path / "b"), [1.0, 0.5], seen_b)
    hist_1 = trainer.fit(new_net(), src, 1, **kw)
    assert hist_1 == hist_a[:1]
    state_file = name("b", trainer.training_state_name("LFT", A, S))
    assert sorted(os.listdir(str(tmp_path / "b"))) == sorted([
        "LFT_2x2_2x_epoch_01_model.pth", "LFT_2x2_2x_epoch_01_ema_model.pth", "LFT_2x2_2x_best_model.pth", "LFT_2x2_2x_training_state.pth"])
    best_stamp = os.stat(name("b", "LFT_2x2_2x_best_model.pth")).st_mtime_ns
    net_b = new_net()
    with torch.no_grad():
        for p in net_b.parameters():                                          # whatever the process starts from is replaced
            p.mul_(0.5)
    hist_b = trainer.fit(net_b, src, 2, resume=state_file, **kw)
    assert hist_b == hist_a, (hist_b, hist_a)
    assert len(seen_b) == 2, "validate is called once per epoch"
    assert trainer.fit.best == best_a
    assert [{k: g[k] for k in COUNTERS} for g in trainer.fit.last_guard] == [{k: g[k] for k in COUNTERS} for g in guard_a]
    for (k, x), (_, y) in zip(net_a.state_dict().items(), net_b.state_dict().items()):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{k}: the resumed fit differs from two epochs straight"
    for f in ("LFT_2x2_2x_epoch_02_model.pth", "LFT_2x2_2x_epoch_02_ema_model.pth", "LFT_2x2_2x_best_model.pth"):
        x, y = torch.load(name("a", f), map_location="cpu"), torch.load(name("b", f), map_location="cpu")
        assert x["epoch"] == y["epoch"] and list(x["state_dict"]) == T.names(64, S)
        assert all(torch.equal(u, v) for u, v in zip(x["state_dict"].values(), y["state_dict"].values())), f
    # the best file: written on improvement only, and it holds the weights that were validated -- the averaged ones
    assert os.stat(name("b", "LFT_2x2_2x_best_model.pth")).st_mtime_ns == best_stamp
    best = torch.load(name("a", "LFT_2x2_2x_best_model.pth"), map_location="cpu")
    ema1 = torch.load(name("a", "LFT_2x2_2x_epoch_01_ema_model.pth"), map_location="cpu")
    live1 = torch.load(name("a", "LFT_2x2_2x_epoch_01_model.pth"), map_location="cpu")
    assert best["epoch"] == 1 and torch.equal(best["state_dict"]["conv_init0.0.weight"], ema1["state_dict"]["conv_init0.0.weight"])
    assert torch.equal(seen_a[0], ema1["state_dict"]["conv_init0.0.weight"]) and not torch.equal(seen_a[0], live1["state_dict"]["conv_init0.0.weight"])
    state = torch.load(state_file, map_location="cpu")
    assert state["epoch"] == 2 and state["history"] == hist_a and state["best"] == best_a and state["seed"] == 3
    assert state["global_batch"] == 2 and state["world"] == 1 and state["train_step"]["t"] == 4
    # another global batch: training continues and says so
    said = []
    kw2 = dict(kw, log=said.append, batch_size=4, validate=None)
    trainer.fit(new_net(), src, 3, resume=state_file, **kw2)
    assert any("global_batch 4 (saved with 2)" in s for s in said), said


def test_two_ranks_resume_with_only_rank_0_reading(tmp_path):
    worker = os.path.join(os.path.dirname(__file__), "dp_resume_worker.py")
    d = str(tmp_path)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    for mode, port in (("first", "29641"), ("resume", "29642")):
        subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", port, worker, mode, d], check=True, env=env, timeout=300)
    full = [torch.load(os.path.join(d, f"full.rank{r}")) for r in (0, 1)]
    got = [torch.load(os.path.join(d, f"resumed.rank{r}")) for r in (0, 1)]
    c = full[0]["counters"]
    assert c["steps_applied"] == 3 and c["steps_skipped"] == 1 and c["steps_clipped"] > 0 and full[0]["t"] == 4
    for r in (0, 1):
        assert got[r]["t"] == 4 and got[r]["counters"] == full[0]["counters"], (r, got[r]["counters"])
        for k in ("p", "m", "v", "ema"):
            assert torch.equal(got[r][k].view(torch.int32), full[r][k].view(torch.int32)), f"rank {r}: {k} differs from the uninterrupted two-rank run"
            assert torch.equal(got[r][k], got[0][k])
