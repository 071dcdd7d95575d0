"""The structural loss term in the plumbing, on the GPU: TrainStep(loss={..., "ssim_weight": w}) captured against eager and against a
hand-run train_forward -> lft_lf_loss -> lft_ssim_loss -> train_backward, the three-entry terms of a spec without the term, the
refusal of views below the 11x11 window, the pure structural objective raising S, and trainer.fit (epoch line, resume).
Shape: A2 / 2x / B2 / 6x6 LR views, 12x12 HR views."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import train as T
from lft_amd import trainer
from lft_amd.loss import lf_loss, ssim_loss
from lft_amd.params import deterministic_state, synthetic_lr
from model import LFT

import gpu_util as G
import ssim_loss_util as U

pytestmark = pytest.mark.gpu

A, S, B, LRV = 2, 2, 2, 6
SPEC = {"penalty": "l1", "ssim_weight": 0.2}


def new_net(flavor="stress"):
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=S))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, S, seed=1, flavor=flavor).items()})
    return net.to(G.DEV).train()


def batch(lrv=LRV):
    lr = torch.from_numpy(synthetic_lr(B, A, lrv, lrv, seed=0)).to(G.DEV)
    hr = torch.from_numpy(np.random.Generator(np.random.PCG64(7)).random((B, 1, A * lrv * S, A * lrv * S), dtype=np.float32)).to(G.DEV)
    return lr, hr


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def test_trainstep_graph_equals_eager_and_the_two_separate_calls():
    lr, hr = batch()
    net = new_net()
    ps = net._params_in_order()
    math = getattr(net, "train_math", "fp32")
    out, tape = T.train_forward(ps, lr, A, S, math=math)
    dout = torch.empty_like(hr)
    terms = torch.zeros(4, dtype=torch.float32, device=G.DEV)
    lf_loss(out, hr, A, "l1", 1e-3, 1.0, 0.0, dsr=dout, loss3=terms)
    ssim_loss(out, hr, A, 2.0, 0.2, dsr=dout, accumulate=True, total=terms[0:1], ssim_out=terms[3:4])
    grads = T.train_backward(ps, lr, tape, dout, A, S, math=math).clone()
    S_ref, _ = U.reference(out.cpu().numpy(), hr.cpu().numpy(), A)
    t = [float(x) for x in terms.cpu()]
    assert abs(t[3] - S_ref) <= 1e-6 * S_ref and abs(t[0] - (t[1] + 0.2 * (1.0 - S_ref))) <= 1e-6, (t, S_ref)
    got = {}
    for graph in (True, False):
        ts = T.TrainStep(new_net(), loss=dict(SPEC), graph=graph)
        assert ts.loss is not None and ts.loss.spec()["ssim_weight"] == 0.2 and ts.last_loss_terms.shape == (4,)
        loss = ts.step(lr, hr)
        assert loss.shape == (1,) and torch.equal(bits(loss), bits(ts.last_loss_terms[:1]))
        assert torch.equal(bits(ts.last_out), bits(out))
        assert torch.equal(bits(ts.last_loss_terms), bits(terms)), (graph, ts.last_loss_terms, terms)
        assert torch.equal(bits(ts.flat_grads), bits(grads)), f"graph={graph}: gradients differ from the two separate calls"
        ts.step(lr, hr)                                           # a second step of the same shape: replay / cached scratch
        assert len(ts._ssim_scratch) == 1 and len(ts._loss_scratch) == 1
        got[graph] = (ts.flat_grads.clone(), ts.last_loss_terms.clone(), ts.flat_params.clone())
    for a, b in zip(got[True], got[False]):
        assert torch.equal(bits(a), bits(b)), "captured and eager steps differ"


def test_a_spec_without_the_term_keeps_three_entries_and_its_bits():
    lr, hr = batch()
    steps = [T.TrainStep(new_net(), loss=spec) for spec in ({"penalty": "charbonnier", "epi_weight": 0.5},
                                                           {"penalty": "charbonnier", "epi_weight": 0.5, "ssim_weight": 0.0, "ssim_range": 1.0})]
    for ts in steps:
        ts.step(lr, hr)
        assert ts.last_loss_terms.shape == (3,) and not ts._ssim_scratch and "ssim_weight" not in ts.loss.spec()
    for name in ("flat_params", "flat_grads", "last_loss_terms"):
        assert torch.equal(bits(getattr(steps[0], name)), bits(getattr(steps[1], name))), name


def test_views_below_the_window_are_refused_before_anything_runs():
    lr, hr = batch(5)                                             # 5x5 LR views: 10x10 HR views
    for graph in (True, False):
        ts = T.TrainStep(new_net(), loss=dict(SPEC), graph=graph)
        before = ts.flat_params.clone()
        with pytest.raises(ValueError, match="10x10"):
            ts.step(lr, hr)
        assert ts.t == 0 and not ts._graphs and not ts._ssim_scratch and not ts._loss_scratch
        assert torch.equal(bits(ts.flat_params), bits(before)) and float(ts.flat_grads.abs().max()) == 0.0
    plain = T.TrainStep(new_net(), loss={"penalty": "charbonnier", "epi_weight": 0.5})
    plain.step(lr, hr)                                            # without the term the same views train as before


def test_lfloss_under_autograd_gives_the_c_calls_gradient():
    _, hr = batch()
    sr = torch.from_numpy(np.random.default_rng(11).random(tuple(hr.shape), dtype=np.float32)).to(G.DEV).requires_grad_(True)
    for w_pix in (1.0, 0.0):
        dsr = torch.empty_like(hr)
        terms = torch.zeros(4, dtype=torch.float32, device=G.DEV)
        if w_pix:
            lf_loss(sr.detach(), hr, A, "l1", 1e-3, w_pix, 0.0, dsr=dsr, loss3=terms)
        ssim_loss(sr.detach(), hr, A, 1.0, 0.3, dsr=dsr, accumulate=bool(w_pix), total=terms[0:1], ssim_out=terms[3:4])
        crit = LFT.get_loss(SimpleNamespace(angRes=A, lft_loss={"pixel_weight": w_pix, "ssim_weight": 0.3, "ssim_range": 1.0}))
        sr.grad = None
        total = crit(sr, hr)
        (3.0 * total).backward()
        assert torch.equal(bits(crit.terms), bits(terms)) and torch.equal(bits(total), bits(terms[0]))
        assert torch.equal(bits(sr.grad), bits(3.0 * dsr))


def test_the_pure_structural_objective_raises_s():
    lr, hr = batch()
    hr = torch.nn.functional.interpolate(lr, scale_factor=S, mode="nearest") * 0.9 + 0.05 * hr      # something a network can approach
    ts = T.TrainStep(new_net("default"), lr=2e-4, loss={"pixel_weight": 0.0, "epi_weight": 0.0, "ssim_weight": 1.0})
    assert not ts.loss.has_lf_terms()
    s_values = []
    for _ in range(30):
        ts.step(lr, hr)
        s_values.append(ts.last_loss_terms.clone())
    first, last = s_values[0].cpu(), s_values[-1].cpu()
    print(f"S over 30 steps of the pure structural objective: {float(first[3]):.5f} -> {float(last[3]):.5f}")
    assert float(first[1]) == 0.0 and float(first[2]) == 0.0
    assert abs(float(last[0]) - (1.0 - float(last[3]))) <= 1e-6
    assert float(last[3]) > float(first[3])


def test_fit_logs_ssim_and_resumes_bit_for_bit(tmp_path):
    src = trainer.SyntheticPatchSource(4, A, S, patch=LRV, seed=0)
    said = []
    runs = {}
    for name in ("whole", "split"):
        d = os.path.join(str(tmp_path), name)
        os.makedirs(d)
        kw = dict(batch_size=2, ckpt_dir=d, seed=3, use_augmentation=False, save_state=True, log=said.append, loss=dict(SPEC))
        net = new_net("default")
        if name == "whole":
            hist = trainer.fit(net, src, 2, **kw)
            lines = [s for s in said if "Train, loss is" in s]
            assert len(lines) == 2 and all(", pix " in s and ", epi " in s and ", ssim " in s for s in lines), said
            pix, ssim = (float(lines[-1].split(", %s " % k)[1].split(",")[0]) for k in ("pix", "ssim"))
            assert 0.0 < ssim < 1.0 and abs(hist[-1] - (pix + 0.2 * (1.0 - ssim))) <= 2e-5, (hist, lines)      # the line prints five decimals
        else:
            trainer.fit(net, src, 1, **kw)
            state_file = os.path.join(d, trainer.training_state_name("LFT", A, S))
            full = {"penalty": "l1", "eps": 1e-3, "pixel_weight": 1.0, "epi_weight": 0.0, "angRes": A, "ssim_weight": 0.2, "ssim_range": 2.0}
            assert torch.load(state_file, map_location="cpu")["loss"] == full
            said.clear()
            net = new_net("default")
            hist = trainer.fit(net, src, 2, resume=state_file, **kw)
            assert not any(s.startswith("WARNING") for s in said), said
        runs[name] = (hist, {k: v.detach().clone() for k, v in net.state_dict().items()})
    assert runs["whole"][0] == runs["split"][0]
    for k, v in runs["whole"][1].items():
        assert torch.equal(bits(v), bits(runs["split"][1][k])), k
