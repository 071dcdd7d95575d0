"""The focal-stack term in the plumbing, on the GPU: TrainStep(loss={..., "focal_weight": w}) captured against eager and against a
hand-run train_forward -> lft_lf_loss -> lft_focal_loss -> train_backward, the gradient against autograd through LFLoss on the same
forward output, the five-entry terms, the step without the term (bit for bit a TrainStep built without the new arguments), and
trainer.fit (epoch line, state-file spec, resume).  Shape: A2 / 2x / B2 / 6x6 LR views, 12x12 HR views; slopes (-1, 0, 1)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import train as T
from lft_amd import trainer
from lft_amd.loss import LFLoss, focal_loss, lf_loss, ssim_loss
from lft_amd.params import deterministic_state, synthetic_lr
from model import LFT

import focal_util as FU
import gpu_util as G

pytestmark = pytest.mark.gpu

A, S, B, LRV = 2, 2, 2, 6
SLOPES = [-1.0, 0.0, 1.0]
SPEC = {"penalty": "l1", "focal_weight": 0.25, "focal_slopes": SLOPES}
FULL = {"penalty": "l1", "eps": 1e-3, "pixel_weight": 1.0, "epi_weight": 0.0, "angRes": A, "focal_weight": 0.25, "focal_slopes": SLOPES,
        "focal_interp": "linear"}


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


def test_trainstep_graph_equals_eager_the_separate_calls_and_autograd():
    lr, hr = batch()
    net = new_net()
    ps = net._params_in_order()
    math = getattr(net, "train_math", "fp32")
    out, tape = T.train_forward(ps, lr, A, S, math=math)
    dout = torch.empty_like(hr)
    terms = torch.zeros(5, dtype=torch.float32, device=G.DEV)
    lf_loss(out, hr, A, "l1", 1e-3, 1.0, 0.0, dsr=dout, loss3=terms)
    focal_loss(out, hr, A, SLOPES, "linear", "full", "l1", 1e-3, 0.25, dsr=dout, accumulate=True, total=terms[0:1], focal_out=terms[4:5])
    grads = T.train_backward(ps, lr, tape, dout, A, S, math=math).clone()
    # the value against the restatement on the forward output
    from lft_amd import refocus as R
    _, F_ref, _, _ = FU.focal_np(out.cpu().numpy(), hr.cpu().numpy(), A, R.shift_table(A, SLOPES, "full", "linear"), 2)
    t = [float(x) for x in terms.cpu()]
    assert abs(t[4] - F_ref) <= 1e-6 * F_ref and t[3] == 0.0 and abs(t[0] - (t[1] + 0.25 * F_ref)) <= 1e-6, (t, F_ref)
    # autograd through LFLoss on the same forward output gives the same dout, hence the same gradients
    sr = out.detach().clone().requires_grad_(True)
    crit = LFT.get_loss(SimpleNamespace(angRes=A, lft_loss=dict(SPEC)))
    total = crit(sr, hr)
    total.backward()
    assert torch.equal(bits(crit.terms), bits(terms)) and torch.equal(bits(total), bits(terms[0])) and torch.equal(bits(sr.grad), bits(dout))
    grads_autograd = T.train_backward(ps, lr, tape, sr.grad.contiguous(), A, S, math=math).clone()
    assert torch.equal(bits(grads_autograd), bits(grads))
    got = {}
    for graph in (True, False):
        ts = T.TrainStep(new_net(), loss=dict(SPEC), graph=graph)
        assert ts.loss is not None and ts.loss.spec() == FULL and ts.last_loss_terms.shape == (5,)
        loss = ts.step(lr, hr)
        assert loss.shape == (1,) and torch.equal(bits(loss), bits(ts.last_loss_terms[:1]))
        assert torch.equal(bits(ts.last_out), bits(out))
        assert torch.equal(bits(ts.last_loss_terms), bits(terms)), (graph, ts.last_loss_terms, terms)
        assert torch.equal(bits(ts.flat_grads), bits(grads)), f"graph={graph}: gradients differ from the separate calls and from autograd"
        ts.step(lr, hr)                                           # a second step of the same shape: replay / cached scratch
        assert len(ts._focal_scratch) == 1 and len(ts._loss_scratch) == 1 and not ts._ssim_scratch
        got[graph] = (ts.flat_grads.clone(), ts.last_loss_terms.clone(), ts.flat_params.clone())
    for a, b in zip(got[True], got[False]):
        assert torch.equal(bits(a), bits(b)), "captured and eager steps differ"


def test_all_three_calls_in_one_step_and_the_pure_focal_objective():
    lr, hr = batch()
    net = new_net()
    ps = net._params_in_order()
    math = getattr(net, "train_math", "fp32")
    out, tape = T.train_forward(ps, lr, A, S, math=math)
    for w_pix in (1.0, 0.0):
        dout = torch.empty_like(hr)
        terms = torch.zeros(5, dtype=torch.float32, device=G.DEV)
        if w_pix:
            lf_loss(out, hr, A, "charbonnier", 1e-3, w_pix, 0.5, dsr=dout, loss3=terms)
            ssim_loss(out, hr, A, 2.0, 0.2, dsr=dout, accumulate=True, total=terms[0:1], ssim_out=terms[3:4])
        focal_loss(out, hr, A, SLOPES, "cubic", "full", "charbonnier", 1e-3, 0.25, dsr=dout, accumulate=bool(w_pix), total=terms[0:1], focal_out=terms[4:5])
        grads = T.train_backward(ps, lr, tape, dout, A, S, math=math).clone()
        spec = {"penalty": "charbonnier", "pixel_weight": w_pix, "epi_weight": 0.5 * w_pix, "focal_weight": 0.25, "focal_slopes": SLOPES, "focal_interp": "cubic"}
        if w_pix:
            spec.update(ssim_weight=0.2)
        ts = T.TrainStep(new_net(), loss=spec)
        loss = ts.step(lr, hr)
        assert ts.last_loss_terms.shape == (5,) and torch.equal(bits(loss), bits(ts.last_loss_terms[:1]))
        assert torch.equal(bits(ts.last_loss_terms), bits(terms)) and torch.equal(bits(ts.flat_grads), bits(grads)), w_pix
        t = [float(x) for x in terms.cpu()]
        if w_pix:
            assert 0.0 < t[3] < 1.0 and abs(t[0] - (t[1] + 0.5 * t[2] + 0.2 * (1.0 - t[3]) + 0.25 * t[4])) <= 1e-6, t
        else:
            assert not ts.loss.has_lf_terms() and t[1] == t[2] == t[3] == 0.0 and abs(t[0] - 0.25 * t[4]) <= 1e-7, t


def test_a_spec_without_the_term_keeps_its_entries_and_its_bits():
    lr, hr = batch()
    for base, n in (({"penalty": "charbonnier", "epi_weight": 0.5}, 3), ({"penalty": "l1", "ssim_weight": 0.2}, 4), (None, None)):
        off = None if base is None else dict(base, focal_weight=0.0, focal_slopes=[0.5, 2.0], focal_interp="cubic")
        steps = [T.TrainStep(new_net(), loss=spec) for spec in (base, off if base is not None else {"penalty": "l1", "focal_weight": 0.0})]
        for ts in steps:
            ts.step(lr, hr)
            assert not ts._focal_scratch
            if n is None:                                         # the default step keeps lft_l1_loss
                assert ts.loss is None and ts.last_loss_terms is None
            else:
                assert ts.last_loss_terms.shape == (n,) and "focal_weight" not in ts.loss.spec() and len(ts.loss.spec()) == (5 if n == 3 else 7)
        for name in ("flat_params", "flat_grads") + (() if n is None else ("last_loss_terms",)):
            assert torch.equal(bits(getattr(steps[0], name)), bits(getattr(steps[1], name))), (base, name)


def test_fit_logs_focal_and_resumes_bit_for_bit(tmp_path):
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
            assert len(lines) == 2 and all(", pix " in s and ", epi " in s and ", focal " in s and ", ssim " not in s for s in lines), said
            pix, focal = (float(lines[-1].split(", %s " % k)[1].split(",")[0]) for k in ("pix", "focal"))
            assert focal > 0.0 and abs(hist[-1] - (pix + 0.25 * focal)) <= 2e-5, (hist, lines)      # the line prints five decimals
        else:
            trainer.fit(net, src, 1, **kw)
            state_file = os.path.join(d, trainer.training_state_name("LFT", A, S))
            stored = torch.load(state_file, map_location="cpu")["loss"]
            assert stored == FULL and LFLoss.from_spec(stored).spec() == FULL
            said.clear()
            net = new_net("default")
            hist = trainer.fit(net, src, 2, resume=state_file, **kw)
            assert not any(s.startswith("WARNING") for s in said), said
        runs[name] = (hist, {k: v.detach().clone() for k, v in net.state_dict().items()})
    assert runs["whole"][0] == runs["split"][0]
    for k, v in runs["whole"][1].items():
        assert torch.equal(bits(v), bits(runs["split"][1][k])), k


def test_focal_error_and_evaluate_focal():
    from lft_amd import evaluate, refocus as R
    from lft_amd.loss import focal_error
    s, h0, w0 = S, 20, 18
    g = np.random.default_rng(3)
    net = new_net("default").eval()
    lr_scene = torch.from_numpy(g.random((A * h0, A * w0), dtype=np.float32))
    hr_scene = torch.from_numpy(g.random((A * h0 * s, A * w0 * s), dtype=np.float32))
    plain = evaluate.test_scene(net, lr_scene, hr_scene, patch=16, stride=8)
    on = evaluate.test_scene(net, lr_scene, hr_scene, patch=16, stride=8, focal=SLOPES)
    both = evaluate.test_scene(net, lr_scene, hr_scene, patch=16, stride=8, epi=True, focal=SLOPES)
    assert len(plain) == 3 and len(on) == 4 and len(both) == 5 and on[3] == both[4]
    for r in (on, both):
        assert r[0] == plain[0] and r[1] == plain[1] and torch.equal(bits(r[2]), bits(plain[2]))
    _, ref, _, _ = FU.focal_np(on[2].cpu().numpy()[None, None], hr_scene.numpy()[None, None], A, R.shift_table(A, SLOPES, "full", "linear"), 2)
    assert abs(on[3] - ref) <= 1e-6 * ref and on[3] == focal_error(on[2], hr_scene.to(G.DEV), A, SLOPES), (on[3], ref)
    p, q, f = evaluate.test(net, [(lr_scene, hr_scene)] * 2, patch=16, stride=8, focal=SLOPES)
    assert (p, q) == evaluate.test(net, [(lr_scene, hr_scene)] * 2, patch=16, stride=8) and abs(f - on[3]) <= 1e-7
    p, q, e, f2 = evaluate.test(net, [(lr_scene, hr_scene)] * 2, patch=16, stride=8, epi=True, focal=SLOPES)
    assert f2 == f and abs(e - both[3]) <= 1e-7
