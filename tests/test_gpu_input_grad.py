"""GPU tests of the gradient with respect to the LR input (include/lft_hip.h: lft_train_backward_input, lft_lr_grad_bwd;
kernel k_lr_grad in lft_amd/csrc/lft_train.cuh).  lr feeds the network in two places (reference LFT.py:54, :65), so
d lr = bicubic^T(dout) + conv_init0^T(d x0):
  * the stage kernel against CPU autograd through O.bicubic_skip + O.conv_views (no kinks: bar 1e-5),
  * the whole backward against oracle autograd told to take our forward's ReLU / LeakyReLU branches (bar 1e-3, as the
    parameter gradients in tests/test_gpu_train.py),
  * against the real reference's d lr (tests/golden/input_grad_*.npz),
  * the parameter gradients unchanged, bit for bit, and d lr deterministic,
  * the module surface: lr.grad in training and eval mode, a trainable front-end, and no graph when none is asked for."""
import glob
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import _lib, train as T
from lft_amd.params import deterministic_state, param_table, synthetic_lr
from oracle import lft_oracle as O
from fixture_util import sub_indices

import gpu_util as G

pytestmark = pytest.mark.gpu
TOL = 1e-3
STAGE_TOL = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(3, 2, 2, 6, 6), (2, 4, 1, 8, 5), (5, 2, 1, 8, 8), (2, 2, 1, 5, 9),      # the shapes of tests/test_gpu_train.py
         (9, 2, 1, 4, 4), (3, 2, 1, 7, 5), (5, 2, 1, 16, 16)]
MATHS = ["fp32", "bf16x3", "bf16x6"]


# ---------------------------------------------------------------------------------------------------- helpers
def our_branches(tape, A, s, B, h, w):
    """ReLU / LeakyReLU decisions of OUR forward, from the tape, in the layouts of the oracle's pre-activations
    (the same map as tests/test_gpu_train.py builds)."""
    V, ss = A * A, s * s
    tv = lambda name, C: T.tape_view(tape, name, B, A, h, w, s, (B, V, h, w, C)).cpu() > 0   # noqa: E731
    m = {}
    for i, name in zip((0, 2, 4), ("c1", "c2", "c3")):
        m[f"conv{i}"] = tv(name, 64).permute(0, 4, 1, 2, 3)                                        # [B,64,V,h,w]
    for l in range(4):
        m[f"ang{l}"] = tv(f"ang{l}.hdn", 128).permute(1, 0, 2, 3, 4).reshape(V, B * h * w, 128)     # 'a (b h w) c'
        m[f"spa{l}"] = tv(f"spa{l}.hdn", 256).permute(2, 3, 0, 1, 4).reshape(h * w, B * V, 256)     # '(h w) (b a) c'
    m["up"] = O.views_to_mosaic(tv("act", 64 * ss).permute(0, 4, 1, 2, 3), A)                       # [B,64ss,A*h,A*w]
    return m


def seeded_dout(A, s, B, h, w, dseed=3):
    rng = np.random.Generator(np.random.PCG64([dseed, B, A, h, w, s]))
    return torch.from_numpy(rng.standard_normal((B, 1, A * h * s, A * w * s), dtype=np.float32))


def device_params(sd_np, s):
    return [torch.from_numpy(sd_np[n]).to(G.DEV).contiguous() for n, _, _ in param_table(64, s)]


def oracle_grads(sd, lr, dout, A, s, masks=None, params=False):
    """d <out, dout> / d lr (and, with params=True, / d every parameter) by autograd over the CPU oracle; masks: O.branch_masks."""
    x = lr.detach().cpu().clone().requires_grad_()
    sdg = {k: v.detach().clone().requires_grad_(params) for k, v in sd.items()}
    O.branch_masks = masks
    try:
        with torch.enable_grad():
            out = O._forward(sdg, x, A, s, None)
            wrt = [x] + ([sdg[n] for n, _, _ in param_table(64, s)] if params else [])
            gs = torch.autograd.grad(out, wrt, dout.cpu())
    finally:
        O.branch_masks = None
    return gs[0], {n: g for (n, _, _), g in zip(param_table(64, s), gs[1:])}


def check(got, ref, tol, what):
    got = got.detach().cpu()
    assert not torch.isnan(got).any(), what
    err = float((got - ref).abs().max())
    scale = float(ref.abs().max())
    assert err <= tol * scale, f"{what}: " + G.err_report(got, ref)
    return err / scale


def run_input_backward(A, s, B, h, w, math, dseed=3, iseed=0):
    sd_np = deterministic_state(64, s, seed=1, flavor="stress")
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=iseed)).to(G.DEV)
    ps = device_params(sd_np, s)
    out, tape = T.train_forward(ps, lr, A, s, math=math)
    dout = seeded_dout(A, s, B, h, w, dseed).to(G.DEV)
    d_lr = torch.empty_like(lr)
    flat = T.train_backward(ps, lr, tape, dout, A, s, math=math, d_lr=d_lr)
    torch.cuda.synchronize()
    return dict(sd_np=sd_np, lr=lr, ps=ps, tape=tape, dout=dout, d_lr=d_lr, flat=flat, math=math)


# ---------------------------------------------------------------------------------------------------- 1. stage kernel
STAGE_VIEWS = [(4, 4), (5, 9), (8, 5), (6, 12), (16, 16), (20, 33)]      # (20, 33): several 16 x 16 tiles per view, ragged ones
STAGE_EDGE_A = [1, 8, 11]             # one view, 64 and 121 views (the C ABI takes A*A <= 128): on the two smallest views only, to bound the count


@pytest.mark.parametrize("with_dout", [True, False], ids=["both_terms", "conv_only"])
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("hw,A", [(hw, A) for hw in STAGE_VIEWS for A in [2, 3, 5, 9]] + [(hw, A) for hw in STAGE_VIEWS[:2] for A in STAGE_EDGE_A],
                         ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_stage_kernel_matches_autograd(hw, A, s, with_dout):
    h, w = hw
    B = 2 if A <= 3 else 1
    gen = torch.Generator().manual_seed(A * 1000 + s * 100 + h * 10 + w)
    dx0 = torch.randn(B * A * A * h * w, 64, generator=gen)
    w0 = torch.randn(64, 1, 1, 3, 3, generator=gen) * 0.3
    dout = torch.randn(B, 1, A * h * s, A * w * s, generator=gen)
    lr = torch.zeros(B, 1, A * h, A * w, dtype=torch.float64, requires_grad=True)
    with torch.enable_grad():
        x0 = O.conv_views(O.mosaic_to_views(lr, A), w0.double())                             # [B,64,V,h,w]
        tot = (x0 * dx0.double().view(B, A * A, h, w, 64).permute(0, 4, 1, 2, 3)).sum()
        if with_dout:
            tot = tot + (O.bicubic_skip(lr, A, s) * dout.double()).sum()
        (ref,) = torch.autograd.grad(tot, lr)
    got = T.lr_grad_bwd(w0.to(G.DEV), dx0.to(G.DEV), dout.to(G.DEV) if with_dout else None, A, s, B, h, w)
    torch.cuda.synchronize()
    check(got.double(), ref, STAGE_TOL, f"A{A} s{s} {h}x{w}")


def test_stage_kernel_bicubic_term_alone():
    """dx0 = 0: the bicubic adjoint on its own, on views where every row and column is a border one (4 x 4) and a larger one."""
    for (A, s, h, w) in [(2, 4, 4, 4), (3, 2, 5, 9), (2, 2, 19, 17)]:
        dout = torch.randn(1, 1, A * h * s, A * w * s, generator=torch.Generator().manual_seed(h * w + s))
        lr = torch.zeros(1, 1, A * h, A * w, dtype=torch.float64, requires_grad=True)
        with torch.enable_grad():
            (ref,) = torch.autograd.grad((O.bicubic_skip(lr, A, s) * dout.double()).sum(), lr)
        got = T.lr_grad_bwd(torch.zeros(576, device=G.DEV), torch.zeros(A * A * h * w, 64, device=G.DEV), dout.to(G.DEV), A, s, 1, h, w)
        torch.cuda.synchronize()
        check(got.double(), ref, STAGE_TOL, f"bicubic^T A{A} s{s} {h}x{w}")


def test_stage_entry_rejects_bad_arguments():
    L = _lib.lib()
    buf = torch.zeros(4 * 4 * 4 * 64, device=G.DEV)
    w0 = torch.zeros(576, device=G.DEV)
    assert L.lft_lr_grad_bwd(w0.data_ptr(), buf.data_ptr(), None, None, 1, 2, 4, 4, 2, G.stream()) == -1     # LFT_ERR_ARG
    assert b"null" in L.lft_last_error()
    assert L.lft_lr_grad_bwd(w0.data_ptr(), buf.data_ptr(), None, buf.data_ptr(), 1, 2, 4, 4, 3, G.stream()) == -2   # LFT_ERR_SHAPE
    assert b"scale" in L.lft_last_error()


# ---------------------------------------------------------------------------------------------------- 2. whole network
_ID = lambda cm: "A%d_s%d_B%d_%dx%d" % cm[0] + "_" + cm[1]      # noqa: E731


@pytest.mark.parametrize("cm", [(c, m) for c in CASES for m in MATHS], ids=_ID)
def test_input_gradient_exact_given_our_branches(cm):
    (A, s, B, h, w), math = cm
    r = run_input_backward(A, s, B, h, w, math)
    masks = our_branches(r["tape"], A, s, B, h, w)
    ref, _ = oracle_grads(O.state_from_numpy(r["sd_np"]), r["lr"], r["dout"], A, s, masks)
    rel = check(r["d_lr"], ref, TOL, f"d lr [{math}]")
    print(f"d lr A{A} s{s} B{B} {h}x{w} [{math}]: rel max err {rel:.2e}")


# ---------------------------------------------------------------------------------------------------- 3. real reference
FILES = sorted(glob.glob(os.path.join(GOLDEN, "input_grad_*.npz")))


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_input_gradient_matches_reference_fixture(path):
    g = np.load(path)
    A, s, B, h, w, wseed, iseed, dseed = (int(v) for v in g["meta"])
    assert wseed == 1 and str(g["flavor"]) == "stress"
    r = run_input_backward(A, s, B, h, w, "fp32", dseed=dseed, iseed=iseed)
    a = r["d_lr"].cpu().numpy().ravel()
    if "d_lr_full" in g.files:
        ref = g["d_lr_full"].ravel()
        got = a
    else:
        ref = g["d_lr_sub"]
        got = a[sub_indices(a.size)]
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"{os.path.basename(path)}: rel max err {err:.2e} (min |pre-activation| of the reference {float(g['min_abs_pre']):.1e})")
    assert err <= TOL
    s_abs = float(np.abs(a.astype(np.float64)).sum())
    assert abs(s_abs - g["d_lr_stats"][2]) <= TOL * g["d_lr_stats"][2]


# ---------------------------------------------------------------------------------------------------- 4. / 5. bits
@pytest.mark.parametrize("math", MATHS)
def test_parameter_gradients_unchanged_and_input_gradient_deterministic(math):
    A, s, B, h, w = 5, 2, 1, 8, 8
    r = run_input_backward(A, s, B, h, w, math)
    plain = T.train_backward(r["ps"], r["lr"], r["tape"], r["dout"], A, s, math=math)
    d2 = torch.empty_like(r["lr"])
    again = T.train_backward(r["ps"], r["lr"], r["tape"], r["dout"], A, s, math=math, d_lr=d2)
    torch.cuda.synchronize()
    assert torch.equal(plain, r["flat"])             # the 78 gradients: what lft_train_backward gives, bit for bit
    assert torch.equal(again, r["flat"])
    assert torch.equal(d2, r["d_lr"])                # d lr: two calls, same bits
    assert float(r["d_lr"].abs().max()) > 0


def test_backward_input_rejects_null_d_lr():
    A, s, B, h, w = 2, 2, 1, 4, 4
    r = run_input_backward(A, s, B, h, w, "fp32")
    rc = _lib.lib().lft_train_backward_input(T._ptr_array(r["ps"]), len(r["ps"]), r["lr"].data_ptr(), r["tape"].data_ptr(),
                                             r["dout"].data_ptr(), r["flat"].data_ptr(), None, B, A, h, w, s, _lib.MATH_F32, G.stream())
    assert rc == -1 and b"null" in _lib.lib().lft_last_error()


# ---------------------------------------------------------------------------------------------------- 6. module surface
def make_net(A, s, train):
    from model import LFT
    sd_np = deterministic_state(64, s, seed=1, flavor="stress")
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
    net = net.to(G.DEV)
    return (net.train() if train else net.eval()), sd_np


def branches_for(net, x, A, s):
    """Our forward's branch decisions on input x: the module's forward is lft_train_forward at net.train_math (deterministic)."""
    B, _, H, W = x.shape
    _, tape = T.train_forward(net._params_in_order(), x.detach().contiguous(), A, s, math=net.train_math)
    torch.cuda.synchronize()
    return our_branches(tape, A, s, B, H // A, W // A)


MOD_CASE = (3, 2, 2, 6, 6)


def test_module_train_mode_fills_input_and_parameter_grads():
    A, s, B, h, w = MOD_CASE
    net, sd_np = make_net(A, s, train=True)
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0)).to(G.DEV).requires_grad_()
    dout = seeded_dout(A, s, B, h, w).to(G.DEV)
    out = net(lr)
    loss = (out * dout).sum()
    loss.backward()
    ref_lr, ref_p = oracle_grads(O.state_from_numpy(sd_np), lr, dout, A, s, branches_for(net, lr, A, s), params=True)
    check(lr.grad, ref_lr, TOL, "lr.grad")
    named = dict(net.named_parameters())
    assert len(ref_p) == 78
    for n, ref in ref_p.items():
        check(named[n].grad, ref, TOL, n)


def test_module_eval_frozen_gives_input_grad_only():
    A, s, B, h, w = MOD_CASE
    net, sd_np = make_net(A, s, train=False)
    for p in net.parameters():
        p.requires_grad_(False)
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0)).to(G.DEV).requires_grad_()
    dout = seeded_dout(A, s, B, h, w).to(G.DEV)
    out = net(lr)
    assert out.grad_fn is not None
    out.backward(dout)
    ref_lr, _ = oracle_grads(O.state_from_numpy(sd_np), lr, dout, A, s, branches_for(net, lr, A, s))
    check(lr.grad, ref_lr, TOL, "lr.grad (eval, frozen)")
    assert all(p.grad is None for p in net.parameters())


def test_module_chains_to_a_trainable_front_end():
    A, s, B, h, w = MOD_CASE
    net, sd_np = make_net(A, s, train=False)
    for p in net.parameters():
        p.requires_grad_(False)
    scale = torch.nn.Parameter(torch.tensor(1.25, device=G.DEV))
    offset = torch.nn.Parameter(torch.tensor(-0.1, device=G.DEV))
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0)).to(G.DEV)
    dout = seeded_dout(A, s, B, h, w).to(G.DEV)
    x = lr * scale + offset
    net(x).backward(dout)
    ref_x, _ = oracle_grads(O.state_from_numpy(sd_np), x, dout, A, s, branches_for(net, x, A, s))
    ref_scale, ref_offset = float((ref_x * lr.cpu()).sum()), float(ref_x.sum())
    ref_norm = float(ref_x.abs().sum())                      # both gradients are sums over all pixels: bar relative to sum |d x|
    assert abs(float(scale.grad) - ref_scale) <= TOL * ref_norm, (float(scale.grad), ref_scale)
    assert abs(float(offset.grad) - ref_offset) <= TOL * ref_norm, (float(offset.grad), ref_offset)


def test_module_builds_no_graph_when_not_asked():
    A, s, B, h, w = MOD_CASE
    net, _ = make_net(A, s, train=False)
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0)).to(G.DEV)
    assert net(lr).grad_fn is None                                          # eval, input without grad
    with torch.no_grad():
        assert net(lr.clone().requires_grad_()).grad_fn is None             # no_grad wins over lr.requires_grad
    net.train()
    with torch.no_grad():
        assert net(lr).grad_fn is None
