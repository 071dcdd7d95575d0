"""CPU-side tests of the structural loss term (lft_ssim_loss, lft_amd.loss): the C ABI's declaration, the refusals that need no GPU,
the fp64 restatement of tests/ssim_loss_util.py against scikit-image's algorithm (oracle/metrics_oracle.py) and against the analytic
adjoint, LFLoss(ssim_weight=...) on CPU tensors against the restatement, the spec rules and the plumbing."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import _lib
from lft_amd.loss import LFLoss

import lf_loss_util as LU
import ssim_loss_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_sigs_and_ssim_loss_exports_agree():
    hdr = open(os.path.join(ROOT, "include", "lft_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert set(_lib.SSIM_LOSS_EXPORTS) == {"lft_ssim_loss_scratch_bytes", "lft_ssim_loss"}
    assert set(_lib.LOSS_EXPORTS) == {"lft_lf_loss_scratch_bytes", "lft_lf_loss"}
    for name in _lib.SSIM_LOSS_EXPORTS:
        m = re.search(r"int %s\(([^)]*)\);" % name, flat)
        assert m, name
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")), name
        for decl, ctype in zip(m.group(1).split(","), args):
            decl = decl.strip()
            want = (ctypes.POINTER(ctypes.c_size_t) if decl.startswith("size_t*") else ctypes.c_void_p if "*" in decl
                    else ctypes.c_float if decl.startswith("float ") else ctypes.c_int)
            assert ctype is want, (name, decl, ctype)
    assert "plain mean" in flat.lower() and "not differentiable" in flat      # the header says how S differs from cal_metrics' mean
    _lib.build()
    L = _lib.lib()
    assert all(hasattr(L, name) for name in _lib.SSIM_LOSS_EXPORTS)
    assert L.lft_version() == 5                                   # additive: no new ABI version


def test_size_query_and_refusals_need_no_gpu():
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.lft_ssim_loss_scratch_bytes(8, 5, 64, 64, ctypes.byref(n)) == 0 and n.value == 8 * 25 * 16 * 8      # one double per tile
    assert L.lft_ssim_loss_scratch_bytes(1, 2, 17, 33, ctypes.byref(n)) == 0 and n.value == 4 * 6 * 8
    assert L.lft_ssim_loss_scratch_bytes(8, 5, 64, 64, None) == -1
    assert L.lft_ssim_loss_scratch_bytes(0, 5, 64, 64, ctypes.byref(n)) == -2
    assert L.lft_ssim_loss_scratch_bytes(1, 1, 10, 11, ctypes.byref(n)) == -2
    assert L.lft_ssim_loss_scratch_bytes(1, 1, 11, 10, ctypes.byref(n)) == -2
    assert L.lft_ssim_loss(None, None, 1, 1, 11, 11, 2.0, 1.0, None, 1.0, 0, None, None, None, None) == -1
    fake = 4096                                                   # never dereferenced: the call is refused before any launch
    assert L.lft_ssim_loss(fake, fake, 1, 1, 10, 11, 2.0, 1.0, None, 1.0, 0, fake, fake, fake, None) == -2
    assert b"10x11" in L.lft_last_error()
    assert L.lft_ssim_loss(fake, fake, 1, 1, 11, 11, 2.0, 1.0, None, 1.0, 2, fake, fake, fake, None) == -1
    assert L.lft_ssim_loss(fake, fake, 1, 1, 11, 11, 0.0, 1.0, None, 1.0, 0, fake, fake, fake, None) == -1
    assert L.lft_ssim_loss(fake, fake, 1, 1, 11, 11, 2.0, float("inf"), None, 1.0, 0, fake, fake, fake, None) == -1
    assert L.lft_ssim_loss(fake, fake, 1, 1, 11, 11, 2.0, 1.0, None, float("nan"), 0, fake, fake, fake, None) == -1


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.SHAPE_IDS)
def test_restatement_equals_the_oracles_mean_over_views(shape):
    from oracle.metrics_oracle import ssim_view
    B, A, H, W = shape
    sr, hr = U.inputs(*shape)
    for R in (1.0, 2.0):
        S, _ = U.reference(sr, hr, A, R)
        want = float(np.mean([ssim_view(x, y, R) for x, y in zip(U.views_of(hr, A), U.views_of(sr, A))]))
        print(f"{shape} range {R}: S {S:.15f} oracle {want:.15f} diff {abs(S - want):.2e}")
        assert abs(S - want) <= 1e-12, (S, want)


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.SHAPE_IDS)
def test_autograd_and_analytic_adjoint_agree(shape):
    sr, hr, S, g = U.case(shape)
    S2, g2 = U.analytic(sr, hr, shape[1])
    err = float(np.abs(g - g2).max() / np.abs(g).max())
    print(f"{shape}: S {S:.12f} / {S2:.12f}, gradients differ by {err:.2e} of the largest element {np.abs(g).max():.3e}")
    assert abs(S - S2) <= 1e-12 and err <= 1e-10
    B, A, H, W = shape
    assert np.all(g.reshape(B, A, H, A, W)[B - 1, A - 1, :, A - 1, :] != 0)     # the constant-hr view still has a gradient


@pytest.mark.parametrize("combined", [False, True], ids=["alone", "with_charbonnier_epi"])
def test_lfloss_on_cpu_tensors_equals_the_restatement(combined):
    for shape in U.SHAPES:
        B, A, H, W = shape
        sr, hr, S, g = U.case(shape)
        w = 0.2
        if combined:
            loss = LFLoss("charbonnier", pixel_weight=1.0, epi_weight=0.5, angRes=A, ssim_weight=w)
            ref3, ref_g = LU.reference(np.array(sr), np.array(hr), A, "charbonnier", 1e-3, 1.0, 0.5)
        else:
            loss = LFLoss(pixel_weight=0.0, epi_weight=0.0, angRes=A, ssim_weight=w)
            ref3, ref_g = [0.0, 0.0, 0.0], np.zeros_like(g)
        want = ref3[0] + w * (1.0 - S)
        want_g = ref_g - w * g
        s = torch.tensor(sr, dtype=torch.float64, requires_grad=True)
        h = torch.tensor(hr, dtype=torch.float64, requires_grad=True)
        total = loss(s, h)
        total.backward()
        terms = [float(v) for v in loss.terms]
        assert len(terms) == 4 and float(total.detach()) == terms[0]
        assert abs(terms[0] - want) <= 1e-12 * max(1.0, abs(want)) and abs(terms[3] - S) <= 1e-12, (shape, terms, want, S)
        assert abs(terms[1] - ref3[1]) <= 1e-12 and abs(terms[2] - ref3[2]) <= 1e-12
        assert float(np.abs(s.grad.numpy() - want_g).max()) <= 1e-12 * float(np.abs(want_g).max()), shape


def test_spec_rules():
    five = {"penalty": "charbonnier", "eps": 0.01, "pixel_weight": 0.5, "epi_weight": 2.0, "angRes": 5}
    assert LFLoss("charbonnier", eps=0.01, pixel_weight=0.5, epi_weight=2.0, angRes=5, ssim_weight=0.0, ssim_range=1.0).spec() == five
    assert LFLoss().spec() == {"penalty": "l1", "eps": 1e-3, "pixel_weight": 1.0, "epi_weight": 0.0, "angRes": None}
    d = LFLoss("l1", angRes=2, ssim_weight=0.2).spec()
    assert d == {"penalty": "l1", "eps": 1e-3, "pixel_weight": 1.0, "epi_weight": 0.0, "angRes": 2, "ssim_weight": 0.2, "ssim_range": 2.0}
    assert LFLoss.from_spec(d).spec() == d
    d1 = dict(d, ssim_range=1.0, pixel_weight=0.0)
    assert LFLoss.from_spec(d1).spec() == d1                      # the pure structural objective is legal
    assert LFLoss().is_plain_l1() and not LFLoss(ssim_weight=0.1).is_plain_l1()
    assert not LFLoss.from_spec(d1).has_lf_terms() and LFLoss.from_spec(d).has_lf_terms()
    for bad in ({"ssim_weight": -0.1}, {"ssim_weight": float("nan")}, {"ssim_weight": float("inf")}, {"ssim_weight": 0.2, "ssim_range": 0.0},
                {"ssim_weight": 0.2, "ssim_range": -1.0}, {"ssim_weight": 0.2, "ssim_range": float("nan")},
                {"pixel_weight": 0.0, "epi_weight": 0.0, "ssim_weight": 0.0}, {"pixel_weight": 0.0, "epi_weight": 0.0},
                {"ssim_weight": 0.2, "ssim": 1.0}, {"ssim_scale": 1.0}):
        with pytest.raises(ValueError):
            LFLoss.from_spec(bad)
    with pytest.raises(ValueError, match="angRes"):
        LFLoss(ssim_weight=1.0)(torch.zeros(1, 1, 12, 12), torch.zeros(1, 1, 12, 12))
    with pytest.raises(ValueError, match="10x12"):
        LFLoss(ssim_weight=1.0, angRes=1)(torch.zeros(1, 1, 10, 12), torch.zeros(1, 1, 10, 12))


def test_plumbing_get_loss_and_unchanged_signatures():
    from lft_amd import train, trainer
    from model import LFT
    crit = LFT.get_loss(SimpleNamespace(angRes=3, lft_loss={"penalty": "charbonnier", "epi_weight": 0.5, "ssim_weight": 0.2, "ssim_range": 1.0}))
    assert isinstance(crit, LFLoss) and crit.spec() == {"penalty": "charbonnier", "eps": 1e-3, "pixel_weight": 1.0, "epi_weight": 0.5, "angRes": 3,
                                                        "ssim_weight": 0.2, "ssim_range": 1.0}
    sr, hr, S, _ = U.case(U.SHAPES[2], 1.0)
    total = crit(torch.tensor(sr), torch.tensor(hr))                 # fp32 CPU tensors: the tensors' own dtype
    assert total.dtype == torch.float32 and crit.terms.shape == (4,) and abs(float(crit.terms[3]) - S) <= 1e-5
    assert list(inspect.signature(train.TrainStep.__init__).parameters) == [
        "self", "net", "lr", "betas", "eps", "process_group", "math", "graph", "weight_decay", "max_grad_norm", "guard", "ema_decay", "ema_warmup",
        "loss"]
    assert inspect.signature(trainer.fit).parameters["loss"].default is None
    sig = inspect.signature(LFLoss.__init__).parameters
    assert sig["ssim_weight"].default == 0.0 and sig["ssim_range"].default == 2.0
