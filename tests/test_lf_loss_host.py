"""CPU-side tests of the light-field loss (lft_amd.loss, lft_lf_loss): the C ABI's declaration, the spec of LFLoss, its CPU path
against the independent restatement of tests/lf_loss_util.py, and the fp32 level the GPU tests' tolerances are written in."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import _lib
from lft_amd.loss import LFLoss

import lf_loss_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_sigs_and_loss_exports_agree():
    hdr = open(os.path.join(ROOT, "include", "lft_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert set(_lib.LOSS_EXPORTS) == {"lft_lf_loss_scratch_bytes", "lft_lf_loss"}
    for name in _lib.LOSS_EXPORTS:
        m = re.search(r"int %s\(([^)]*)\);" % name, flat)
        assert m, name
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")), name
        for decl, ctype in zip(m.group(1).split(","), args):
            decl = decl.strip()
            want = (ctypes.POINTER(ctypes.c_size_t) if decl.startswith("size_t*") else ctypes.c_void_p if "*" in decl
                    else ctypes.c_float if decl.startswith("float ") else ctypes.c_int)
            assert ctype is want, (name, decl, ctype)
    for k, v in U.PEN_ENUM.items():
        assert re.search(r"#define LFT_LOSS_%s %d\b" % (k.upper(), v), hdr), k
    assert (_lib.LOSS_L1, _lib.LOSS_MSE, _lib.LOSS_CHARBONNIER) == (0, 1, 2)
    _lib.build()
    L = _lib.lib()
    assert all(hasattr(L, name) for name in _lib.LOSS_EXPORTS)
    assert L.lft_version() == 5                                   # additive: no new ABI version


def test_size_query_and_refusals_need_no_gpu():
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.lft_lf_loss_scratch_bytes(8, 5, 64, 64, ctypes.byref(n)) == 0 and n.value % 40 == 0 and n.value > 0
    assert L.lft_lf_loss_scratch_bytes(8, 5, 64, 64, None) == -1
    assert L.lft_lf_loss_scratch_bytes(0, 5, 64, 64, ctypes.byref(n)) == -2
    assert L.lft_lf_loss_scratch_bytes(1, 12, 4, 4, ctypes.byref(n)) == -2          # 144 views
    assert L.lft_lf_loss(None, None, 1, 1, 1, 1, 0, 1e-3, 1.0, 0.0, None, 1.0, None, None, None) == -1


def test_spec_round_trip_and_bad_specs():
    a = LFLoss("charbonnier", eps=0.01, pixel_weight=0.5, epi_weight=2.0, angRes=5)
    d = a.spec()
    assert d == {"penalty": "charbonnier", "eps": 0.01, "pixel_weight": 0.5, "epi_weight": 2.0, "angRes": 5}
    assert LFLoss.from_spec(d).spec() == d and LFLoss.from_spec("mse").spec()["penalty"] == "mse"
    assert LFLoss().spec() == {"penalty": "l1", "eps": 1e-3, "pixel_weight": 1.0, "epi_weight": 0.0, "angRes": None}
    assert LFLoss().is_plain_l1() and not LFLoss(epi_weight=0.1).is_plain_l1() and not LFLoss("mse").is_plain_l1()
    for bad in ({"penalty": "huber"}, {"penalty": "charbonnier", "eps": 0.0}, {"penalty": "charbonnier", "eps": float("nan")},
                {"pixel_weight": -1.0}, {"epi_weight": float("nan")}, {"pixel_weight": 0.0, "epi_weight": 0.0}, {"weight": 1.0},
                {"angRes": 0}, 3):
        with pytest.raises(ValueError):
            LFLoss.from_spec(bad)
    with pytest.raises(ValueError, match="angRes"):
        LFLoss(epi_weight=1.0)(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))


@pytest.mark.parametrize("penalty", U.PENALTIES)
def test_lfloss_on_cpu_tensors_equals_the_restatement(penalty):
    for (B, A, H, W) in U.SHAPES[:-1]:
        for w_pix, w_epi in U.WEIGHTS:
            sr, hr = U.lattice_inputs(B, A, H, W, seed=1)
            ref3, ref_g = U.reference(sr, hr, A, penalty, 0.1, w_pix, w_epi)
            loss = LFLoss(penalty, eps=0.1, pixel_weight=w_pix, epi_weight=w_epi, angRes=A)
            s = torch.from_numpy(sr).double().requires_grad_(True)
            h = torch.from_numpy(hr).double().requires_grad_(True)
            total = loss(s, h)
            total.backward()
            got3 = [float(x) for x in loss.terms]
            assert U.loss_error(got3, ref3) <= 1e-12, (B, A, H, W, got3, ref3)
            assert float(total.detach()) == got3[0]
            assert U.grad_error(s.grad.numpy(), ref_g) <= 1e-12, (B, A, H, W)


def test_get_loss_without_a_spec_is_still_the_l1_module():
    from lft_amd import module
    from model import LFT
    for args in (None, SimpleNamespace(angRes=5)):
        crit = LFT.get_loss(args)
        assert type(crit) is module.get_loss and not isinstance(crit, LFLoss)
        a, b = torch.rand(2, 1, 6, 6), torch.rand(2, 1, 6, 6)
        assert torch.equal(crit(a, b), (a - b).abs().mean())
    crit = LFT.get_loss(SimpleNamespace(angRes=3, lft_loss={"penalty": "charbonnier", "epi_weight": 0.5}))
    assert isinstance(crit, LFLoss) and crit.spec() == {"penalty": "charbonnier", "eps": 1e-3, "pixel_weight": 1.0, "epi_weight": 0.5, "angRes": 3}


def test_trainstep_and_fit_take_a_loss():
    import inspect
    from lft_amd import evaluate, train, trainer
    assert inspect.signature(train.TrainStep.__init__).parameters["loss"].default is None
    assert inspect.signature(trainer.fit).parameters["loss"].default is None
    for fn in (evaluate.test_scene, evaluate.test, evaluate.test_sets):
        assert inspect.signature(fn).parameters["epi"].default is False


def fp32_levels():
    """Worst error of the restatement run in fp32 on the CPU against fp64, over every shape, weight pair, eps and smooth penalty of the
    GPU tests, on their lattice inputs: (gradient error / largest gradient element, relative loss error)."""
    worst = {}
    for penalty, eps in (("mse", 0.0), ("charbonnier", U.EPS_VALUES[0]), ("charbonnier", U.EPS_VALUES[1])):
        g, l = 0.0, 0.0
        for (B, A, H, W) in U.SHAPES:
            sr, hr = U.lattice_inputs(B, A, H, W)
            for w_pix, w_epi in U.WEIGHTS:
                ref3, ref_g = U.reference(sr, hr, A, penalty, eps, w_pix, w_epi)
                got3, got_g = U.reference(sr, hr, A, penalty, eps, w_pix, w_epi, dtype=torch.float32)
                g, l = max(g, U.grad_error(got_g, ref_g)), max(l, U.loss_error(got3, ref3))
        worst[(penalty, eps)] = (g, l)
    return worst


def test_gpu_tolerances_are_4x_fp32_torch():
    """No GPU: the levels written into tests/test_gpu_lf_loss.py are what fp32 torch shows against fp64 on these very cases."""
    import test_gpu_lf_loss as T
    worst = fp32_levels()
    for key, (g, l) in worst.items():
        print(f"{key}: fp32 torch vs fp64 torch: gradient {g:.3e} of the largest element, loss {l:.3e} relative")
    gmax = max(g for g, _ in worst.values())
    lmax = max(l for _, l in worst.values())
    assert T.GRAD_LEVEL / 2 <= gmax <= T.GRAD_LEVEL * 1.001, (gmax, T.GRAD_LEVEL)
    assert lmax <= U.LOSS_RTOL, lmax                                     # the loss bound is the project's, not measured
    assert T.GRAD_TOL == 4 * T.GRAD_LEVEL
