"""CPU-side tests of the focal-stack term (lft_focal_loss, lft_refocus_adjoint; lft_amd.loss, lft_amd.refocus): the new header and
its binding, every refusal of the three entry points on the host, the fp64 restatement of tests/focal_util.py against fp64 autograd
of focal_loss_torch and against the dot-product identity, LFLoss(focal_weight=...) on CPU tensors against the restatement, the spec
rules and the plumbing, and the scene the term is there for: an error that follows the parallax against an independent one."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import _lib, loss as L, refocus as R
from lft_amd._lib import LftError
from lft_amd.loss import LFLoss

import focal_util as FU
import lf_loss_util as LU
import refocus_util as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = -1, -2
NAMES = ("lft_focal_loss_scratch_bytes", "lft_focal_loss", "lft_refocus_adjoint")


# ---- 1. the header and its binding ----
def test_header_declares_and_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "lft_hip_focal.h")).read()
    assert tuple(re.findall(r"^int\s+(lft_\w+)\s*\(", hdr, flags=re.M)) == NAMES
    assert _lib.FOCAL_EXPORTS == NAMES and _lib.ADDON_HEADERS["lft_hip_focal.h"] == "FOCAL_" and list(_lib.ADDON_HEADERS)[-1] == "lft_hip_focal.h"
    assert _lib.FOCAL_MAX_D == 64 and "#define LFT_FOCAL_MAX_D 64" in hdr
    assert "Added beside ABI 5; lft_version unchanged" in " ".join(hdr.split())
    assert set(NAMES) <= _lib.OPTIONAL_EXPORTS and set(NAMES[1:]) <= _lib.ADDON_STREAM_LAST and NAMES[0] not in _lib.ADDON_STREAM_LAST
    from ctypes import POINTER, c_float, c_int, c_size_t, c_void_p
    assert _lib._ADDON_SIGS[NAMES[0]] == (c_int, [c_int] * 5 + [POINTER(c_size_t)])
    assert _lib._ADDON_SIGS[NAMES[1]] == (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_float, c_float,
                                                  c_void_p, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p])
    assert _lib._ADDON_SIGS[NAMES[2]] == (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p])
    params = lambda name: [p.split()[-1].lstrip("*") for p in re.search(r"int\s+%s\s*\(([^)]*)\)" % name, hdr, flags=re.S).group(1).split(",")]
    assert params(NAMES[0]) == ["B", "D", "A", "H", "W", "out_bytes"]
    assert params(NAMES[1]) == ["sr", "hr", "B", "A", "H", "W", "table", "D", "taps", "penalty", "eps", "w_focal", "dsr", "gscale", "accumulate",
                                "total", "focal_out", "residual", "scratch", "stream"]
    assert params(NAMES[2]) == ["stack_grad", "B", "A", "H", "W", "table", "D", "taps", "out", "accumulate", "stream"]
    # the 59 prototypes of the two older headers and the five older add-on headers keep their contents
    assert len(_lib._SIGS) == 59 and not set(NAMES) & (set(_lib.EXPORTS) | set(_lib.TEST_EXPORTS))
    for other in ("lft_hip.h", "lft_hip_test.h", "lft_hip_views.h", "lft_hip_sgm.h", "lft_hip_visibility.h", "lft_hip_occlusion.h", "lft_hip_aif.h"):
        assert "focal_loss" not in open(os.path.join(ROOT, "include", other)).read() and "refocus_adjoint" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert (len(_lib.VIEW_EXPORTS), len(_lib.SGM_EXPORTS), len(_lib.VISIBILITY_EXPORTS), len(_lib.OCCLUSION_EXPORTS), len(_lib.AIF_EXPORTS)) == (2, 2, 3, 3, 1)
    # one new kernel file, in the unit of the losses; three units as before
    assert _lib.UNITS == ("lft_network", "lft_lightfield", "lft_objective") and "lft_focal.cuh" in _lib.SOURCES
    assert [u for u in _lib.UNITS if "lft_focal.cuh" in open(os.path.join(_lib.CSRC, u + ".hip")).read()] == ["lft_objective"]
    assert "lft_hip_focal.h" in open(os.path.join(_lib.CSRC, "lft_objective.hip")).read()
    _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, name) for name in NAMES)
    assert _lib.lib().lft_version() == 5
    # the definition's sentences stand in the header, the kernel file's comment and the module docstring
    kernel = open(os.path.join(_lib.CSRC, "lft_focal.cuh")).read()
    for text in (hdr, kernel, L.__doc__):
        flat = " ".join(re.sub(r"^\s*(//|\*|/\*)\s?", "", line).strip() for line in text.splitlines())
        for words in ("sr, hr: fp32 mosaics [B,1,A*H,A*W]. View (u,v) is at rows u*H... and columns v*W....",
                      "The refocus table [D, A*A] of lft_refocus_record, from refocus.shift_table(A, slopes, aperture, interp, centre).",
                      "taps in {1,2,4}.", "1 <= D <= LFT_FOCAL_MAX_D = 64.", "A*A <= 128.",
                      "These are the constants and the rho of lft_lf_loss.", "A weight w_focal > 0.",
                      "e = fl(sr - hr) per element, in fp32.",
                      "r_k[b,y,x] is lft_refocus's fp32 output for the light field e and the same table.",
                      "views in (u,v) order, rows first, clamped taps, explicit FMAs, skipped views not read.",
                      "r is bit for bit lft_refocus run on the materialised difference mosaic.",
                      "F = (1/N) sum_{b,k,y,x} rho(r), with N = B*D*H*W.", "rho is evaluated in fp64 on the fp32 r.",
                      "The sum is fp64, from per-block partial sums folded in a fixed order.", "No atomics.",
                      "G_k[b,y,x] = fl32(gscale * w_focal * rho'(r)/N).", "rho' is evaluated in fp64 and rounded once.", "For L1, rho'(0) = 0.",
                      "dsr[b,u,v,y',x'] = sum_k a_{k,n} * sum_{jy} wy[jy] sum_{y in Py} sum_{jx} wx[jx] sum_{x in Px} G_k[b,y,x]",
                      "Py = {y in [0,H) : clamp(y + oy + jy, 0, H-1) = y'}. Px is likewise.", "Skipped views get 0.",
                      "An interior pixel has one y per tap.", "A border pixel collects every y whose tap was clamped onto it.",
                      "The adjoint is fp32.", "The order of the sums is fixed:", "two runs give the same bits.",
                      "*focal_out = fl32(F).", "With accumulate == 0: *total = fl32(w_focal*F), and dsr is fully overwritten.",
                      "With accumulate == 1: both are added to what total and dsr hold, in stream order.",
                      "This takes one rounding each, as lft_ssim_loss does.", "dsr may be NULL (values only).",
                      "An optional output residual: NULL, or fp32 [B,D,H,W] for r.",
                      "Every count scales with B. A mean over equal local shards is therefore the global-batch objective."):
            assert words in flat, words
    # rho and rho' are written once, the sampling reads through refocus's rule, the kernels take no atomics
    assert "loss_rho<PEN, double>(" in kernel and "loss_drho<PEN, double>(" in kernel and "rf_x<float>(" in kernel and "kRfRec" in kernel
    assert "fabs" not in kernel and "sqrt" not in kernel and "atomic" not in kernel.split("#pragma once")[1].lower()
    for name in ("k_focal_residual", "k_focal_fold", "k_focal_adjoint"):
        assert "void %s(" % name in kernel, name


# ---- 2. every refusal of the three entry points is answered on the host ----
P = 1 << 20                                                                    # addresses that are never dereferenced
GOOD = dict(sr=P, hr=2 * P, B=2, A=3, H=5, W=7, table=3 * P, D=3, taps=2, penalty=0, eps=1e-3, w_focal=1.0, dsr=4 * P, gscale=1.0, accumulate=0,
            total=5 * P, focal_out=5 * P + 64, residual=None, scratch=6 * P, stream=None)
GOOD_ADJ = dict(stack_grad=P, B=2, A=3, H=5, W=7, table=3 * P, D=3, taps=2, out=4 * P, accumulate=0, stream=None)
NAN, INF = float("nan"), float("inf")
SHARED = [(dict(taps=3), ERR_ARG, "3 taps"), (dict(taps=0), ERR_ARG, "0 taps"), (dict(D=0), ERR_ARG, "0 slopes outside 1 .. 64"),
          (dict(D=65), ERR_ARG, "65 slopes outside 1 .. 64"), (dict(A=12), ERR_SHAPE, "144 views"), (dict(B=0), ERR_SHAPE, "sizes must be positive"),
          (dict(A=0), ERR_SHAPE, "sizes must be positive"), (dict(H=0), ERR_SHAPE, "sizes must be positive"), (dict(W=-1), ERR_SHAPE, "sizes must be positive"),
          (dict(table=None), ERR_ARG, "null pointer"), (dict(table=3 * P + 2), ERR_ARG, "4-byte aligned"), (dict(accumulate=2), ERR_ARG, "accumulate must be 0 or 1"),
          (dict(accumulate=-1), ERR_ARG, "accumulate must be 0 or 1"), (dict(H=1 << 15, W=1 << 15), ERR_SHAPE, "2^31 - 1 elements"),
          (dict(B=1 << 20, A=1, H=1 << 15, W=1 << 15), ERR_SHAPE, "2^31 - 1 blocks")]


def test_every_refusal_comes_before_any_device_work():
    _lib.build()
    lib = _lib.lib()

    def refused(name, good, change, rc, words):
        lib.lft_scene_counts(1, 1, 1, 1, None, None)                            # leaves another call's message behind
        args = dict(good, **change)
        assert getattr(lib, name)(*args.values()) == rc, (name, change)
        msg = lib.lft_last_error().decode()
        assert msg.startswith(name + ":") and words in msg, (name, change, msg)

    n_mosaic = 2 * 9 * 35
    loss_only = [(dict(sr=None), ERR_ARG, "null pointer"), (dict(hr=None), ERR_ARG, "null pointer"), (dict(total=None), ERR_ARG, "null pointer"),
                 (dict(focal_out=None), ERR_ARG, "null pointer"), (dict(scratch=None), ERR_ARG, "null pointer"),
                 (dict(sr=P + 1), ERR_ARG, "4-byte aligned"), (dict(hr=2 * P + 2), ERR_ARG, "4-byte aligned"), (dict(dsr=4 * P + 3), ERR_ARG, "4-byte aligned"),
                 (dict(total=5 * P + 1), ERR_ARG, "4-byte aligned"), (dict(focal_out=5 * P + 2), ERR_ARG, "4-byte aligned"),
                 (dict(residual=7 * P + 1), ERR_ARG, "4-byte aligned"), (dict(scratch=6 * P + 4), ERR_ARG, "scratch 8-byte aligned"),
                 (dict(penalty=3), ERR_ARG, "unknown penalty 3"), (dict(penalty=-1), ERR_ARG, "unknown penalty -1"),
                 (dict(penalty=2, eps=0.0), ERR_ARG, "Charbonnier eps"), (dict(penalty=2, eps=-1.0), ERR_ARG, "Charbonnier eps"),
                 (dict(penalty=2, eps=NAN), ERR_ARG, "Charbonnier eps"), (dict(w_focal=0.0), ERR_ARG, "w_focal"), (dict(w_focal=-1.0), ERR_ARG, "w_focal"),
                 (dict(w_focal=NAN), ERR_ARG, "w_focal"), (dict(w_focal=INF), ERR_ARG, "w_focal"), (dict(gscale=NAN), ERR_ARG, "gscale is NaN"),
                 (dict(dsr=P), ERR_ARG, "dsr overlaps sr or hr"), (dict(dsr=2 * P + 4 * (n_mosaic - 1)), ERR_ARG, "dsr overlaps sr or hr"),
                 (dict(dsr=P - 4 * (n_mosaic - 1)), ERR_ARG, "dsr overlaps sr or hr")]
    for change, rc, words in SHARED + loss_only:
        refused("lft_focal_loss", GOOD, change, rc, words)
    adj_only = [(dict(stack_grad=None), ERR_ARG, "null pointer"), (dict(out=None), ERR_ARG, "null pointer"), (dict(stack_grad=P + 2), ERR_ARG, "4-byte aligned"),
                (dict(out=4 * P + 1), ERR_ARG, "4-byte aligned"), (dict(out=P), ERR_ARG, "out overlaps stack_grad"),
                (dict(out=P + 4 * (2 * 3 * 35 - 1)), ERR_ARG, "out overlaps stack_grad"), (dict(out=P - 4 * (n_mosaic - 1)), ERR_ARG, "out overlaps stack_grad")]
    for change, rc, words in SHARED + adj_only:
        refused("lft_refocus_adjoint", GOOD_ADJ, change, rc, words)
    # the size query: per-block sums (one double per 32 x 8 tile, slope and batch element, padded to 256 bytes) and G
    n = ctypes.c_size_t(0)
    assert lib.lft_focal_loss_scratch_bytes(8, 5, 5, 64, 64, ctypes.byref(n)) == 0 and n.value == 8 * 5 * 16 * 8 + 4 * 8 * 5 * 64 * 64
    assert lib.lft_focal_loss_scratch_bytes(1, 3, 2, 9, 33, ctypes.byref(n)) == 0 and n.value == 256 + 4 * 3 * 9 * 33
    assert _lib.query("lft_focal_loss_scratch_bytes", 1, 3, 2, 9, 33) == n.value == L.focal_scratch_bytes(1, 3, 2, 9, 33)
    for args, rc, words in (((8, 5, 5, 64, 64, None), ERR_ARG, "null pointer"), ((0, 5, 5, 64, 64, ctypes.byref(n)), ERR_SHAPE, "sizes must be positive"),
                            ((1, 0, 5, 64, 64, ctypes.byref(n)), ERR_ARG, "0 slopes"), ((1, 65, 5, 64, 64, ctypes.byref(n)), ERR_ARG, "65 slopes"),
                            ((1, 1, 12, 64, 64, ctypes.byref(n)), ERR_SHAPE, "144 views")):
        assert lib.lft_focal_loss_scratch_bytes(*args) == rc and lib.lft_last_error().decode().startswith("lft_focal_loss_scratch_bytes:") \
            and words in lib.lft_last_error().decode(), args


def test_python_refusals_need_no_device():
    sr, hr = torch.zeros(2, 1, 15, 21), torch.zeros(2, 1, 15, 21)
    with pytest.raises(LftError, match="lft_focal_loss runs on a HIP device only"):
        L.focal_loss(sr, hr, 3, [0.0])
    g = torch.zeros(2, 3, 5, 7)
    for bad, words in ((g.double(), "contiguous float32"), (g[0], "contiguous float32"), (g.transpose(2, 3), "contiguous float32"), (g.numpy(), "contiguous float32")):
        with pytest.raises(LftError, match=words):
            R.refocus_adjoint(bad, [-1.0, 0.0, 1.0], 3)
    with pytest.raises(LftError, match="interp"):
        R.refocus_adjoint(g, [-1.0, 0.0, 1.0], 3, interp="sinc")
    with pytest.raises(LftError, match="2 slopes for a stack of 3 slices"):
        R.refocus_adjoint(g, [-1.0, 0.0], 3)
    with pytest.raises(LftError, match="accumulate adds to"):
        R.refocus_adjoint(g, [-1.0, 0.0, 1.0], 3, accumulate=True)
    with pytest.raises(LftError, match=r"out must be a contiguous float32 tensor \[2, 1, 15, 21\]"):
        R.refocus_adjoint(g, [-1.0, 0.0, 1.0], 3, out=torch.zeros(2, 1, 15, 20))
    with pytest.raises(LftError, match="no CPU path"):                           # everything right: the device is asked for last
        R.refocus_adjoint(g, [-1.0, 0.0, 1.0], 3)
    assert R.parse_slopes("-1:1:5") == [-1.0, -0.5, 0.0, 0.5, 1.0] and R.parse_slopes("0.5,2") == [0.5, 2.0]


# ---- 3. the restatement against fp64 autograd, and its own adjoint identity ----
def tensors(sr, hr):
    return torch.tensor(sr, dtype=torch.float64, requires_grad=True), torch.tensor(hr, dtype=torch.float64)


@pytest.mark.parametrize("penalty", FU.PENALTIES)
@pytest.mark.parametrize("interp", ["nearest", "linear", "cubic"])
@pytest.mark.parametrize("A", [1, 2, 3, 5])
def test_restatement_gradient_equals_fp64_autograd(A, interp, penalty):
    B, H, W = 2, 5, 7
    sr, hr = FU.exact_pair(np.random.default_rng(100 * A + len(interp)), B, A, H, W)
    table, taps = R.shift_table(A, RU.SLOPES, "full", interp), R.TAPS[interp]
    r, F, G, dsr = FU.focal_np(sr, hr, A, table, taps, penalty, 1e-3, w_focal=0.7, gscale=1.3)
    s, h = tensors(sr, hr)
    stack = L.refocus_torch(s - h, A, RU.SLOPES, interp)
    Ft = L.focal_loss_torch(s, h, A, RU.SLOPES, interp, "full", penalty, 1e-3)
    (1.3 * 0.7 * Ft).backward()
    err_r, err_g = float(np.abs(stack.detach().numpy() - r).max()), float(np.abs(s.grad.numpy() - dsr).max())
    print(f"A{A} {interp} {penalty}: F {F:.12f}, |r - torch| {err_r:.2e}, |dsr - autograd| {err_g:.2e} (largest element {np.abs(dsr).max():.3e})")
    assert r.shape == (B, len(RU.SLOPES), H, W) and err_r <= 1e-12 and abs(F - float(Ft.detach())) <= 1e-12 and err_g <= 1e-12
    if A > 1:                                                                 # slope 40 clamps every tap of the outer views onto a border
        k, n = RU.SLOPES.index(40.0), 0
        assert abs(int(table[k, n]["oy"])) > H and abs(int(table[k, n]["ox"])) > W
        v = FU.views(dsr, A)[:, 0, 0]
        assert np.all(v[:, 1:-1, 1:-1] == FU.views(FU.adjoint_np(G[:, :k], A, table[:k], taps), A)[:, 0, 0][:, 1:-1, 1:-1])


@pytest.mark.parametrize("interp", ["nearest", "linear", "cubic"])
@pytest.mark.parametrize("A", [1, 2, 3, 5])
def test_restatement_satisfies_the_dot_product_identity(A, interp):
    rng = np.random.default_rng(7 * A)
    B, H, W = 2, 5, 7
    for aperture in ("full", RU.user_aperture(A, A)):
        table, taps = R.shift_table(A, RU.SLOPES, aperture, interp), R.TAPS[interp]
        x = rng.standard_normal((B, 1, A * H, A * W))
        g = rng.standard_normal((B, len(RU.SLOPES), H, W))
        Rx = np.stack([RU.refocus_np(v[..., None], table, taps)[..., 0] for v in FU.views(x, A)])
        RTg, cnt, mag = FU.adjoint_np(g, A, table, taps, bound=True)
        lhs, rhs = float((Rx * g).sum()), float((x * RTg).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (A, interp, lhs, rhs)
        # every product is counted once: taps^2 per stack pixel and active view
        active = int((table["skip"] == 0).sum())
        assert cnt.sum() == B * active * taps * taps * H * W and np.all(mag >= np.abs(RTg) - 1e-15)
        skipped = FU.views(RTg, A).reshape(B, A * A, H, W)[:, table["skip"].all(0)]
        assert np.all(skipped == 0.0)


# ---- 4. LFLoss on CPU tensors ----
@pytest.mark.parametrize("combined", [False, True], ids=["alone", "with_charbonnier_epi"])
def test_lfloss_on_cpu_tensors_equals_the_restatement(combined):
    B, A, H, W = 2, 3, 5, 7
    slopes, w = [-1.0, 0.25, 2.0], 0.3
    sr, hr = FU.exact_pair(np.random.default_rng(3), B, A, H, W)
    penalty = "charbonnier" if combined else "l1"
    table = R.shift_table(A, slopes, "full", "cubic")
    _, F, _, g = FU.focal_np(sr, hr, A, table, 4, penalty, 1e-3, w_focal=w)
    if combined:
        loss = LFLoss("charbonnier", pixel_weight=1.0, epi_weight=0.5, angRes=A, focal_weight=w, focal_slopes=slopes, focal_interp="cubic")
        ref3, ref_g = LU.reference(np.array(sr), np.array(hr), A, "charbonnier", 1e-3, 1.0, 0.5)
    else:
        loss = LFLoss(pixel_weight=0.0, epi_weight=0.0, angRes=A, focal_weight=w, focal_slopes=slopes, focal_interp="cubic")
        ref3, ref_g = [0.0, 0.0, 0.0], np.zeros_like(g)
    s, h = tensors(sr, hr)
    total = loss(s, h)
    total.backward()
    terms = [float(v) for v in loss.terms]
    want = ref3[0] + w * F
    assert len(terms) == 5 and float(total.detach()) == terms[0] and terms[3] == 0.0
    assert abs(terms[0] - want) <= 1e-12 * max(1.0, abs(want)) and abs(terms[4] - F) <= 1e-12, (terms, want, F)
    assert abs(terms[1] - ref3[1]) <= 1e-12 and abs(terms[2] - ref3[2]) <= 1e-12
    assert float(np.abs(s.grad.numpy() - (ref_g + g)).max()) <= 1e-12 * float(np.abs(ref_g + g).max())
    # with the SSIM term as well, S takes its place and F stays last
    both = LFLoss(angRes=1, ssim_weight=0.2, focal_weight=w, focal_slopes=[0.0])
    x = torch.rand(1, 1, 12, 13, dtype=torch.float64)
    y = x + 0.1 * torch.rand(1, 1, 12, 13, dtype=torch.float64)
    t = both(x, y)
    P, S, Fv = float((x - y).abs().mean()), float(both.terms[3]), float(both.terms[4])
    assert both.terms.shape == (5,) and 0.0 < S < 1.0 and abs(Fv - P) <= 1e-15              # A = 1, slope 0: the stack is the difference
    assert abs(float(t) - (P + 0.2 * (1.0 - S) + w * Fv)) <= 1e-12


def test_spec_rules():
    five = {"penalty": "charbonnier", "eps": 0.01, "pixel_weight": 0.5, "epi_weight": 2.0, "angRes": 5}
    assert LFLoss("charbonnier", eps=0.01, pixel_weight=0.5, epi_weight=2.0, angRes=5, focal_weight=0.0, focal_slopes=[0.5], focal_interp="cubic").spec() == five
    seven = dict(five, ssim_weight=0.2, ssim_range=2.0)
    assert LFLoss.from_spec(dict(seven, focal_weight=0.0)).spec() == seven
    d = LFLoss("l1", angRes=2, focal_weight=0.2).spec()
    assert d == {"penalty": "l1", "eps": 1e-3, "pixel_weight": 1.0, "epi_weight": 0.0, "angRes": 2, "focal_weight": 0.2, "focal_slopes": [-1.0, 0.0, 1.0],
                 "focal_interp": "linear"}
    assert LFLoss.from_spec(d).spec() == d and LFLoss.from_spec(LFLoss.from_spec(d)).spec() == d
    d1 = dict(d, pixel_weight=0.0, focal_slopes=[-2.0, 0.5], focal_interp="cubic", ssim_weight=0.1, ssim_range=1.0)
    assert LFLoss.from_spec(d1).spec() == d1 and list(LFLoss.from_spec(d1).spec())[-3:] == ["focal_weight", "focal_slopes", "focal_interp"]
    pure = dict(d, pixel_weight=0.0)
    assert LFLoss.from_spec(pure).spec() == pure and not LFLoss.from_spec(pure).has_lf_terms()      # a pure focal objective is legal
    assert LFLoss.from_spec(dict(d, focal_slopes=np.linspace(-1, 1, 3))).spec() == d                 # arrays and tuples are taken as lists
    assert not LFLoss(focal_weight=0.1).is_plain_l1() and LFLoss(focal_slopes=[1.0]).is_plain_l1()
    for bad in ({"focal_weight": -0.1}, {"focal_weight": NAN}, {"focal_weight": INF}, {"focal_weight": 0.2, "focal_interp": "sinc"},
                {"focal_weight": 0.2, "focal_slopes": []}, {"focal_weight": 0.2, "focal_slopes": [0.0, NAN]}, {"focal_weight": 0.2, "focal_slopes": [INF]},
                {"focal_weight": 0.2, "focal_slopes": list(range(65))}, {"focal_weight": 0.2, "focal_slopes": "wide"},
                {"pixel_weight": 0.0, "epi_weight": 0.0, "focal_weight": 0.0}, {"focal_weight": 0.2, "focal": 1.0}, {"focal_slope": [0.0]}):
        with pytest.raises(ValueError):
            LFLoss.from_spec(bad)
    assert LFLoss.from_spec({"focal_weight": 0.2, "focal_slopes": list(range(64))}).focal_slopes == tuple(float(i) for i in range(64))
    with pytest.raises(ValueError, match="angRes"):
        LFLoss(focal_weight=1.0)(torch.zeros(1, 1, 12, 12), torch.zeros(1, 1, 12, 12))


def test_plumbing_get_loss_tools_and_signatures():
    import sys
    from lft_amd import evaluate, train, trainer
    from model import LFT
    spec = {"penalty": "mse", "focal_weight": 0.2, "focal_slopes": [-1.0, 1.0], "focal_interp": "nearest"}
    crit = LFT.get_loss(SimpleNamespace(angRes=3, lft_loss=spec))
    assert isinstance(crit, LFLoss) and crit.spec() == {"penalty": "mse", "eps": 1e-3, "pixel_weight": 1.0, "epi_weight": 0.0, "angRes": 3, **{k: spec[k] for k in list(spec)[1:]}}
    sr, hr = FU.exact_pair(np.random.default_rng(1), 1, 3, 4, 4)
    total = crit(torch.tensor(sr), torch.tensor(hr))                             # fp32 CPU tensors: the tensors' own dtype
    _, F, _, _ = FU.focal_np(sr, hr, 3, R.shift_table(3, [-1.0, 1.0], "full", "nearest"), 1, "mse")
    assert total.dtype == torch.float32 and crit.terms.shape == (5,) and abs(float(crit.terms[4]) - F) <= 1e-5 * F
    assert list(inspect.signature(train.TrainStep.__init__).parameters)[-1] == "loss"
    sig = inspect.signature(LFLoss.__init__).parameters
    assert sig["focal_weight"].default == 0.0 and sig["focal_slopes"].default is None and sig["focal_interp"].default == "linear"
    assert list(inspect.signature(L.focal_loss).parameters)[:15] == ["sr", "hr", "angRes", "slopes", "interp", "aperture", "penalty", "eps", "focal_weight", "dsr",
                                                                    "accumulate", "total", "focal_out", "residual", "scratch"]
    assert list(inspect.signature(L.focal_error).parameters) == ["sr", "hr", "angRes", "slopes", "interp"]
    assert list(inspect.signature(R.refocus_adjoint).parameters)[:6] == ["stack_grad", "slopes", "angRes", "aperture", "interp", "centre"]
    for fn in (evaluate.test_scene, evaluate.test, evaluate.test_sets):
        assert inspect.signature(fn).parameters["focal"].default is None
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import train_dp
        args = train_dp.parse_args(["--focal_weight", "0.2", "--focal_slopes=-1:1:5", "--focal_interp", "cubic"])
        assert train_dp.loss_spec(args) == {"penalty": "l1", "eps": 1e-3, "pixel_weight": 1.0, "epi_weight": 0.0, "focal_weight": 0.2,
                                            "focal_slopes": [-1.0, -0.5, 0.0, 0.5, 1.0], "focal_interp": "cubic"}
        assert train_dp.loss_spec(train_dp.parse_args([])) is None and train_dp.loss_spec(train_dp.parse_args(["--focal_slopes=0:2:3"])) is None
    finally:
        sys.path.pop(0)
    bench = open(os.path.join(ROOT, "tools", "train_bench.py")).read()
    assert all(opt in bench for opt in ('"--focal_weight"', '"--focal_slopes"', '"--focal_interp"'))


# ---- 5. what the term is there for ----
def test_an_error_that_follows_the_parallax_survives_the_aperture_sum():
    """A = 5, one slope.  Two error fields with the same pixel L1: one is a single noise image seen through every view along the
    slope's parallax, the other is independent noise in every view.  The focal term keeps the first and averages the second out by
    1/A (the CPU gives a ratio of 5.09; 3 is asserted)."""
    A, H, W, d0 = 5, 24, 24, 1.0
    rng = np.random.default_rng(0)
    uc, pad = (A - 1) // 2, 2
    f = rng.standard_normal((H + 2 * pad, W + 2 * pad))
    coherent = np.zeros((1, A, A, H, W))
    for u in range(A):
        for v in range(A):                                                       # L[u, v, y, x] = f(y - d0 (u - uc), x - d0 (v - uc))
            coherent[0, u, v] = f[pad - (u - uc):pad - (u - uc) + H, pad - (v - uc):pad - (v - uc) + W]
    independent = rng.standard_normal((1, A, A, H, W))
    hr = torch.zeros(1, 1, A * H, A * W, dtype=torch.float64)
    figures = {}
    for name, field in (("coherent", coherent), ("independent", independent)):
        sr = torch.tensor(FU.mosaic(field))
        crit = LFLoss(angRes=A, focal_weight=1.0, focal_slopes=[d0])
        crit(sr, hr)
        figures[name] = (float(crit.terms[1]), float(crit.terms[4]))
    (pc, fc), (pi, fi) = figures["coherent"], figures["independent"]
    print(f"pixel L1 {pc:.3f} (coherent) and {pi:.3f} (independent); focal L1 {fc:.3f} and {fi:.3f}: ratio {fc / fi:.2f}")
    assert abs(pc - pi) <= 0.05 * pi
    assert fc / fi >= 3.0
