"""Training objectives beyond the reference's L1 (model/LFT.py:269-277): a pixel penalty -- L1, MSE or Charbonnier -- plus the same
penalty on the gradients of the epipolar-plane images (EPIs), the structure term that keeps parallax lines straight.  The definition
is in include/lft_hip.h (lft_lf_loss); on a HIP device value and gradient come from that one fused kernel, on the CPU from torch ops.

``LFLoss(..., ssim_weight=a)`` adds a structural term a * (1 - S), S the plain mean over all views of the Gaussian-window SSIM that
``lft_view_metrics`` reports (lft_ssim_loss in include/lft_hip.h: fp64 inside, value and gradient from one more fused kernel).

``LFLoss(..., focal_weight=a, focal_slopes=slopes)`` adds a * F, F the same penalty on the focal stack of SR - HR (lft_focal_loss in
include/lft_hip_focal.h; the definition is restated below).

``TrainStep(loss=LFLoss(...))`` / ``fit(loss=...)`` put the kernel inside the captured step; ``LFLoss()(SR, HR)`` under autograd serves
the reference's own loop; ``epi_error`` is the EPI term with the L1 penalty as an evaluation figure of angular consistency,
``focal_error`` the focal term with the L1 penalty as the figure of what a refocused image shows.

The focal-stack term (lft_focal_loss, lft_refocus_adjoint)
----------------------------------------------------------
Refocusing is linear.  A term on the focal stack of SR - HR therefore weights an error by how much of it survives the aperture sum:
independent per-view errors average out by 1/A, errors that follow the scene's parallax do not.

Inputs.
- sr, hr: fp32 mosaics [B,1,A*H,A*W]. View (u,v) is at rows u*H... and columns v*W....
- The refocus table [D, A*A] of lft_refocus_record, from refocus.shift_table(A, slopes, aperture, interp, centre).
- taps in {1,2,4}.
- 1 <= D <= LFT_FOCAL_MAX_D = 64.
- A*A <= 128.
- A penalty rho out of LFT_LOSS_L1, LFT_LOSS_MSE and LFT_LOSS_CHARBONNIER, with eps. These are the constants and the rho of
  lft_lf_loss.
- A weight w_focal > 0.
- gscale.

1. Residual stack.
- e = fl(sr - hr) per element, in fp32.
- r_k[b,y,x] is lft_refocus's fp32 output for the light field e and the same table. That means: views in (u,v) order, rows
  first, clamped taps, explicit FMAs, skipped views not read.
- r is bit for bit lft_refocus run on the materialised difference mosaic.

2. Value.
- F = (1/N) sum_{b,k,y,x} rho(r), with N = B*D*H*W.
- rho is evaluated in fp64 on the fp32 r.
- The sum is fp64, from per-block partial sums folded in a fixed order.
- No atomics.

3. Stack gradient.
- G_k[b,y,x] = fl32(gscale * w_focal * rho'(r)/N).
- rho' is evaluated in fp64 and rounded once.
- For L1, rho'(0) = 0.

4. Adjoint.  For view n = (u,v) and its pixel (y',x'):
  dsr[b,u,v,y',x'] = sum_k a_{k,n} * sum_{jy} wy[jy] sum_{y in Py} sum_{jx} wx[jx] sum_{x in Px} G_k[b,y,x]
- Py = {y in [0,H) : clamp(y + oy + jy, 0, H-1) = y'}. Px is likewise.
- Skipped views get 0.
- An interior pixel has one y per tap.
- A border pixel collects every y whose tap was clamped onto it.
- The adjoint is fp32.
- The order of the sums is fixed: over k, then jy, then y ascending, then jx, then x ascending; the sums over x and y are plain
  fp32 additions from 0, each product enters by one explicit FMA (wx into the sum over jx, wy into the sum over jy, a into the sum
  over k), with contraction off. Nothing depends on launch shape, tile or arrival order, there are no atomics, and two runs give
  the same bits.

5. Outputs.
- *focal_out = fl32(F).
- With accumulate == 0: *total = fl32(w_focal*F), and dsr is fully overwritten.
- With accumulate == 1: both are added to what total and dsr hold, in stream order. This takes one rounding each, as
  lft_ssim_loss does.
- dsr may be NULL (values only).
- An optional output residual: NULL, or fp32 [B,D,H,W] for r.
Every count scales with B. A mean over equal local shards is therefore the global-batch objective.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _lib

PENALTIES = {"l1": _lib.LOSS_L1, "mse": _lib.LOSS_MSE, "charbonnier": _lib.LOSS_CHARBONNIER}
_SPEC_KEYS = ("penalty", "eps", "pixel_weight", "epi_weight", "angRes")
_SSIM_KEYS = ("ssim_weight", "ssim_range")
_FOCAL_KEYS = ("focal_weight", "focal_slopes", "focal_interp")
FOCAL_SLOPES = (-1.0, 0.0, 1.0)           # what focal_weight > 0 refocuses to when no slopes are given


def scratch_bytes(B: int, A: int, H: int, W: int) -> int:
    return _lib.query("lft_lf_loss_scratch_bytes", B, A, H, W)


def _mosaics(entry: str, sr, hr, dsr, angRes):
    """What lf_loss and ssim_loss ask of their tensors; (B, A, H, W) of the mosaics [B,1,A*H,A*W]."""
    if not sr.is_cuda:
        raise _lib.LftError(f"{entry} runs on a HIP device only")
    for t in (sr, hr) + (() if dsr is None else (dsr,)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != sr.shape or t.device != sr.device or t.dim() != 4 or t.shape[1] != 1:
            raise _lib.LftError("sr, hr and dsr must be contiguous float32 tensors [B,1,A*H,A*W] on one device")
    B, _, R, C = sr.shape
    A = int(angRes)
    if A < 1 or R % A or C % A:
        raise _lib.LftError(f"a {R} x {C} mosaic does not divide into {A} x {A} views")
    return B, A, R // A, C // A


def lf_loss(sr: torch.Tensor, hr: torch.Tensor, angRes: int, penalty="l1", eps: float = 1e-3, pixel_weight: float = 1.0,
            epi_weight: float = 0.0, dsr: Optional[torch.Tensor] = None, gscale: float = 1.0, loss3: Optional[torch.Tensor] = None,
            scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """lft_lf_loss on contiguous float32 HIP tensors [B,1,A*H,A*W]: returns loss3 = (total, P, E) on the device and, if `dsr` is
    given, writes gscale * d total / d sr there.  loss3 / scratch: buffers to use (a captured step owns its own).  Only enqueues."""
    B, A, H, W = _mosaics("lft_lf_loss", sr, hr, dsr, angRes)
    pen = PENALTIES[penalty] if isinstance(penalty, str) else int(penalty)
    loss3 = torch.empty(3, dtype=torch.float32, device=sr.device) if loss3 is None else loss3
    scratch = torch.empty(scratch_bytes(B, A, H, W), dtype=torch.uint8, device=sr.device) if scratch is None else scratch
    _lib.enqueue("lft_lf_loss", sr.device, sr.data_ptr(), hr.data_ptr(), B, A, H, W, pen, eps, pixel_weight, epi_weight,
                 None if dsr is None else dsr.data_ptr(), gscale, loss3.data_ptr(), scratch.data_ptr())
    return loss3


def _rho(x, penalty, eps):
    if penalty == "l1":
        return x.abs()
    if penalty == "mse":
        return x * x
    return torch.sqrt(x * x + eps * eps)


def lf_loss_torch(sr: torch.Tensor, hr: torch.Tensor, angRes: int, penalty="l1", eps=1e-3, pixel_weight=1.0, epi_weight=0.0):
    """The definition with torch ops, in the tensors' own dtype (the CPU path of LFLoss): (total, P, E), differentiable."""
    B, _, R, C = sr.shape
    A = int(angRes)
    H, W = R // A, C // A
    d = (sr - hr).reshape(B, A, H, A, W)
    P = _rho(d, penalty, eps).mean()
    terms = [_rho(d.narrow(dim, 1, size - 1) - d.narrow(dim, 0, size - 1), penalty, eps).mean()
             for dim, size in ((4, W), (2, H), (3, A), (1, A)) if size > 1]            # Dx, Dy, Dv, Du
    E = sum(terms) / len(terms) if terms else P.new_zeros(())
    return pixel_weight * P + epi_weight * E, P, E


def ssim_scratch_bytes(B: int, A: int, H: int, W: int) -> int:
    return _lib.query("lft_ssim_loss_scratch_bytes", B, A, H, W)


def ssim_loss(sr: torch.Tensor, hr: torch.Tensor, angRes: int, ssim_range: float = 2.0, ssim_weight: float = 1.0,
              dsr: Optional[torch.Tensor] = None, gscale: float = 1.0, accumulate: bool = False, total: Optional[torch.Tensor] = None,
              ssim_out: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None):
    """lft_ssim_loss on contiguous float32 HIP tensors [B,1,A*H,A*W]: returns (total, ssim_out), one-element device tensors holding
    ssim_weight * (1 - S) and S, and, if `dsr` is given, writes gscale * ssim_weight * d(1 - S) / d sr there.  accumulate: total and
    dsr are added to instead (both must then be given).  total / ssim_out / scratch: buffers to use.  Only enqueues."""
    B, A, H, W = _mosaics("lft_ssim_loss", sr, hr, dsr, angRes)
    if accumulate and total is None:
        raise _lib.LftError("accumulate adds to `total`: pass the tensor that holds the other terms")
    for t in (total, ssim_out):
        if t is not None and (t.dtype != torch.float32 or t.numel() != 1 or t.device != sr.device):
            raise _lib.LftError("total and ssim_out are one-element float32 tensors on the device of sr")
    total = torch.empty(1, dtype=torch.float32, device=sr.device) if total is None else total
    ssim_out = torch.empty(1, dtype=torch.float32, device=sr.device) if ssim_out is None else ssim_out
    scratch = torch.empty(ssim_scratch_bytes(B, A, H, W), dtype=torch.uint8, device=sr.device) if scratch is None else scratch
    _lib.enqueue("lft_ssim_loss", sr.device, sr.data_ptr(), hr.data_ptr(), B, A, H, W, ssim_range, ssim_weight,
                 None if dsr is None else dsr.data_ptr(), gscale, int(bool(accumulate)), total.data_ptr(), ssim_out.data_ptr(), scratch.data_ptr())
    return total, ssim_out


def ssim_loss_torch(sr: torch.Tensor, hr: torch.Tensor, angRes: int, ssim_range: float = 2.0) -> torch.Tensor:
    """S of include/lft_hip.h (lft_ssim_loss) with torch ops, in the tensors' own dtype (the CPU path of LFLoss), differentiable: the
    plain mean over all views of the interior mean of the Gaussian-window SSIM map.  Valid-mode separable conv2d per view."""
    B, _, R, C = sr.shape
    A = int(angRes)
    H, W = R // A, C // A
    if H < 11 or W < 11:
        raise ValueError(f"views of {H}x{W} are smaller than the 11x11 SSIM window")
    k = torch.arange(-5, 6, dtype=torch.float64)
    g = torch.exp(-0.5 * k * k / (1.5 * 1.5))
    g = (g / g.sum()).to(dtype=sr.dtype, device=sr.device)

    def views(t):
        return t.reshape(B, A, H, A, W).permute(0, 1, 3, 2, 4).reshape(B * A * A, 1, H, W)

    def filt(t):
        return torch.nn.functional.conv2d(torch.nn.functional.conv2d(t, g.view(1, 1, 1, 11)), g.view(1, 1, 11, 1))

    x, y = views(hr), views(sr)
    mx, my = filt(x), filt(y)
    cov = 121.0 / 120.0
    vx, vy, vxy = cov * (filt(x * x) - mx * mx), cov * (filt(y * y) - my * my), cov * (filt(x * y) - mx * my)
    C1, C2 = (0.01 * ssim_range) ** 2, (0.03 * ssim_range) ** 2
    smap = ((2 * mx * my + C1) * (2 * vxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    return smap.mean(dim=(1, 2, 3)).mean()


def focal_scratch_bytes(B: int, D: int, A: int, H: int, W: int) -> int:
    return _lib.query("lft_focal_loss_scratch_bytes", B, D, A, H, W)


def focal_loss(sr: torch.Tensor, hr: torch.Tensor, angRes: int, slopes: Sequence[float], interp: str = "linear", aperture="full",
               penalty="l1", eps: float = 1e-3, focal_weight: float = 1.0, dsr: Optional[torch.Tensor] = None, accumulate: bool = False,
               total: Optional[torch.Tensor] = None, focal_out: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
               scratch: Optional[torch.Tensor] = None, gscale: float = 1.0):
    """lft_focal_loss on contiguous float32 HIP tensors [B,1,A*H,A*W]: returns (total, focal_out), one-element device tensors holding
    focal_weight * F and F, and, if `dsr` is given, writes gscale * focal_weight * dF/dsr there.  accumulate: total and dsr are added
    to instead (total must then be given).  residual: a contiguous float32 [B,D,H,W] that receives the refocused difference.  total /
    focal_out / scratch: buffers to use.  Only enqueues."""
    from . import refocus
    B, A, H, W = _mosaics("lft_focal_loss", sr, hr, dsr, angRes)
    if interp not in refocus.TAPS:
        raise _lib.LftError(f"interp must be nearest, linear or cubic, got {interp!r}")
    if accumulate and total is None:
        raise _lib.LftError("accumulate adds to `total`: pass the tensor that holds the other terms")
    for t in (total, focal_out):
        if t is not None and (t.dtype != torch.float32 or t.numel() != 1 or t.device != sr.device):
            raise _lib.LftError("total and focal_out are one-element float32 tensors on the device of sr")
    table = refocus._device_table(A, slopes, aperture, interp, sr.device)
    D = int(table.shape[0])
    if residual is not None and (residual.dtype != torch.float32 or not residual.is_contiguous() or tuple(residual.shape) != (B, D, H, W)
                                 or residual.device != sr.device):
        raise _lib.LftError(f"residual must be a contiguous float32 tensor [{B}, {D}, {H}, {W}] on the device of sr")
    pen = PENALTIES[penalty] if isinstance(penalty, str) else int(penalty)
    total = torch.empty(1, dtype=torch.float32, device=sr.device) if total is None else total
    focal_out = torch.empty(1, dtype=torch.float32, device=sr.device) if focal_out is None else focal_out
    scratch = torch.empty(focal_scratch_bytes(B, D, A, H, W), dtype=torch.uint8, device=sr.device) if scratch is None else scratch
    _lib.enqueue("lft_focal_loss", sr.device, sr.data_ptr(), hr.data_ptr(), B, A, H, W, table.data_ptr(), D, refocus.TAPS[interp], pen, eps,
                 focal_weight, None if dsr is None else dsr.data_ptr(), gscale, int(bool(accumulate)), total.data_ptr(), focal_out.data_ptr(),
                 None if residual is None else residual.data_ptr(), scratch.data_ptr())
    return total, focal_out


def refocus_torch(lf: torch.Tensor, angRes: int, slopes: Sequence[float], interp: str = "linear", aperture="full", centre=None) -> torch.Tensor:
    """The focal stack [B,D,H,W] of mosaics [B,1,A*H,A*W] with torch ops, in the tensor's own dtype and differentiable: refocus's
    definition (rows first, clamped taps, skipped views not read) from the fp32-rounded table of ``refocus.shift_table``."""
    from . import refocus
    B, _, R, C = lf.shape
    A = int(angRes)
    H, W = R // A, C // A
    table, taps = refocus.shift_table(A, slopes, aperture, interp, centre), refocus.TAPS[interp]
    views = lf.reshape(B, A, H, A, W)
    ys, xs = torch.arange(H, device=lf.device), torch.arange(W, device=lf.device)
    stack = []
    for k in range(table.shape[0]):
        r = lf.new_zeros(B, H, W)
        for n in range(A * A):
            rec = table[k, n]
            if rec["skip"]:
                continue
            v = views[:, n // A, :, n % A, :]
            rows = sum(float(rec["wy"][j]) * v[:, (ys + int(rec["oy"]) + j).clamp(0, H - 1)] for j in range(taps))
            r = r + float(rec["a"]) * sum(float(rec["wx"][j]) * rows[:, :, (xs + int(rec["ox"]) + j).clamp(0, W - 1)] for j in range(taps))
        stack.append(r)
    return torch.stack(stack, 1)


def focal_loss_torch(sr: torch.Tensor, hr: torch.Tensor, angRes: int, slopes: Sequence[float], interp: str = "linear", aperture="full",
                     penalty="l1", eps=1e-3) -> torch.Tensor:
    """F of the focal-stack term with torch ops, in the tensors' own dtype (the CPU path of LFLoss), differentiable: the mean of rho
    over the focal stack of sr - hr."""
    return _rho(refocus_torch(sr - hr, angRes, slopes, interp, aperture), penalty, eps).mean()


class _LFLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sr, hr, A, pen, eps, w_pix, w_epi, w_ssim, ssim_range, w_focal=0.0, focal_slopes=None, focal_interp="linear"):
        sr_c, hr_c = sr.detach().contiguous().float(), hr.detach().contiguous().float()
        dsr = torch.empty_like(sr_c)
        lf = w_pix > 0.0 or w_epi > 0.0
        terms = torch.zeros(5 if w_focal > 0.0 else 4 if w_ssim > 0.0 else 3, dtype=torch.float32, device=sr_c.device)
        if lf:
            lf_loss(sr_c, hr_c, A, pen, eps, w_pix, w_epi, dsr=dsr, loss3=terms[:3])
        if w_ssim > 0.0:
            ssim_loss(sr_c, hr_c, A, ssim_range, w_ssim, dsr=dsr, accumulate=lf, total=terms[0:1], ssim_out=terms[3:4])
        if w_focal > 0.0:
            focal_loss(sr_c, hr_c, A, focal_slopes, focal_interp, "full", pen, eps, w_focal, dsr=dsr, accumulate=lf or w_ssim > 0.0,
                       total=terms[0:1], focal_out=terms[4:5])
        ctx.save_for_backward(dsr)
        ctx.mark_non_differentiable(terms)
        return terms[0].clone(), terms

    @staticmethod
    def backward(ctx, gtotal, _gterms):
        (dsr,) = ctx.saved_tensors
        return (gtotal * dsr,) + (None,) * 11


class LFLoss(nn.Module):
    """total = pixel_weight * mean rho(SR - HR) + epi_weight * (rho on the EPI gradients of SR - HR), rho = 'l1', 'mse' or
    'charbonnier' (sqrt(x^2 + eps^2)).  angRes: views per side of the mosaics; needed for the EPI term (``get_loss(args)`` and
    TrainStep fill it in).  ``forward`` returns the total -- with a gradient for SR only -- and leaves (total, P, E) in ``.terms``.

    ssim_weight > 0 adds ssim_weight * (1 - S): S is the plain mean over all views of the SSIM that lft_view_metrics computes with
    data range ``ssim_range`` (2.0 is what fit and evaluate report with, so the term is one minus the logged figure).  ``.terms``
    is then (total, P, E, S), the spec carries the two keys, and pixel_weight == epi_weight == 0 is the pure structural objective.

    focal_weight > 0 adds focal_weight * F: F is the mean of rho over the focal stack of SR - HR, refocused to ``focal_slopes``
    (default FOCAL_SLOPES) over the full aperture with ``focal_interp`` (the module docstring has the definition).  ``.terms`` is
    then (total, P, E, S, F), S being 0 without the SSIM term; the spec carries the three keys; the term alone is a legal objective."""

    def __init__(self, penalty: str = "l1", eps: float = 1e-3, pixel_weight: float = 1.0, epi_weight: float = 0.0, angRes: Optional[int] = None,
                 ssim_weight: float = 0.0, ssim_range: float = 2.0, focal_weight: float = 0.0, focal_slopes: Optional[Sequence[float]] = None,
                 focal_interp: str = "linear"):
        super().__init__()
        focal_weight = float(focal_weight)
        if not (focal_weight >= 0.0 and math.isfinite(focal_weight)):
            raise ValueError(f"focal_weight must be finite and not negative, got {focal_weight}")
        if focal_interp not in ("nearest", "linear", "cubic"):
            raise ValueError(f"focal_interp must be nearest, linear or cubic, got {focal_interp!r}")
        if focal_slopes is None:
            focal_slopes = FOCAL_SLOPES
        try:
            focal_slopes = tuple(float(x) for x in np.array(focal_slopes, dtype=np.float64).reshape(-1))
        except (TypeError, ValueError):
            raise ValueError(f"focal_slopes must be a sequence of numbers, got {focal_slopes!r}") from None
        if not 1 <= len(focal_slopes) <= _lib.FOCAL_MAX_D or not all(math.isfinite(x) for x in focal_slopes):
            raise ValueError(f"focal_slopes must be 1 to {_lib.FOCAL_MAX_D} finite numbers, got {focal_slopes!r}")
        self.focal_weight, self.focal_slopes, self.focal_interp = focal_weight, focal_slopes, focal_interp
        ssim_weight, ssim_range = float(ssim_weight), float(ssim_range)
        if not (ssim_weight >= 0.0 and math.isfinite(ssim_weight)):
            raise ValueError(f"ssim_weight must be finite and not negative, got {ssim_weight}")
        if not (ssim_range > 0.0 and math.isfinite(ssim_range)):
            raise ValueError(f"ssim_range must be positive and finite, got {ssim_range}")
        if penalty not in PENALTIES:
            raise ValueError(f"penalty must be one of {sorted(PENALTIES)}, got {penalty!r}")
        eps, pixel_weight, epi_weight = float(eps), float(pixel_weight), float(epi_weight)
        if penalty == "charbonnier" and not (eps > 0.0 and math.isfinite(eps)):
            raise ValueError(f"the Charbonnier eps must be positive and finite, got {eps}")
        for name, w in (("pixel_weight", pixel_weight), ("epi_weight", epi_weight)):
            if not (w >= 0.0 and math.isfinite(w)):
                raise ValueError(f"{name} must be finite and not negative, got {w}")
        if pixel_weight == 0.0 and epi_weight == 0.0 and ssim_weight == 0.0 and focal_weight == 0.0:
            raise ValueError("pixel_weight and epi_weight are both zero")
        if angRes is not None and int(angRes) < 1:
            raise ValueError(f"angRes must be positive, got {angRes}")
        self.penalty, self.eps, self.pixel_weight, self.epi_weight = penalty, eps, pixel_weight, epi_weight
        self.ssim_weight, self.ssim_range = ssim_weight, ssim_range
        self.angRes = None if angRes is None else int(angRes)
        self.terms = None

    def spec(self) -> dict:
        d = {"penalty": self.penalty, "eps": self.eps, "pixel_weight": self.pixel_weight, "epi_weight": self.epi_weight,
             "angRes": self.angRes}
        if self.ssim_weight > 0.0:                                # without the term: the five keys of every earlier state file
            d.update(ssim_weight=self.ssim_weight, ssim_range=self.ssim_range)
        if self.focal_weight > 0.0:                               # likewise: the three keys only with the term
            d.update(focal_weight=self.focal_weight, focal_slopes=list(self.focal_slopes), focal_interp=self.focal_interp)
        return d

    @classmethod
    def from_spec(cls, d) -> "LFLoss":
        if isinstance(d, cls):
            return d
        if isinstance(d, str):
            d = {"penalty": d}
        if not isinstance(d, dict):
            raise ValueError(f"a loss spec is a dict with keys out of {_SPEC_KEYS + _SSIM_KEYS + _FOCAL_KEYS}, got {type(d).__name__}")
        unknown = sorted(set(d) - set(_SPEC_KEYS + _SSIM_KEYS + _FOCAL_KEYS))
        if unknown:
            raise ValueError(f"unknown key(s) {unknown} in the loss spec; known: {_SPEC_KEYS + _SSIM_KEYS + _FOCAL_KEYS}")
        return cls(**d)

    def is_plain_l1(self) -> bool:
        """The reference's objective, which TrainStep serves with lft_l1_loss."""
        return self.penalty == "l1" and self.pixel_weight == 1.0 and self.epi_weight == 0.0 and self.ssim_weight == 0.0 and self.focal_weight == 0.0

    def has_lf_terms(self) -> bool:
        """False for the pure structural objective, which skips lft_lf_loss."""
        return self.pixel_weight > 0.0 or self.epi_weight > 0.0

    def _args(self):
        A = self.angRes
        if A is None:                                             # the pixel term alone does not look at the views
            if self.epi_weight > 0.0:
                raise ValueError("the EPI term needs angRes: LFLoss(..., angRes=A)")
            if self.ssim_weight > 0.0:
                raise ValueError("the SSIM term needs angRes: LFLoss(..., angRes=A)")
            if self.focal_weight > 0.0:
                raise ValueError("the focal term needs angRes: LFLoss(..., angRes=A)")
            A = 1
        return A, self.penalty, self.eps, self.pixel_weight, self.epi_weight

    def forward(self, SR, HR):
        if SR.is_cuda:
            A, pen, eps, wp, we = self._args()
            total, terms = _LFLossFunction.apply(SR, HR, A, pen, eps, wp, we, self.ssim_weight, self.ssim_range, self.focal_weight,
                                                 self.focal_slopes, self.focal_interp)
            self.terms = terms
            return total
        args = self._args()
        if self.has_lf_terms():
            total, P, E = lf_loss_torch(SR, HR, *args)
        else:
            total = P = E = SR.new_zeros(())
        if self.ssim_weight == 0.0 and self.focal_weight == 0.0:
            self.terms = torch.stack([total.detach(), P.detach(), E.detach()])
            return total
        S = SR.new_zeros(())
        if self.ssim_weight > 0.0:
            S = ssim_loss_torch(SR, HR, args[0], self.ssim_range)
            total = total + self.ssim_weight * (1.0 - S)
        if self.focal_weight == 0.0:
            self.terms = torch.stack([total.detach(), P.detach(), E.detach(), S.detach()])
            return total
        F = focal_loss_torch(SR, HR, args[0], self.focal_slopes, self.focal_interp, "full", self.penalty, self.eps)
        total = total + self.focal_weight * F
        self.terms = torch.stack([total.detach(), P.detach(), E.detach(), S.detach(), F.detach()])
        return total


def epi_error(sr: torch.Tensor, hr: torch.Tensor, angRes: int) -> float:
    """Angular-consistency figure of an SR result: the EPI term E with the L1 penalty -- the mean absolute difference between the EPI
    gradients of SR and HR -- for mosaics [B,1,A*H,A*W] or [A*H,A*W] on a HIP device (values only, no gradient)."""
    if sr.dim() == 2:
        sr, hr = sr[None, None], hr[None, None]
    loss3 = lf_loss(sr.contiguous().float(), hr.contiguous().float(), angRes, "l1", 1e-3, 0.0, 1.0)
    return float(loss3[2])


def focal_error(sr: torch.Tensor, hr: torch.Tensor, angRes: int, slopes: Sequence[float], interp: str = "linear") -> float:
    """What a refocused image shows of an SR result's error: the focal term F with the L1 penalty -- the mean absolute difference
    between the focal stacks of SR and HR at `slopes`, full aperture -- for mosaics [B,1,A*H,A*W] or [A*H,A*W] on a HIP device
    (values only, no gradient)."""
    if sr.dim() == 2:
        sr, hr = sr[None, None], hr[None, None]
    _, F = focal_loss(sr.contiguous().float(), hr.contiguous().float(), angRes, slopes, interp)
    return float(F)
