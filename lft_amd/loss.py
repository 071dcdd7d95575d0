"""Training objectives beyond the reference's L1 (model/LFT.py:269-277): a pixel penalty -- L1, MSE or Charbonnier -- plus the same
penalty on the gradients of the epipolar-plane images (EPIs), the structure term that keeps parallax lines straight.  The definition
is in include/lft_hip.h (lft_lf_loss); on a HIP device value and gradient come from that one fused kernel, on the CPU from torch ops.

``TrainStep(loss=LFLoss(...))`` / ``fit(loss=...)`` put the kernel inside the captured step; ``LFLoss()(SR, HR)`` under autograd serves
the reference's own loop; ``epi_error`` is the EPI term with the L1 penalty as an evaluation figure of angular consistency.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch
from torch import nn

from . import _lib

PENALTIES = {"l1": _lib.LOSS_L1, "mse": _lib.LOSS_MSE, "charbonnier": _lib.LOSS_CHARBONNIER}
_SPEC_KEYS = ("penalty", "eps", "pixel_weight", "epi_weight", "angRes")


def scratch_bytes(B: int, A: int, H: int, W: int) -> int:
    n = ctypes.c_size_t(0)
    _lib.check(_lib.lib().lft_lf_loss_scratch_bytes(B, A, H, W, ctypes.byref(n)), "lft_lf_loss_scratch_bytes")
    return n.value


def lf_loss(sr: torch.Tensor, hr: torch.Tensor, angRes: int, penalty="l1", eps: float = 1e-3, pixel_weight: float = 1.0,
            epi_weight: float = 0.0, dsr: Optional[torch.Tensor] = None, gscale: float = 1.0, loss3: Optional[torch.Tensor] = None,
            scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """lft_lf_loss on contiguous float32 HIP tensors [B,1,A*H,A*W]: returns loss3 = (total, P, E) on the device and, if `dsr` is
    given, writes gscale * d total / d sr there.  loss3 / scratch: buffers to use (a captured step owns its own).  Only enqueues."""
    if not sr.is_cuda:
        raise _lib.LftError("lft_lf_loss runs on a HIP device only")
    for t in (sr, hr) + (() if dsr is None else (dsr,)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != sr.shape or t.device != sr.device or t.dim() != 4 or t.shape[1] != 1:
            raise _lib.LftError("sr, hr and dsr must be contiguous float32 tensors [B,1,A*H,A*W] on one device")
    B, _, R, C = sr.shape
    A = int(angRes)
    if A < 1 or R % A or C % A:
        raise _lib.LftError(f"a {R} x {C} mosaic does not divide into {A} x {A} views")
    H, W = R // A, C // A
    pen = PENALTIES[penalty] if isinstance(penalty, str) else int(penalty)
    with torch.cuda.device(sr.device):
        if loss3 is None:
            loss3 = torch.empty(3, dtype=torch.float32, device=sr.device)
        if scratch is None:
            scratch = torch.empty(scratch_bytes(B, A, H, W), dtype=torch.uint8, device=sr.device)
        _lib.check(_lib.lib().lft_lf_loss(sr.data_ptr(), hr.data_ptr(), B, A, H, W, pen, eps, pixel_weight, epi_weight,
                                          None if dsr is None else dsr.data_ptr(), gscale, loss3.data_ptr(), scratch.data_ptr(),
                                          torch.cuda.current_stream(sr.device).cuda_stream), "lft_lf_loss")
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


class _LFLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sr, hr, A, pen, eps, w_pix, w_epi):
        sr_c, hr_c = sr.detach().contiguous().float(), hr.detach().contiguous().float()
        dsr = torch.empty_like(sr_c)
        loss3 = lf_loss(sr_c, hr_c, A, pen, eps, w_pix, w_epi, dsr=dsr)
        ctx.save_for_backward(dsr)
        ctx.mark_non_differentiable(loss3)
        return loss3[0].clone(), loss3

    @staticmethod
    def backward(ctx, gtotal, _gterms):
        (dsr,) = ctx.saved_tensors
        return gtotal * dsr, None, None, None, None, None, None


class LFLoss(nn.Module):
    """total = pixel_weight * mean rho(SR - HR) + epi_weight * (rho on the EPI gradients of SR - HR), rho = 'l1', 'mse' or
    'charbonnier' (sqrt(x^2 + eps^2)).  angRes: views per side of the mosaics; needed for the EPI term (``get_loss(args)`` and
    TrainStep fill it in).  ``forward`` returns the total -- with a gradient for SR only -- and leaves (total, P, E) in ``.terms``."""

    def __init__(self, penalty: str = "l1", eps: float = 1e-3, pixel_weight: float = 1.0, epi_weight: float = 0.0, angRes: Optional[int] = None):
        super().__init__()
        if penalty not in PENALTIES:
            raise ValueError(f"penalty must be one of {sorted(PENALTIES)}, got {penalty!r}")
        eps, pixel_weight, epi_weight = float(eps), float(pixel_weight), float(epi_weight)
        if penalty == "charbonnier" and not (eps > 0.0 and math.isfinite(eps)):
            raise ValueError(f"the Charbonnier eps must be positive and finite, got {eps}")
        for name, w in (("pixel_weight", pixel_weight), ("epi_weight", epi_weight)):
            if not (w >= 0.0 and math.isfinite(w)):
                raise ValueError(f"{name} must be finite and not negative, got {w}")
        if pixel_weight == 0.0 and epi_weight == 0.0:
            raise ValueError("pixel_weight and epi_weight are both zero")
        if angRes is not None and int(angRes) < 1:
            raise ValueError(f"angRes must be positive, got {angRes}")
        self.penalty, self.eps, self.pixel_weight, self.epi_weight = penalty, eps, pixel_weight, epi_weight
        self.angRes = None if angRes is None else int(angRes)
        self.terms = None

    def spec(self) -> dict:
        return {"penalty": self.penalty, "eps": self.eps, "pixel_weight": self.pixel_weight, "epi_weight": self.epi_weight,
                "angRes": self.angRes}

    @classmethod
    def from_spec(cls, d) -> "LFLoss":
        if isinstance(d, cls):
            return d
        if isinstance(d, str):
            d = {"penalty": d}
        if not isinstance(d, dict):
            raise ValueError(f"a loss spec is a dict with keys out of {_SPEC_KEYS}, got {type(d).__name__}")
        unknown = sorted(set(d) - set(_SPEC_KEYS))
        if unknown:
            raise ValueError(f"unknown key(s) {unknown} in the loss spec; known: {_SPEC_KEYS}")
        return cls(**d)

    def is_plain_l1(self) -> bool:
        """The reference's objective, which TrainStep serves with lft_l1_loss."""
        return self.penalty == "l1" and self.pixel_weight == 1.0 and self.epi_weight == 0.0

    def _args(self):
        A = self.angRes
        if A is None:                                             # the pixel term alone does not look at the views
            if self.epi_weight > 0.0:
                raise ValueError("the EPI term needs angRes: LFLoss(..., angRes=A)")
            A = 1
        return A, self.penalty, self.eps, self.pixel_weight, self.epi_weight

    def forward(self, SR, HR):
        if SR.is_cuda:
            A, pen, eps, wp, we = self._args()
            total, terms = _LFLossFunction.apply(SR, HR, A, pen, eps, wp, we)
            self.terms = terms
            return total
        total, P, E = lf_loss_torch(SR, HR, *self._args())
        self.terms = torch.stack([total.detach(), P.detach(), E.detach()])
        return total


def epi_error(sr: torch.Tensor, hr: torch.Tensor, angRes: int) -> float:
    """Angular-consistency figure of an SR result: the EPI term E with the L1 penalty -- the mean absolute difference between the EPI
    gradients of SR and HR -- for mosaics [B,1,A*H,A*W] or [A*H,A*W] on a HIP device (values only, no gradient)."""
    if sr.dim() == 2:
        sr, hr = sr[None, None], hr[None, None]
    loss3 = lf_loss(sr.contiguous().float(), hr.contiguous().float(), angRes, "l1", 1e-3, 0.0, 1.0)
    return float(loss3[2])
