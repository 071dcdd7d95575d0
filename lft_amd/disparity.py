"""Disparity from a light field: a plane sweep over the slopes, windowed aggregation, winner-take-all.

Inputs are the same as for lft_refocus:
- B light fields of A×A views, H×W pixels, C ≤ 4 channels, read in place through six element strides.
- uint8 enters as x/255, float32 as stored.
- Slopes `d_0 < d_1 < … < d_{D-1}` are strictly increasing; they need not be uniform.
- `aperture`, `interp` (1, 2 or 4 taps) and the table are those of `refocus.shift_table`.
- The sample `s_k[u,v,y,x,c] = S(L[u,v,:,:,c], y + d_k(u−uc), x + d_k(v−uc))` is exactly refocus's: rows first, clamped taps,
  weights not renormalised.

The outputs are defined as follows.

1. **Moments.** `m_k[y,x,c] = Σ_{u,v} a·s`, which is the refocus stack. `q_k[y,x,c] = Σ_{u,v} a·s²`.
2. **Raw cost.** `V_k[y,x] = Σ_c max(q_k − m_k², 0)`. This is the aperture-weighted variance of the views at slope `d_k`, summed
   over channels.
3. **Aggregated cost.** `E_k[y,x] = (2r+1)^-2 · Σ_{dy,dx ∈ [−r,r]} V_k[clamp(y+dy,0,H−1), clamp(x+dx,0,W−1)]`.
   - The radius `r` is in 0..8. `r = 0` gives `E = V`.
4. **Index.** `k* = argmin_k E_k`, the lowest k on an exact tie.
5. **Sub-sample refinement.** All of it is fp32, each step a single rounded operation, with the compiler's contraction off as in
   `k_refocus`.
   - For `0 < k* < D−1`: `den = (E_{k*−1} − E_{k*}) + (E_{k*+1} − E_{k*})`. Both terms are ≥ 0, so there is no cancellation.
   - `δ = 0.5·(E_{k*−1} − E_{k*+1})/den` if `den > 0`, clamped to [−0.5, 0.5]. Otherwise, and at either end of the sweep, `δ = 0`.
   - `disparity = d_{k*} + δ·(d_{k*+1} − d_{k*})` for `δ ≥ 0`, and `d_{k*} + δ·(d_{k*} − d_{k*−1})` for `δ < 0`.
   - The slopes are rounded once to fp32 on the host.
6. **Confidence.** `Ē = (Σ_k E_k)/D`, summed in k order. `conf = 1 − E_{k*}/Ē` if `Ē > 0`, else 0.
   - A flat region, `A = 1` and `D = 1` all give 0.
7. **All-in-focus.** `aif[y,x,c] = m_{k*(y,x)}[y,x,c]`, fp32 or uint8 by refocus's rule.
   - `m` is accumulated in refocus's order: views in (u,v) order, taps in table order, explicit FMAs.
   - So `aif` equals `lft_refocus`'s fp32 stack gathered at `k*`, **bit for bit**.

A pixel's results must not depend on the tile, on the image around the support of its taps and window, or on the launch shape.
That requires a fixed aggregation order, dy then dx.

``disparity`` hands the light field as it lies in memory, refocus's table and the fp32 slopes to one call of lft_disparity
(csrc/lft_disparity.cuh: k_sweep_cost, then k_disparity_pick); there is no CPU path.  ``disparity_error`` compares two light fields
by their disparity maps: the figure for super-resolved views against ground-truth views.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import LftError
from .refocus import TAPS, Aperture, _CLASS, _device_table, _field

MAX_RADIUS = 8


class DisparityResult(NamedTuple):
    disparity: torch.Tensor                    # fp32 [H, W] ([B, H, W] for a batch): slope units, pixels per view step
    confidence: torch.Tensor                   # fp32, the same shape: 1 - E_best / mean E, in [0, 1]
    index: torch.Tensor                        # int32, the same shape: k*
    all_in_focus: Optional[torch.Tensor]       # [H, W, C] for views with channels, else the shape of disparity; None unless asked for
    cost: Optional[torch.Tensor]               # fp32 [D, H, W] ([B, D, H, W]): E; None unless asked for


_slopes: Dict[tuple, torch.Tensor] = {}
_scratch: Dict[tuple, torch.Tensor] = {}


def _device_slopes(sl: Tuple[float, ...], device) -> torch.Tensor:
    key = (sl, str(device))
    if key not in _slopes:
        _slopes[key] = torch.from_numpy(np.array(sl, dtype=np.float64).astype(np.float32)).to(device)     # rounded once, here
    return _slopes[key]


def _device_scratch(B: int, D: int, H: int, W: int, C: int, flags: int, device) -> torch.Tensor:
    """The sweep's volume (and stack), one buffer per shape and device: calls of one shape on different streams must not overlap."""
    key = (B, D, H, W, C, flags, str(device))
    if key not in _scratch:
        n = _lib.query("lft_disparity_scratch_bytes", B, D, H, W, C, flags)
        _scratch[key] = torch.empty(max(n // 4, 1), dtype=torch.float32, device=device)
    return _scratch[key]


def clear_cache() -> None:
    """Drop the cached scratch buffers and slope arrays (the volume of a large sweep is D*H*W*(1 + C) floats)."""
    _scratch.clear()
    _slopes.clear()


def check_slopes(slopes) -> Tuple[float, ...]:
    sl = np.array(slopes, dtype=np.float64).reshape(-1)
    if sl.size < 1 or not np.all(np.isfinite(sl)):
        raise LftError(f"slopes must be a non-empty sequence of finite numbers, got {slopes!r}")
    if np.any(np.diff(sl.astype(np.float32)) <= 0):
        raise LftError(f"slopes must be strictly increasing (as float32), got {slopes!r}")
    return tuple(float(s) for s in sl)


def disparity(lf: torch.Tensor, slopes: Sequence[float], angRes: Optional[int] = None, aperture: Aperture = "full",
              interp: str = "linear", radius: int = 2, all_in_focus: bool = False, cost_volume: bool = False,
              aif_dtype=None, centre=None) -> DisparityResult:
    """The disparity map of a light field on the GPU, on lf's device and current stream (enqueue only).

      views  [A, A, H, W, C] (C <= 4) or [A, A, H, W]   ->  maps [H, W], all_in_focus [H, W, C] or [H, W], cost [D, H, W]
      mosaic [A*H, A*W] with angRes                       ->  maps [H, W], all_in_focus [H, W], cost [D, H, W]
      batch  [B, 1, A*H, A*W] with angRes                 ->  maps [B, H, W], all_in_focus [B, H, W], cost [B, D, H, W]

    Layouts, strides, input classes, aperture and interp are ``refocus.refocus``'s.  radius: the aggregation window is
    (2 radius + 1)^2, 0 .. 8.  all_in_focus: also return the refocus stack gathered at the index, as aif_dtype (default: the
    input's; torch.float32 is the unclipped sum, torch.uint8 clips, scales and rounds half to even).  cost_volume: also return E.
    centre: the angular position (cu, cv) the sweep is seen from (``refocus.shift_table``), default the centre of the views: the
    map then belongs to that position, and all_in_focus is the plane-sweep rendering of a view there."""
    sl = ()

    def sweep_arguments():                  # radius, interp and slopes are refused before a tensor off the GPU
        nonlocal sl
        if isinstance(radius, bool) or int(radius) != radius or not 0 <= int(radius) <= MAX_RADIUS:
            raise LftError(f"radius must be an integer in 0 .. {MAX_RADIUS}, got {radius!r}")
        if interp not in TAPS:
            raise LftError(f"interp must be nearest, linear or cubic, got {interp!r}")
        sl = check_slopes(slopes)

    B, A, H, W, C, strides, kind = _field(lf, angRes, "aif_dtype", aif_dtype, before_device=sweep_arguments)
    aif_dtype = lf.dtype if aif_dtype is None else aif_dtype
    table = _device_table(A, sl, aperture, interp, lf.device, centre)
    D = len(sl)
    dev = lf.device
    disp = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    conf = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    index = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    cost = torch.empty(B, D, H, W, dtype=torch.float32, device=dev) if cost_volume else None
    aif = torch.empty(B, H, W, C, dtype=aif_dtype, device=dev) if all_in_focus else None
    if B and H and W:
        scratch = _device_scratch(B, D, H, W, C, _lib.DISPARITY_AIF if all_in_focus else 0, dev)
        _lib.enqueue("lft_disparity", dev, lf.data_ptr(), _CLASS[lf.dtype], B, A, H, W, C, strides, table.data_ptr(),
                     _device_slopes(sl, dev).data_ptr(), D, TAPS[interp], int(radius), scratch.data_ptr(), disp.data_ptr(), conf.data_ptr(),
                     index.data_ptr(), cost.data_ptr() if cost_volume else None, aif.data_ptr() if all_in_focus else None, _CLASS[aif_dtype])
    if kind != "batch":
        disp, conf, index = disp[0], conf[0], index[0]
        cost = None if cost is None else cost[0]
        aif = None if aif is None else (aif[0] if kind == "views5" else aif[0, ..., 0])
    elif aif is not None:
        aif = aif[..., 0]
    return DisparityResult(disp, conf, index, aif, cost)


def disparity_error(a: torch.Tensor, b: torch.Tensor, slopes: Sequence[float], angRes: Optional[int] = None,
                    min_confidence: float = 0.5, **kw) -> Tuple[float, float]:
    """(mean |disparity(a) - disparity(b)| over the pixels where b's confidence >= min_confidence, the share of those pixels).
    b is the trusted side: ground-truth views against a's super-resolved ones.  kw goes to ``disparity`` for both.  With no
    confident pixel the mean is nan and the share 0."""
    ra, rb = disparity(a, slopes, angRes, **kw), disparity(b, slopes, angRes, **kw)
    if ra.disparity.shape != rb.disparity.shape:
        raise LftError(f"disparity maps of {tuple(ra.disparity.shape)} and {tuple(rb.disparity.shape)} do not compare")
    keep = rb.confidence >= min_confidence
    n = keep.sum()
    err = ((ra.disparity - rb.disparity).abs().double() * keep).sum() / n
    return float(err), float(n.double() / max(keep.numel(), 1))
