"""View synthesis: views at fractional angular positions from the A×A views of a light field and a disparity map.

**Inputs**

- B light fields of A×A views, H×W, C ≤ 4. They are uint8 (enters as x/255 via `rf_x`) or float32, read in place through refocus's
  six strides and layouts (`refocus._field`).
- A disparity map `Dr`, fp32 `[B,H,W]`, given at the angular position `reference=(ur,vr)`. The default is the centre `(uc,uc)`,
  which is what `disparity()` returns.
- A required `d_range=(lo,hi)`, `lo ≤ hi`, rounded once to fp32. Finite `Dr` is clamped into it before use; non-finite pixels are
  skipped.
- T targets `(ut,vt)` in view-index units, as fp64 on the host.
- The sign convention is refocus's: a point seen at `y` in view `u` is seen at `y + d·(u'−u)` in view `u'`.

All coordinate arithmetic below is fp32, one rounded operation per step. Contraction is off, as in `k_refocus`, so a numpy float32
restatement reproduces it bit for bit.

1. **Splat.** `Δu = fl32(ut−ur)`, `Δv` likewise. Each source pixel `(y,x)` with clamped `d` lands at `py = fl(y + fl(d·Δu))`,
   `px = fl(x + fl(d·Δv))`. It covers `(floor(py)+a, floor(px)+b)` for `a,b ∈ {0,1}`.
   - `a=1` is dropped when `py` is integral. `b=1` is dropped when `px` is integral. Pixels outside the image are dropped.
   - `Dt0[y',x']` is the nearest `d` among the coverers: `near="larger"` (default) takes the max, `near="smaller"` the min.
   - The result does not depend on arrival order.
   - `reach = ceil(max(|lo|,|hi|)·max(|Δu|,|Δv|)) + 1`. `reach > 64` is refused with a shape error.
2. **Fill.** A hole is a pixel with no coverer.
   - It takes the farther (`near="larger"`: the smaller) of the nearest non-hole `Dt0` values to its left and right in the row, each
     searched up to `fill` pixels (0..64, default 32). If only one side has a value, the hole takes that one.
   - If neither side has a value, the same search runs up and down the column.
   - If that also finds nothing, the hole takes clamped `Dr[y,x]`, or the far end of `d_range` if that pixel is non-finite.
   - Only pre-fill values are read. `holes[t,y,x] = 1` for filled pixels.
3. **Render.** Host weights `w[t,u,v] ≥ 0`, sum 1, are computed in fp64 and rounded once. A 16-byte record per (target, view) holds
   `{du=fl32(u−ut), dv, w, skip}`; ``record_table`` is the only place weights are computed. For `d = Dt[y,x]` and each view with
   `w>0`, in (u,v) order:
   - `sy = fl(y + fl(d·du))`, `sx` likewise. The view is *inside* iff `0 ≤ sy ≤ H−1` and `0 ≤ sx ≤ W−1`.
   - `iy = floor(sy)`, `f = sy − iy`, which is exact.
   - `interp="linear"` uses taps `iy, iy+1` with weights `fl(1−f), f`. `interp="cubic"` uses taps `iy−1..iy+2` with Keys a=−0.5 at
     `f+1, f, 1−f, 2−f`, evaluated in fp32 in the factored forms `1 − t²(2.5 − 1.5t)` and `−0.5·t·(1−t)²`, which do not cancel.
     `nearest` is not offered; it is discontinuous in `d`.
   - Taps are clamped (replicate). Rows are filtered first, then columns, with explicit FMAs as in `k_refocus`.
   - `out = (Σ_inside w·s) / (Σ_inside w)`. If no view is inside, the same quotient is taken over all views with `w>0`.
   - Output is fp32 or uint8 by refocus's rule: clip, ×255, round half to even.

**Blends** (host only): `"quad"`: `max(0,1−|u−ut|)·max(0,1−|v−vt|)`; `"gaussian"`: `sigma` in view steps, default 0.75; `"nearest"`:
one view, lowest index on a tie; or a `[T,A,A]` array. `exclude`: a bool `[A,A]` of views never used. A target whose weights come
out all zero is an `LftError`.

At an integer target with `quad` the taps are `(1,0)` / `(0,1,0,0)` exactly, so the output equals the input view bit for bit, for
fp32 and for uint8.

**Visibility** (``render(..., visibility=dict(tau=...))``). Inputs are those of `lft_view_render`, plus:

- `Dv`: the per-view disparity maps, fp32 `[B, A, A, H, W]`. `Dv[u,v]` is the map at integer view position `(u,v)`.
- `tau`: a threshold, finite, ≥ 0, rounded once to fp32.

Steps 1 (splat) and 2 (fill) are unchanged. `Dt` and `holes` carry the same bits as the plain call.

Step 3 gains a test per view of non-zero weight. Use the same `sy`, `sx`, `inside` as now. Then:

- **Footprint.** `iy = floor(sy)`, `ix = floor(sx)`. The footprint is `(iy+a, ix+b)` for `a, b ∈ {0,1}`.
  - `a = 1` is dropped when `sy` is integral. `b = 1` is dropped when `sx` is integral. Indices are clamped into the image.
  - The footprint is the same for linear and cubic.
- **Occluded.** For `near = larger`: some finite footprint value `q = Dv[u,v,·,·]` satisfies `q > fl(d + tau)`. For `near = smaller`:
  `q < fl(d − tau)`. Non-finite `q` never occludes. All comparisons are fp32, so a numpy float32 restatement gives the same booleans.
- **Three classes.** `visible` = inside and not occluded. `inside`. `all`: every view with `w > 0`.
- **Output.** `out = Σ w·s / Σ w` over the first non-empty class in that order. Accumulate in `(u,v)` order with the same FMAs as
  now. Views outside the chosen class contribute nothing. So when nothing is occluded, the bits equal `lft_view_render`'s.
- **New output** `visible`: uint8 `[B,T,H,W]`, the number of views in the `visible` class, saturated at 255.

By default `Dv` is made from `Dr` itself: splat and fill (steps 1–2) to the A×A integer positions (``warp_disparity``). The hole fill
already takes the farther neighbour, which is what a disocclusion needs. A caller may pass their own maps instead, for example from
per-view sweeps with ``disparity(centre=(u,v))``. Rendered at the reference position with nothing excluded, `visible` is an occlusion
map: how many views see the surface at each pixel.

``render`` hands the light field as it lies in memory, the map, the record table and the target offsets to one call of
lft_view_render (csrc/lft_views.cuh: k_view_splat, then k_view_render; declared in include/lft_hip_views.h); with `visibility`, to
one call of lft_view_render_visible (csrc/lft_visibility.cuh: k_view_splat, then k_view_render_vis; include/lft_hip_visibility.h),
after one of lft_view_warp_disparity (k_view_splat, then k_view_fill) where the maps are not given.  There is no CPU path.
``densify`` renders the views between the given ones, ``leave_one_out`` scores how well the other views predict each view.
"""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import LftError
from .refocus import _CLASS, _as_given, _device_scratch, _field, _layout

TAPS = {"linear": 2, "cubic": 4}
NEAR = {"larger": _lib.VIEW_NEAR_LARGER, "smaller": _lib.VIEW_NEAR_SMALLER}
MAX_REACH, MAX_FILL = _lib.VIEW_MAX_REACH, _lib.VIEW_MAX_FILL
# lft_view_record of include/lft_hip_views.h
RECORD = np.dtype([("du", np.float32), ("dv", np.float32), ("w", np.float32), ("skip", np.int32)])
Blend = Union[str, np.ndarray, Sequence]


class RenderResult(NamedTuple):
    views: torch.Tensor          # [T, H, W, C] for views with channels, [T, H, W] for views without and mosaics, [B, T, H, W] for a batch
    disparity: torch.Tensor      # fp32 [T, H, W] ([B, T, H, W]): Dt, the map at each target after the fill
    holes: torch.Tensor          # uint8, the same shape: 1 where Dt was filled


class VisibleRenderResult(NamedTuple):
    views: torch.Tensor          # as RenderResult's
    disparity: torch.Tensor
    holes: torch.Tensor
    visible: torch.Tensor        # uint8, the shape of holes: the views of non-zero weight that see the pixel's surface, at most 255


def check_targets(targets) -> np.ndarray:
    """fp64 [T, 2] of a sequence of (ut, vt)."""
    t = np.array(targets, dtype=np.float64)
    if t.ndim == 1 and t.size == 2:
        t = t[None]
    if t.ndim != 2 or t.shape[1] != 2 or t.shape[0] < 1 or not np.all(np.isfinite(t)):
        raise LftError(f"targets must be a non-empty sequence of finite (ut, vt) pairs, got {targets!r}")
    return t


def check_range(d_range) -> Tuple[float, float]:
    """(lo, hi) as the fp32 values the kernels clamp to."""
    try:
        lo, hi = (float(np.float32(v)) for v in d_range)
    except (TypeError, ValueError):
        raise LftError(f"d_range must be (lo, hi), got {d_range!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise LftError(f"d_range must be finite with lo <= hi, got {d_range!r}")
    return lo, hi


def _reference(A: int, reference) -> Tuple[float, float]:
    uc = (A - 1) / 2
    if reference is None:
        return uc, uc
    r = np.array(reference, dtype=np.float64).reshape(-1)
    if r.size != 2 or not np.all(np.isfinite(r)):
        raise LftError(f"reference must be two finite view coordinates (ur, vr), got {reference!r}")
    return float(r[0]), float(r[1])


def target_deltas(A: int, targets, reference=None) -> np.ndarray:
    """fp32 [T, 2]: (Δu, Δv) = fl32(target − reference), the difference taken in fp64."""
    t = check_targets(targets)
    return (t - np.array(_reference(A, reference), dtype=np.float64)).astype(np.float32)


def splat_reach(d_range, deltas: np.ndarray) -> int:
    """ceil(max(|lo|, |hi|) · max(|Δu|, |Δv|)) + 1 over the targets: how far, in pixels, a source can lie from what it covers."""
    lo, hi = check_range(d_range)
    return int(math.ceil(max(abs(lo), abs(hi)) * float(np.abs(deltas.astype(np.float64)).max(initial=0.0)))) + 1


def blend_weights(A: int, targets, blend: Blend = "quad", sigma: float = 0.75, exclude=None) -> np.ndarray:
    """fp64 [T, A, A], >= 0, each target's weights summing to 1."""
    if A < 1:
        raise LftError(f"angRes must be positive, got {A}")
    t = check_targets(targets)
    idx = np.arange(A, dtype=np.float64)
    au, av = np.abs(idx[None, :] - t[:, 0:1]), np.abs(idx[None, :] - t[:, 1:2])                       # [T, A] each
    keep = np.ones((A, A), dtype=bool)
    if exclude is not None:
        ex = np.array(exclude.detach().cpu().numpy() if isinstance(exclude, torch.Tensor) else exclude)
        if ex.shape != (A, A):
            raise LftError(f"exclude must be a boolean [{A}, {A}], got shape {ex.shape}")
        keep = ~ex.astype(bool)
    if isinstance(blend, str):
        if blend == "quad":
            w = np.maximum(0.0, 1.0 - au)[:, :, None] * np.maximum(0.0, 1.0 - av)[:, None, :]
        elif blend == "gaussian":
            s = float(sigma)
            if not s > 0 or not math.isfinite(s):
                raise LftError(f"gaussian blend: sigma must be positive and finite, got {sigma!r}")
            r2 = (au ** 2)[:, :, None] + (av ** 2)[:, None, :]
            w = np.exp(-(r2 - r2.reshape(len(t), -1).min(1)[:, None, None]) / (2 * s * s))           # the nearest view at 1: no underflow
        elif blend == "nearest":
            r2 = np.where(keep[None], (au ** 2)[:, :, None] + (av ** 2)[:, None, :], np.inf)
            w = np.zeros((len(t), A, A))
            for k in range(len(t)):
                if np.isfinite(r2[k]).any():
                    w[k].flat[int(np.argmin(r2[k]))] = 1.0                                              # the first of equal minima: lowest index
        else:
            raise LftError(f"blend must be quad, gaussian, nearest or a [T, A, A] array, got {blend!r}")
    else:
        w = np.array(blend.detach().cpu().numpy() if isinstance(blend, torch.Tensor) else blend, dtype=np.float64)
        if w.shape != (len(t), A, A):
            raise LftError(f"a blend array must be [{len(t)}, {A}, {A}], got shape {w.shape}")
        if not np.all(np.isfinite(w)) or np.any(w < 0):
            raise LftError("the blend's weights must be finite and >= 0")
    w = w * keep[None]
    total = w.reshape(len(t), -1).sum(1)
    if np.any(total <= 0):
        k = int(np.argmax(total <= 0))
        raise LftError(f"target {k} at ({t[k, 0]:g}, {t[k, 1]:g}): every view has weight 0 (blend {blend if isinstance(blend, str) else 'array'}"
                       f"{', after exclude' if exclude is not None else ''})")
    return w / total[:, None, None]


def record_table(A: int, targets, weights: np.ndarray) -> np.ndarray:
    """The host table [T, A*A] of RECORD, target-major, views in (u, v) order: the only place the render's weights are rounded."""
    t = check_targets(targets)
    tab = np.zeros((len(t), A * A), dtype=RECORD)
    idx = np.arange(A, dtype=np.float64)
    tab["du"] = np.repeat((idx[None, :] - t[:, 0:1]), A, axis=1)                                     # u-major
    tab["dv"] = np.tile((idx[None, :] - t[:, 1:2]), (1, A))
    tab["w"] = weights.reshape(len(t), A * A)
    tab["skip"] = tab["w"] == 0
    return tab


_tables: Dict[tuple, Tuple[torch.Tensor, ...]] = {}
_scratch: Dict[tuple, torch.Tensor] = {}      # the pre-fill maps


def _device_tables(A: int, t: np.ndarray, deltas: np.ndarray, weights: np.ndarray, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """(records [T, A*A, 4] int32, deltas [T, 2] fp32) on the device, cached."""
    key = (A, t.tobytes(), deltas.tobytes(), weights.tobytes(), str(device))
    if key not in _tables:
        tab = record_table(A, t, weights)
        _tables[key] = (torch.from_numpy(tab.view(np.int32).reshape(len(t), A * A, RECORD.itemsize // 4).copy()).to(device),
                        torch.from_numpy(deltas.copy()).to(device))
    return _tables[key]


def clear_cache() -> None:
    """Drop the cached record tables, target offsets and scratch buffers (a pre-fill map is B*T*H*W dwords)."""
    _tables.clear()
    _scratch.clear()


def _check_fill(near, fill) -> None:
    if near not in NEAR:
        raise LftError(f"near must be larger or smaller, got {near!r}")
    if isinstance(fill, bool) or int(fill) != fill or not 0 <= int(fill) <= MAX_FILL:
        raise LftError(f"fill must be an integer in 0 .. {MAX_FILL}, got {fill!r}")


def _check_reach(lo: float, hi: float, deltas_h: np.ndarray) -> None:
    reach = splat_reach((lo, hi), deltas_h)
    if reach > MAX_REACH:
        raise LftError(f"reach {reach} pixels (d_range {lo:g} .. {hi:g} times the largest target offset "
                       f"{float(np.abs(deltas_h).max()):g}) above {MAX_REACH}: a shape error")


def _warp(dr: torch.Tensor, B: int, H: int, W: int, deltas_h: np.ndarray, lo: float, hi: float, near: str, fill: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(maps fp32 [B, N, H, W], holes uint8 [B, N, H, W]) of the contiguous map dr [B, H, W] at the N offsets deltas_h: one enqueue."""
    dev, N = dr.device, len(deltas_h)
    key = ("deltas", deltas_h.tobytes(), str(dev))
    if key not in _tables:
        _tables[key] = (torch.from_numpy(deltas_h.copy()).to(dev),)
    maps = torch.empty(B, N, H, W, dtype=torch.float32, device=dev)
    holes = torch.empty(B, N, H, W, dtype=torch.uint8, device=dev)
    if B and H and W:
        scratch = _device_scratch(_scratch, "lft_view_visible_scratch_bytes", (B, N, H, W), dev)
        _lib.enqueue("lft_view_warp_disparity", dev, dr.data_ptr(), B, H, W, _tables[key][0].data_ptr(), float(np.abs(deltas_h).max()), N, lo, hi,
                     NEAR[near], int(fill), scratch.data_ptr(), maps.data_ptr(), holes.data_ptr())
    return maps, holes


def warp_disparity(disparity: torch.Tensor, positions, d_range, reference, near: str = "larger", fill: int = 32) -> Tuple[torch.Tensor, torch.Tensor]:
    """(maps, holes): the disparity map, given at the angular position `reference` = (ur, vr), at each of the N `positions` (u, v) --
    steps 1 and 2 of the module's definition alone, on the map's device and current stream (enqueue only).

      disparity [H, W]     ->  maps fp32 [N, H, W],    holes uint8 [N, H, W]
      disparity [B, H, W]  ->  maps fp32 [B, N, H, W], holes uint8 [B, N, H, W]

    With the A×A integer positions in (u, v) order, maps reshaped to [A, A, H, W] is what ``render(visibility=...)`` uses by default."""
    _check_fill(near, fill)
    lo, hi = check_range(d_range)
    t = check_targets(positions)
    if reference is None:
        raise LftError("warp_disparity: reference (ur, vr), the position the map is given at, is required")
    if not isinstance(disparity, torch.Tensor) or disparity.dtype != torch.float32 or disparity.dim() not in (2, 3):
        raise LftError("the disparity map must be a float32 torch tensor [H, W] or [B, H, W]")
    deltas_h = (t - np.array(_reference(1, reference), dtype=np.float64)).astype(np.float32)
    _check_reach(lo, hi, deltas_h)
    if disparity.device.type != "cuda":
        raise LftError("warp_disparity runs on the GPU only (no CPU path): the disparity map is on " + str(disparity.device))
    dr = disparity.contiguous()
    maps, holes = _warp(dr if dr.dim() == 3 else dr[None], 1 if dr.dim() == 2 else int(dr.shape[0]), int(dr.shape[-2]), int(dr.shape[-1]), deltas_h, lo, hi, near, fill)
    return (maps, holes) if disparity.dim() == 3 else (maps[0], holes[0])


def _check_visibility(visibility) -> Tuple[float, Optional[torch.Tensor]]:
    """(tau as the fp32 value the kernel adds, the caller's maps or None) of ``render``'s `visibility`."""
    if not isinstance(visibility, dict) or "tau" not in visibility or set(visibility) - {"tau", "view_disparity"}:
        raise LftError(f"visibility must be a dict with tau and, optionally, view_disparity, got {visibility!r}")
    try:
        tau = float(np.float32(visibility["tau"]))
    except (TypeError, ValueError):
        raise LftError(f"visibility: tau must be a number, got {visibility['tau']!r}") from None
    if not (math.isfinite(tau) and tau >= 0):
        raise LftError(f"visibility: tau must be finite and >= 0, got {visibility['tau']!r}")
    dv = visibility.get("view_disparity")
    if dv is not None and (not isinstance(dv, torch.Tensor) or dv.dtype != torch.float32):
        raise LftError("visibility: view_disparity must be a float32 torch tensor")
    return tau, dv


def render(lf: torch.Tensor, disparity: torch.Tensor, targets, d_range, angRes: Optional[int] = None, reference=None,
           blend: Blend = "quad", sigma: float = 0.75, exclude=None, interp: str = "linear", near: str = "larger", fill: int = 32,
           out_dtype=None, visibility: Optional[dict] = None) -> Union[RenderResult, VisibleRenderResult]:
    """The views of a light field at the angular positions `targets`, on lf's device and current stream (enqueue only).

      views  [A, A, H, W, C] (C <= 4) or [A, A, H, W], disparity [H, W]   ->  views [T, H, W, C] or [T, H, W], maps [T, H, W]
      mosaic [A*H, A*W] with angRes, disparity [H, W]                     ->  views [T, H, W], maps [T, H, W]
      batch  [B, 1, A*H, A*W] with angRes, disparity [B, H, W]            ->  views [B, T, H, W], maps [B, T, H, W]

    Layouts, strides and input classes are ``refocus.refocus``'s; out_dtype (default: the input's) is torch.float32, the quotient
    itself, or torch.uint8.  disparity: fp32, on lf's device, at `reference` (default the centre, where ``disparity.disparity``
    gives it; with its ``centre=`` anywhere else).  d_range: the ends of the sweep the map came from.

    visibility: None, or dict(tau=..., view_disparity=None) for the per-view visibility test of the module's definition; the result
    is then a VisibleRenderResult, whose fourth field counts the views that see each pixel.  view_disparity: the per-view maps
    [A, A, H, W] ([B, A, A, H, W] for a batch), fp32 on lf's device; None: `disparity` warped to the A×A views first, one more
    enqueue (``warp_disparity``; its reach, to the farthest view from `reference`, falls under the same limit as the targets')."""
    t = lo = hi = weights = deltas_h = tau = dv = None

    def own_arguments():                   # refused before a tensor off the GPU
        nonlocal t, lo, hi, weights, deltas_h, tau, dv
        if interp not in TAPS:
            raise LftError(f"interp must be linear or cubic (nearest is discontinuous in the disparity), got {interp!r}")
        _check_fill(near, fill)
        if visibility is not None:
            tau, dv = _check_visibility(visibility)
        lo, hi = check_range(d_range)
        t = check_targets(targets)
        if not isinstance(disparity, torch.Tensor) or disparity.dtype != torch.float32:
            raise LftError("the disparity map must be a float32 torch tensor")
        A = _layout(lf, angRes)[1]
        weights = blend_weights(A, t, blend, sigma, exclude)
        deltas_h = target_deltas(A, t, reference)
        _check_reach(lo, hi, deltas_h)

    B, A, H, W, C, strides, kind = _field(lf, angRes, "out_dtype", out_dtype, before_device=own_arguments)
    out_dtype = lf.dtype if out_dtype is None else out_dtype
    dev = lf.device
    if disparity.device != dev:
        raise LftError(f"the disparity map is on {disparity.device}, the light field on {dev}")
    want = (B, H, W) if kind == "batch" else (H, W)
    if tuple(disparity.shape) != want and tuple(disparity.shape) != (B, H, W):
        raise LftError(f"the disparity map must be {list(want)} for this light field, got shape {tuple(disparity.shape)}")
    records, deltas = _device_tables(A, t, deltas_h, weights, dev)
    T = len(t)
    dr = disparity.contiguous()
    out = torch.empty(B, T, H, W, C, dtype=out_dtype, device=dev)
    dt = torch.empty(B, T, H, W, dtype=torch.float32, device=dev)
    holes = torch.empty(B, T, H, W, dtype=torch.uint8, device=dev)
    seen = None
    if visibility is not None:
        if dv is None:
            views_at = target_deltas(A, [(u, v) for u in range(A) for v in range(A)], reference)
            _check_reach(lo, hi, views_at)
            dv = _warp(dr if dr.dim() == 3 else dr[None], B, H, W, views_at, lo, hi, near, fill)[0]
        else:
            if dv.device != dev:
                raise LftError(f"visibility: view_disparity is on {dv.device}, the light field on {dev}")
            if tuple(dv.shape) not in ((B, A, A, H, W),) + (((A, A, H, W),) if B == 1 else ()):
                raise LftError(f"visibility: view_disparity must be {[A, A, H, W] if kind != 'batch' else [B, A, A, H, W]} for this light field, "
                               f"got shape {tuple(dv.shape)}")
            dv = dv.contiguous()
        seen = torch.empty(B, T, H, W, dtype=torch.uint8, device=dev)
    # lft_view_render_visible takes lft_view_render's arguments with (Dv, tau) after the map and `visible` after the holes
    name, with_map, with_holes = ("lft_view_render", (), ()) if seen is None else ("lft_view_render_visible", (dv.data_ptr(), tau), (seen.data_ptr(),))
    if B and H and W:
        scratch = _device_scratch(_scratch, "lft_view_render_scratch_bytes" if seen is None else "lft_view_visible_scratch_bytes", (B, T, H, W), dev)
        _lib.enqueue(name, dev, lf.data_ptr(), _CLASS[lf.dtype], B, A, H, W, C, strides, dr.data_ptr(), *with_map, deltas.data_ptr(),
                     float(np.abs(deltas_h).max()), records.data_ptr(), T, TAPS[interp], lo, hi, NEAR[near], int(fill),
                     scratch.data_ptr(), out.data_ptr(), _CLASS[out_dtype], dt.data_ptr(), holes.data_ptr(), *with_holes)
    results = [_as_given(kind, out, image=True)] + [_as_given(kind, t) for t in (dt, holes, seen) if t is not None]
    return RenderResult(*results) if seen is None else VisibleRenderResult(*results)


def grid_targets(A: int, factor: int) -> np.ndarray:
    """fp64 [A', A', 2], A' = factor·(A−1)+1: the positions (i/factor, j/factor) of the A×A grid refined `factor` times."""
    if A < 1 or isinstance(factor, bool) or int(factor) != factor or factor < 1:
        raise LftError(f"grid_targets: angRes {A!r} and factor {factor!r} must be positive integers")
    n = int(factor) * (A - 1) + 1
    p = np.arange(n, dtype=np.float64) / int(factor)
    return np.stack(np.meshgrid(p, p, indexing="ij"), axis=-1)


def densify(lf: torch.Tensor, disparity: torch.Tensor, factor: int, d_range, angRes: Optional[int] = None, **kw) -> torch.Tensor:
    """The light field with `factor` times as many view steps: [A', A', H, W(, C)], A' = factor·(A−1)+1.  The given views are
    copied to their places, the ones between them rendered in one ``render`` call (kw goes there, `visibility` included).  Views and
    mosaics, not batches."""
    if not isinstance(lf, torch.Tensor):
        raise LftError(f"the light field must be a torch tensor, got {type(lf).__name__}")
    if lf.dim() == 4 and not (angRes is None or (lf.shape[0] == lf.shape[1] == angRes and lf.shape[1] != 1)):
        raise LftError("densify takes views [A, A, H, W(, C)] or a mosaic [A*H, A*W], not a batch")
    if lf.dim() == 2:
        if angRes is None or angRes < 1 or lf.shape[0] % angRes or lf.shape[1] % angRes:
            raise LftError(f"a mosaic of {tuple(lf.shape)} needs an angRes that divides it")
        views = lf.reshape(angRes, lf.shape[0] // angRes, angRes, lf.shape[1] // angRes).permute(0, 2, 1, 3)
    else:
        views = lf
    A = int(views.shape[0])
    g = grid_targets(A, factor)
    n = g.shape[0]
    f = int(factor)
    new = [(i, j) for i in range(n) for j in range(n) if i % f or j % f]
    out_dtype = kw.get("out_dtype") or views.dtype
    out = torch.empty((n, n) + tuple(views.shape[2:]), dtype=out_dtype, device=views.device)
    if new:
        r = render(views, disparity, [g[i, j] for i, j in new], d_range, **kw)
        ii, jj = (torch.tensor(ix, device=views.device) for ix in zip(*new))
        out[ii, jj] = r.views
    else:
        _field(views, None, "out_dtype", kw.get("out_dtype"))
    if out_dtype == views.dtype:
        out[::f, ::f] = views
    else:                              # the given views in the class asked for, by refocus's rule
        v = views.float() / 255 if views.dtype == torch.uint8 else views
        out[::f, ::f] = v if out_dtype == torch.float32 else (v.clamp(0, 1) * 255).round().to(torch.uint8)
    return out


def leave_one_out(lf: torch.Tensor, slopes: Sequence[float], positions=None, angRes: Optional[int] = None, sigma: float = 0.75,
                  interp: str = "linear", radius: int = 2, disparity: Optional[torch.Tensor] = None, reference=None, regularize: Optional[dict] = None,
                  occlusion=None, **kw) -> List[float]:
    """PSNR (dB, peak 1) of every held-out view (u, v) of `positions` (default: all, in (u, v) order) predicted from the others:
    the disparity is swept at (u, v) with that view's aperture weight 0 (``disparity.disparity(centre=(u, v))``), the view rendered
    there with the gaussian blend and the view excluded, and compared on the GPU over the interior left by the reach of one view
    step, ceil(max|slope|) + 1 pixels: the nearest views carry the gaussian's weight.  With `disparity` (a map [H, W] at
    `reference`, default the centre) nothing is swept: every held-out view is rendered from that map, the slopes give d_range, and
    the interior is left by the splat's reach where that is larger.  regularize goes to the sweeps (``disparity.disparity``: None, or
    the arguments of the semi-global aggregation), and so does occlusion (None, or the subsets of the occlusion-aware cost).  kw goes to ``render``, `visibility` included: with it the views that do not see a
    pixel's surface leave its blend.  An angularly inconsistent field scores
    low however good its single views are.  A view reproduced exactly scores inf."""
    from . import disparity as Dm
    from .refocus import _views
    sl = Dm.check_slopes(slopes)
    if not isinstance(lf, torch.Tensor):
        raise LftError(f"the light field must be a torch tensor, got {type(lf).__name__}")
    if lf.dim() not in (2, 5) and not (lf.dim() == 4 and lf.shape[0] == lf.shape[1]):
        raise LftError("leave_one_out takes views [A, A, H, W(, C)] or a mosaic [A*H, A*W] with angRes, not a batch")
    views = _views(lf, angRes)
    A, H, W = int(views.shape[0]), int(views.shape[2]), int(views.shape[3])
    if A < 2:
        raise LftError("leave_one_out needs at least two views a side")
    pos = [(u, v) for u in range(A) for v in range(A)] if positions is None else [(int(u), int(v)) for u, v in positions]
    if any(not (0 <= u < A and 0 <= v < A) for u, v in pos):
        raise LftError(f"leave_one_out: positions {positions!r} outside the {A} x {A} views")
    d_range = (min(sl), max(sl))
    m = int(math.ceil(max(abs(sl[0]), abs(sl[-1])))) + 1
    if disparity is not None:
        m = max(m, splat_reach(d_range, target_deltas(A, pos, reference)))
    if H - 2 * m < 1 or W - 2 * m < 1:
        raise LftError(f"leave_one_out: views of {H} x {W} have no interior {m} pixels from the border")
    scores = []
    for u, v in pos:
        ap = np.ones((A, A))
        ap[u, v] = 0.0
        if disparity is None:
            dr, ref = Dm.disparity(views, sl, aperture=ap, interp=interp, radius=radius, centre=(u, v), regularize=regularize,
                                   occlusion=occlusion).disparity, (u, v)
        else:
            dr, ref = disparity, reference
        got = render(views, dr, [(u, v)], d_range, reference=ref, blend="gaussian", sigma=sigma, exclude=ap == 0, interp=interp,
                     out_dtype=torch.float32, **kw).views[0]
        held = views[u, v]
        held = held.double() / 255 if held.dtype == torch.uint8 else held.double()
        err = (got.double() - held)[m:H - m, m:W - m]
        mse = float((err * err).mean())
        scores.append(float("inf") if mse == 0 else 10.0 * math.log10(1.0 / mse))
    return scores
