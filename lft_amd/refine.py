"""Refinement of a selected disparity map: a cross-view consistency check, a farther-neighbour fill and a guided weighted median.

The winner-take-all or SGM map of ``disparity.disparity`` has speckles in flat regions and ragged depth edges.  The three steps
below say which of its pixels can be trusted, smooth it along the image's edges and not across them, and fill what is left.

**Common rules**

- `near` is `"larger"` or `"smaller"`, `LFT_VIEW_NEAR_LARGER` / `LFT_VIEW_NEAR_SMALLER` of `lft_hip_views.h`.
- All floating-point comparisons are fp32.
- Coordinates are fp32, one rounded operation per step, contraction off: the `fl(y + fl(d·Δu))` convention of ``views``.
- No result may depend on tile, launch shape or arrival order.

**1. Check** (lft_disp_check, kernel k_disp_check): cross-view consistency.

- `Dr`: fp32 `[B,H,W]`, the map at the reference position. `Dv`: fp32 `[B,N,H,W]`, the maps of `N` other positions,
  `1 ≤ N ≤ LFT_REFINE_MAX_VIEWS = 128`.
- `deltas`: `N` pairs `(Δu, Δv)` = position − reference, fp32. These are the pairs of `lft_view_warp_disparity`.
- `tau ≥ 0`, finite, rounded once to fp32. `min_agree ≥ 0` and `max_conflict ≥ 0`, ints.

Per pixel `(y,x)` with `d = Dr[y,x]`, over the views in order `n = 0..N−1`:

- `py = fl(y + fl(d·Δu))`, and `px` likewise.
- Footprint: `(floor(py)+a, floor(px)+b)` for `a, b ∈ {0,1}`. `a = 1` is dropped when `py` is integral. `b = 1` is dropped when `px`
  is integral. Positions outside the image are *dropped*, not clamped. That is decided in fp32 before any conversion to int, so a
  huge or non-finite `py` is simply outside.
- Let `Q` be the finite values `Dv[n, ·, ·]` on the footprint. View `n` falls in the first class that applies:
  - *agree*: some `q ∈ Q` has `fl(d − tau) ≤ q ≤ fl(d + tau)`.
  - *occluded*: some `q ∈ Q` is nearer than the band. That is `q > fl(d + tau)` for near = larger, and `q < fl(d − tau)` for
    near = smaller.
  - *conflict*: `Q` is non-empty, so every `q` is farther than the band. The view looks through the surface the map claims.
  - *unseen*: `Q` is empty.

Outputs, all uint8 `[B,H,W]`: `agree`, the count of agreeing views; `conflict`, the count of conflicting views;
`valid = finite(d) && agree ≥ min_agree && conflict ≤ max_conflict`. A non-finite `d` gives 0, 0, 0. Every step is a comparison,
so a numpy float32 restatement gives the same bytes.

**2. Fill** (lft_disp_fill, kernel k_disp_fill): farther-neighbour fill.

- `D`: fp32 `[B,H,W]`. `valid`: uint8 `[B,H,W]`, or NULL for all valid. `reach`: 0..`LFT_REFINE_MAX_FILL = 64`.
- A pixel is *good* iff `valid != 0` and `D` is finite there. A good pixel passes through bit for bit, with `holes = 0`.
- Any other pixel takes the farther of the nearest good values to its left and to its right in the row. "Farther" means the smaller
  for near = larger. Each side is searched up to `reach` pixels. If only one side has a good value, the pixel takes that one.
- If neither side has one, the same search runs up and down the column. A pixel that got a value has `holes = 1`.
- If nothing is found, `out` has the bits of `D` and `holes = 2`.
- Only input values are read. A filled pixel never feeds another.

This is step 2 of `lft_view_render` with a mask in the place of "no coverer"; the search is one device function for both.

**3. Weighted median** (lft_disp_wmedian, kernel k_disp_wmedian): guided weighted median.

- `D`: fp32 `[B,H,W]`. `valid`: uint8 or NULL. `guide`: uint8 `[B,H,W,C]`, `1 ≤ C ≤ 4`. `table`: uint16 `[LFT_REFINE_TABLE = 1024]`.
  `radius r`: 0..`LFT_REFINE_MAX_RADIUS = 7`.
- The window of pixel `p` is every `q = p + (dy,dx)` with `|dy|, |dx| ≤ r` that lies inside the image. Positions outside are dropped.
- `q` is a *sample* iff it is good, in the sense of 2. Its weight is the integer `w_q = table[min(1023, Σ_c |g_c(p) − g_c(q)|)]`.
- `T = Σ w_q` over the samples. It is at most 225·65535, so `2T` fits 32 bits.
- If `T = 0`: `out` has the bits of `D[p]` and `flag = 2`.
- Otherwise `out = min{ v : 2·Σ_{q: D[q] ≤ v} w_q ≥ T }` over the sample values `v`. This is the lower weighted median.
  `flag = 0` if `p` was good, else `flag = 1`.
- The sums are integers, so the definition has no order to fix and is exact. The result is the value of a sample. Values are
  compared as numbers. Where −0 and +0 both occur, either may come back.

``range_table`` is the only place weights are computed: `w[s] = rint(4096·exp(−(s/(255·channels))/sigma))` in fp64.

``refine`` runs the chain: the sweep at the centre, ``disparity_views``, ``consistency``, ``weighted_median`` with that mask, ``fill``
of what is left at flag 2.  Every step hands plain device pointers to one entry point of include/lft_hip_refine.h
(csrc/lft_refine.cuh), on the input's device and current stream; there is no CPU path.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import LftError
from .disparity import DisparityResult, check_slopes, disparity as _disparity
from .refocus import _layout, _views
from .views import NEAR

MAX_VIEWS, MAX_RADIUS, MAX_FILL, TABLE = _lib.REFINE_MAX_VIEWS, _lib.REFINE_MAX_RADIUS, _lib.REFINE_MAX_FILL, _lib.REFINE_TABLE
WHICH = ("cross", "corners", "all")


class ConsistencyResult(NamedTuple):
    valid: torch.Tensor          # uint8, the shape of the map: 1 where the map can be trusted
    agree: torch.Tensor          # uint8, the same shape: the views that agree
    conflict: torch.Tensor       # uint8, the same shape: the views that look through the claimed surface


class RefineResult(NamedTuple):
    disparity: torch.Tensor      # fp32 [H, W] ([B, H, W] for a batch): the refined map
    raw: DisparityResult         # the unrefined result of the sweep at the centre
    valid: torch.Tensor          # the three maps of ``consistency``
    agree: torch.Tensor
    conflict: torch.Tensor
    flags: torch.Tensor          # uint8: the median's flags (0 a good pixel, 1 one that got a value, 2 one whose window had no weight)


_tables: Dict[tuple, torch.Tensor] = {}      # device copies of the deltas and of the weight tables


def clear_cache() -> None:
    """Drop the cached device copies of the position offsets and weight tables."""
    _tables.clear()


def _integer(name: str, v, lo: int, hi: Optional[int] = None) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
        raise LftError(f"{name} must be an integer {'>= ' + str(lo) if hi is None else 'in ' + str(lo) + ' .. ' + str(hi)}, got {v!r}")
    return int(v)


def _check_near(near) -> None:
    if near not in NEAR:
        raise LftError(f"near must be larger or smaller, got {near!r}")


def _pair(name: str, p) -> Tuple[float, float]:
    r = np.array(p, dtype=np.float64).reshape(-1)
    if r.size != 2 or not np.all(np.isfinite(r)):
        raise LftError(f"{name} must be two finite view coordinates, got {p!r}")
    return float(r[0]), float(r[1])


def _positions(positions) -> np.ndarray:
    try:
        t = np.array(positions, dtype=np.float64)
    except (TypeError, ValueError):
        raise LftError(f"positions must be cross, corners, all or an [N, 2] array of finite view coordinates, got {positions!r}") from None
    if t.ndim != 2 or t.shape[1] != 2 or t.shape[0] < 1 or not np.all(np.isfinite(t)):
        raise LftError(f"positions must be cross, corners, all or an [N, 2] array of finite view coordinates, got {positions!r}")
    return t


def view_positions(A: int, which, reference=None) -> np.ndarray:
    """fp64 [N, 2]: the angular positions (u, v) whose maps the check compares the map at `reference` (default the centre
    ((A−1)/2, (A−1)/2)) with.  which: "cross", the four views (ur±R, vr) and (ur, vr±R) with R the largest whole step that stays
    inside the array; "corners", the array's four corner views; "all", every integer view; each without the reference itself; or an
    [N, 2] array, returned as given.  No position left, as for A = 1, is an LftError."""
    A = _integer("angRes", A, 1)
    ur, vr = ((A - 1) / 2,) * 2 if reference is None else _pair("reference", reference)
    if not isinstance(which, str):
        return _positions(which)
    if which not in WHICH:
        raise LftError(f"positions must be cross, corners, all or an [N, 2] array of finite view coordinates, got {which!r}")
    if which == "cross":
        R = math.floor(min(ur, A - 1 - ur, vr, A - 1 - vr))
        pos = [(ur - R, vr), (ur + R, vr), (ur, vr - R), (ur, vr + R)] if R >= 1 else []
    elif which == "corners":
        pos = [(0, 0), (0, A - 1), (A - 1, 0), (A - 1, A - 1)]
    else:
        pos = [(u, v) for u in range(A) for v in range(A)]
    pos = [p for i, p in enumerate(pos) if p != (ur, vr) and p not in pos[:i]]
    if not pos:
        raise LftError(f"positions {which}: {A} x {A} views leave no position beside the reference ({ur:g}, {vr:g})")
    return np.array(pos, dtype=np.float64)


def disparity_views(lf: torch.Tensor, slopes: Sequence[float], positions, **sweep_kw) -> torch.Tensor:
    """The disparity maps at the N `positions` (an [N, 2] array), fp32 [N, H, W] ([B, N, H, W] for a batch of mosaics): one
    ``disparity.disparity(lf, slopes, centre=p, **sweep_kw)`` per position, written into one tensor.  sweep_kw are ``disparity``'s
    own arguments (angRes, aperture, interp, radius, regularize, occlusion, ...) but centre, which is the position."""
    if "centre" in sweep_kw:
        raise LftError("disparity_views: centre is set per position, it cannot be given")
    pos = _positions(positions)
    out = None
    for n, p in enumerate(pos):
        d = _disparity(lf, slopes, centre=(float(p[0]), float(p[1])), **sweep_kw).disparity
        if out is None:
            out = torch.empty(d.shape[:-2] + (len(pos),) + d.shape[-2:], dtype=torch.float32, device=d.device)
        out[..., n, :, :] = d
    return out


def _map(name: str, t, dtype=torch.float32, shape=None, device=None, dims=(2, 3)):
    """The refusals of one map argument: a tensor of `dtype` with 2 or 3 axes, or of `shape` on `device` when those are given."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or (shape is None and t.dim() not in dims) or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = "[H, W] or [B, H, W]" if shape is None else str(list(shape))
        raise LftError(f"the {name} must be a {dtype} tensor of shape {want}, got {getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")
    if device is not None and t.device != device:
        raise LftError(f"the {name} is on {t.device}, the disparity map on {device}")


def _on_gpu(t: torch.Tensor) -> None:
    if t.device.type != "cuda":
        raise LftError(f"the disparity map must be on the GPU, got a tensor on {t.device} (there is no CPU path)")


def _bhw(t: torch.Tensor) -> Tuple[int, int, int]:
    return (1 if t.dim() == 2 else int(t.shape[0])), int(t.shape[-2]), int(t.shape[-1])


def _finite_tau(tau) -> float:
    try:
        t = float(np.float32(tau))
    except (TypeError, ValueError):
        raise LftError(f"tau must be a number, got {tau!r}") from None
    if isinstance(tau, bool) or not (math.isfinite(t) and t >= 0):
        raise LftError(f"tau must be finite and >= 0 (as float32), got {tau!r}")
    return t


def consistency(disparity: torch.Tensor, view_disparity: torch.Tensor, positions, reference=None, *, tau, near: str = "larger",
                min_agree: int = 1, max_conflict: int = 0) -> ConsistencyResult:
    """The cross-view consistency check of the module docstring (one launch of lft_disp_check, enqueue only).

      disparity [H, W],    view_disparity [N, H, W]     ->  valid, agree, conflict uint8 [H, W]
      disparity [B, H, W], view_disparity [B, N, H, W]  ->  valid, agree, conflict uint8 [B, H, W]

    disparity: fp32, the map at `reference`; view_disparity: fp32, the maps at the N `positions` (``disparity_views``), on the same
    device.  positions: an [N, 2] array of (u, v); reference: (ur, vr), or None where the positions are already offsets from it.
    tau: the half-width of the band in which two maps agree, in slope units.  A pixel is valid iff at least min_agree views agree
    and at most max_conflict views conflict.  The defaults 1 and 0 are choices that nobody has tuned."""
    _check_near(near)
    tau = _finite_tau(tau)
    min_agree, max_conflict = _integer("min_agree", min_agree, 0), _integer("max_conflict", max_conflict, 0)
    pos = _positions(positions)
    ref = (0.0, 0.0) if reference is None else _pair("reference", reference)
    if len(pos) > MAX_VIEWS:
        raise LftError(f"{len(pos)} positions: the check takes at most {MAX_VIEWS}")
    _map("disparity map", disparity)
    N = len(pos)
    _map("view disparity", view_disparity, shape=tuple(disparity.shape[:-2]) + (N,) + tuple(disparity.shape[-2:]), device=disparity.device)
    _on_gpu(disparity)
    dev = disparity.device
    B, H, W = _bhw(disparity)
    deltas_h = (pos - np.array(ref, dtype=np.float64)).astype(np.float32)       # the difference in fp64, rounded once
    key = ("deltas", deltas_h.tobytes(), str(dev))
    if key not in _tables:
        _tables[key] = torch.from_numpy(deltas_h.copy()).to(dev)
    out = tuple(torch.empty(disparity.shape, dtype=torch.uint8, device=dev) for _ in range(3))
    if B and H and W:
        dr, dv = disparity.contiguous(), view_disparity.contiguous()
        _lib.enqueue("lft_disp_check", dev, dr.data_ptr(), dv.data_ptr(), _tables[key].data_ptr(), B, N, H, W, tau, NEAR[near], min_agree, max_conflict,
                     *(t.data_ptr() for t in out))
    return ConsistencyResult(*out)


def _check_valid(disparity, valid) -> None:
    _map("disparity map", disparity)
    if valid is not None:
        _map("valid mask", valid, dtype=torch.uint8, shape=disparity.shape, device=disparity.device)


def fill(disparity: torch.Tensor, valid: Optional[torch.Tensor] = None, reach: int = 32, near: str = "larger") -> Tuple[torch.Tensor, torch.Tensor]:
    """(filled, holes): the farther-neighbour fill of the module docstring (one launch of lft_disp_fill, enqueue only).  disparity:
    fp32 [H, W] or [B, H, W]; valid: None (all valid; the non-finite pixels are then the only ones filled) or uint8 of the same
    shape; reach: how far each side is searched, 0 .. 64.  filled: fp32, holes: uint8 (0 a good pixel, 1 a filled one, 2 one for
    which nothing was found and which keeps its bits), both of disparity's shape."""
    _check_near(near)
    reach = _integer("reach", reach, 0, MAX_FILL)
    _check_valid(disparity, valid)
    _on_gpu(disparity)
    dev = disparity.device
    B, H, W = _bhw(disparity)
    out = torch.empty(disparity.shape, dtype=torch.float32, device=dev)
    holes = torch.empty(disparity.shape, dtype=torch.uint8, device=dev)
    if B and H and W:
        d, m = disparity.contiguous(), None if valid is None else valid.contiguous()
        _lib.enqueue("lft_disp_fill", dev, d.data_ptr(), None if m is None else m.data_ptr(), B, H, W, reach, NEAR[near], out.data_ptr(), holes.data_ptr())
    return out, holes


def range_table(sigma: Optional[float], channels: int) -> np.ndarray:
    """np.uint16 [1024]: w[s] = rint(4096·exp(−(s/(255·channels))/sigma)) in fp64, the weight of a sample whose guide differs from
    the pixel's by s in sum over the channels; sigma > 0 and finite, in units of the guide's full range per channel.  sigma=None:
    all ones, the plain median.  This is the only place weights are computed."""
    channels = _integer("channels", channels, 1, 4)
    if sigma is None:
        return np.ones(TABLE, dtype=np.uint16)
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)) or not (math.isfinite(sigma) and sigma > 0):
        raise LftError(f"sigma must be None or a finite number > 0, got {sigma!r}")
    s = np.arange(TABLE, dtype=np.float64)
    return np.rint(4096.0 * np.exp(-(s / (255.0 * channels)) / float(sigma))).astype(np.uint16)


def quantise_guide(guide: torch.Tensor) -> torch.Tensor:
    """A guide as uint8: a uint8 tensor as it is, a float32 one by refocus's rule (clip to [0, 1], × 255, round half to even)."""
    return guide if guide.dtype == torch.uint8 else (guide.clamp(0, 1) * 255).round().to(torch.uint8)


def _device_weights(table: np.ndarray, device) -> torch.Tensor:
    key = ("weights", table.tobytes(), str(device))
    if key not in _tables:
        _tables[key] = torch.from_numpy(table.view(np.int16).copy()).to(device)          # the bits; torch has no arithmetic on uint16 to offer
    return _tables[key]


def weighted_median(disparity: torch.Tensor, guide: torch.Tensor, radius: int = 3, valid: Optional[torch.Tensor] = None,
                    sigma: Optional[float] = 0.1, table: Optional[np.ndarray] = None, iterations: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """(out, flags): the guided weighted median of the module docstring (one launch of lft_disp_wmedian per iteration, enqueue only).

      disparity [H, W],    guide [H, W] or [H, W, C]        ->  out fp32 [H, W],    flags uint8 [H, W]
      disparity [B, H, W], guide [B, H, W] or [B, H, W, C]  ->  out fp32 [B, H, W], flags uint8 [B, H, W]

    guide: C <= 4 channels, a uint8 tensor, or a float32 one that is quantised by refocus's rule (``quantise_guide``).  radius: the
    window is (2 radius + 1)^2, 0 .. 7.  valid: None or a uint8 mask, as for ``fill``.  The weights are ``range_table(sigma, C)``, or
    `table`, an np.uint16 [1024] array (sigma is then not read).  iterations > 1 ping-pongs: each pass reads the last one's output,
    with valid := flags != 2 of that pass.  flags (of the last pass): 0 a good pixel, 1 one that got a value, 2 one whose window
    had no weight and which keeps its bits."""
    radius = _integer("radius", radius, 0, MAX_RADIUS)
    iterations = _integer("iterations", iterations, 1)
    _check_valid(disparity, valid)
    lead = tuple(disparity.shape)
    if not isinstance(guide, torch.Tensor) or guide.dtype not in (torch.uint8, torch.float32) or \
            not (tuple(guide.shape) == lead or (guide.dim() == len(lead) + 1 and tuple(guide.shape[:-1]) == lead and 1 <= guide.shape[-1] <= 4)):
        raise LftError(f"the guide must be a uint8 or float32 tensor of shape {list(lead)} or {list(lead)} + [C], C in 1 .. 4, got "
                       f"{getattr(guide, 'dtype', type(guide).__name__)} {tuple(getattr(guide, 'shape', ()))}")
    if guide.device != disparity.device:
        raise LftError(f"the guide is on {guide.device}, the disparity map on {disparity.device}")
    C = 1 if guide.dim() == len(lead) else int(guide.shape[-1])
    if table is None:
        table = range_table(sigma, C)
    elif not isinstance(table, np.ndarray) or table.dtype != np.uint16 or table.shape != (TABLE,):
        raise LftError(f"table must be an np.uint16 array [{TABLE}], got {getattr(table, 'dtype', type(table).__name__)} {getattr(table, 'shape', ())}")
    _on_gpu(disparity)
    dev = disparity.device
    B, H, W = _bhw(disparity)
    g = quantise_guide(guide).contiguous()
    w = _device_weights(np.ascontiguousarray(table), dev)
    d, m = disparity.contiguous(), None if valid is None else valid.contiguous()
    out = flags = None
    for _ in range(iterations):
        out = torch.empty(disparity.shape, dtype=torch.float32, device=dev)
        flags = torch.empty(disparity.shape, dtype=torch.uint8, device=dev)
        if B and H and W:
            _lib.enqueue("lft_disp_wmedian", dev, d.data_ptr(), None if m is None else m.data_ptr(), g.data_ptr(), w.data_ptr(), B, H, W, C, radius,
                         out.data_ptr(), flags.data_ptr())
        d, m = out, (flags != 2).to(torch.uint8)
    return out, flags


def centre_view(lf: torch.Tensor, angRes: Optional[int] = None) -> torch.Tensor:
    """The view (A // 2, A // 2) of a light field in any of ``refocus``'s layouts, by indexing: [H, W(, C)], [B, H, W] for a batch
    of mosaics.  ``refine``'s default guide."""
    B, A, H, W, _, _, kind = _layout(lf, angRes)
    if kind == "batch":
        return lf.reshape(B, A, H, A, W)[:, A // 2, :, A // 2]
    return _views(lf, angRes)[A // 2, A // 2]


def refine(lf: torch.Tensor, slopes: Sequence[float], angRes: Optional[int] = None, positions: Union[str, np.ndarray, Sequence] = "cross",
           tau: Optional[float] = None, radius: int = 3, sigma: Optional[float] = 0.1, iterations: int = 1, reach: int = 32, near: str = "larger",
           min_agree: int = 1, max_conflict: int = 0, guide: Optional[torch.Tensor] = None, sweep_radius: Optional[int] = None, **sweep_kw) -> RefineResult:
    """The refined disparity map of a light field, on lf's device and current stream (enqueue only).  The chain is
    1. the sweep at the centre, ``disparity.disparity(lf, slopes, angRes, **sweep_kw)``: the field `raw`;
    2. ``disparity_views`` at ``view_positions(A, positions)`` with the same sweep_kw (regularize and occlusion included);
    3. ``consistency`` of the two with tau, near, min_agree, max_conflict: the fields valid, agree, conflict;
    4. ``weighted_median`` of the raw map with that mask, guide, radius, sigma, iterations: the field flags;
    5. ``fill`` of what is left at flag 2, with reach and near: the field disparity.
    tau defaults to the largest slope step (0 for one slope), as the visibility test's does.  guide defaults to ``centre_view``.
    sweep_kw are ``disparity``'s other arguments (aperture, interp, regularize, occlusion, ...).  `radius` here is the median's, so the
    sweep's aggregation radius is sweep_radius (None: ``disparity``'s default).  sweep_kw must not hold centre: the chain refines the
    map at the centre."""
    if "centre" in sweep_kw:
        raise LftError("refine: centre cannot be given, the chain refines the map at the centre of the views")
    if sweep_radius is not None:
        sweep_kw = dict(sweep_kw, radius=sweep_radius)
    sl = check_slopes(slopes)
    if not isinstance(lf, torch.Tensor):
        raise LftError(f"the light field must be a torch tensor, got {type(lf).__name__}")
    # every refusal of the later steps that needs no tensor work comes before the first sweep
    _check_near(near)
    _integer("radius", radius, 0, MAX_RADIUS), _integer("iterations", iterations, 1), _integer("reach", reach, 0, MAX_FILL)
    _integer("min_agree", min_agree, 0), _integer("max_conflict", max_conflict, 0)
    tau = _finite_tau(max(np.diff(np.array(sl, dtype=np.float64)), default=0.0) if tau is None else tau)
    A = _layout(lf, angRes)[1]
    range_table(sigma, 1)
    pos = view_positions(A, positions)
    if len(pos) > MAX_VIEWS:
        raise LftError(f"{len(pos)} positions: the check takes at most {MAX_VIEWS}")
    raw = _disparity(lf, slopes, angRes, **sweep_kw)
    dv = disparity_views(lf, slopes, pos, angRes=angRes, **sweep_kw)
    c = consistency(raw.disparity, dv, pos, reference=((A - 1) / 2,) * 2, tau=tau, near=near, min_agree=min_agree, max_conflict=max_conflict)
    med, flags = weighted_median(raw.disparity, centre_view(lf, angRes) if guide is None else guide, radius, c.valid, sigma, None, iterations)
    filled, _ = fill(med, (flags != 2).to(torch.uint8), reach, near)
    return RefineResult(filled, raw, c.valid, c.agree, c.conflict, flags)
