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

Semi-global aggregation
-----------------------
Winner-take-all decides each pixel from its own window; where the window sees no texture every slope costs the same and the lowest
k wins.  ``regularize`` (lft_sgm, csrc/lft_sgm.cuh: k_sgm_scan, then k_sgm_pick; declared in include/lft_hip_sgm.h) aggregates a
cost volume along 4 or 8 paths before the selection, and ``disparity(..., regularize=dict(p1=, p2=, ...))`` sweeps and then does so.

**Inputs**
- `E`: fp32 `[B, D, H, W]`, the aggregated cost of `lft_disparity` or any other cost. It must be finite. The bit-for-bit promise is
  for costs ≥ +0.
- Slopes: as for `lft_disparity`.
- Host floats `P1`, `P2` with `0 ≤ P1 ≤ P2`, and `gain ≥ 0`, each rounded once to fp32.
- An optional guide `g`: fp32 `[B, H, W]`.
- `paths` R ∈ {4, 8}.
- `1 ≤ D ≤ LFT_SGM_MAX_D = 256`.

**Directions**, in this order; `paths = 4` takes the first four. Here `q = p − r` is the predecessor of `p` on the path.
- `r0 = (0,+1)`, `r1 = (0,−1)`, `r2 = (+1,0)`, `r3 = (−1,0)`
- `r4 = (+1,+1)`, `r5 = (−1,−1)`, `r6 = (+1,−1)`, `r7 = (−1,+1)`, each written (dy, dx).

**Recurrence.** All of it is fp32, one rounded operation per step, contraction off.
- If `q` lies outside the image: `L_r(p,k) = E(p,k)`.
- Otherwise:
  - `M = min_j L_r(q,j)`.
  - `P2' = P2` without a guide.
  - With a guide: `P2' = max(P1, P2 − fl(gain·|fl(g(p) − g(q))|))`.
  - `c = fl(M + P2')`.
  - `b_k = fl(min(L_r(q,k−1), L_r(q,k+1)) + P1)` over the neighbours that exist. With `D = 1` there is none and `b` is absent.
  - `t_k = min(L_r(q,k), b_k, c)`.
  - `L_r(p,k) = fl(E(p,k) + fl(t_k − M))`.

**Sum.** `S = fl(…fl(fl(L_0 + L_1) + L_2)… + L_{R−1}) · fl(1/R)`. The scaling is exact for R = 4 and 8.

**Selection.** Steps 4–7 of `lft_disparity`, word for word, applied to `S` in the place of `E`:
- index: the lowest k on a tie,
- the parabola refinement,
- `conf = 1 − S_{k*}/S̄`,
- `aif` gathered from a stack at `k*`.

Nothing may depend on launch shape, tile or arrival order. Every sum has a fixed order, and `min` has none to fix.

Occlusion-aware cost from partial apertures
-------------------------------------------
Next to a foreground edge the views on the far side of the edge see the foreground at the background's true slope: the variance of
all views is large there and a wrong slope wins.  ``disparity(..., occlusion="halves" | "quadrants" | dict(subsets=, margin=2.0,
min_views=2))`` also scores each slope by the variance of up to four subsets of the views (lft_disparity_occ,
csrc/lft_occlusion.cuh: k_sweep_cost_occ, then the unchanged k_disparity_pick, then k_occ_gather; declared in
include/lft_hip_occlusion.h).

The inputs, the table, the samples `s`, the aperture `a` (fp64 on the host, sum 1) and the centre `(cu, cv)` are those of
`lft_disparity`. Everything below is fp32, one rounded operation per step, with contraction off.

**Subsets (host only).** Let `δu = u − cu` and `δv = v − cv` in fp64.
- `"halves"`: the four subsets `δu ≤ 0`, `δu ≥ 0`, `δv ≤ 0`, `δv ≥ 0`.
- `"quadrants"`: `(≤,≤)`, `(≤,≥)`, `(≥,≤)`, `(≥,≥)` in `(δu, δv)`.
- A boolean array `[P, A, A]` with 1 ≤ P ≤ 4.
- A subset is *kept* iff at least `min_views` of its views have `a > 0`. `min_views` is an integer ≥ 2, default 2. One view has
  variance 0 at every slope and would win everywhere.
- Dropped subsets never reach the kernel. Subset ids in the outputs are positions in the kept list.
- If no subset is kept, raise `LftError`.
- For a kept subset `p`: `W_p = Σ_{p} a` in fp64. The row `b_p[u,v] = fl32(a/W_p)` for members and 0 for the rest.
- The table `[P', A·A]` fp32, views in (u, v) order, is the only place these weights are rounded.

**Moments.**
- The full aperture is unchanged: `m`, `q`, `V_full` exactly as today, the same FMAs in the same order. `m` stays refocus's stack
  bit for bit, and `aif` is still gathered from it.
- Per kept subset, over its members in (u, v) order:
  - `m_p = fma(b_p, s, m_p)`
  - `q_p = fma(fl(b_p·s), s, q_p)`
  - `V_p = Σ_c max(q_p − fl(m_p·m_p), 0)`, with c = 0 first.

**Combination.**
- `t = min_p V_p` and `U = fl(β·t)`.
- `V = min(V_full, U)`.
- `choice = 0` if `V_full ≤ U`, else the lowest `p` (1-based) with `V_p = t`.
- `β` is the margin: finite, ≥ 1, rounded once to fp32. A subset wins only where it is β times better than the whole aperture.
- Default β = 2. This is a choice and nobody has tuned it.

**After that.** Steps 3 to 7 of `lft_disparity` run word for word on this `V`, through the existing `k_disparity_pick` unchanged.

**New outputs.**
- `subset`: uint8 `[B, H, W]`, equal to `choice` at `(k*, y, x)`.
- Optionally the whole `choice` volume, uint8 `[B, D, H, W]` (``occlusion_volume``).
- Read together with `index`, `subset` is an occlusion-edge map: 0 where all views agree.

No result may depend on the tile, the launch shape or the arrival order.

All-in-focus image from the winning partial aperture
----------------------------------------------------
With `occlusion` the map is right next to a foreground edge, but `all_in_focus=True` is still gathered from `m`, the mean over all
views, which mixes the background with the foreground the far-side views see.  ``all_in_focus_at`` and
``disparity(..., occlusion=, all_in_focus="subset")`` render the mean of the subset that won, at the slope that won (lft_aif_at,
csrc/lft_aif.cuh: k_aif_at, one launch; declared in include/lft_hip_aif.h).

**Inputs.**
- The light field, layout classes, six strides, refocus table `[D, A·A]` of `lft_refocus_record`, `taps` ∈ {1, 2, 4} and the centre
  are those of `lft_refocus`.
- `subsets`: DEVICE fp32 `[P, A·A]`, the rows `b_p` of `lft_disparity_occ`. `0 ≤ P ≤ LFT_OCC_MAX_SUBSETS`. `subsets` is NULL iff
  `P = 0`.
- `index`: int32 `[B, H, W]`. A value outside `0 .. D−1` is clamped into it, as in `lft_occ_gather`.
- `subset`: NULL, or uint8 `[B, H, W]`. `0` means the whole aperture. `p ≥ 1` means row `p−1` of `subsets`. NULL and any id above
  `P` count as 0.

**Output** `aif[b, y, x, c]`, fp32 or uint8 by `rf_byte`.
- Let `k` be the clamped index and `p` the id of the pixel.
- Over the views `n` in (u, v) order, each view has a weight and a membership. For `p = 0` the weight is `w_n = a` of record
  `(k, n)`, and the view is skipped iff the record's `skip` is set. For `p ≥ 1` the weight is `w_n = b_p[n]`, and the view is
  skipped iff `b_p[n] == 0` or the record's `skip` is set.
- The sample `s` is refocus's sample from record `(k, n)`. It uses offsets `oy, ox` and clamped taps. The row pass over `wy` comes
  first, then the column pass over `wx`. Every step after a sum's first product is one explicit FMA, with contraction off.
- `acc = fma(w_n, s, acc)` from `acc = 0`.

**Consequences.**
- `p = 0`: the bits of `lft_refocus`'s stack (fp32 and uint8) at `k`.
- `p ≥ 1`: the bits of `lft_refocus` run with a table whose `a` / `skip` columns are `b_p` / `b_p == 0`, at `k`.
- A pixel's bits must not depend on the tile, on the launch shape, on its neighbours' `k` or `p`, or on which code path served it.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import LftError
from .refocus import TAPS, Aperture, _CLASS, _aperture, _as_given, _centre, _device_scratch, _device_table, _field, _layout

MAX_RADIUS = 8


class DisparityResult(NamedTuple):
    disparity: torch.Tensor                    # fp32 [H, W] ([B, H, W] for a batch): slope units, pixels per view step
    confidence: torch.Tensor                   # fp32, the same shape: 1 - E_best / mean E, in [0, 1]
    index: torch.Tensor                        # int32, the same shape: k*
    all_in_focus: Optional[torch.Tensor]       # [H, W, C] for views with channels, else the shape of disparity; None unless asked for
    cost: Optional[torch.Tensor]               # fp32 [D, H, W] ([B, D, H, W]): E; None unless asked for
    subset = None                              # these two are set on an OcclusionDisparityResult only: the plain tuple keeps its five
    subsets_kept = None


class OcclusionDisparityResult(NamedTuple):
    """DisparityResult with `occlusion`: its fields in their order, then the two new ones."""
    disparity: torch.Tensor
    confidence: torch.Tensor
    index: torch.Tensor
    all_in_focus: Optional[torch.Tensor]
    cost: Optional[torch.Tensor]
    subset: torch.Tensor                       # uint8, the shape of index: 0 where the whole aperture set the cost at k*, else the
    #                                            kept subset (1-based) that did
    subsets_kept: Tuple[int, ...]              # which of the given subsets (0-based) the ids of `subset` stand for


_slopes: Dict[tuple, torch.Tensor] = {}
_scratch: Dict[tuple, torch.Tensor] = {}      # the sweep's volume (and stack); the path volumes of ``regularize``
_subset_tables: Dict[tuple, tuple] = {}       # (device table [P', A*A], kept ids) of ``subset_table``


def _device_slopes(sl: Tuple[float, ...], device) -> torch.Tensor:
    key = (sl, str(device))
    if key not in _slopes:
        _slopes[key] = torch.from_numpy(np.array(sl, dtype=np.float64).astype(np.float32)).to(device)     # rounded once, here
    return _slopes[key]


def clear_cache() -> None:
    """Drop the cached scratch buffers and slope arrays (the volume of a large sweep is D*H*W*(1 + C) floats, the path volumes
    of ``regularize`` paths*D*H*W)."""
    _scratch.clear()
    _slopes.clear()
    _subset_tables.clear()


def check_slopes(slopes) -> Tuple[float, ...]:
    sl = np.array(slopes, dtype=np.float64).reshape(-1)
    if sl.size < 1 or not np.all(np.isfinite(sl)):
        raise LftError(f"slopes must be a non-empty sequence of finite numbers, got {slopes!r}")
    if np.any(np.diff(sl.astype(np.float32)) <= 0):
        raise LftError(f"slopes must be strictly increasing (as float32), got {slopes!r}")
    return tuple(float(s) for s in sl)


def _finite_number(name: str, v, lo: int) -> None:
    """The refusal of a host float that is no finite number in [lo, the largest float32]: margin, p1, p2, edge_gain."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not lo <= v <= float(np.finfo(np.float32).max):
        raise LftError(f"{name} must be a finite number >= {lo} (as float32), got {v!r}")


SUBSET_MODES = ("halves", "quadrants")
_OCC_KEYS = ("subsets", "margin", "min_views")


def _occlusion_arguments(occlusion) -> Tuple[object, float, int]:
    """(subsets, margin, min_views) of an `occlusion` argument, with the refusals that need no light field: the shape of an array
    against A is ``subset_table``'s."""
    if isinstance(occlusion, str):
        occlusion = dict(subsets=occlusion)
    if not isinstance(occlusion, dict) or set(occlusion) - set(_OCC_KEYS):
        raise LftError(f"occlusion must be None, halves, quadrants or a dict with any of subsets, margin, min_views, got {occlusion!r}")
    subsets, margin, min_views = occlusion.get("subsets", "halves"), occlusion.get("margin", 2.0), occlusion.get("min_views", 2)
    if isinstance(subsets, str) and subsets not in SUBSET_MODES:
        raise LftError(f"subsets must be halves, quadrants or a boolean array [P, A, A], got {subsets!r}")
    _finite_number("margin", margin, 1)
    if isinstance(min_views, bool) or not isinstance(min_views, (int, np.integer)) or min_views < 2:
        raise LftError(f"min_views must be an integer >= 2, got {min_views!r}")
    return subsets, float(margin), int(min_views)


def subset_table(A: int, aperture: Aperture = "full", centre=None, subsets="halves", min_views: int = 2) -> Tuple[np.ndarray, Tuple[int, ...]]:
    """(the host table fp32 [P', A*A] of the kept subsets' weights b_p, views in (u, v) order; the kept subsets' positions in the
    given list).  The module docstring has the definition; this is the only place these weights are computed and rounded."""
    subsets, _, min_views = _occlusion_arguments(dict(subsets=subsets, min_views=min_views))
    a = _aperture(A, aperture)
    cu, cv = _centre(A, centre)
    du = np.broadcast_to((np.arange(A, dtype=np.float64) - cu)[:, None], (A, A))
    dv = np.broadcast_to((np.arange(A, dtype=np.float64) - cv)[None, :], (A, A))
    if isinstance(subsets, str):
        lo_u, hi_u, lo_v, hi_v = du <= 0, du >= 0, dv <= 0, dv >= 0
        masks = np.stack([lo_u, hi_u, lo_v, hi_v] if subsets == "halves" else [lo_u & lo_v, lo_u & hi_v, hi_u & lo_v, hi_u & hi_v])
    else:
        masks = np.asarray(subsets.detach().cpu().numpy() if isinstance(subsets, torch.Tensor) else subsets)
        if masks.dtype != np.bool_ or masks.ndim != 3 or masks.shape[1:] != (A, A) or not 1 <= masks.shape[0] <= _lib.OCC_MAX_SUBSETS:
            raise LftError(f"subsets must be a boolean array [P, {A}, {A}] with 1 <= P <= {_lib.OCC_MAX_SUBSETS}, got {masks.dtype} {masks.shape}")
    kept = tuple(p for p in range(masks.shape[0]) if int((masks[p] & (a > 0)).sum()) >= min_views)
    if not kept:
        raise LftError(f"none of the {masks.shape[0]} subsets has {min_views} views of non-zero aperture weight")
    table = np.zeros((len(kept), A * A), dtype=np.float32)
    for row, p in enumerate(kept):
        member = masks[p].reshape(-1)
        W = math.fsum(a.reshape(-1)[member])                        # the exactly rounded fp64 sum: no order to fix
        table[row, member] = (a.reshape(-1)[member] / W).astype(np.float32)      # rounded once, here
    return table, kept


def _device_subsets(A: int, aperture: Aperture, centre, subsets, min_views: int, device) -> Tuple[torch.Tensor, Tuple[int, ...]]:
    ap = aperture if isinstance(aperture, str) else _aperture(A, aperture).tobytes()
    how = subsets if isinstance(subsets, str) else (np.asarray(subsets.cpu() if isinstance(subsets, torch.Tensor) else subsets).shape,
                                                    np.asarray(subsets.cpu() if isinstance(subsets, torch.Tensor) else subsets).tobytes())
    key = (A, ap, None if centre is None else _centre(A, centre), how, min_views, str(device))
    if key not in _subset_tables:
        table, kept = subset_table(A, aperture, centre, subsets, min_views)
        _subset_tables[key] = (torch.from_numpy(table).to(device), kept)
    return _subset_tables[key]


def _sweep_arguments(radius, interp, slopes) -> Tuple[float, ...]:
    """The refusals of a sweep that need no tensor; returns the checked slopes."""
    if isinstance(radius, bool) or int(radius) != radius or not 0 <= int(radius) <= MAX_RADIUS:
        raise LftError(f"radius must be an integer in 0 .. {MAX_RADIUS}, got {radius!r}")
    if interp not in TAPS:
        raise LftError(f"interp must be nearest, linear or cubic, got {interp!r}")
    return check_slopes(slopes)


def _new_maps(B: int, H: int, W: int, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """disparity, confidence and index [B, H, W], for an entry point to fill."""
    return tuple(torch.empty(B, H, W, dtype=t, device=device) for t in (torch.float32, torch.float32, torch.int32))


def _result(kind: str, maps, aif, cost, *occ):
    """The maps, image and volume [B, ...] of an entry point in the layout of the caller's input (``refocus._as_given``), as a
    DisparityResult, or with occ = (subset, subsets_kept) as an OcclusionDisparityResult."""
    fields = [_as_given(kind, t) for t in maps] + [_as_given(kind, aif, image=True), _as_given(kind, cost)]
    return OcclusionDisparityResult(*fields, _as_given(kind, occ[0]), occ[1]) if occ else DisparityResult(*fields)


def _sweep(lf, slopes, angRes, aperture, interp, radius, all_in_focus, cost_volume, aif_dtype, centre, occlusion=None, choice_volume: bool = False):
    """One plane sweep and its selection: one call of lft_disparity, or with `occlusion` of lft_disparity_occ.  Returns (the
    result, the choice volume uint8 [D, H, W] ([B, D, H, W] for a batch) when asked for, else None)."""
    sl, how = (), None

    def sweep_arguments():                  # radius, interp, slopes and occlusion are refused before a tensor off the GPU
        nonlocal sl, how
        sl = _sweep_arguments(radius, interp, slopes)
        how = None if occlusion is None else _occlusion_arguments(occlusion)

    B, A, H, W, C, strides, kind = _field(lf, angRes, "aif_dtype", aif_dtype, before_device=sweep_arguments)
    aif_dtype = lf.dtype if aif_dtype is None else aif_dtype
    dev, D = lf.device, len(sl)
    table = _device_table(A, sl, aperture, interp, dev, centre)
    maps = _new_maps(B, H, W, dev)
    cost = torch.empty(B, D, H, W, dtype=torch.float32, device=dev) if cost_volume else None
    aif = torch.empty(B, H, W, C, dtype=aif_dtype, device=dev) if all_in_focus else None
    name, with_subsets, with_subset, occ, choice = "lft_disparity", (), (), (), None
    if how is not None:
        subsets, margin, min_views = how
        btable, kept = _device_subsets(A, aperture, centre, subsets, min_views, dev)
        subset = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
        choice = torch.empty(B, D, H, W, dtype=torch.uint8, device=dev) if choice_volume else None
        # lft_disparity_occ takes lft_disparity's arguments with (subsets, P, beta) after the table and (subset, choice) after the index
        name, with_subsets = "lft_disparity_occ", (btable.data_ptr(), len(kept), margin)
        with_subset, occ = (subset.data_ptr(), choice.data_ptr() if choice_volume else None), (subset, kept)
    if B and H and W:
        scratch = _device_scratch(_scratch, name + "_scratch_bytes", (B, D, H, W, C, _lib.DISPARITY_AIF if all_in_focus else 0), dev)
        _lib.enqueue(name, dev, lf.data_ptr(), _CLASS[lf.dtype], B, A, H, W, C, strides, table.data_ptr(), *with_subsets,
                     _device_slopes(sl, dev).data_ptr(), D, TAPS[interp], int(radius), scratch.data_ptr(), *(t.data_ptr() for t in maps), *with_subset,
                     cost.data_ptr() if cost_volume else None, aif.data_ptr() if all_in_focus else None, _CLASS[aif_dtype])
    return _result(kind, maps, aif, cost, *occ), _as_given(kind, choice)


def occlusion_volume(lf: torch.Tensor, slopes: Sequence[float], angRes: Optional[int] = None, aperture: Aperture = "full",
                     interp: str = "linear", centre=None, occlusion="halves") -> torch.Tensor:
    """The whole `choice` volume of ``disparity(..., occlusion=occlusion)``, uint8 [D, H, W] ([B, D, H, W] for a batch): per pixel
    and slope 0 where the whole aperture set the raw cost V, else the kept subset (1-based) that did.  It does not depend on the
    aggregation radius."""
    return _sweep(lf, slopes, angRes, aperture, interp, 0, False, False, None, centre, occlusion, choice_volume=True)[1]


def disparity(lf: torch.Tensor, slopes: Sequence[float], angRes: Optional[int] = None, aperture: Aperture = "full",
              interp: str = "linear", radius: int = 2, all_in_focus: Union[bool, str] = False, cost_volume: bool = False,
              aif_dtype=None, centre=None, regularize: Optional[dict] = None, occlusion=None) -> DisparityResult:
    """The disparity map of a light field on the GPU, on lf's device and current stream (enqueue only).

      views  [A, A, H, W, C] (C <= 4) or [A, A, H, W]   ->  maps [H, W], all_in_focus [H, W, C] or [H, W], cost [D, H, W]
      mosaic [A*H, A*W] with angRes                       ->  maps [H, W], all_in_focus [H, W], cost [D, H, W]
      batch  [B, 1, A*H, A*W] with angRes                 ->  maps [B, H, W], all_in_focus [B, H, W], cost [B, D, H, W]

    Layouts, strides, input classes, aperture and interp are ``refocus.refocus``'s.  radius: the aggregation window is
    (2 radius + 1)^2, 0 .. 8.  all_in_focus: also return the refocus stack gathered at the index, as aif_dtype (default: the
    input's; torch.float32 is the unclipped sum, torch.uint8 clips, scales and rounds half to even).  cost_volume: also return E.
    centre: the angular position (cu, cv) the sweep is seen from (``refocus.shift_table``), default the centre of the views: the
    map then belongs to that position, and all_in_focus is the plane-sweep rendering of a view there.
    regularize: None, or dict(p1=, p2=, paths=8, guide=None, edge_gain=0.0): sweep with the cost volume, then ``regularize`` it with
    these arguments and select from S (cost is then S); all_in_focus gathers from ``refocus.refocus``'s fp32 stack, which is the
    sweep's m bit for bit.
    occlusion: None, "halves", "quadrants" or dict(subsets="halves" | "quadrants" | a boolean array [P, A, A], margin=2.0,
    min_views=2): the occlusion-aware cost of the module docstring (one call of lft_disparity_occ in the sweep's place).  The
    result is then an ``OcclusionDisparityResult``, DisparityResult's fields and then `subset` and `subsets_kept`: `subset` is 0
    where the whole aperture set the cost at the index and else the kept subset (1-based) that did, `subsets_kept` says which of
    the given subsets those ids stand for; with regularize, SGM runs on the new E and `subset` is the choice volume gathered at
    SGM's index.  Without it nothing changes (the five-field result answers None for both names): the same launches, the same bits.
    all_in_focus="subset" (it needs occlusion): the image is ``all_in_focus_at`` of this call's index and subset, the mean of the
    winning subset's views and not of all of them; the sweep then keeps no stack (with regularize no stack is computed either), and
    every other field has the bits of the same call with all_in_focus=True."""
    if isinstance(all_in_focus, str):
        if all_in_focus != "subset":
            raise LftError(f"all_in_focus must be False, True or subset, got {all_in_focus!r}")
        if occlusion is None:
            raise LftError("all_in_focus = subset needs occlusion: the image is rendered from the subset that set the cost")
        res = disparity(lf, slopes, angRes, aperture, interp, radius, False, cost_volume, aif_dtype, centre, regularize, occlusion)
        image = all_in_focus_at(lf, slopes, res.index, res.subset, angRes, aperture, interp, centre, occlusion, aif_dtype)
        return res._replace(all_in_focus=image)
    if regularize is not None:
        return _sweep_and_regularize(lf, slopes, angRes, aperture, interp, radius, all_in_focus, cost_volume, aif_dtype, centre, regularize, occlusion)
    return _sweep(lf, slopes, angRes, aperture, interp, radius, all_in_focus, cost_volume, aif_dtype, centre, occlusion)[0]


def penalties_from_cost(cost: torch.Tensor, p1_rel: float = 0.1, p2_rel: float = 1.0) -> Tuple[float, float]:
    """(p1, p2) for ``regularize`` as multiples of the mean of `cost`.  It reads the mean back from the device: it synchronises.
    The defaults are a starting point, nobody has tuned them."""
    if not isinstance(cost, torch.Tensor):
        raise LftError(f"the cost must be a torch tensor, got {type(cost).__name__}")
    if not (np.isfinite(p1_rel) and np.isfinite(p2_rel) and 0 <= p1_rel <= p2_rel):
        raise LftError(f"p1_rel and p2_rel must be finite with 0 <= p1_rel <= p2_rel, got {p1_rel!r}, {p2_rel!r}")
    mean = float(cost.mean(dtype=torch.float64)) if cost.numel() else 0.0
    return float(p1_rel) * mean, float(p2_rel) * mean


def _sgm_arguments(D: Optional[int], slopes, p1, p2, paths, edge_gain, has_guide: bool, aif_dtype, has_stack: bool) -> Tuple[float, ...]:
    """The refusals of ``regularize`` that need no tensor (D: the slices of the cost volume, None before it exists); returns the
    checked slopes."""
    if isinstance(paths, bool) or paths not in (4, 8):
        raise LftError(f"paths must be 4 or 8, got {paths!r}")
    for name, v in (("p1", p1), ("p2", p2), ("edge_gain", edge_gain)):
        _finite_number(name, v, 0)
    if np.float32(p2) < np.float32(p1):
        raise LftError(f"p2 must not be below p1, got p1 = {p1!r}, p2 = {p2!r}")
    if np.float32(edge_gain) > 0 and not has_guide:
        raise LftError(f"edge_gain {edge_gain!r} needs a guide")
    if aif_dtype is not None and aif_dtype not in _CLASS:
        raise LftError(f"aif_dtype must be torch.uint8 or torch.float32, got {aif_dtype}")
    if aif_dtype is not None and not has_stack:
        raise LftError("aif_dtype without a stack: the all-in-focus image is gathered from one")
    sl = check_slopes(slopes)
    if D is not None and len(sl) != D:
        raise LftError(f"{len(sl)} slopes for a cost volume of {D} slices")
    if len(sl) > _lib.SGM_MAX_D:
        raise LftError(f"{len(sl)} slopes: regularize takes at most {_lib.SGM_MAX_D}")
    return sl


def regularize(cost: torch.Tensor, slopes: Sequence[float], p1: float, p2: float, paths: int = 8, guide: Optional[torch.Tensor] = None,
               edge_gain: float = 0.0, stack: Optional[torch.Tensor] = None, aif_dtype=None, aggregated: bool = False) -> DisparityResult:
    """Semi-global aggregation of a cost volume and the selection from it (the module docstring has the definition), on cost's
    device and current stream (enqueue only).

      cost [D, H, W]     ->  maps [H, W];     guide [H, W];     stack [D, H, W] or [D, H, W, C]        ->  all_in_focus [H, W] or [H, W, C]
      cost [B, D, H, W]  ->  maps [B, H, W];  guide [B, H, W];  stack [B, D, H, W] or [B, D, H, W, C]  ->  all_in_focus [B, H, W(, C)]

    cost, guide and stack are float32.  p1 <= p2 are the penalties of a step of one slope and of a larger jump along a path
    (``penalties_from_cost``); with a guide, p2 falls by edge_gain times the guide's step, not below p1.  paths: 4 or 8.  stack:
    what all_in_focus is gathered from at the index (``refocus.refocus``'s fp32 stack), as aif_dtype (default torch.float32).
    aggregated: DisparityResult.cost holds S."""
    if not isinstance(cost, torch.Tensor):
        raise LftError(f"the cost must be a torch tensor, got {type(cost).__name__}")
    if cost.dtype != torch.float32 or cost.dim() not in (3, 4):
        raise LftError(f"the cost must be float32 [D, H, W] or [B, D, H, W], got {cost.dtype} {tuple(cost.shape)}")
    batch = cost.dim() == 4
    B, D, H, W = (int(n) for n in (cost.shape if batch else (1,) + tuple(cost.shape)))
    if D < 1:
        raise LftError(f"a cost volume of {D} slices")
    sl = _sgm_arguments(D, slopes, p1, p2, paths, edge_gain, guide is not None, aif_dtype, stack is not None)
    lead = (B,) if batch else ()
    for name, t, shapes in (("guide", guide, [lead + (H, W)]), ("stack", stack, [lead + (D, H, W)] + [lead + (D, H, W, c) for c in (1, 2, 3, 4)])):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) not in shapes:
            raise LftError(f"the {name} must be a float32 tensor of shape {' or '.join(str(list(x)) for x in shapes[:2])}, got "
                           f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")
        if t.device != cost.device:
            raise LftError(f"the {name} is on {t.device}, the cost on {cost.device}")
    if cost.device.type != "cuda":
        raise LftError(f"the cost must be on the GPU, got a tensor on {cost.device} (there is no CPU path)")
    dev = cost.device
    channels = stack is not None and stack.dim() == cost.dim() + 1
    C = int(stack.shape[-1]) if channels else 1
    aif_dtype = torch.float32 if aif_dtype is None else aif_dtype
    maps = _new_maps(B, H, W, dev)
    S = torch.empty(B, D, H, W, dtype=torch.float32, device=dev) if aggregated else None
    aif = torch.empty(B, H, W, C, dtype=aif_dtype, device=dev) if stack is not None else None
    if B and H and W:
        cost, guide, stack = (None if t is None else t.contiguous() for t in (cost, guide, stack))
        scratch = _device_scratch(_scratch, "lft_sgm_scratch_bytes", (B, D, H, W, int(paths)), dev)
        _lib.enqueue("lft_sgm", dev, cost.data_ptr(), B, D, H, W, C, _device_slopes(sl, dev).data_ptr(), int(paths), float(p1), float(p2),
                     None if guide is None else guide.data_ptr(), float(edge_gain), None if stack is None else stack.data_ptr(),
                     scratch.data_ptr(), *(t.data_ptr() for t in maps), None if S is None else S.data_ptr(),
                     None if aif is None else aif.data_ptr(), _CLASS[aif_dtype])
    return _result(("batch" if batch else "views") + ("5" if channels else "4"), maps, aif, S)


_SGM_KEYS = ("p1", "p2", "paths", "guide", "edge_gain")


def _sweep_and_regularize(lf, slopes, angRes, aperture, interp, radius, all_in_focus, cost_volume, aif_dtype, centre, how, occlusion=None) -> DisparityResult:
    """``disparity`` with regularize=how: the sweep's E, refocus's stack when all_in_focus, then ``regularize``.  With occlusion
    the sweep is lft_disparity_occ's, and `subset` its choice volume gathered at the regularized index (lft_occ_gather)."""
    from . import refocus as Rf
    if not isinstance(how, dict) or set(how) - set(_SGM_KEYS) or not {"p1", "p2"} <= set(how):
        raise LftError(f"regularize must be None or a dict with p1, p2 and any of paths, guide, edge_gain, got {how!r}")
    _sgm_arguments(None, slopes, how["p1"], how["p2"], how.get("paths", 8), how.get("edge_gain", 0.0), how.get("guide") is not None, None, False)
    # aif_dtype goes along for its refusal only: the sweep gathers no image here
    swept, choice = _sweep(lf, slopes, angRes, aperture, interp, radius, False, True, aif_dtype, centre, occlusion, choice_volume=occlusion is not None)
    stack = Rf.refocus(lf, slopes, angRes, aperture, interp, out_dtype=torch.float32, centre=centre) if all_in_focus else None
    res = regularize(swept.cost, slopes, stack=stack, aif_dtype=(aif_dtype or lf.dtype) if all_in_focus else None, aggregated=cost_volume, **how)
    if choice is None:
        return res
    return OcclusionDisparityResult(*res, gather_choice(res.index, choice), swept.subsets_kept)


def gather_choice(index: torch.Tensor, choice: torch.Tensor) -> torch.Tensor:
    """subset[..., y, x] = choice[..., index[..., y, x], y, x] on the GPU (lft_occ_gather, enqueue only): index int32 [H, W] or
    [B, H, W], choice uint8 [D, H, W] or [B, D, H, W]; an index outside 0 .. D-1 is clamped into it."""
    for name, t, dtype in (("index", index, torch.int32), ("choice", choice, torch.uint8)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise LftError(f"the {name} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    batch = index.dim() == 3
    if index.dim() not in (2, 3) or choice.dim() != index.dim() + 1 or choice.shape[-2:] != index.shape[-2:] or choice.shape[:-3] != index.shape[:-2] \
            or choice.shape[-3] < 1:
        raise LftError(f"an index of {tuple(index.shape)} does not gather from a choice volume of {tuple(choice.shape)}")
    if index.device.type != "cuda" or choice.device != index.device:
        raise LftError(f"the index and the choice volume must be on one GPU, got {index.device} and {choice.device} (there is no CPU path)")
    B, D, H, W = (int(n) for n in (choice.shape if batch else (1,) + tuple(choice.shape)))
    index, choice = index.contiguous(), choice.contiguous()
    subset = torch.empty(index.shape, dtype=torch.uint8, device=index.device)
    if B and H and W:
        _lib.enqueue("lft_occ_gather", index.device, index.data_ptr(), choice.data_ptr(), B, D, H, W, subset.data_ptr())
    return subset


def all_in_focus_at(lf: torch.Tensor, slopes: Sequence[float], index: torch.Tensor, subset: Optional[torch.Tensor] = None,
                    angRes: Optional[int] = None, aperture: Aperture = "full", interp: str = "linear", centre=None, occlusion=None,
                    out_dtype=None) -> torch.Tensor:
    """The all-in-focus image at a given index map, each pixel the mean of the views of its subset (the module docstring has the
    definition), on lf's device and current stream (one launch of lft_aif_at, enqueue only).

      views  [A, A, H, W, C] (C <= 4) or [A, A, H, W]   index, subset [H, W]     ->  [H, W, C] or [H, W]
      mosaic [A*H, A*W] with angRes                       index, subset [H, W]     ->  [H, W]
      batch  [B, 1, A*H, A*W] with angRes                 index, subset [B, H, W]  ->  [B, H, W]

    Layouts, strides, input classes, slopes, aperture, interp and centre are ``disparity``'s.  index: int32, k per pixel, clamped
    into 0 .. D-1.  subset: None (the whole aperture everywhere), or uint8 of index's shape: 0 the whole aperture, p >= 1 the p-th
    kept subset of `occlusion` ("halves", "quadrants" or a dict with subsets / min_views, as for ``disparity``; ids are positions
    in the kept list, and an id above their number counts as 0).  A subset map without occlusion is refused.  out_dtype (default:
    the input's) is torch.float32, the unclipped sum, or torch.uint8: clip to [0, 1], * 255, round half to even.  With the index
    and subset of ``disparity(..., occlusion=)`` this is the image of ``all_in_focus="subset"``."""
    sl, how = (), None

    def arguments():                        # everything that needs no device, the maps' shapes included
        nonlocal sl, how
        sl = _sweep_arguments(0, interp, slopes)
        how = None if occlusion is None else _occlusion_arguments(occlusion)
        if subset is not None and how is None:
            raise LftError("a subset map needs occlusion: it says which subsets the ids stand for")
        B, _, H, W, _, _, kind = _layout(lf, angRes)
        shape = (B, H, W) if kind.startswith("batch") else (H, W)
        for name, t, dtype in (("index", index, torch.int32), ("subset", subset, torch.uint8)):
            if t is None and name == "subset":
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape:
                raise LftError(f"the {name} must be a {dtype} tensor of shape {list(shape)}, got {getattr(t, 'dtype', type(t).__name__)} "
                               f"{tuple(getattr(t, 'shape', ()))}")
            if t.device != lf.device:
                raise LftError(f"the {name} is on {t.device}, the light field on {lf.device}")

    B, A, H, W, C, strides, kind = _field(lf, angRes, "out_dtype", out_dtype, before_device=arguments)
    out_dtype = lf.dtype if out_dtype is None else out_dtype
    dev = lf.device
    table = _device_table(A, sl, aperture, interp, dev, centre)
    btable, kept = _device_subsets(A, aperture, centre, how[0], how[2], dev) if how is not None else (None, ())
    aif = torch.empty(B, H, W, C, dtype=out_dtype, device=dev)
    if B and H and W:
        index = index.contiguous()
        subset = None if subset is None else subset.contiguous()
        _lib.enqueue("lft_aif_at", dev, lf.data_ptr(), _CLASS[lf.dtype], B, A, H, W, C, strides, table.data_ptr(), len(sl),
                     None if btable is None else btable.data_ptr(), len(kept), index.data_ptr(), None if subset is None else subset.data_ptr(),
                     TAPS[interp], aif.data_ptr(), _CLASS[out_dtype])
    return _as_given(kind, aif, image=True)


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
