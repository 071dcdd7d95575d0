"""The all-in-focus image from the winning partial aperture (lft_amd/disparity.py, "All-in-focus image from the winning partial
aperture") restated in fp64 numpy from its definition.

``aif_at_np`` takes the fp32-rounded tables (refocus.shift_table and the subset table) as fp64, so only the GPU's fp32 arithmetic
(and its x / 255 of uint8 input) separates the two.  A pixel's value is a refocus value with other weights of sum 1 (within 2^-24
each), so refocus_util.tol bounds the difference."""
import numpy as np

import disparity_util as DU
from lft_amd import refocus as R


def aif_at_np(views, table, taps, btable, index, subset):
    """views [A, A, H, W, C], table [D, A*A] of RECORD, btable fp32 [P, A*A] or None (P = 0), index int [H, W], subset uint8 [H, W]
    or None -> fp64 [H, W, C].  Per pixel: k = the index clamped into 0 .. D-1, p = the id (None and ids above P count as 0); the
    sum over the views in (u, v) order of w_n * s, w_n the record's a (p = 0) or b_p[n] (p >= 1), a view skipped iff the record's
    skip is set or, for p >= 1, b_p[n] == 0."""
    D = table.shape[0]
    H, W, C = views.shape[2:]
    P = 0 if btable is None else btable.shape[0]
    k = np.clip(np.asarray(index).astype(np.int64), 0, D - 1)
    p = np.zeros((H, W), np.int64) if subset is None else np.asarray(subset).astype(np.int64)
    p = np.where(p > P, 0, p)
    out = np.zeros((H, W, C))
    for d, n, a, s in DU.samples_np(views, table, taps):
        at = k == d
        if not at.any():
            continue
        w = np.where(p == 0, a, 0.0)
        for q in range(1, P + 1):
            w = np.where(p == q, float(btable[q - 1, n]), w)
        out += np.where(at, w, 0.0)[..., None] * s
    return out


def masked_table(table, b):
    """`table` with the a / skip columns b / b == 0: the table lft_refocus would run with for the aperture a * mask_p."""
    t = table.copy()
    t["a"] = np.asarray(b, np.float32)[None, :]
    t["skip"] = (t["a"] == 0).astype(np.int32)
    return t


def subset_masks(A, centre, subsets):
    """Boolean [P, A, A] of "halves" / "quadrants" at `centre` (None: the middle), or the array itself."""
    if not isinstance(subsets, str):
        return np.asarray(subsets, bool)
    cu, cv = R._centre(A, centre)
    du = np.broadcast_to((np.arange(A, dtype=np.float64) - cu)[:, None], (A, A))
    dv = np.broadcast_to((np.arange(A, dtype=np.float64) - cv)[None, :], (A, A))
    lo_u, hi_u, lo_v, hi_v = du <= 0, du >= 0, dv <= 0, dv >= 0
    return np.stack([lo_u, hi_u, lo_v, hi_v] if subsets == "halves" else [lo_u & lo_v, lo_u & hi_v, hi_u & lo_v, hi_u & hi_v])
