"""The occlusion-aware sweep cost (lft_amd/disparity.py, "Occlusion-aware cost from partial apertures") restated in fp64 numpy
from its definition: the subset table, V_full, the V_p, V = min(V_full, beta * min_p V_p) and choice.  Also the bound the GPU tests
hold E to, the masks of well-conditioned choices, and the noisy two-layer scene with its band.

``occ_cost_np`` takes the fp32-rounded tables (refocus.shift_table and the subset table) as fp64, so only the GPU's fp32 arithmetic
separates the two.

The bound ``tol_occ``.  V_p is V_full with the weights b_p in the place of a: the same sample, at most A^2 accumulations, the same
square and channel sum, weights >= 0 of sum 1 (within 2^-24 each, which the step counts of tol_E absorb).  So |V_p - V_p'| <=
tol_E' = C (3 A^2 + 66) 2^-23 S^4 X^2 (disparity_util.tol_E without the box sum's steps), and the same for V_full.  t = min_p V_p
is 1-Lipschitz in the sup norm, U = fl(beta t) adds one rounding of a product that is at most beta C S^4 X^2 (a variance of values
bounded by S^2 X is at most S^4 X^2 per channel), and V = min(V_full, U) is 1-Lipschitz again:
    |V - V'| <= max(1, beta) tol_E' + 2^-24 beta C S^4 X^2.
The box sum of E averages these errors and adds its own (2r+1)^2 steps on values <= max(1, beta) C S^4 X^2, which is what tol_E's
(2r+1)^2 term is, scaled by beta.  Together: tol_occ = max(1, beta) * tol_E(A, C, r, ...) + 2^-24 beta C S^4 X^2."""
import math

import numpy as np

import disparity_util as DU
import refocus_util as RU


def subset_table_np(A, a, centre, subsets, min_views=2):
    """(fp32 [P', A*A], kept ids) from the definition.  a: the fp64 aperture [A, A] of sum 1; centre: (cu, cv); subsets: "halves",
    "quadrants" or a boolean [P, A, A]."""
    cu, cv = centre
    masks = []
    if isinstance(subsets, str):
        for p in range(4):
            mk = np.zeros((A, A), bool)
            for u in range(A):
                for v in range(A):
                    du, dv = float(u) - cu, float(v) - cv
                    if subsets == "halves":
                        mk[u, v] = (du <= 0, du >= 0, dv <= 0, dv >= 0)[p]
                    else:
                        mk[u, v] = ((du <= 0) if p < 2 else (du >= 0)) and ((dv <= 0) if p % 2 == 0 else (dv >= 0))
            masks.append(mk)
    else:
        masks = [np.asarray(mk, bool) for mk in subsets]
    rows, kept = [], []
    for p, mk in enumerate(masks):
        if sum(1 for u in range(A) for v in range(A) if mk[u, v] and a[u, v] > 0) < min_views:
            continue
        W = math.fsum(a[u, v] for u in range(A) for v in range(A) if mk[u, v])
        rows.append([np.float32(a[u, v] / W) if mk[u, v] else np.float32(0) for u in range(A) for v in range(A)])
        kept.append(p)
    return np.array(rows, np.float32).reshape(len(kept), A * A), tuple(kept)


def occ_cost_np(views, table, taps, btable, beta):
    """views [A, A, H, W, C], table [D, A*A] of RECORD, btable fp32 [P', A*A], beta -> fp64 dict: V_full [D, H, W], Vp [P', D, H, W],
    U, V, choice (uint8 [D, H, W]) and m [D, H, W, C].  A view is a member of p iff btable[p, view] != 0 (and it is not skipped)."""
    shape = (table.shape[0],) + views.shape[2:]
    P = btable.shape[0]
    b = btable.astype(np.float64)
    beta = float(np.float32(beta))
    m, q = np.zeros(shape), np.zeros(shape)
    mp, qp = np.zeros((P,) + shape), np.zeros((P,) + shape)
    for d, n, a, s in DU.samples_np(views, table, taps):
        m[d] += a * s
        q[d] += a * s * s
        for p in range(P):
            if b[p, n] != 0:
                mp[p, d] += b[p, n] * s
                qp[p, d] += b[p, n] * s * s
    V_full = np.maximum(q - m * m, 0.0).sum(-1)
    Vp = np.maximum(qp - mp * mp, 0.0).sum(-1)
    t = Vp.min(0)
    U = beta * t
    choice = np.where(V_full <= U, 0, np.argmin(Vp, 0) + 1).astype(np.uint8)         # argmin: the first of equal minima
    return dict(V_full=V_full, Vp=Vp, U=U, V=np.minimum(V_full, U), choice=choice, m=m)


def tol_occ(A, C, radius, table, taps, max_abs, beta):
    """The bound of the module docstring on |E - E'| (radius 0: on |V - V'|)."""
    scale = RU.abs_sum(table, taps) ** 4 * max_abs ** 2
    return max(1.0, beta) * DU.tol_E(A, C, radius, table, taps, max_abs) + 2.0 ** -24 * beta * C * scale


def well_conditioned(o, tol):
    """Boolean [D, H, W]: where the restatement's choice cannot flip within `tol` on each side: |V_full - U| > 2 tol, and where a
    subset wins, its gap to the next subset (times nothing: the V_p themselves are within tol) > 2 tol too."""
    ok = np.abs(o["V_full"] - o["U"]) > 2 * tol
    if o["Vp"].shape[0] > 1:
        srt = np.sort(o["Vp"], 0)
        ok &= (o["choice"] == 0) | (srt[1] - srt[0] > 2 * tol)
    return ok


# ---- the noisy two-layer scene of the feature test ----
BOX = (12, 28, 12, 28)
SCENE = dict(A=5, H=40, W=40, radius=1, interp="linear", beta=2.0, subsets="halves")
SLOPES = [float(s) for s in np.linspace(-2.0, 2.0, 9)]
K_BG, K_FG = 2, 6                        # the indices of the slopes -1 (background) and +1 (foreground)


def noisy_two_layer():
    """fp32 views [5, 5, 40, 40, 1]: disparity_util.two_layer with the box above plus 0.02 N(0, 1) per view from default_rng(7)."""
    L, _ = DU.two_layer(5, 40, 40, box=BOX)
    return (L + 0.02 * np.random.default_rng(7).standard_normal(L.shape)).astype(np.float32)


def band(A=5, H=40, W=40, box=BOX, d_bg=-1.0, d_fg=1.0):
    """Boolean [H, W]: the background pixels within the rectangle's reach ceil(|d_fg - d_bg| uc) outside the box (320 of them for
    the scene above); they lie away from the border by more than the sweep's largest shift."""
    reach = int(np.ceil(abs(d_fg - d_bg) * (A - 1) / 2))
    y0, y1, x0, x1 = box
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    inside = (yy >= y0) & (yy < y1) & (xx >= x0) & (xx < x1)
    grown = (yy >= y0 - reach) & (yy < y1 + reach) & (xx >= x0 - reach) & (xx < x1 + reach)
    assert y0 - reach > 0 and x0 - reach > 0 and y1 + reach < H and x1 + reach < W
    return grown & ~inside


def interior(A=5, H=40, W=40, radius=1, max_slope=2.0):
    """Boolean [H, W]: the pixels away from the border by the sweep's largest shift, the window and two more (the margin of
    disparity_util.two_layer_interiors)."""
    edge = int(np.ceil(max_slope * (A - 1) / 2)) + radius + 2
    inner = np.zeros((H, W), bool)
    inner[edge:H - edge, edge:W - edge] = True
    return inner
