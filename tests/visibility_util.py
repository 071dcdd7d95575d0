"""The per-view visibility test of view synthesis (lft_amd/views.py, "Visibility") restated in numpy: the mask and the count in
float32, comparison for comparison, so that `visible` compares exactly; the render in fp64 with that mask, from the float32
coordinates, as tests/views_util.py:render_np does for the plain definition."""
import numpy as np

from lft_amd import views as V

import views_util as VU

F = np.float32


def warp_np(Dr, A, d_range, reference=None, near="larger", fill=32):
    """Dv fp32 [A, A, H, W]: Dr splatted and filled to the A x A integer positions, as ``render`` does by default."""
    deltas = V.target_deltas(A, [(u, v) for u in range(A) for v in range(A)], reference)
    maps = [VU.fill_np(VU.splat_np(Dr, d, d_range, near), Dr, d_range, near, fill)[0] for d in deltas]
    return np.stack(maps).reshape(A, A, *Dr.shape)


def _footprint(s, n):
    """The two clamped indices of one axis: floor(s), and floor(s) + 1 unless s is integral."""
    fl = np.floor(s)
    i = np.clip(fl, -4, n + 4).astype(np.int64)
    return np.clip(i, 0, n - 1), np.clip(np.where(s != fl, i + 1, i), 0, n - 1)


def classes_np(Dt, records, Dv, tau, near="larger"):
    """Dt fp32 [H, W], records [A*A], Dv fp32 [A, A, H, W] -> (used [V] view numbers of non-zero weight, inside bool [V, H, W],
    visible bool [V, H, W], count uint8 [H, W])."""
    A, _, H, W = Dv.shape
    thr = (Dt + F(tau)).astype(F) if near == "larger" else (Dt - F(tau)).astype(F)
    used, inside, visible = [], [], []
    for n, r in enumerate(records):
        if r["skip"]:
            continue
        sy, sx, ins = VU.coords_np(Dt, r)
        q = Dv[n // A, n % A]
        occ = np.zeros((H, W), bool)
        for iy in _footprint(sy, H):
            for ix in _footprint(sx, W):
                v = q[iy, ix]
                with np.errstate(invalid="ignore"):
                    occ |= np.isfinite(v) & ((v > thr) if near == "larger" else (v < thr))
        used.append(n)
        inside.append(ins)
        visible.append(ins & ~occ)
    inside, visible = np.stack(inside), np.stack(visible)
    return np.array(used), inside, visible, np.minimum(visible.sum(0), 255).astype(np.uint8)


def render_np(views, Dt, records, taps, Dv, tau, near="larger"):
    """(fp64 [H, W, C], count uint8 [H, W], class int [H, W]: 0 visible, 1 inside, 2 all): views_util.render_np over the first
    non-empty class."""
    A, _, H, W, C = views.shape
    X = VU.as_fp64(views)
    used, inside, visible, count = classes_np(Dt, records, Dv, tau, near)
    cls = np.where(visible.any(0), 0, np.where(inside.any(0), 1, 2))
    num, den = np.zeros((H, W, C)), np.zeros((H, W))
    for k, n in enumerate(used):
        r = records[n]
        sy, sx, _ = VU.coords_np(Dt, r)
        s = VU.sample_np(X[n // A, n % A], sy, sx, taps)
        member = np.where(cls == 0, visible[k], np.where(cls == 1, inside[k], True))
        w = float(r["w"])
        num += np.where(member[..., None], w * s, 0.0)
        den += np.where(member, w, 0.0)
    return num / den[..., None], count, cls
