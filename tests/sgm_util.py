"""The semi-global aggregation of lft_sgm (lft_amd/disparity.py has the definition) restated in numpy float32, operation for
operation, and the constant-patch scene on which winner-take-all fails.

``sgm_np`` treats all lines of a direction at once: it iterates y (x for the horizontal pair) and takes a whole row of lines per
step, so every operation is one float32 numpy operation on a [D, N] array, rounded once as the kernel's."""
import numpy as np

DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1))          # (dy, dx), the definition's order
F = np.float32


def _step(E, Lq, valid, p1, p2, gain, gp, gq):
    """L_r(p, .) [D, N] from E(p, .), L_r(q, .) and, with a guide, g(p) and g(q) [N]; valid [N]: q lies inside the image."""
    D = E.shape[0]
    M = Lq.min(axis=0)
    p2e = p2 if gp is None else np.maximum(p1, p2 - gain * np.abs(gp - gq))
    c = M + p2e
    lo, hi = np.full_like(Lq, np.inf), np.full_like(Lq, np.inf)
    lo[1:], hi[:-1] = Lq[:-1], Lq[1:]
    t = np.minimum(Lq, c[None])
    if D > 1:
        t = np.minimum(t, np.minimum(lo, hi) + p1)
    return np.where(valid[None], E + (t - M[None]), E).astype(F)


def path_np(E, r, p1, p2, guide=None, gain=0.0):
    """L_r [D, H, W] of E [D, H, W] (float32) for the direction r = (dy, dx)."""
    E = np.ascontiguousarray(E, dtype=F)
    p1, p2, gain = F(p1), F(p2), F(gain)
    g = None if guide is None else np.asarray(guide, dtype=F)
    D, H, W = E.shape
    dy, dx = r
    L = np.empty_like(E)
    with np.errstate(invalid="ignore"):
        if dy == 0:
            xs = range(W) if dx > 0 else range(W - 1, -1, -1)
            for n, x in enumerate(xs):
                if n == 0:
                    L[:, :, x] = E[:, :, x]
                else:
                    q = x - dx
                    L[:, :, x] = _step(E[:, :, x], L[:, :, q], np.ones(H, bool), p1, p2, gain, None if g is None else g[:, x], None if g is None else g[:, q])
            return L
        ys = range(H) if dy > 0 else range(H - 1, -1, -1)
        x = np.arange(W)
        src = np.clip(x - dx, 0, W - 1)
        inside = (x - dx >= 0) & (x - dx < W)
        for n, y in enumerate(ys):
            if n == 0:
                L[:, y] = E[:, y]
            else:
                L[:, y] = _step(E[:, y], L[:, y - dy][:, src], inside, p1, p2, gain, None if g is None else g[y], None if g is None else g[y - dy][src])
    return L


def sgm_np(E, p1, p2, paths, guide=None, gain=0):
    """S [D, H, W] (float32) of E [D, H, W]: the `paths` (4 or 8) volumes L_r added in direction order, times fl(1 / paths)."""
    assert paths in (4, 8)
    S = path_np(E, DIRECTIONS[0], p1, p2, guide, gain)
    for r in DIRECTIONS[1:paths]:
        S = S + path_np(E, r, p1, p2, guide, gain)
    return (S * F(1.0 / paths)).astype(F)


def clamp_bites(guide, r, p1, p2, gain):
    """(steps along r where P2 - gain |dg| falls below P1, steps where it does not), over the steps with q inside the image."""
    g = np.asarray(guide, dtype=F)
    H, W = g.shape
    dy, dx = r
    p = g[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)]
    q = g[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
    low = F(p2) - F(gain) * np.abs(p - q) < F(p1)
    return int(low.sum()), int((~low).sum())


# The constant-patch scene: a fronto-parallel plane at slope 1 with random texture and a constant 14 x 14 patch.
A, N, PATCH, D_PLANE = 5, 48, (17, 31), 1.0
SLOPES = np.linspace(-2.0, 2.0, 9)
K_PLANE = 6                                                                       # SLOPES[6] == 1.0
PATCH_INTERIOR = (slice(19, 29), slice(19, 29))                                   # the 3 x 3 windows of slopes 0.5 .. 1.5 see the patch alone
TEXTURE_INTERIOR = (slice(8, -8), slice(8, -8))
PENALTIES = ((0.5, 4.0), (0.1, 1.0), (0.02, 0.2))                                 # (p1, p2) as multiples of the mean cost


def patch_scene(seed=0):
    """fp32 views [A, A, N, N, 1]: view (u, v) shows the centre view displaced by D_PLANE * (u - uc, v - uc) whole pixels."""
    rng = np.random.default_rng(seed)
    uc, pad = (A - 1) // 2, 2 * ((A - 1) // 2)
    tex = rng.random((N + 2 * pad, N + 2 * pad)).astype(F)
    tex[pad + PATCH[0]:pad + PATCH[1], pad + PATCH[0]:pad + PATCH[1]] = 0.5
    L = np.zeros((A, A, N, N, 1), dtype=F)
    for u in range(A):
        for v in range(A):
            oy, ox = pad - int(D_PLANE) * (u - uc), pad - int(D_PLANE) * (v - uc)
            L[u, v, ..., 0] = tex[oy:oy + N, ox:ox + N]
    return L


def mask_of(region):
    m = np.zeros((N, N), bool)
    m[region] = True
    return m
