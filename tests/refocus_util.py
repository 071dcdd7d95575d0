"""The refocus definition restated in fp64 numpy, and the tolerance the GPU tests hold the kernel to.

  R_d[y, x, c] = sum_{u,v} a[u,v] * S(L[u,v,:,:,c], y + d*(u-uc), x + d*(v-uc))

S separable, rows then columns, tap indices clamped into the view.  ``refocus_np`` takes the fp32-rounded table of
lft_amd.refocus.shift_table as fp64, so only the GPU's fp32 accumulation (and its x / 255 of uint8 input) separates the two."""
import numpy as np

SLOPES = [-2.5, -1.0, -0.3, 0.0, 0.75, 2.0, 40.0]       # slope 40 shifts every off-centre view out of it: all taps clamp


def refocus_np(views, table, taps):
    """views [A, A, H, W, C] (uint8: scaled by / 255; floats as stored), table [D, A*A] of lft_amd.refocus.RECORD -> fp64 [D, H, W, C]."""
    A, _, H, W, C = views.shape
    x = views.astype(np.float64) / 255.0 if views.dtype == np.uint8 else views.astype(np.float64)
    D = table.shape[0]
    out = np.zeros((D, H, W, C), dtype=np.float64)
    ys, xs = np.arange(H), np.arange(W)
    for d in range(D):
        for u in range(A):
            for v in range(A):
                r = table[d, u * A + v]
                if r["skip"]:
                    continue
                rows = np.zeros((H, W, C), dtype=np.float64)
                for k in range(taps):
                    rows += float(r["wy"][k]) * x[u, v][np.clip(ys + int(r["oy"]) + k, 0, H - 1)]
                s = np.zeros((H, W, C), dtype=np.float64)
                for k in range(taps):
                    s += float(r["wx"][k]) * rows[:, np.clip(xs + int(r["ox"]) + k, 0, W - 1)]
                out[d] += float(r["a"]) * s
    return out


def abs_sum(table, taps):
    """S: the largest 1-D sum |tap weight| of the table (1 for nearest and linear, at most 1.25 for cubic)."""
    return float(max(np.abs(table["wy"][..., :taps].astype(np.float64)).sum(-1).max(),
                     np.abs(table["wx"][..., :taps].astype(np.float64)).sum(-1).max()))


def tol(A, table, taps, max_abs):
    """(A^2 + 16) * 2^-23 * S^2 * max|x|: A^2 + 16 bounds the depth of any summation order (4 row taps, 4 column taps, the
    aperture product, A^2 accumulations)."""
    return (A * A + 16) * 2.0 ** -23 * abs_sum(table, taps) ** 2 * max_abs


def quantise(ref):
    """convertDouble2Byte: clip to [0, 1], * 255, round half to even."""
    return np.rint(255.0 * np.clip(ref, 0.0, 1.0)).astype(np.uint8)


def tie_distance(ref):
    """Distance of 255 * ref from the nearest half-integer."""
    z = 255.0 * ref
    return np.abs(z - np.floor(z) - 0.5)


def plane(A, H, W, d0):
    """The Lambertian plane L[u,v,y,x] = f(y - d0*(u-uc), x - d0*(v-uc)) as fp32 views [A, A, H, W], and f on the pixel grid
    (fp64), f a smooth product of sinusoids in [0, 1]."""
    def f(y, x):
        return 0.5 + 0.5 * np.sin(0.45 * y + 0.3) * np.cos(0.37 * x - 0.2)
    uc = (A - 1) / 2
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    L = np.zeros((A, A, H, W), dtype=np.float64)
    for u in range(A):
        for v in range(A):
            L[u, v] = f(y - d0 * (u - uc), x - d0 * (v - uc))
    return L.astype(np.float32), f(y, x)


def user_aperture(A, seed):
    """A random [A, A] aperture with zeros (at least one view kept)."""
    rng = np.random.default_rng(seed)
    a = rng.random((A, A)) * (rng.random((A, A)) < 0.6)
    a[A // 2, A // 2] = max(a[A // 2, A // 2], 0.25)
    return a
