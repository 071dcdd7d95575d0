"""Windowed blending of overlapping SR patches (lft_amd/scene.py has the definition) restated in numpy float32: the same order of
the sum and one rounding per operation, so the GPU is compared bit for bit.  The restatement goes the other way round from the
kernel: it walks every patch pixel forwards to the scene pixel it shows (a scatter in ascending patch order) where the kernel
gathers a pixel's candidates, so the kernel's candidate range is checked, not repeated.  The window builders are restated too."""
import numpy as np

import shear_util as SU

WINDOWS = ("hann", "linear", "flat")
EPS = 2.0 ** -24


def window_np(kind, pz):
    """fp64, rounded once to fp32."""
    i = np.arange(pz, dtype=np.float64)
    if kind == "hann":
        w = np.sin(np.pi * (i + 0.5) / pz) ** 2
    elif kind == "linear":
        w = np.minimum(i + 0.5, pz - i - 0.5) * 2.0 / pz
    else:
        assert kind == "flat"
        w = np.ones(pz)
    return w.astype(np.float32)


def _maps(A, h0, w0, patch, stride, s, k):
    """For every patch n: (Y [A, pz], okY, X [A, pz], okX): the scene pixel that pixel a (b) of view u (v) shows, and whether it is
    inside the view."""
    nu, nv = SU.counts_np(h0, w0, patch, stride)
    assert (patch - stride) % 2 == 0
    pz, S = patch * s, stride * s
    bdr, u0 = (pz - S) // 2, A // 2
    kmax = SU.kmax_np(A, patch, stride)
    sk = np.zeros(nu * nv, dtype=np.int64) if k is None else s * np.clip(np.asarray(k, dtype=np.int64).reshape(-1), -kmax, kmax)
    assert sk.shape == (nu * nv,)
    a, d = np.arange(pz)[None, :], (np.arange(A) - u0)[:, None]
    for n in range(nu * nv):
        ku, kv = divmod(n, nv)
        Y, X = ku * S + a - bdr + sk[n] * d, kv * S + a - bdr + sk[n] * d
        yield n, Y, (Y >= 0) & (Y < h0 * s), X, (X >= 0) & (X < w0 * s)


def blend_np(sr, A, h0, w0, patch, stride, s, w, k=None):
    """SR patches [N, A*pz, A*pz] float32 -> (the blended SR scene mosaic [A*h0*s, A*w0*s] float32, the number of terms per pixel)."""
    pz = patch * s
    w = np.asarray(w)
    assert sr.dtype == np.float32 and w.dtype == np.float32 and w.shape == (pz,)
    num = np.zeros((A, h0 * s, A, w0 * s), dtype=np.float32)
    den = np.zeros_like(num)
    terms = np.zeros(num.shape, dtype=np.int32)
    ww = w[:, None] * w[None, :]                        # float32 x float32 -> one rounding
    assert ww.dtype == np.float32
    for n, Y, okY, X, okX in _maps(A, h0, w0, patch, stride, s, k):
        views = sr[n].reshape(A, pz, A, pz)
        for u in range(A):
            ay = np.nonzero(okY[u])[0]
            for v in range(A):
                bx = np.nonzero(okX[v])[0]
                if not len(ay) or not len(bx):
                    continue
                at = (u, Y[u, ay][:, None], v, X[v, bx][None, :])   # every scene pixel at most once per patch: += keeps the patch order
                wt = ww[ay[:, None], bx[None, :]]
                num[at] = num[at] + wt * views[u, ay[:, None], v, bx[None, :]]
                den[at] = den[at] + wt
                terms[at] += 1
    assert terms.min() >= 1
    out = num / den                                     # IEEE float32 division: correctly rounded
    assert out.dtype == np.float32
    shape = (A * h0 * s, A * w0 * s)
    return out.reshape(shape), terms.reshape(shape)


def cut_np(G, A, patch, stride, s, k=None):
    """The SR patches a perfect network would give for the SR-size mosaic G: lft_scene_divide's rule at SR size (patch*s, stride*s),
    with the shear s*k.  The SR-size shear is not clamped again: s*clamp(k) is what the blend puts back."""
    h, w = G.shape[0] // A, G.shape[1] // A
    N = int(np.prod(SU.counts_np(h, w, patch * s, stride * s)))
    if k is None:
        return SU.divide_plain_np(G, A, patch * s, stride * s)
    kmax = SU.kmax_np(A, patch, stride)
    return SU.divide_np(G, A, patch * s, stride * s, s * np.clip(np.asarray(k, dtype=np.int64), -kmax, kmax).reshape(N))


# ---- the bounds the CPU and the GPU tests share ----
SEAM = dict(A=2, s=2, h0=28, w0=30, patch=8, stride=4)       # SR views of 56 x 60 with pz = 16: pixels pz from the border remain, three crop borders a side


def reproduction_slack(terms, values):
    """(T+2) * 2^-24 * max|values|: a weighted mean of equal values picks up only the rounding of T products, T sums and one
    quotient."""
    return (int(terms.max()) + 2) * EPS * float(np.abs(values).max())


def seam_case(seed):
    """(G, the patches G + c_n, c, the crop of those patches): one bias per patch."""
    A, s, h0, w0, patch, stride = (SEAM[k] for k in ("A", "s", "h0", "w0", "patch", "stride"))
    rng = np.random.default_rng([41, seed])
    G = rng.random((A * h0 * s, A * w0 * s), dtype=np.float32)
    cut = cut_np(G, A, patch, stride, s)
    c = (rng.random(cut.shape[0], dtype=np.float32) - np.float32(0.5))
    return G, cut + c[:, None, None], c


def seam_excess(out, G, c, patches, terms_max=4):
    """(the largest |difference between adjacent pixels of out, minus G's own| over the pixels at least pz from the view border,
    the bound (2*pi/pz) * (max c - min c) + the fp32 slack)."""
    A, s, h0, w0, patch = (SEAM[k] for k in ("A", "s", "h0", "w0", "patch"))
    pz = patch * s
    d = (out.astype(np.float64) - G.astype(np.float64)).reshape(A, h0 * s, A, w0 * s)[:, pz:h0 * s - pz, :, pz:w0 * s - pz]
    assert d.shape[1] >= 3 * SEAM["stride"] * s and d.shape[3] >= 3 * SEAM["stride"] * s
    worst = max(np.abs(np.diff(d, axis=1)).max(), np.abs(np.diff(d, axis=3)).max())
    bound = 2 * np.pi / pz * float(c.max() - c.min()) + (terms_max + 2) * EPS * float(np.abs(patches).max())
    return float(worst), bound
