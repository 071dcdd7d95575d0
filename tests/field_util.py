"""Angular tiling of a U x V field (lft_amd/field.py has the definition) restated in numpy float32: the same order of the sum and one
rounding per operation, so the GPU is compared bit for bit.  The per-window maps are those of tests/shear_util.py (the cut, the crop's
gather) and tests/blend_util.py (the blend's scatter): a window's sub-mosaic is sliced out here, which the kernels never do."""
import numpy as np

import blend_util as BU
import shear_util as SU

EPS = BU.EPS


def origins_np(L, A, astride):
    assert 1 <= astride <= A <= L
    m = 1 if L == A else -(-(L - A) // astride) + 1
    return [min(i * astride, L - A) for i in range(m)]


def windows_np(U, V, A, astride):
    """[(w, o_u, o_v)] in batch order."""
    ou, ov = origins_np(U, A, astride), origins_np(V, A, astride)
    return [(wu * len(ov) + wv, ou[wu], ov[wv]) for wu in range(len(ou)) for wv in range(len(ov))]


def sub_mosaic(field, U, V, A, o_u, o_v):
    """The A x A sub-mosaic of views (o_u + u, o_v + v) of a field mosaic [U*h, V*w]."""
    h, w = field.shape[0] // U, field.shape[1] // V
    views = field.reshape(U, h, V, w)[o_u:o_u + A, :, o_v:o_v + A, :]
    return np.ascontiguousarray(views.reshape(A * h, A * w))


def divide_np(field, U, V, A, astride, patch, stride, k=None):
    """field [U*h0, V*w0] -> [mu*mv*N, A*patch, A*patch]; k: None or [mu*mv*N] (any integers: clamped as in the kernel)."""
    h0, w0 = field.shape[0] // U, field.shape[1] // V
    N = int(np.prod(SU.counts_np(h0, w0, patch, stride)))
    out = []
    for w, o_u, o_v in windows_np(U, V, A, astride):
        sub = sub_mosaic(field, U, V, A, o_u, o_v)
        out.append(SU.divide_plain_np(sub, A, patch, stride) if k is None else SU.divide_np(sub, A, patch, stride, np.asarray(k)[w * N:(w + 1) * N]))
    return np.concatenate(out, axis=0)


def integrate_np(sr, U, V, A, astride, h0, w0, patch, stride, s, g, win=None, k=None):
    """SR patches [mu*mv*N, A*pz, A*pz] float32 -> (the SR field mosaic [U*h0*s, V*w0*s] float32, the number of terms per pixel T)."""
    pz, H, W = patch * s, h0 * s, w0 * s
    N = int(np.prod(SU.counts_np(h0, w0, patch, stride)))
    g = np.asarray(g)
    assert sr.dtype == np.float32 and g.dtype == np.float32 and g.shape == (A,)
    wins = windows_np(U, V, A, astride)
    assert sr.shape == (len(wins) * N, A * pz, A * pz)
    num = np.zeros((U, H, V, W), dtype=np.float32)
    den = np.zeros_like(num)
    terms = np.zeros(num.shape, dtype=np.int32)
    if win is not None:
        win = np.asarray(win)
        assert win.dtype == np.float32 and win.shape == (pz,)
        ww = win[:, None] * win[None, :]
    for w, o_u, o_v in wins:                            # ascending wu, then wv
        sub = sr[w * N:(w + 1) * N]
        kw = None if k is None else np.asarray(k)[w * N:(w + 1) * N]
        if win is None:                                 # one term: the element the crop's integrate reads for this window's sub-scene
            x = (SU.integrate_plain_np(sub, A, h0, w0, patch, stride, s) if kw is None else SU.integrate_np(sub, A, h0, w0, patch, stride, s, kw)).reshape(A, H, A, W)
            for u in range(A):
                for v in range(A):
                    ga = g[u] * g[v]
                    at = (o_u + u, slice(None), o_v + v, slice(None))
                    num[at] = num[at] + ga * x[u, :, v, :]
                    den[at] = den[at] + ga
                    terms[at] += 1
            continue
        for n, Y, okY, X, okX in BU._maps(A, h0, w0, patch, stride, s, kw):       # ascending ku, then kv
            views = sub[n].reshape(A, pz, A, pz)
            for u in range(A):
                ay = np.nonzero(okY[u])[0]
                for v in range(A):
                    bx = np.nonzero(okX[v])[0]
                    if not len(ay) or not len(bx):
                        continue
                    ga = g[u] * g[v]
                    at = (o_u + u, Y[u, ay][:, None], o_v + v, X[v, bx][None, :])
                    wt = ga * ww[ay[:, None], bx[None, :]]
                    assert wt.dtype == np.float32
                    num[at] = num[at] + wt * views[u, ay[:, None], v, bx[None, :]]
                    den[at] = den[at] + wt
                    terms[at] += 1
    assert terms.min() >= 1
    out = num / den                                     # IEEE float32 division: correctly rounded
    assert out.dtype == np.float32
    return out.reshape(U * H, V * W), terms.reshape(U * H, V * W)


def cut_np(G, U, V, A, astride, patch, stride, s, k=None):
    """The SR patches a perfect network would give for the SR-size field mosaic G: the divide at SR size with the shear s*clamp(k)."""
    h, w = G.shape[0] // U, G.shape[1] // V
    N = int(np.prod(SU.counts_np(h, w, patch * s, stride * s)))
    out = []
    for wdx, o_u, o_v in windows_np(U, V, A, astride):
        out.append(BU.cut_np(sub_mosaic(G, U, V, A, o_u, o_v), A, patch, stride, s, None if k is None else np.asarray(k)[wdx * N:(wdx + 1) * N]))
    return np.concatenate(out, axis=0)
