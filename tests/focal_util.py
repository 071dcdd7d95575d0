"""The focal-stack term (include/lft_hip_focal.h) restated in fp64 numpy, and the tolerances the GPU tests hold the kernels to.

Steps 1 to 4 of the definition, from the fp32-rounded table of lft_amd.refocus.shift_table taken as fp64:

  1. e = fl32(sr - hr);  r_k[b, y, x] = sum_n a * sum_jx wx[jx] * sum_jy wy[jy] * e[b, n, clamp(y + oy + jy), clamp(x + ox + jx)]
  2. F = mean rho(r)
  3. G = gscale * w_focal * rho'(r) / N,  rho'(0) = 0 for L1
  4. dsr = R^T G: every product a * wy[jy] * wx[jx] * G_k[b, y, x] is added to the view pixel its tap read (``adjoint_np`` scatters, the
     kernel gathers: the same set of products per view pixel).

The tolerance of the adjoint.  Let a view pixel p collect n[p] products t_i = a * wy * wx * G, and let M[p] = sum |t_i|.  A kernel
that forms every t_i with three roundings (three multiplications, in any association) and adds the n of them in ANY order -- any
summation tree, factored or not, fused multiply-adds or not -- commits at most n - 1 + 3 roundings on the path of any one term, so

  |computed - exact| <= ((1 + u)^(n + 2) - 1) * M  <=  (n + 4) * u * M,      u = 2^-24,

the second step for (n + 2) * u < 0.01, which holds for every shape here.  The two spare roundings cover the rounding of G itself
to fp32 (step 3) and the second-order terms.  ``tol_adj`` is that bound; the tests add one store rounding, u * |value|.
For r the tolerance is tests/refocus_util.py's ``tol``, with max |e| as the input bound."""
import numpy as np

import refocus_util as RU

PENALTIES = ("l1", "mse", "charbonnier")
U24 = 2.0 ** -24


def views(m, A):
    """A batch of mosaics [B, 1, A*H, A*W] as views [B, A, A, H, W] (a view of the same memory)."""
    B, _, R, C = m.shape
    return m.reshape(B, A, R // A, A, C // A).transpose(0, 1, 3, 2, 4)


def mosaic(v):
    """Views [B, A, A, H, W] as a batch of mosaics [B, 1, A*H, A*W]."""
    B, A, _, H, W = v.shape
    return np.ascontiguousarray(v.transpose(0, 1, 3, 2, 4)).reshape(B, 1, A * H, A * W)


def difference(sr, hr):
    """Step 1's e: the fp32 difference of two fp32 mosaics, as the kernel forms it."""
    return sr.astype(np.float32) - hr.astype(np.float32)


def refocus_batch_np(e, A, table, taps):
    """fp64 [B, D, H, W]: refocus_util.refocus_np on every mosaic of the batch e [B, 1, A*H, A*W]."""
    return np.stack([RU.refocus_np(v[..., None], table, taps)[..., 0] for v in views(e, A)])


def rho(x, penalty, eps):
    return np.abs(x) if penalty == "l1" else x * x if penalty == "mse" else np.sqrt(x * x + eps * eps)


def drho(x, penalty, eps):
    return np.sign(x) if penalty == "l1" else 2.0 * x if penalty == "mse" else x / np.sqrt(x * x + eps * eps)


def stack_grad_np(r, penalty, eps, w_focal=1.0, gscale=1.0):
    """Step 3 in fp64, unrounded: G of the residual stack r."""
    return gscale * w_focal * drho(np.asarray(r, dtype=np.float64), penalty, eps) / r.size


def adjoint_np(G, A, table, taps, bound=False):
    """Step 4 in fp64: the mosaic [B, 1, A*H, A*W] of R^T G for G [B, D, H, W].  bound: also n, the product count of every mosaic
    pixel, and M, the same adjoint over |G| and the absolute weights (both as mosaics)."""
    B, D, H, W = G.shape
    G = np.asarray(G, dtype=np.float64)
    out, cnt, mag = (np.zeros((B, A, A, H, W), dtype=np.float64) for _ in range(3))
    ys, xs = np.arange(H), np.arange(W)
    for k in range(D):
        for n in range(A * A):
            rec = table[k, n]
            if rec["skip"]:
                continue
            u, v = divmod(n, A)
            for jy in range(taps):
                rows = np.clip(ys + int(rec["oy"]) + jy, 0, H - 1)[:, None]
                for jx in range(taps):
                    cols = np.clip(xs + int(rec["ox"]) + jx, 0, W - 1)[None, :]
                    c = float(rec["a"]) * float(rec["wy"][jy]) * float(rec["wx"][jx])
                    for b in range(B):
                        np.add.at(out[b, u, v], (rows, cols), c * G[b, k])
                        if bound:
                            np.add.at(cnt[b, u, v], (rows, cols), 1.0)
                            np.add.at(mag[b, u, v], (rows, cols), abs(c) * np.abs(G[b, k]))
    return (mosaic(out), mosaic(cnt), mosaic(mag)) if bound else mosaic(out)


def tol_adj(n, M):
    """(n + 4) * 2^-24 * M per mosaic pixel (the module docstring has the derivation)."""
    return (n + 4.0) * U24 * M


def focal_np(sr, hr, A, table, taps, penalty="l1", eps=1e-3, w_focal=1.0, gscale=1.0):
    """Steps 1 to 4: (r [B, D, H, W], F, G, dsr [B, 1, A*H, A*W]), all fp64."""
    r = refocus_batch_np(difference(sr, hr), A, table, taps)
    G = stack_grad_np(r, penalty, eps, w_focal, gscale)
    return r, float(rho(r, penalty, eps).mean()), G, adjoint_np(G, A, table, taps)


def exact_pair(rng, B, A, H, W, bits=10):
    """fp32 mosaics (sr, hr) on a grid of 2^-bits whose difference is exact in fp32, so an fp64 evaluation of sr - hr sees step
    1's e: hr in [0, 1], sr - hr in [-2, 2]."""
    q = float(1 << bits)
    hr = rng.integers(0, (1 << bits) + 1, (B, 1, A * H, A * W)) / q
    e = rng.integers(-2 << bits, (2 << bits) + 1, (B, 1, A * H, A * W)) / q
    return (hr + e).astype(np.float32), hr.astype(np.float32)
