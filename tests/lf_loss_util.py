"""The light-field loss of include/lft_hip.h (lft_lf_loss) restated independently of lft_amd.loss: torch slicing on the CPU in a
chosen dtype, the gradient from autograd; plus the shapes, inputs and error figures the loss tests share.

d = sr - hr seen as d[b, a1, y, a2, x]; P = mean rho(d); E = mean over the forward differences that exist (Dx, Dy inside a view, Dv
between views a2 / a2 + 1, Du between views a1 / a1 + 1) of mean rho(D_t d); total = w_pix P + w_epi E."""
import numpy as np
import torch

PENALTIES = ("l1", "mse", "charbonnier")
PEN_ENUM = {"l1": 0, "mse": 1, "charbonnier": 2}                  # LFT_LOSS_* of include/lft_hip.h
WEIGHTS = [(1.0, 0.0), (0.0, 1.0), (1.0, 0.5)]
# (B, A, H, W) of the issue: T = 0; no angular terms; no Dy; no Dx and a pitch that is no multiple of 4; ragged; ...; straddles
# blocks with an odd pitch; 81 views; the BASELINE training shape
SHAPES = [(1, 1, 1, 1), (1, 1, 3, 5), (2, 2, 1, 4), (1, 3, 4, 1), (2, 3, 5, 7), (1, 5, 16, 16), (3, 2, 33, 65), (1, 9, 8, 8), (8, 5, 64, 64)]
EPS_VALUES = (1e-3, 0.1)
LOSS_RTOL = 1e-5                  # the project's bound on loss values (tests/test_gpu_loss_adam.py)


def rho(x, penalty, eps):
    if penalty == "l1":
        return x.abs()
    if penalty == "mse":
        return x.square()
    assert penalty == "charbonnier"
    return (x.square() + eps * eps).sqrt()


def counts(B, A, H, W):
    """n and (n_x, n_y, n_v, n_u)."""
    return B * A * A * H * W, (B * A * A * H * (W - 1), B * A * A * (H - 1) * W, B * A * (A - 1) * H * W, B * A * (A - 1) * H * W)


def terms(sr, hr, A, penalty, eps):
    """(P, E) as 0-dim tensors in the dtype of sr."""
    B, _, R, C = sr.shape
    H, W = R // A, C // A
    d = (sr - hr).view(B, A, H, A, W)
    P = rho(d, penalty, eps).sum() / d.numel()
    diffs = [d[..., 1:] - d[..., :-1],                            # Dx
             d[:, :, 1:] - d[:, :, :-1],                          # Dy
             d[:, :, :, 1:] - d[:, :, :, :-1],                    # Dv
             d[:, 1:] - d[:, :-1]]                                # Du
    n, nt = counts(B, A, H, W)
    assert d.numel() == n and [t.numel() for t in diffs] == list(nt)
    live = [t for t in diffs if t.numel() > 0]
    E = sum(rho(t, penalty, eps).sum() / t.numel() for t in live) / len(live) if live else torch.zeros((), dtype=sr.dtype)
    return P, E


def reference(sr, hr, A, penalty, eps, w_pix, w_epi, dtype=torch.float64):
    """((total, P, E) as floats, d total / d sr as a float64 numpy array [B,1,A*H,A*W]) evaluated in `dtype`."""
    s = torch.as_tensor(sr).to(dtype).clone().requires_grad_(True)
    h = torch.as_tensor(hr).to(dtype)
    P, E = terms(s, h, A, penalty, float(eps))
    total = w_pix * P + w_epi * E
    total.backward()
    return (float(total.detach()), float(P.detach()), float(E.detach())), s.grad.double().numpy()


def lattice_inputs(B, A, H, W, seed=0, ties=True):
    """sr, hr float32 [B,1,A*H,A*W], multiples of 2^-8 in [0, 1): d and every difference of d are exact in fp32, so no sign and no
    Charbonnier argument hangs on rounding.  ties: runs of sr == hr -- the last 40 and elements 240..262 of the flat buffer (across
    the first block boundary of either path where there is one), and, in image 0, a band of rows and a band of columns around a view
    border (several views) and the 3x3 corner of every view (views of 3x3 and more: elements whose nine contributions all tie)."""
    rng = np.random.default_rng([seed, B, A, H, W])
    shape = (B, 1, A * H, A * W)
    sr = rng.integers(0, 256, shape).astype(np.float32) / 256.0
    hr = rng.integers(0, 256, shape).astype(np.float32) / 256.0
    if ties:
        n = sr.size
        fs, fh = sr.reshape(-1), hr.reshape(-1)
        fh[max(0, n - 40):max(0, n - 3)] = fs[max(0, n - 40):max(0, n - 3)]
        fh[240:262] = fs[240:262]
        fh[1020:1030] = fs[1020:1030]                             # 256 threads of 4 pixels
        if A > 1:                                                 # image 0: the middle third of a band across the first view border
            R, C = A * H, A * W
            hr[0, :, H - 1:H + 2, C // 3:2 * C // 3 + 1] = sr[0, :, H - 1:H + 2, C // 3:2 * C // 3 + 1]
            hr[0, :, R // 3:2 * R // 3 + 1, W - 1:W + 2] = sr[0, :, R // 3:2 * R // 3 + 1, W - 1:W + 2]
        if H >= 3 and W >= 3:                                     # image 0: a 3x3 corner of every view, so that pixel (1, 1) of each view and
            v, w = hr[0, 0].reshape(A, H, A, W), sr[0, 0].reshape(A, H, A, W)           # all the neighbours it is paired with tie
            v[:, :3, :, :3] = w[:, :3, :, :3]
    return sr, hr


def l1_grad_bound(B, A, H, W, w_pix, w_epi, gscale):
    """Per-element bound on |dsr - ref| for the L1 penalty: every rho' is exactly -1, 0 or 1, each of the five coefficients is rounded
    once, at most eight additions follow and one scale: 16 * 2^-24 * gscale * (w_pix / n + (w_epi / T) * sum_t 2 / n_t)."""
    n, nt = counts(B, A, H, W)
    live = [c for c in nt if c > 0]
    epi = (w_epi / len(live)) * sum(2.0 / c for c in live) if live else 0.0
    return 16 * 2.0 ** -24 * abs(gscale) * (w_pix / n + epi)


def grad_error(got, ref):
    """Worst gradient error as a fraction of the largest gradient element."""
    m = float(np.abs(ref).max())
    return float(np.abs(got - ref).max() / m) if m > 0 else float(np.abs(got).max())


def loss_error(got3, ref3):
    """Worst relative error of (total, P, E); an exactly zero reference (E at T = 0) must be met exactly."""
    return max(abs(g - r) / abs(r) if r != 0 else (0.0 if g == 0 else float("inf")) for g, r in zip(got3, ref3))
