"""What the structural-loss tests share: the shapes, the input builder, an fp64 restatement of the definition in include/lft_hip.h
(lft_ssim_loss) that does not import lft_amd.loss -- torch fp64, one valid-mode 11x11 convolution per moment, gradient from
autograd -- and, as a second opinion on the gradient, the analytic a/b/c adjoint in numpy."""
import functools

import numpy as np
import torch

# (B, A, H, W): one interior pixel; odd pitch; exactly one 16x16 tile; a remainder of one row and one column across three tiles;
# the training view at batch 1
SHAPES = [(1, 1, 11, 11), (2, 2, 12, 13), (1, 3, 16, 16), (1, 2, 17, 33), (1, 5, 64, 64)]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
COV = 121.0 / 120.0


def window():
    k = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-0.5 * k * k / (1.5 * 1.5))
    return g / g.sum()


def views_of(m, A):
    """[B,1,A*H,A*W] -> [B*A*A,H,W] in (b, a1, a2) order (numpy or torch)."""
    B, _, R, C = m.shape
    H, W = R // A, C // A
    return m.reshape(B, A, H, A, W).transpose(2, 3).reshape(B * A * A, H, W) if isinstance(m, torch.Tensor) \
        else m.reshape(B, A, H, A, W).transpose(0, 1, 3, 2, 4).reshape(B * A * A, H, W)


def inputs(B, A, H, W, seed=0):
    """(sr, hr) float32 [B,1,A*H,A*W]: hr = 0.5 + 0.3 sin(0.11 row + 0.07 col) over the mosaic, sr = hr + 0.02 N(0,1) -- small variances,
    where E[v^2] - mu^2 cancels.  The LAST view has a constant hr (sigma_x = 0); with more than one view, the FIRST has sr == hr."""
    R, C = A * H, A * W
    row, col = np.arange(R, dtype=np.float64)[:, None], np.arange(C, dtype=np.float64)[None, :]
    hr = np.broadcast_to(0.5 + 0.3 * np.sin(0.11 * row + 0.07 * col), (B, 1, R, C)).astype(np.float32)
    hr = np.ascontiguousarray(hr)
    sr = (hr + 0.02 * np.random.default_rng(seed).standard_normal(hr.shape)).astype(np.float32)
    hr[B - 1, 0, (A - 1) * H:, (A - 1) * W:] = 0.375
    if B * A * A > 1:
        sr[0, 0, :H, :W] = hr[0, 0, :H, :W]
    return sr, hr


def clean_inputs(B, A, H, W):
    """sr == hr over the whole case (S = 1, gradient 0)."""
    _, hr = inputs(B, A, H, W)
    return hr.copy(), hr


def ssim_torch(sr, hr, A, ssim_range):
    """S as an fp64 torch scalar, differentiable with respect to sr [B,1,A*H,A*W] (float64 tensors)."""
    g = torch.from_numpy(window())
    k2 = (g[:, None] * g[None, :]).view(1, 1, 11, 11)
    x, y = views_of(hr, A).unsqueeze(1), views_of(sr, A).unsqueeze(1)
    f = lambda t: torch.nn.functional.conv2d(t, k2)                     # noqa: E731
    mx, my = f(x), f(y)
    vx, vy, vxy = COV * (f(x * x) - mx * mx), COV * (f(y * y) - my * my), COV * (f(x * y) - mx * my)
    C1, C2 = (0.01 * ssim_range) ** 2, (0.03 * ssim_range) ** 2
    smap = (2 * mx * my + C1) * (2 * vxy + C2) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    return smap.flatten(1).mean(dim=1).mean()


def reference(sr, hr, A, ssim_range=2.0):
    """(S, dS/dsr as float64 numpy of sr's shape) from float32 or float64 numpy inputs, all in fp64."""
    s = torch.from_numpy(np.asarray(sr, dtype=np.float64)).requires_grad_(True)
    h = torch.from_numpy(np.asarray(hr, dtype=np.float64))
    S = ssim_torch(s, h, A, ssim_range)
    S.backward()
    return float(S.detach()), s.grad.numpy()


@functools.lru_cache(maxsize=None)
def case(shape, ssim_range=2.0, seed=0):
    """(sr, hr, S, dS/dsr) of a shape, computed once and shared; the arrays are read-only."""
    sr, hr = inputs(*shape, seed=seed)
    S, g = reference(sr, hr, shape[1], ssim_range)
    for a in (sr, hr, g):
        a.setflags(write=False)
    return sr, hr, S, g


def _filter_valid(v, g):
    w = np.lib.stride_tricks.sliding_window_view(v, (11, 11), axis=(-2, -1))
    return np.einsum("...ij,i,j->...", w, g, g)


def analytic(sr, hr, A, ssim_range=2.0):
    """(S, dS/dsr) in numpy fp64 from the closed form: dS/dy(p) = (1/N) sum_q g(q-p) [a(q) + b(q) y(p) + c(q) x(p)]."""
    g = window()
    x, y = views_of(np.asarray(hr, dtype=np.float64), A), views_of(np.asarray(sr, dtype=np.float64), A)
    mx, my = _filter_valid(x, g), _filter_valid(y, g)
    vx, vy, vxy = COV * (_filter_valid(x * x, g) - mx * mx), COV * (_filter_valid(y * y, g) - my * my), COV * (_filter_valid(x * y, g) - mx * my)
    C1, C2 = (0.01 * ssim_range) ** 2, (0.03 * ssim_range) ** 2
    A1, A2, B1, B2 = 2 * mx * my + C1, 2 * vxy + C2, mx * mx + my * my + C1, vx + vy + C2
    S = A1 * A2 / (B1 * B2)
    d_mu = 2 * mx * A2 / (B1 * B2) - 2 * my * S / B1
    b = 2 * COV * (-S / B2)
    c = COV * 2 * A1 / (B1 * B2)
    a = d_mu - b * my - c * mx
    back = lambda m: _filter_valid(np.pad(m, ((0, 0), (10, 10), (10, 10))), g)      # noqa: E731  the window is symmetric
    grad = (back(a) + back(b) * y + back(c) * x) / S.size
    V, H, W = x.shape
    B = V // (A * A)
    grad = grad.reshape(B, A, A, H, W).transpose(0, 1, 3, 2, 4).reshape(B, 1, A * H, A * W)
    return float(S.reshape(V, -1).mean(axis=1).mean()), grad
