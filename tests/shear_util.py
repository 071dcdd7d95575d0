"""The sheared scene tiling and the shear vote (lft_amd/scene.py has the definition) restated in numpy: integers only, no tolerance
anywhere.  Today's rule (reflect_idx, the plain cut) is restated on its own, so that "k = 0 is today's rule" is a statement about two
pieces of code; the scenes the tests share are built here too."""
import numpy as np

SHEAR_MAX = 16


def counts_np(h0, w0, patch, stride):
    """(numU, numV) of lft_scene_counts."""
    bdr = (patch - stride) // 2
    h, w = h0 + 2 * bdr, w0 + 2 * bdr
    assert 1 <= stride <= patch and h >= patch and w >= patch
    return tuple((n - patch) // stride + (2 if (n - patch) % stride else 1) for n in (h, w))


def kmax_np(A, patch, stride):
    u0 = A // 2
    R = max(u0, A - 1 - u0)
    return SHEAR_MAX if R == 0 else min(SHEAR_MAX, (patch - stride) // 2 // R)


def fold(i, n):
    m = np.mod(i, 2 * n)                                # non-negative for any integer i
    return np.where(m < n, m, 2 * n - 1 - m)


def reflect(i, n):
    """Today's reflect_idx; it is only defined on [-n, 2n-1]."""
    assert np.all((i >= -n) & (i <= 2 * n - 1))
    i = np.where(i < 0, -i - 1, i)
    return np.where(i >= n, 2 * n - 1 - i, i)


def _clamped(k, N, A, patch, stride):
    kmax = kmax_np(A, patch, stride)
    k = np.asarray(k, dtype=np.int64).reshape(-1)
    assert k.shape == (N,)
    return np.clip(k, -kmax, kmax)


def divide_np(scene, A, patch, stride, k):
    """scene [A*h0, A*w0] -> patches [N, A*patch, A*patch] cut with the shear k [N] (any integers: clamped here as in the kernel)."""
    h0, w0 = scene.shape[0] // A, scene.shape[1] // A
    nu, nv = counts_np(h0, w0, patch, stride)
    bdr, u0 = (patch - stride) // 2, A // 2
    k = _clamped(k, nu * nv, A, patch, stride)
    T = np.arange(A * patch)
    t, p = T // patch, T % patch                        # the view and the pixel of a mosaic coordinate, the same along both axes
    out = np.zeros((nu * nv, A * patch, A * patch), dtype=scene.dtype)
    for n in range(nu * nv):
        ku, kv = divmod(n, nv)
        ey, ex = ku * stride + p, kv * stride + p
        rows = t * h0 + fold(ey - bdr + k[n] * (t - u0), h0)
        cols = t * w0 + fold(ex - bdr + k[n] * (t - u0), w0)
        val = scene[rows[:, None], cols[None, :]]
        val[(ey >= h0 + 2 * bdr)[:, None] | (ex >= w0 + 2 * bdr)[None, :]] = 0
        out[n] = val
    return out


def divide_plain_np(scene, A, patch, stride):
    """Today's rule: symmetric extension by bdr (reflect_idx), zero fill beyond it, every view cut at the same position."""
    h0, w0 = scene.shape[0] // A, scene.shape[1] // A
    nu, nv = counts_np(h0, w0, patch, stride)
    bdr = (patch - stride) // 2
    views = scene.reshape(A, h0, A, w0).transpose(0, 2, 1, 3)
    ext = np.zeros((A, A, (nu - 1) * stride + patch, (nv - 1) * stride + patch), dtype=scene.dtype)
    ys, xs = reflect(np.arange(h0 + 2 * bdr) - bdr, h0), reflect(np.arange(w0 + 2 * bdr) - bdr, w0)
    ext[:, :, :h0 + 2 * bdr, :w0 + 2 * bdr] = views[:, :, ys[:, None], xs[None, :]]
    out = np.zeros((nu * nv, A * patch, A * patch), dtype=scene.dtype)
    for n in range(nu * nv):
        ku, kv = divmod(n, nv)
        cut = ext[:, :, ku * stride:ku * stride + patch, kv * stride:kv * stride + patch]
        out[n] = cut.transpose(0, 2, 1, 3).reshape(A * patch, A * patch)
    return out


def integrate_np(sr, A, h0, w0, patch, stride, s, k):
    """SR patches [N, A*patch*s, A*patch*s] -> the SR scene mosaic [A*h0*s, A*w0*s], put back against the shear k [N]."""
    nu, nv = counts_np(h0, w0, patch, stride)
    u0, pz, st, bs = A // 2, patch * s, stride * s, (patch - stride) // 2 * s
    k = _clamped(k, nu * nv, A, patch, stride)
    assert sr.shape == (nu * nv, A * pz, A * pz)
    Ym, Xm = np.arange(A * h0 * s), np.arange(A * w0 * s)
    u, Y, v, X = Ym // (h0 * s), Ym % (h0 * s), Xm // (w0 * s), Xm % (w0 * s)
    n = (Y // st)[:, None] * nv + (X // st)[None, :]
    assert n.max() < nu * nv
    sk = s * k[n]
    row = (bs + Y % st)[:, None] - sk * (u - u0)[:, None]
    col = (bs + X % st)[None, :] - sk * (v - u0)[None, :]
    assert row.min() >= 0 and col.min() >= 0 and row.max() < pz and col.max() < pz      # inside the patch's own view
    return sr[n, u[:, None] * pz + row, v[None, :] * pz + col]


def integrate_plain_np(sr, A, h0, w0, patch, stride, s):
    """Today's rule: the central stride*s region of every view of every SR patch, side by side, cropped to the view."""
    nu, nv = counts_np(h0, w0, patch, stride)
    pz, st, bs = patch * s, stride * s, (patch - stride) // 2 * s
    v = sr.reshape(nu, nv, A, pz, A, pz)[:, :, :, bs:bs + st, :, bs:bs + st]            # [nu, nv, A, st, A, st]
    full = v.transpose(2, 0, 3, 4, 1, 5).reshape(A, nu * st, A, nv * st)[:, :h0 * s, :, :w0 * s]
    return full.reshape(A * h0 * s, A * w0 * s)


def replicate(x, s):
    """Pixel replication x s of the last two axes: of a mosaic it is the mosaic of the replicated views."""
    return np.repeat(np.repeat(x, s, axis=-2), s, axis=-1)


def inside_np(A, h0, w0, patch, stride, k):
    """bool [N, A*patch, A*patch]: the pixels of the sheared cut whose own read and the centre view's read (k = 0) both lie inside
    the scene, before any fold."""
    nu, nv = counts_np(h0, w0, patch, stride)
    bdr, u0 = (patch - stride) // 2, A // 2
    k = _clamped(k, nu * nv, A, patch, stride)
    T = np.arange(A * patch)
    t, p = T // patch, T % patch
    out = np.zeros((nu * nv, A * patch, A * patch), dtype=bool)
    for n in range(nu * nv):
        ku, kv = divmod(n, nv)
        ok = []
        for e, size in ((ku * stride + p - bdr, h0), (kv * stride + p - bdr, w0)):
            own = e + k[n] * (t - u0)
            ok.append((e >= 0) & (e < size) & (own >= 0) & (own < size))
        out[n] = ok[0][:, None] & ok[1][None, :]
    return out


def vote_np(index, confidence, slopes, margin, min_confidence):
    """(shear int32 [B], counts int32 [B, D]) of index / confidence [B, H, W] and the whole-number slopes [D]."""
    B, H, W = index.shape
    D = len(slopes)
    counts = np.zeros((B, D), dtype=np.int32)
    shear = np.zeros(B, dtype=np.int32)
    region = (slice(None), slice(margin, H - margin), slice(margin, W - margin))
    j = np.clip(index[region], 0, D - 1)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(confidence[region]) & (confidence[region] >= np.float32(min_confidence))
    for b in range(B):
        counts[b] = np.bincount(j[b][ok[b]], minlength=D)
        if counts[b].max() > 0:
            best = [int(slopes[i]) for i in range(D) if counts[b, i] == counts[b].max()]
            shear[b] = min(best, key=lambda sl: (abs(sl), sl))
    return shear, counts


def mosaic(views):
    """views [A, A, h, w] -> the mosaic [A*h, A*w]."""
    A, _, h, w = views.shape
    return np.ascontiguousarray(views.transpose(0, 2, 1, 3).reshape(A * h, A * w))


def patch_views(patches, A):
    """patch mosaics [N, A*P, A*P] -> views [N, A, A, P, P, 1], as tests/disparity_util.py takes them."""
    N, P = patches.shape[0], patches.shape[1] // A
    return np.ascontiguousarray(patches.reshape(N, A, P, A, P).transpose(0, 1, 3, 2, 4)[..., None])


def translated_scene(A, h0, w0, d, seed=0):
    """The mosaic of views that are whole-pixel translations of one random image: a point seen at y in the view u0 is seen at
    y + d*(u - u0) in view u."""
    u0, pad = A // 2, abs(d) * A
    base = np.random.default_rng(seed).random((h0 + 2 * pad, w0 + 2 * pad)).astype(np.float32)
    views = np.stack([np.stack([base[pad - d * (u - u0):pad - d * (u - u0) + h0, pad - d * (v - u0):pad - d * (v - u0) + w0] for v in range(A)])
                      for u in range(A)])
    return mosaic(views)


TWO_PLANES = dict(A=3, h0=24, w0=40, patch=16, stride=8, d_left=2, d_right=-1)


def two_plane_scene(A=3, h0=24, w0=40, d_left=2, d_right=-1, seed=1, **_):
    """The mosaic of a scene of two fronto-parallel planes with random texture: in the view u0 the left half (x < w0/2) lies at the
    slope d_left and the right half at d_right.  In another view each plane is translated by its slope; where both land the left one
    is in front, where neither does the right one goes on."""
    u0, pad = A // 2, max(abs(d_left), abs(d_right)) * A
    rng = np.random.default_rng(seed)
    left, right = (rng.random((h0 + 2 * pad, w0 + 2 * pad)).astype(np.float32) for _ in range(2))
    yy, xx = np.meshgrid(np.arange(h0), np.arange(w0), indexing="ij")
    views = np.zeros((A, A, h0, w0), dtype=np.float32)
    for u in range(A):
        for v in range(A):
            ly, lx = yy - d_left * (u - u0), xx - d_left * (v - u0)
            ry, rx = yy - d_right * (u - u0), xx - d_right * (v - u0)
            views[u, v] = np.where(lx < w0 // 2, left[ly + pad, lx + pad], right[ry + pad, rx + pad])
    return mosaic(views)


def one_plane_patches(h0=24, w0=40, patch=16, stride=8, d_left=2, d_right=-1, **_):
    """{patch n: its plane's slope} for the patches whose central region (the stride x stride pixels the patch contributes) lies in
    one half of the two-plane scene."""
    nu, nv = counts_np(h0, w0, patch, stride)
    want = {}
    for n in range(nu * nv):
        x0 = (n % nv) * stride
        if x0 + stride <= w0 // 2:
            want[n] = d_left
        elif x0 >= w0 // 2:
            want[n] = d_right
    return want
