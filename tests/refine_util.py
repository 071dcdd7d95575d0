"""The refinement of a disparity map (lft_amd/refine.py) restated in numpy from its definitions, not from the kernels: the
cross-view check, the farther-neighbour fill, the guided weighted median and the weight table.  Every step of the definitions is a
comparison or an integer sum, so the restatements are exact and the GPU tests ask for equality.  Also the noisy two-layer scene of
tests/occlusion_util.py at 48 x 64 with its band."""
import numpy as np

import disparity_util as DU
import occlusion_util as OU

F = np.float32
TABLE = 1024


def good_np(d, valid):
    """A pixel is good iff valid != 0 (None: all) and D is finite there."""
    g = np.isfinite(d)
    return g if valid is None else g & (np.asarray(valid) != 0)


def same_values(a, b):
    """Values compared as numbers (so -0 equals +0), or bit for bit where they are no numbers."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(np.all((a == b) | (a.view(np.uint32) == b.view(np.uint32))))


def check_np(dr, dv, deltas, tau, near="larger", min_agree=1, max_conflict=0):
    """dr fp32 [B, H, W], dv fp32 [B, N, H, W], deltas fp32 [N, 2] -> (valid, agree, conflict) uint8 [B, H, W]."""
    dr, dv, deltas, tau = np.asarray(dr, F), np.asarray(dv, F), np.asarray(deltas, F), F(tau)
    B, H, W = dr.shape
    N = dv.shape[1]
    yy, xx = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    fin = np.isfinite(dr)
    d = np.where(fin, dr, F(0))
    lo, hi = d - tau, d + tau                                       # fp32, one rounding each
    bi = np.broadcast_to(np.arange(B)[:, None, None], dr.shape)
    agree, conflict = np.zeros(dr.shape, np.int64), np.zeros(dr.shape, np.int64)
    assert lo.dtype == F and hi.dtype == F
    with np.errstate(all="ignore"):
        for n in range(N):
            py, px = yy + d * deltas[n, 0], xx + d * deltas[n, 1]    # fl(y + fl(d * du)): numpy rounds each fp32 operation once
            assert py.dtype == F and px.dtype == F
            fy, fx = np.floor(py), np.floor(px)
            some = np.zeros(dr.shape, bool)
            agrees, nearer = some.copy(), some.copy()
            for a in (0, 1):
                ya = fy + F(a)
                oky = ((py != fy) if a else np.ones(dr.shape, bool)) & (ya >= 0) & (ya <= F(H - 1))        # decided in fp32; NaN is outside
                for b in (0, 1):
                    xb = fx + F(b)
                    ok = oky & ((px != fx) if b else True) & (xb >= 0) & (xb <= F(W - 1))
                    q = dv[bi, n, np.where(ok, ya, 0).astype(np.int64), np.where(ok, xb, 0).astype(np.int64)]
                    ok = ok & np.isfinite(q)
                    some |= ok
                    agrees |= ok & (q >= lo) & (q <= hi)
                    nearer |= ok & ((q > hi) if near == "larger" else (q < lo))
            agree += agrees
            conflict += some & ~agrees & ~nearer
    agree, conflict = np.where(fin, agree, 0), np.where(fin, conflict, 0)
    valid = fin & (agree >= min_agree) & (conflict <= max_conflict)
    return valid.astype(np.uint8), agree.astype(np.uint8), conflict.astype(np.uint8)


def _nearest(good, d, axis, step, reach):
    """(found, value): per pixel the nearest good value at 1 .. reach pixels along `axis` in direction `step`."""
    found, value = np.zeros(d.shape, bool), np.zeros(d.shape, F)
    n = d.shape[axis]
    for s in range(1, min(reach, n - 1) + 1):
        src = [slice(None)] * d.ndim
        dst = [slice(None)] * d.ndim
        src[axis], dst[axis] = (slice(s, None), slice(0, n - s)) if step > 0 else (slice(0, n - s), slice(s, None))
        src, dst = tuple(src), tuple(dst)
        take = np.zeros(d.shape, bool)
        take[dst] = good[src] & ~found[dst]
        shifted = np.zeros(d.shape, F)
        shifted[dst] = d[src]
        value = np.where(take, shifted, value)
        found |= take
    return found, value


def fill_np(d, valid=None, reach=32, near="larger"):
    """d fp32 [B, H, W], valid uint8 or None -> (out fp32, holes uint8)."""
    d = np.asarray(d, F)
    good = good_np(d, valid)
    farther = np.minimum if near == "larger" else np.maximum

    def along(axis):
        f0, v0 = _nearest(good, d, axis, -1, reach)
        f1, v1 = _nearest(good, d, axis, +1, reach)
        return f0 | f1, np.where(f0 & f1, farther(v0, v1), np.where(f0, v0, v1))

    fr, vr = along(2)
    fc, vc = along(1)
    got = fr | fc
    out = np.where(good, d, np.where(fr, vr, np.where(fc, vc, d)))
    out = np.where(good | got, out, 0).astype(F)
    out.view(np.uint32)[~(good | got)] = d.view(np.uint32)[~(good | got)]                # the bits of D
    return out, np.where(good, 0, np.where(got, 1, 2)).astype(np.uint8)


def range_table_np(sigma, channels):
    """w[s] = rint(4096 exp(-(s / (255 channels)) / sigma)) in fp64, s = 0 .. 1023; sigma None: all ones."""
    if sigma is None:
        return np.ones(TABLE, np.uint16)
    return np.array([np.rint(4096.0 * np.exp(-(s / (255.0 * channels)) / sigma)) for s in range(TABLE)]).astype(np.uint16)


def wmedian_np(d, guide, table, radius, valid=None):
    """d fp32 [B, H, W], guide uint8 [B, H, W, C], table uint16 [1024] -> (out fp32, flags uint8): gather the window, sort by value,
    integer cumulative sum."""
    d, g, table = np.asarray(d, F), np.asarray(guide).astype(np.int64), np.asarray(table).astype(np.int64)
    B, H, W = d.shape
    good = good_np(d, valid)
    r = int(radius)
    vals, wts = [], []
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))        # q = p + (dy, dx): source, destination
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            v, w = np.full(d.shape, np.inf, np.float64), np.zeros(d.shape, np.int64)
            if ys.stop > ys.start and xs.stop > xs.start:
                sample = good[:, ys, xs]
                s = np.minimum(TABLE - 1, np.abs(g[:, yd, xd] - g[:, ys, xs]).sum(-1))
                v[:, yd, xd] = np.where(sample, d[:, ys, xs].astype(np.float64), np.inf)         # positions outside and non-samples: no weight
                w[:, yd, xd] = np.where(sample, table[s], 0)
            vals.append(v)
            wts.append(w)
    vals, wts = np.stack(vals), np.stack(wts)
    order = np.argsort(vals, axis=0, kind="stable")
    vals, wts = np.take_along_axis(vals, order, 0), np.take_along_axis(wts, order, 0)
    T = wts.sum(0)
    first = np.argmax(2 * np.cumsum(wts, 0) >= np.maximum(T, 1), axis=0)
    med = np.take_along_axis(vals, first[None], 0)[0]
    out = np.where(T > 0, med, 0).astype(F)
    out.view(np.uint32)[T == 0] = d.view(np.uint32)[T == 0]         # the bits of D
    return out, np.where(T == 0, 2, np.where(good, 0, 1)).astype(np.uint8)


def wmedian_iter_np(d, guide, table, radius, valid=None, iterations=1):
    """``wmedian_np`` iterated: each pass reads the last one's output, with valid := flags != 2."""
    out = flags = None
    for _ in range(iterations):
        out, flags = wmedian_np(d, guide, table, radius, valid)
        d, valid = out, (flags != 2).astype(np.uint8)
    return out, flags


def wmedian_brute(values, weights):
    """The definition itself on one window: min{v : 2 sum_{q: D[q] <= v} w_q >= T} over the sample values v, None for T = 0."""
    T = sum(int(w) for w in weights)
    if T == 0:
        return None
    return min(v for v in values if 2 * sum(int(w) for u, w in zip(values, weights) if u <= v) >= T)


# ---- the two-layer scene of the feature test: occlusion_util's, at 48 x 64 ----
SCENE = dict(OU.SCENE, H=48, W=64)
SLOPES, BOX, K_BG, K_FG = OU.SLOPES, OU.BOX, OU.K_BG, OU.K_FG


def noisy_two_layer():
    """fp32 views [5, 5, 48, 64, 1]: disparity_util.two_layer with occlusion_util's box plus its noise, 0.02 N(0, 1) from default_rng(7)."""
    L, _ = DU.two_layer(5, 48, 64, box=BOX)
    return (L + 0.02 * np.random.default_rng(7).standard_normal(L.shape)).astype(np.float32)


def band():
    return OU.band(5, 48, 64, BOX)


def truth():
    """fp32 [48, 64]: the true slope of the centre view, +1 inside the box and -1 outside."""
    t = np.full((48, 64), -1.0, F)
    t[BOX[0]:BOX[1], BOX[2]:BOX[3]] = 1.0
    return t
