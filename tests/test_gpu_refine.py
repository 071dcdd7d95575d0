"""GPU tests of the refinement of a disparity map (lft_disp_check, lft_disp_fill, lft_disp_wmedian; lft_amd/refine.py has the
definitions) against the numpy restatements of tests/refine_util.py, with equality of every output: values compared as numbers,
flags and counts as bytes.

Shapes (H, W): (1, 1), (1, 37), (37, 1), (5, 3), (33, 65), (70, 29), (66, 130), each with B = 1 and 2: below any tile, one past a
wave or tile in each direction, taller than wide and wider than tall.  The inputs of a shape are made once and shared."""
import functools

import numpy as np
import pytest
import torch

from lft_amd import disparity as Dm, refine as R, train as Tr

import refine_util as RU

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1), (1, 37), (37, 1), (5, 3), (33, 65), (70, 29), (66, 130)]
BATCH = [1, 2]
F = np.float32


def gpu(x):
    return None if x is None else torch.from_numpy(np.array(x)).to(DEV)         # a copy: the shared cases are read-only


def host(t):
    return t.cpu().numpy()


def sprinkle(rng, a, share=0.03):
    """NaN, +inf and -inf over `share` of a."""
    bad = rng.random(a.shape) < share
    a[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), int(bad.sum()))
    return a


@functools.lru_cache(maxsize=None)
def maps(B, H, W, quantised, seed=0):
    """fp32 [B, H, W]: multiples of 1/8 in [-1, 1] (exact band edges, integral py, exact ties, both zeros) or normal values, negative
    ones among them; NaN and +-inf sprinkled; a few d large enough to leave the image, up to the largest float."""
    rng = np.random.default_rng([61, B, H, W, quantised, seed])
    d = (rng.integers(-8, 9, (B, H, W)) / 8).astype(F) if quantised else rng.standard_normal((B, H, W)).astype(F)
    d[rng.random(d.shape) < 0.05] = -0.0
    far = rng.random(d.shape) < 0.04
    d[far] = rng.choice(np.array([1000.0, -1000.0, 3.0e38, -3.0e38, 40.0, -17.5], F), int(far.sum()))
    sprinkle(rng, d)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def view_maps(B, N, H, W, quantised):
    rng = np.random.default_rng([62, B, N, H, W, quantised])
    dv = (rng.integers(-10, 11, (B, N, H, W)) / 8).astype(F) if quantised else (1.3 * rng.standard_normal((B, N, H, W))).astype(F)
    sprinkle(rng, dv)
    dv.setflags(write=False)
    return dv


@functools.lru_cache(maxsize=None)
def deltas(N):
    """fp32 [N, 2]: (0, 0) first, then whole, half and quarter steps in [-2, 2]."""
    rng = np.random.default_rng([63, N])
    t = (rng.integers(-8, 9, (N, 2)) / 4).astype(F)
    t[::3] = np.round(t[::3])
    t[0] = 0
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def mask(kind, B, H, W, reach=5):
    """uint8 [B, H, W] or None: the share of invalid pixels of "10" and "60", all invalid, one valid pixel, a hole wider than `reach`."""
    rng = np.random.default_rng([64, B, H, W, len(kind)])
    if kind == "null":
        return None
    if kind in ("10", "60"):
        m = (rng.random((B, H, W)) >= int(kind) / 100).astype(np.uint8) * rng.integers(1, 256, (B, H, W)).astype(np.uint8)     # any non-zero byte is valid
    elif kind == "none":
        m = np.zeros((B, H, W), np.uint8)
    elif kind == "one":
        m = np.zeros((B, H, W), np.uint8)
        m[:, H // 2, W // 3] = 1
    else:
        m = np.ones((B, H, W), np.uint8)
        m[:, :, W // 4:W // 4 + 2 * reach + 3] = 0
        m[:, H // 4:H // 4 + 2 * reach + 3, :] = 0
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def guide(B, H, W, C):
    """uint8 [B, H, W, C]: flat regions with a step edge and some noise, so that equal and very different guides both occur."""
    rng = np.random.default_rng([65, B, H, W, C])
    g = np.where(np.arange(W)[None, None, :, None] * 2 < W, 40, 200) + rng.integers(-12, 13, (B, H, W, C))
    g = np.clip(g, 0, 255).astype(np.uint8)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def table(kind, C):
    if kind == "ones":
        return RU.range_table_np(None, C)
    if kind == "range":
        return RU.range_table_np(0.05, C)
    t = RU.range_table_np(0.05, C).copy()                           # zeros from s = 6 on, and at s = 0 itself: T = 0 occurs
    t[6:] = 0
    t[0] = 0
    return t


# ---- 1. the check ----
CHECKS = [(1, True, "larger", 0.0, (0, 0)), (4, True, "smaller", 0.125, (1, 0)), (24, True, "larger", 0.125, (3, 1)), (128, True, "larger", 0.3, (1, 0)),
          (4, False, "larger", 0.3, (3, 1)), (24, False, "smaller", 0.0, (0, 0)), (128, False, "smaller", 0.125, (3, 1)), (1, False, "larger", 0.125, (1, 0))]


@pytest.mark.parametrize("B", BATCH)
@pytest.mark.parametrize("H,W", SHAPES)
def test_check_equals_the_restatement(H, W, B):
    seen = np.zeros(4, np.int64)
    for N, quantised, near, tau, (min_agree, max_conflict) in CHECKS:
        dr, dv, dl = maps(B, H, W, quantised), view_maps(B, N, H, W, quantised), deltas(N)
        want = RU.check_np(dr, dv, dl, tau, near, min_agree, max_conflict)
        got = R.consistency(gpu(dr), gpu(dv), dl, tau=tau, near=near, min_agree=min_agree, max_conflict=max_conflict)
        for name, g, w in zip(got._fields, got, want):
            assert g.dtype == torch.uint8 and np.array_equal(host(g), w), (name, N, quantised, near, tau, int((host(g) != w).sum()))
        seen += [int(want[1].max()), int(want[2].max()), int(want[0].max()), int((want[0] == 0).sum())]
        assert not want[0][~np.isfinite(dr)].any() and not want[1][~np.isfinite(dr)].any()
    if H * W > 100:
        assert seen.all(), seen                                      # agreeing and conflicting views, valid and invalid pixels all occur
    # a single map [H, W] with its views [N, H, W], and a reference that makes the offsets
    dr, dv, dl = maps(B, H, W, True), view_maps(B, 4, H, W, True), deltas(4)
    got = R.consistency(gpu(dr[0]), gpu(dv[0]), dl.astype(np.float64) + np.array([2.0, 1.5]), reference=(2.0, 1.5), tau=0.125)
    want = RU.check_np(dr[:1], dv[:1], dl, 0.125)
    assert all(np.array_equal(host(g), w[0]) for g, w in zip(got, want))


# ---- 2. the fill ----
@pytest.mark.parametrize("B", BATCH)
@pytest.mark.parametrize("H,W", SHAPES)
def test_fill_equals_the_restatement(H, W, B):
    seen = set()
    for reach in (0, 1, 5, 64):
        for kind in ("null", "10", "60", "none", "one", "wide"):
            for near in ("larger", "smaller"):
                d, m = maps(B, H, W, kind in ("null", "60", "one")), mask(kind, B, H, W, reach)
                want, want_holes = RU.fill_np(d, m, reach, near)
                got, holes = R.fill(gpu(d), gpu(m), reach, near)
                assert got.dtype == torch.float32 and holes.dtype == torch.uint8
                assert np.array_equal(host(holes), want_holes), (reach, kind, near, int((host(holes) != want_holes).sum()))
                assert RU.same_values(host(got), want), (reach, kind, near)
                keep = want_holes != 1                              # good pixels, and those nothing was found for, keep their bits
                assert np.array_equal(host(got).view(np.int32)[keep], d.view(np.int32)[keep])
                seen |= set(np.unique(want_holes).tolist())
    assert seen == ({0, 1, 2} if H * W > 1 else {0, 2})
    got, holes = R.fill(gpu(maps(B, H, W, True)[0]), None, 5)       # a single map [H, W]
    want, want_holes = RU.fill_np(maps(B, H, W, True)[:1], None, 5)
    assert RU.same_values(host(got), want[0]) and np.array_equal(host(holes), want_holes[0])


# ---- 3. the weighted median ----
MEDIANS = [(1, "ones", "null", True), (3, "range", "10", False), (4, "zeros", "60", True), (3, "ones", "none", True), (1, "range", "one", False),
           (4, "range", "wide", True), (3, "zeros", "null", False)]


@pytest.mark.parametrize("r", [0, 1, 3, 7])
@pytest.mark.parametrize("B", BATCH)
@pytest.mark.parametrize("H,W", SHAPES)
def test_wmedian_equals_the_restatement(H, W, B, r):
    seen = set()
    for C, tkind, mkind, quantised in MEDIANS:
        d, m, g, t = maps(B, H, W, quantised), mask(mkind, B, H, W), guide(B, H, W, C), table(tkind, C)
        want, want_flags = RU.wmedian_np(d, g, t, r, m)
        got, flags = R.weighted_median(gpu(d), gpu(g), r, gpu(m), table=t)
        assert got.dtype == torch.float32 and flags.dtype == torch.uint8
        assert np.array_equal(host(flags), want_flags), (C, tkind, mkind, int((host(flags) != want_flags).sum()))
        assert RU.same_values(host(got), want), (C, tkind, mkind, quantised)
        keep = want_flags == 2
        assert np.array_equal(host(got).view(np.int32)[keep], d.view(np.int32)[keep])       # T = 0: the bits of D
        seen |= set(np.unique(want_flags).tolist())
    assert seen == ({0, 1, 2} if H * W > 1 and r > 0 else {0, 2})       # a window of the pixel alone gives no value to a pixel that is not good
    # sigma in the table's place, a guide without a channel axis, a single map
    d, g = maps(B, H, W, True), guide(B, H, W, 1)
    got, flags = R.weighted_median(gpu(d[0]), gpu(g[0, ..., 0]), r, sigma=0.05)
    want, want_flags = RU.wmedian_np(d[:1], g[:1], RU.range_table_np(0.05, 1), r)
    assert RU.same_values(host(got), want[0]) and np.array_equal(host(flags), want_flags[0])


@pytest.mark.parametrize("H,W,B,r", [(33, 65, 2, 1), (33, 65, 1, 3), (5, 3, 2, 7), (66, 130, 1, 2)])
def test_wmedian_iterations_and_a_float_guide(H, W, B, r):
    d, m, g, t = maps(B, H, W, False), mask("60", B, H, W), guide(B, H, W, 3), table("zeros", 3)
    for iterations in (1, 3):
        want, want_flags = RU.wmedian_iter_np(d, g, t, r, m, iterations)
        got, flags = R.weighted_median(gpu(d), gpu(g), r, gpu(m), table=t, iterations=iterations)
        assert RU.same_values(host(got), want) and np.array_equal(host(flags), want_flags), iterations
    # an fp32 guide is quantised by refocus's rule: clip, x 255, round half to even
    gf = np.random.default_rng(66).uniform(-0.1, 1.1, (B, H, W, 3)).astype(F)
    gf[0, 0, 0] = (0.5 / 255, 1.5 / 255, 2.5 / 255)
    gq = np.rint(np.clip(gf, 0, 1) * F(255)).astype(np.uint8)
    assert np.array_equal(host(R.quantise_guide(gpu(gf))), gq)
    want, want_flags = RU.wmedian_np(d, gq, RU.range_table_np(0.1, 3), r, m)
    got, flags = R.weighted_median(gpu(d), gpu(gf), r, gpu(m))
    assert RU.same_values(host(got), want) and np.array_equal(host(flags), want_flags)


# ---- 4. independence of the surroundings ----
def test_a_crop_that_holds_a_pixels_support_gives_the_pixels_outputs():
    B, H, W = 2, 70, 90
    y0, y1, x0, x1 = 8, 61, 16, 83
    d, m, g = maps(B, H, W, True, seed=1), mask("60", B, H, W), guide(B, H, W, 3)
    crop = lambda a: None if a is None else np.ascontiguousarray(a[:, y0:y1, x0:x1])
    inner = lambda a, k: a[:, k:a.shape[1] - k, k:a.shape[2] - k]

    def same(full, part, k):
        a, b = inner(crop(host(full)), k), inner(host(part), k)
        return RU.same_values(a, b) if a.dtype == F else np.array_equal(a, b)

    # the check: quantised maps and offsets, so that fl(y + fl(d du)) is exact wherever the pixel lies; |d du| <= 2 away from the
    # values that leave the image, which are outside the crop as they are outside the image
    N = 4
    dv, dl = view_maps(B, N, H, W, True), deltas(N)
    dr = np.where(np.abs(d) > 1, F(0.5), d)
    full = R.consistency(gpu(dr), gpu(dv), dl, tau=0.125, min_agree=1, max_conflict=1)
    part = R.consistency(gpu(crop(dr)), gpu(np.ascontiguousarray(dv[:, :, y0:y1, x0:x1])), dl, tau=0.125, min_agree=1, max_conflict=1)
    assert all(same(f, p, 3) for f, p in zip(full, part))
    for reach in (1, 5):
        full, part = R.fill(gpu(d), gpu(m), reach), R.fill(gpu(crop(d)), gpu(crop(m)), reach)
        assert all(same(f, p, reach) for f, p in zip(full, part))
    for r in (1, 3, 7):
        t = table("range", 3)
        full, part = R.weighted_median(gpu(d), gpu(g), r, gpu(m), table=t), R.weighted_median(gpu(crop(d)), gpu(crop(g)), r, gpu(crop(m)), table=t)
        assert all(same(f, p, r) for f, p in zip(full, part))


# ---- 5. capture ----
def test_captured_runs_replay_the_eager_bytes():
    B, H, W, N = 2, 33, 65, 4
    d, dv, m, g = gpu(maps(B, H, W, True)), gpu(view_maps(B, N, H, W, True)), gpu(mask("60", B, H, W)), gpu(guide(B, H, W, 3))
    runs = (lambda: R.consistency(d, dv, deltas(N), tau=0.125), lambda: R.fill(d, m, 5), lambda: R.weighted_median(d, g, 3, m, sigma=0.05, iterations=2))
    for run in runs:
        want = run()                                                 # eager; the tables are on the device from here on
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side, capture_error_mode=Tr.CAPTURE_MODE):
                got = run()
            for t in got:
                t.fill_(9)
            graph.replay()
        side.synchronize()
        torch.cuda.current_stream().wait_stream(side)
        for a, b in zip(got, want):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ---- 6. the chain ----
def same_tensors(a, b):
    if a is None or b is None or not isinstance(a, torch.Tensor):
        return a == b if not isinstance(a, torch.Tensor) else False
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("sweep_kw", [dict(), dict(radius=1, interp="cubic"), dict(regularize=dict(p1=0.002, p2=0.02, paths=4), occlusion="halves")],
                         ids=["plain", "radius-cubic", "sgm-occlusion"])
def test_refine_is_its_five_steps(sweep_kw):
    views = gpu(RU.noisy_two_layer()[:, :, 8:36, 4:44])             # [5, 5, 28, 40, 1]
    sl = RU.SLOPES
    kw = dict(positions="corners", tau=0.4, radius=2, sigma=0.08, iterations=2, reach=7, near="larger", min_agree=2, max_conflict=1)
    res = R.refine(views, sl, **kw, **{("sweep_radius" if k == "radius" else k): v for k, v in sweep_kw.items()})
    raw = Dm.disparity(views, sl, **sweep_kw)
    assert type(res.raw) is type(raw) and all(same_tensors(a, b) for a, b in zip(res.raw, raw))
    pos = R.view_positions(5, "corners")
    dv = R.disparity_views(views, sl, pos, **sweep_kw)
    assert dv.shape == (4, 28, 40)
    for n, p in enumerate(pos):                                      # every per-view map is made with the sweep's arguments
        assert same_tensors(dv[n], Dm.disparity(views, sl, centre=tuple(p), **sweep_kw).disparity)
    c = R.consistency(raw.disparity, dv, pos, reference=(2, 2), tau=0.4, min_agree=2, max_conflict=1)
    med, flags = R.weighted_median(raw.disparity, views[2, 2], 2, c.valid, 0.08, iterations=2)
    filled, _ = R.fill(med, (flags != 2).to(torch.uint8), 7)
    for name, a, b in (("disparity", res.disparity, filled), ("valid", res.valid, c.valid), ("agree", res.agree, c.agree), ("conflict", res.conflict, c.conflict),
                       ("flags", res.flags, flags)):
        assert same_tensors(a, b), name
    # the defaults: the cross, the largest slope step, the centre view
    as_refine = {("sweep_radius" if k == "radius" else k): v for k, v in sweep_kw.items()}      # `radius` is the median's there
    res = R.refine(views, sl, **as_refine)
    pos = R.view_positions(5, "cross")
    c = R.consistency(raw.disparity, R.disparity_views(views, sl, pos, **sweep_kw), pos, reference=(2, 2), tau=0.5)
    med, flags = R.weighted_median(raw.disparity, R.centre_view(views), 3, c.valid, 0.1)
    assert same_tensors(res.disparity, R.fill(med, (flags != 2).to(torch.uint8), 32)[0]) and same_tensors(res.valid, c.valid)
    # a batch of mosaics goes through with its batch axis
    mosaic = views[..., 0].permute(0, 2, 1, 3).reshape(1, 1, 5 * 28, 5 * 40).repeat(2, 1, 1, 1).contiguous()
    rb = R.refine(mosaic, sl, 5, **as_refine)
    assert rb.disparity.shape == (2, 28, 40) and same_tensors(rb.disparity[1], res.disparity) and same_tensors(rb.flags[0], res.flags)


def test_two_layer_scene():
    """Asserted: what the definitions guarantee.  Printed: the figures against the scene's known truth, before and after, for the
    plain sweep and for occlusion="halves"; no gate rests on them."""
    views, sl = gpu(RU.noisy_two_layer()), RU.SLOPES
    truth, band = RU.truth(), RU.band()
    half = 0.5 * (sl[1] - sl[0])
    for name, sweep_kw in (("plain", dict(sweep_radius=RU.SCENE["radius"])), ("halves", dict(sweep_radius=RU.SCENE["radius"], occlusion="halves"))):
        res = R.refine(views, sl, **sweep_kw)
        out, valid, conflict = host(res.disparity), host(res.valid), host(res.conflict)
        assert np.isfinite(out).all() and out.min() >= F(sl[0]) and out.max() <= F(sl[-1])
        assert not valid[conflict > 0].any()                         # max_conflict = 0
        wrong_raw, wrong = np.abs(host(res.raw.disparity) - truth) > half, np.abs(out - truth) > half
        marked = float((wrong_raw & (valid == 0)).sum()) / max(int(wrong_raw.sum()), 1)
        print(f"two-layer 48 x 64, {name}: wrong by more than half a slope step: band {int((wrong_raw & band).sum())} -> {int((wrong & band).sum())} of "
              f"{int(band.sum())}, all {int(wrong_raw.sum())} -> {int(wrong.sum())} of {truth.size}; invalid {int((valid == 0).sum())}, "
              f"share of the raw map's wrong pixels marked invalid {marked:.3f}")
