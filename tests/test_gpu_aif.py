"""GPU tests of the all-in-focus image from the winning partial aperture (lft_aif_at: k_aif_at; lft_amd.disparity.all_in_focus_at
and disparity(..., all_in_focus="subset")).

The anchor is bitwise: a pixel of subset p at index k has the bits of lft_refocus's stack for the masked aperture a * mask_p at
slice k (p = 0: the whole aperture), because a subset's row b_p is that aperture's `a` column bit for bit
(tests/test_aif_host.py::test_a_subset_row_is_the_masked_apertures_column).  The fp32 image is also held to refocus_util.tol against
the fp64 restatement (tests/aif_util.py): a pixel is a refocus value with other weights of sum 1."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from lft_amd import disparity as Dm, refocus as R

import aif_util as AU
import disparity_util as DU
import occlusion_util as OU
import refocus_util as RU

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def views(A, H, W, C, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (A, A, H, W, C)).astype(np.uint8)
    return rng.random((A, A, H, W, C)).astype(np.float32)


def held_out(A):
    """The full aperture without the view (0, 0): one of the apertures the table identity is asserted for."""
    a = np.ones((A, A))
    a[0, 0] = 0.0
    return a


def rows_of_three():
    m = np.zeros((3, 5, 5), bool)
    m[0, :2] = True                      # the first two view rows
    m[1, 2, 2] = True                    # the centre view alone: dropped
    m[2, :, 3:] = True                   # the last two view columns
    return m


# kept: P', the subsets that reach the kernel
CASES = {
    "A1_C1_f32_nearest_whole": dict(A=1, C=1, dtype=np.float32, interp="nearest", occ=None, kept=0),
    "A2_C3_u8_linear_halves": dict(A=2, C=3, dtype=np.uint8, interp="linear", occ="halves", kept=4),
    "A3_C4_f32_cubic_quadrants": dict(A=3, C=4, dtype=np.float32, interp="cubic", occ="quadrants", kept=4),
    "A5_C3_u8_linear_halves": dict(A=5, C=3, dtype=np.uint8, interp="linear", occ="halves", kept=4),
    "A5_C4_f32_linear_array": dict(A=5, C=4, dtype=np.float32, interp="linear", occ=dict(subsets=rows_of_three()), kept=2, shape=(9, 37)),
    "A3_C1_u8_cubic_one_subset": dict(A=3, C=1, dtype=np.uint8, interp="cubic", occ=dict(subsets=np.tril(np.ones((3, 3), bool))[None]), kept=1),
    "A3_C3_f32_linear_corner": dict(A=3, C=3, dtype=np.float32, interp="linear", occ="quadrants", kept=3, centre=(0, 0), aperture="held_out"),
    "A5_C1_f32_cubic_whole": dict(A=5, C=1, dtype=np.float32, interp="cubic", occ=None, kept=0, shape=(9, 37), aperture="gaussian"),
    "A3_C3_u8_nearest_one_pixel": dict(A=3, C=3, dtype=np.uint8, interp="nearest", occ="halves", kept=4, shape=(1, 1)),
    "A5_C4_u8_nearest_quadrants": dict(A=5, C=4, dtype=np.uint8, interp="nearest", occ="quadrants", kept=4, shape=(9, 37)),
}


def anchor_stacks(g, slopes, aperture, interp, centre, occ, out_dtype, angRes=None):
    """[1 + P'] stacks of lft_refocus: the whole aperture, then the aperture masked to each kept subset."""
    A = angRes or int(g.shape[0])
    stacks = [R.refocus(g, slopes, angRes, aperture, interp, out_dtype, centre)]
    if occ is not None:
        subsets, _, min_views = Dm._occlusion_arguments(occ)
        a = R._aperture(A, aperture)
        _, kept = Dm.subset_table(A, aperture, centre, subsets, min_views)
        masks = AU.subset_masks(A, centre, subsets)
        stacks += [R.refocus(g, slopes, angRes, a * masks[p], interp, out_dtype, centre) for p in kept]
    return stacks


def select(stacks, index, subset):
    """Per pixel the slice clamp(index) of stack subset (ids above P' count as 0): stacks of [D, H, W, C], maps [H, W]."""
    S = torch.stack(stacks)
    D = S.shape[1]
    k = index.long().clamp(0, D - 1)
    p = torch.zeros_like(k) if subset is None else subset.long()
    p = torch.where(p >= S.shape[0], torch.zeros_like(p), p)
    yy, xx = torch.meshgrid(torch.arange(k.shape[0], device=k.device), torch.arange(k.shape[1], device=k.device), indexing="ij")
    return S[p, k, yy, xx]


def maps(H, W, D, kept, seed, how):
    """(index int32, subset uint8) [H, W].  random: index uniform over -1 .. D (both clamps), subset over 0 .. P' + 1 per pixel;
    waves: the same draws per wave of k_aif_at (two rows of a 32-pixel-wide tile), so every wave is uniform; constant: one pair."""
    rng = np.random.default_rng(seed)
    if how == "random":
        k, p = rng.integers(-1, D + 1, (H, W)), rng.integers(0, kept + 2, (H, W))
    elif how == "waves":
        gy, gx = (H + 1) // 2, (W + 31) // 32
        k = rng.integers(-1, D + 1, (gy, gx)).repeat(2, 0).repeat(32, 1)[:H, :W]
        p = rng.integers(0, kept + 2, (gy, gx)).repeat(2, 0).repeat(32, 1)[:H, :W]
    else:
        k, p = np.full((H, W), D - 2), np.full((H, W), kept)
    return k.astype(np.int32), p.astype(np.uint8)


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_refocus_of_the_masked_apertures(name):
    """Random maps (the worst case for divergence), maps constant per wave and a constant map (the wave-uniform path): bitwise the
    per-pixel selection from refocus's stacks, fp32 and uint8 out; fp32 within refocus's bound of the restatement; and the same
    bits from either code path where the maps coincide."""
    c = CASES[name]
    A, C, interp, occ, centre = c["A"], c["C"], c["interp"], c["occ"], c.get("centre")
    H, W = c.get("shape", (33, 35))
    aperture = held_out(A) if c.get("aperture") == "held_out" else c.get("aperture", "full")
    lf = views(A, H, W, C, c["dtype"], seed=len(name))
    g = torch.from_numpy(lf).to(DEV)
    slopes, D, taps = RU.SLOPES, len(RU.SLOPES), R.TAPS[interp]
    table = R.shift_table(A, slopes, aperture, interp, centre)
    btable = None
    if occ is not None:
        subsets, _, min_views = Dm._occlusion_arguments(occ)
        btable, kept = Dm.subset_table(A, aperture, centre, subsets, min_views)
        assert len(kept) == c["kept"]
    tol = RU.tol(A, table, taps, 1.0 if lf.dtype == np.uint8 else float(np.abs(lf).max()))
    stacks = {dt: anchor_stacks(g, slopes, aperture, interp, centre, occ, dt) for dt in (torch.float32, torch.uint8)}
    assert len(stacks[torch.float32]) == 1 + c["kept"]
    got = {}
    for how in ("random", "waves", "constant"):
        k, p = maps(H, W, D, c["kept"], seed=len(name) + 1, how=how)
        index = torch.from_numpy(k).to(DEV)
        subset = torch.from_numpy(p).to(DEV) if occ is not None else None
        for dt in (torch.float32, torch.uint8):
            out = Dm.all_in_focus_at(g, slopes, index, subset, aperture=aperture, interp=interp, centre=centre, occlusion=occ, out_dtype=dt)
            assert out.dtype == dt and tuple(out.shape) == (H, W, C)
            want = select(stacks[dt], index, subset)
            differ = int((out != want).any(-1).sum())
            print(f"{name} {how} {dt}: differs from the selection of refocus's stacks at {differ} of {H * W} pixels")
            assert torch.equal(out.view(torch.int32) if dt == torch.float32 else out, want.view(torch.int32) if dt == torch.float32 else want), (name, how, dt)
            got[how, dt] = out
        ref = AU.aif_at_np(lf, table, taps, btable, k, p if occ is not None else None)
        err = float(np.abs(got[how, torch.float32].cpu().numpy().astype(np.float64) - ref).max())
        print(f"{name} {how}: max error against the restatement {err:.3e}, tol {tol:.3e}")
        assert err <= tol, (name, how)
    # either code path, the same bits: where a uniform wave's (k, p) is the random map's, clamped and folded as the kernel does
    kr, pr = maps(H, W, D, c["kept"], seed=len(name) + 1, how="random")
    fold = lambda k, p: (np.clip(k, 0, D - 1), np.where(p > c["kept"], 0, p) if occ is not None else np.zeros_like(p))
    for how in ("waves", "constant"):
        ku, pu = maps(H, W, D, c["kept"], seed=len(name) + 1, how=how)
        (a, b), (cc, d) = fold(kr, pr), fold(ku, pu)
        same = torch.from_numpy((a == cc) & (b == d)).to(DEV)
        for dt in (torch.float32, torch.uint8):
            x, y = got["random", dt][same], got[how, dt][same]
            assert torch.equal(x.view(torch.int32) if dt == torch.float32 else x, y.view(torch.int32) if dt == torch.float32 else y), (name, how, dt)
        print(f"{name}: {how} and random maps coincide at {int(same.sum())} pixels, the same bits")


def test_batch_of_mosaics_a_strided_window_two_calls_and_empty_shapes():
    A, H, W = 5, 33, 35
    rng = np.random.default_rng(11)
    big = torch.from_numpy(rng.random((2, 1, A * H + 3, A * W + 5)).astype(np.float32)).to(DEV)
    lf = big[:, :, 2:2 + A * H, 1:1 + A * W]
    assert not lf.is_contiguous()
    D = len(RU.SLOPES)
    index = torch.from_numpy(rng.integers(-1, D + 1, (2, H, W)).astype(np.int32)).to(DEV)
    subset = torch.from_numpy(rng.integers(0, 6, (2, H, W)).astype(np.uint8)).to(DEV)
    kw = dict(angRes=A, interp="cubic", occlusion="quadrants")
    out = Dm.all_in_focus_at(lf, RU.SLOPES, index, subset, **kw)
    assert out.dtype == torch.float32 and tuple(out.shape) == (2, H, W)
    stacks = anchor_stacks(lf, RU.SLOPES, "full", "cubic", None, "quadrants", torch.float32, angRes=A)      # each [B, D, H, W]
    for b in range(2):
        want = select([s[b][..., None] for s in stacks], index[b], subset[b])[..., 0]
        assert torch.equal(out[b].view(torch.int32), want.view(torch.int32)), b
    # two calls give the same bits, and so do the contiguous copy and maps that are windows of larger tensors
    wide_i, wide_s = torch.zeros(2, H + 2, W + 3, dtype=torch.int32, device=DEV), torch.zeros(2, H + 2, W + 3, dtype=torch.uint8, device=DEV)
    wide_i[:, 1:1 + H, 2:2 + W], wide_s[:, 1:1 + H, 2:2 + W] = index, subset
    for again in (Dm.all_in_focus_at(lf, RU.SLOPES, index, subset, **kw), Dm.all_in_focus_at(lf.contiguous(), RU.SLOPES, index, subset, **kw),
                  Dm.all_in_focus_at(lf, RU.SLOPES, wide_i[:, 1:1 + H, 2:2 + W], wide_s[:, 1:1 + H, 2:2 + W], **kw)):
        assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    # a mosaic [A*H, A*W] takes maps [H, W]
    one = Dm.all_in_focus_at(lf[0, 0], RU.SLOPES, index[0], subset[0], **kw)
    assert tuple(one.shape) == (H, W) and torch.equal(one.view(torch.int32), out[0].view(torch.int32))
    # strided views with channels: a window of a larger uint8 tensor
    bigv = torch.from_numpy(views(3, H + 4, W + 6, 4, np.uint8, 4)).to(DEV)
    win = bigv[:, :, 3:3 + H, 2:2 + W, :3]
    a = Dm.all_in_focus_at(win, RU.SLOPES, index[0], subset[0], occlusion="halves")
    assert a.dtype == torch.uint8 and torch.equal(a, Dm.all_in_focus_at(win.contiguous(), RU.SLOPES, index[0], subset[0], occlusion="halves"))
    # empty shapes: no work, the result's shape
    for shape in ((3, 3, 0, 7, 2), (3, 3, 6, 0, 2)):
        e = torch.zeros(shape, device=DEV)
        z = Dm.all_in_focus_at(e, RU.SLOPES, torch.zeros(shape[2:4], dtype=torch.int32, device=DEV), torch.zeros(shape[2:4], dtype=torch.uint8, device=DEV), occlusion="halves")
        assert tuple(z.shape) == (shape[2], shape[3], 2)
    zb = Dm.all_in_focus_at(torch.zeros(0, 1, 15, 20, device=DEV), RU.SLOPES, torch.zeros(0, 3, 4, dtype=torch.int32, device=DEV), angRes=5)
    assert tuple(zb.shape) == (0, 3, 4)
    r = Dm.disparity(torch.zeros(3, 3, 0, 7, device=DEV), [-1.0, 0.0, 1.0], occlusion="halves", all_in_focus="subset")
    assert tuple(r.all_in_focus.shape) == (0, 7) and tuple(r.subset.shape) == (0, 7)


def test_capture_and_replay():
    from lft_amd import train as T
    A, H, W = 3, 33, 40
    lf = torch.from_numpy(views(A, H, W, 3, np.uint8, 15)).to(DEV)
    rng = np.random.default_rng(16)
    index = torch.from_numpy(rng.integers(0, 5, (H, W)).astype(np.int32)).to(DEV)
    subset = torch.from_numpy(rng.integers(0, 5, (H, W)).astype(np.uint8)).to(DEV)
    sl = [-1.5, -0.4, 0.0, 0.75, 2.0]
    want = Dm.all_in_focus_at(lf, sl, index, subset, occlusion="halves")   # eager; the tables are on the device from here on
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side, capture_error_mode=T.CAPTURE_MODE):
            got = Dm.all_in_focus_at(lf, sl, index, subset, occlusion="halves")
        got.fill_(9)
        graph.replay()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(got, want)


SWEEP = [-1.5, -0.4, 0.0, 0.75, 2.0]


@pytest.mark.parametrize("regularize", [None, dict(p1=0.002, p2=0.02, paths=8)], ids=["wta", "sgm"])
def test_disparity_with_the_subset_image(regularize):
    """The maps, subset and cost are bitwise those of all_in_focus=True; the image is all_in_focus_at of the call's own maps."""
    for A, (H, W), C, dtype, occ, interp in ((5, (33, 35), 3, np.uint8, dict(subsets="halves", margin=1.0), "linear"),
                                                 (3, (9, 37), 4, np.float32, dict(subsets="quadrants", margin=1.0), "cubic")):
        g = torch.from_numpy(views(A, H, W, C, dtype, seed=A + C)).to(DEV)
        kw = dict(interp=interp, radius=1, cost_volume=True, occlusion=occ, regularize=regularize)
        for aif_dtype in (None, torch.float32, torch.uint8):
            old = Dm.disparity(g, SWEEP, all_in_focus=True, aif_dtype=aif_dtype, **kw)
            new = Dm.disparity(g, SWEEP, all_in_focus="subset", aif_dtype=aif_dtype, **kw)
            assert type(new) is Dm.OcclusionDisparityResult and new.subsets_kept == old.subsets_kept
            for field in ("disparity", "confidence", "index", "subset", "cost"):
                x, y = getattr(old, field), getattr(new, field)
                assert x.dtype == y.dtype and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), field
            want_dtype = aif_dtype or g.dtype
            assert new.all_in_focus.dtype == want_dtype and new.all_in_focus.shape == old.all_in_focus.shape
            image = Dm.all_in_focus_at(g, SWEEP, new.index, new.subset, interp=interp, occlusion=occ, out_dtype=aif_dtype)
            assert torch.equal(new.all_in_focus, image)
            assert bool(new.subset.any()) and not torch.equal(new.all_in_focus, old.all_in_focus)     # random views: subsets do win, and the image moves
        # one all-true subset and margin 1: b_1 is the record's own weight, so the image is the True image bit for bit
        whole = dict(subsets=np.ones((1, A, A), bool), margin=1.0)
        kw["occlusion"] = whole
        old, new = Dm.disparity(g, SWEEP, all_in_focus=True, aif_dtype=torch.float32, **kw), Dm.disparity(g, SWEEP, all_in_focus="subset", aif_dtype=torch.float32, **kw)
        assert torch.equal(old.all_in_focus.view(torch.int32), new.all_in_focus.view(torch.int32))
        ones = torch.ones_like(new.subset)
        assert torch.equal(Dm.all_in_focus_at(g, SWEEP, new.index, ones, interp=interp, occlusion=whole, out_dtype=torch.float32).view(torch.int32),
                           old.all_in_focus.view(torch.int32))


@functools.lru_cache(maxsize=None)
def centre_view():
    clean, centre = DU.two_layer(5, 40, 40, box=OU.BOX)
    return clean, centre.astype(np.float64)


@pytest.mark.parametrize("subsets", ["halves", "quadrants"])
def test_the_band_round_the_foreground_loses_its_ghost(subsets):
    """The feature test: on the noisy two-layer scene the image gathered from all views is off by more than 0.05 at >= 100 of the
    320 band pixels, the winning subset's image at none; on the clean scene it is the centre view within refocus's bound."""
    S, band = OU.SCENE, OU.band()
    clean, centre = centre_view()
    g = torch.from_numpy(OU.noisy_two_layer()).to(DEV)
    kw = dict(interp=S["interp"], radius=S["radius"], occlusion=dict(subsets=subsets, margin=S["beta"]), aif_dtype=torch.float32)
    old = Dm.disparity(g, OU.SLOPES, all_in_focus=True, **kw)
    new = Dm.disparity(g, OU.SLOPES, all_in_focus="subset", **kw)
    off_old = np.abs(old.all_in_focus.cpu().numpy()[..., 0].astype(np.float64) - centre)[band]
    off_new = np.abs(new.all_in_focus.cpu().numpy()[..., 0].astype(np.float64) - centre)[band]
    print(f"{subsets}, noisy: all views off by > 0.05 at {int((off_old > 0.05).sum())} of {int(band.sum())} band pixels (max {off_old.max():.4f}), "
          f"the winning subset at {int((off_new > 0.05).sum())} (max {off_new.max():.4f})")
    assert band.sum() == 320 and int((off_old > 0.05).sum()) >= 100
    assert int((off_new > 0.05).sum()) == 0
    r = Dm.disparity(torch.from_numpy(clean).to(DEV), OU.SLOPES, all_in_focus="subset", **kw)
    err = float(np.abs(r.all_in_focus.cpu().numpy()[..., 0].astype(np.float64) - centre)[band].max())
    tol = RU.tol(S["A"], R.shift_table(S["A"], OU.SLOPES, "full", S["interp"]), R.TAPS[S["interp"]], 1.0)
    print(f"{subsets}, clean: within {err:.3e} of the centre view on the band, tol {tol:.3e}")
    assert err <= tol


def test_tool_writes_the_subset_image(golden_dir, tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import disparity as tool
    from lft_amd import png, prepare
    A = 3
    mat = os.path.join(golden_dir, "prepare_lf_v73.mat")
    lf = prepare.to_device(prepare.load_lf(mat), A, DEV)             # [3, 3, 9, 7, 3] uint8
    slopes = [-1.0, -0.5, 0.0, 0.5, 1.0]
    names = ["disparity.png", "confidence.png", "all_in_focus.png", "disparity.npy", "occlusion.png"]
    base = ["--lf", mat, "--angRes", str(A), "--slopes=-1:1:5", "--radius", "1", "--occlusion", "quadrants", "--margin", "1.0"]
    occ = dict(subsets="quadrants", margin=1.0, min_views=2)
    images = {}
    for flags, how in ((["--subset_aif"], "subset"), ([], True)):
        out_dir = str(tmp_path / ("with" if flags else "without"))
        paths = tool.main(base + ["--out_dir", out_dir] + flags)
        assert [os.path.basename(p) for p in paths] == names and sorted(os.listdir(out_dir)) == sorted(names)
        want = Dm.disparity(lf, slopes, radius=1, occlusion=occ, all_in_focus=how, aif_dtype=torch.uint8)
        images[how] = png.read_png(os.path.join(out_dir, "all_in_focus.png"))
        assert np.array_equal(images[how], want.all_in_focus.cpu().numpy())
        assert np.array_equal(np.load(os.path.join(out_dir, "disparity.npy")), want.disparity.cpu().numpy())
        assert np.array_equal(png.read_png(os.path.join(out_dir, "occlusion.png")), (want.subset.cpu().numpy() * 63)[..., None].repeat(3, axis=2))
    with pytest.raises(SystemExit):
        tool.main(["--lf", mat, "--angRes", str(A), "--out_dir", str(tmp_path / "refused"), "--subset_aif"])
    assert not os.path.exists(str(tmp_path / "refused"))
