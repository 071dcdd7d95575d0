"""GPU tests of the occlusion-aware sweep cost (lft_disparity_occ: k_sweep_cost_occ + k_disparity_pick + k_occ_gather,
lft_amd.disparity(..., occlusion=)) against the fp64 numpy restatement of its definition (tests/occlusion_util.py), which takes the
same fp32-rounded tables.

E is held to the derived bound tol_occ = max(1, beta) tol_E + 2^-24 beta C S^4 X^2 (occlusion_util's docstring).  Index, disparity
and confidence are then checked from the GPU's own E with the selection steps restated in numpy float32 (``pick_np``), bit for bit,
and the all-in-focus image against refocus's fp32 stack, bit for bit.  `subset` is compared with the restatement's choice where that
is well conditioned (occlusion_util.well_conditioned with the same bound)."""
import functools

import numpy as np
import pytest
import torch

from lft_amd import disparity as Dm, refocus as R, views as V

import disparity_util as DU
import occlusion_util as OU
import refocus_util as RU

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SLOPES = [-1.5, -0.4, 0.0, 0.75, 2.0]


def views(A, H, W, C, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (A, A, H, W, C)).astype(np.uint8)
    return rng.random((A, A, H, W, C)).astype(np.float32)


def held_out(A, seed):
    """A random aperture whose view (0, 0) has weight 0, every other one a positive weight."""
    a = 0.25 + np.random.default_rng(seed).random((A, A))
    a[0, 0] = 0.0
    return a


def rows_of_three():
    m = np.zeros((3, 5, 5), bool)
    m[0, :2] = True                      # the first two view rows
    m[1, 2, 2] = True                    # the centre view alone: dropped
    m[2, :, 3:] = True                   # the last two view columns
    return m


CASES = {
    "A5_C3_u8_linear_halves": dict(A=5, C=3, dtype=np.uint8, interp="linear", occ=dict(subsets="halves", margin=1.0), radius=1, kept=4),
    "A3_C4_f32_cubic_quadrants": dict(A=3, C=4, dtype=np.float32, interp="cubic", occ="quadrants", radius=2, kept=4),
    "A2_C1_f32_nearest_halves": dict(A=2, C=1, dtype=np.float32, interp="nearest", occ=dict(subsets="halves", margin=1.0), radius=0, kept=4),
    "A3_C1_u8_cubic_one_subset": dict(A=3, C=1, dtype=np.uint8, interp="cubic", occ=dict(subsets=np.tril(np.ones((3, 3), bool))[None], margin=4.0), radius=1, kept=1),
    "A5_C4_f32_linear_array": dict(A=5, C=4, dtype=np.float32, interp="linear", occ=dict(subsets=rows_of_three(), margin=1.5), radius=3, kept=2, shape=(9, 37)),
    "A3_C3_f32_linear_corner": dict(A=3, C=3, dtype=np.float32, interp="linear", occ="quadrants", radius=1, kept=3, centre=(0, 0), aperture="held_out"),
    "A2_C3_u8_linear_corner": dict(A=2, C=3, dtype=np.uint8, interp="linear", occ=dict(subsets="halves", margin=1.0), radius=1, kept=2, centre=(0, 0),
                                   aperture="held_out"),
}


def restate(lf, A, slopes, aperture, interp, centre, occ, radius):
    """The fp64 restatement for one light field [A, A, H, W, C]: (dict of occ_cost_np, E, the bound on E, kept ids)."""
    subsets, beta, min_views = Dm._occlusion_arguments(occ)
    a = R._aperture(A, aperture)
    table = R.shift_table(A, slopes, aperture, interp, centre)
    btable, kept = OU.subset_table_np(A, a, R._centre(A, centre), subsets, min_views)
    taps = R.TAPS[interp]
    o = OU.occ_cost_np(lf, table, taps, btable, beta)
    max_abs = 1.0 if lf.dtype == np.uint8 else float(np.abs(lf).max())
    return o, DU.aggregate_np(o["V"], radius), OU.tol_occ(A, lf.shape[-1], radius, table, taps, max_abs, beta), kept


def check_selection_bits(r, slopes, what):
    """index, disparity and confidence equal steps 4-6 applied in float32 to the result's own cost volume, bit for bit."""
    E = r.cost.cpu().numpy()
    lead = E.ndim == 4
    for b in range(E.shape[0] if lead else 1):
        Eb = E[b] if lead else E
        k, disp, conf = DU.pick_np(Eb, slopes)
        got = [(t[b] if lead else t).cpu().numpy() for t in (r.index, r.disparity, r.confidence)]
        d_err = float(np.abs(got[1].astype(np.float64) - disp).max(initial=0))
        c_err = float(np.abs(got[2].astype(np.float64) - conf).max(initial=0))
        print(f"{what}: index differs at {int((got[0] != k).sum())}, disparity by {d_err:.2e}, confidence by {c_err:.2e} from pick_np")
        assert got[0].dtype == np.int32 and np.array_equal(got[0], k), what
        assert np.array_equal(got[1].view(np.int32), disp.view(np.int32)), (what, d_err)
        assert np.array_equal(got[2].view(np.int32), conf.view(np.int32)), (what, c_err)


def check_subset(subset, index, o, tol, what, where=None):
    """`subset` against the restatement's choice at the GPU's index, at the well-conditioned pixels (of `where`); returns the
    share left out."""
    k = index.cpu().numpy().astype(np.int64)
    want = np.take_along_axis(o["choice"], k[None], 0)[0]
    ok = np.take_along_axis(OU.well_conditioned(o, tol), k[None], 0)[0]
    if where is not None:
        ok &= where
    got = subset.cpu().numpy()
    wrong = int((got[ok] != want[ok]).sum())
    left_out = 1.0 - float(ok.sum()) / float(ok.size if where is None else where.sum())
    print(f"{what}: subset differs at {wrong} of {int(ok.sum())} well-conditioned pixels, {left_out:.3f} left out; ids seen {sorted(set(got.reshape(-1).tolist()))}")
    assert subset.dtype == torch.uint8 and got.shape == want.shape and wrong == 0, what
    return left_out


@pytest.mark.parametrize("name", list(CASES))
def test_cost_selection_aif_and_subset(name):
    """Tests 4, 5 and 6 on 33 x 35 views: ragged tiles on both axes."""
    c = CASES[name]
    A, C = c["A"], c["C"]
    H, W = c.get("shape", (33, 35))
    lf = views(A, H, W, C, c["dtype"], seed=len(name))
    aperture = held_out(A, 5) if c.get("aperture") == "held_out" else "full"
    centre = c.get("centre")
    o, E, tol, kept = restate(lf, A, SLOPES, aperture, c["interp"], centre, c["occ"], c["radius"])
    assert len(kept) == c["kept"]
    g = torch.from_numpy(lf).to(DEV)
    r = Dm.disparity(g, SLOPES, aperture=aperture, interp=c["interp"], radius=c["radius"], centre=centre, cost_volume=True, all_in_focus=True,
                     aif_dtype=torch.float32, occlusion=c["occ"])
    assert r.subsets_kept == kept and r.cost.dtype == torch.float32 and tuple(r.cost.shape) == E.shape
    err = float(np.abs(r.cost.cpu().numpy().astype(np.float64) - E).max())
    print(f"{name}: max error of E {err:.3e}, tol_occ {tol:.3e}; choice != 0 at {float((o['choice'] != 0).mean()):.3f} of the volume")
    assert err <= tol, name
    check_selection_bits(r, SLOPES, name)
    stack = R.refocus(g, SLOPES, aperture=aperture, interp=c["interp"], out_dtype=torch.float32, centre=centre)
    assert torch.equal(r.all_in_focus, stack.gather(0, r.index.long()[None, :, :, None].expand(1, H, W, C))[0]), name
    check_subset(r.subset, r.index, o, tol, name)
    # the choice volume: the same comparison at every slope, and subset is its gather
    vol = Dm.occlusion_volume(g, SLOPES, aperture=aperture, interp=c["interp"], centre=centre, occlusion=c["occ"])
    assert vol.dtype == torch.uint8 and tuple(vol.shape) == o["choice"].shape and int(vol.max()) <= len(kept)
    ok = OU.well_conditioned(o, tol)
    assert np.array_equal(vol.cpu().numpy()[ok], o["choice"][ok]), name
    assert torch.equal(r.subset, vol.gather(0, r.index.long()[None])[0]) and torch.equal(r.subset, Dm.gather_choice(r.index, vol))


def test_batch_of_mosaics_through_strides():
    """B = 2 of the network's mosaic batch [B, 1, A*H, A*W], a window of a larger tensor; also test 10's strided window."""
    A, H, W = 5, 33, 35
    rng = np.random.default_rng(11)
    big = torch.from_numpy(rng.random((2, 1, A * H + 3, A * W + 5)).astype(np.float32)).to(DEV)
    lf = big[:, :, 2:2 + A * H, 1:1 + A * W]
    assert not lf.is_contiguous()
    kw = dict(angRes=A, interp="linear", radius=2, cost_volume=True, all_in_focus=True, occlusion="halves")
    r = Dm.disparity(lf, SLOPES, **kw)
    assert tuple(r.cost.shape) == (2, len(SLOPES), H, W) and tuple(r.subset.shape) == (2, H, W) and r.subsets_kept == (0, 1, 2, 3)
    host = lf.cpu().numpy()
    for b in range(2):
        v5 = host[b, 0].reshape(A, H, A, W).transpose(0, 2, 1, 3)[..., None].copy()
        o, E, tol, _ = restate(v5, A, SLOPES, "full", "linear", None, "halves", 2)
        err = float(np.abs(r.cost[b].cpu().numpy().astype(np.float64) - E).max())
        print(f"batch element {b}: max error of E {err:.3e}, tol_occ {tol:.3e}")
        assert err <= tol
        check_subset(r.subset[b], r.index[b], o, tol, f"batch element {b}")
    check_selection_bits(r, SLOPES, "batch")
    stack = R.refocus(lf, SLOPES, angRes=A, interp="linear", out_dtype=torch.float32)
    assert torch.equal(r.all_in_focus, stack.gather(1, r.index.long()[:, None])[:, 0])
    # two calls give the same bits, and so does the contiguous copy
    for again in (Dm.disparity(lf, SLOPES, **kw), Dm.disparity(lf.contiguous(), SLOPES, **kw)):
        for x, y in zip(r[:6], again[:6]):
            assert torch.equal(x, y)
    assert torch.equal(Dm.occlusion_volume(lf, SLOPES, angRes=A), Dm.occlusion_volume(lf.contiguous(), SLOPES, angRes=A))


def test_strided_views_give_the_same_bits():
    A, H, W, C = 3, 33, 35, 3
    big = torch.from_numpy(views(A, H + 4, W + 6, C + 1, np.uint8, 4)).to(DEV)
    lf = big[:, :, 3:3 + H, 2:2 + W, :C]
    kw = dict(interp="cubic", radius=1, cost_volume=True, all_in_focus=True, occlusion="quadrants")
    a, b, c = Dm.disparity(lf, SLOPES, **kw), Dm.disparity(lf, SLOPES, **kw), Dm.disparity(lf.contiguous(), SLOPES, **kw)
    for other in (b, c):
        for x, y in zip(a[:6], other[:6]):
            assert torch.equal(x, y)


@pytest.mark.parametrize("interp", ["nearest", "linear", "cubic"])
def test_one_whole_subset_and_margin_one_is_the_plain_sweep(interp):
    """The anchor: b_1 = fl32(a / 1) is the record's own weight, so V_1 = V_full bit for bit, U = V_1 and V = V_full."""
    for A, (H, W), C, dtype, aperture in ((5, (33, 35), 3, np.uint8, "full"), (3, (9, 37), 4, np.float32, "gaussian"), (2, (33, 35), 1, np.float32, RU.user_aperture(2, 1))):
        g = torch.from_numpy(views(A, H, W, C, dtype, seed=A + C)).to(DEV)
        kw = dict(aperture=aperture, interp=interp, radius=2, cost_volume=True, all_in_focus=True)
        plain = Dm.disparity(g, RU.SLOPES, **kw)
        occ = Dm.disparity(g, RU.SLOPES, occlusion=dict(subsets=np.ones((1, A, A), bool), margin=1.0), **kw)
        for name, x, y in zip(plain._fields[:5], plain[:5], occ[:5]):
            assert torch.equal(x, y), (A, interp, name)
        assert plain.subset is None and plain.subsets_kept is None and occ.subsets_kept == (0,)
        assert occ.subset.dtype == torch.uint8 and not bool(occ.subset.any())
        assert not bool(Dm.occlusion_volume(g, RU.SLOPES, aperture=aperture, interp=interp, occlusion=dict(subsets=np.ones((1, A, A), bool), margin=1.0)).any())


@functools.lru_cache(maxsize=None)
def scene():
    S = OU.SCENE
    L = OU.noisy_two_layer()
    o, E, tol, _ = restate(L, S["A"], OU.SLOPES, "full", S["interp"], None, dict(subsets=S["subsets"], margin=S["beta"]), S["radius"])
    return L, o, E, tol


def test_the_band_round_the_foreground_gets_the_background_slope():
    """The feature test: on the noisy two-layer scene the plain sweep picks a wrong slope in the band the rectangle's images reach,
    and the occlusion-aware cost picks the background's at every band pixel."""
    S = OU.SCENE
    L, o, E, tol = scene()
    band = OU.band()
    g = torch.from_numpy(L).to(DEV)
    plain = Dm.disparity(g, OU.SLOPES, interp=S["interp"], radius=S["radius"])
    wrong_plain = int((plain.index.cpu().numpy()[band] != OU.K_BG).sum())
    r = Dm.disparity(g, OU.SLOPES, interp=S["interp"], radius=S["radius"], cost_volume=True, occlusion=S["subsets"])
    k = r.index.cpu().numpy()
    wrong_new = int((k[band] != OU.K_BG).sum())
    err = float(np.abs(r.cost.cpu().numpy().astype(np.float64) - E).max())
    print(f"band of {int(band.sum())}: plain wrong at {wrong_plain}, occlusion-aware at {wrong_new}; max error of E {err:.3e}, tol_occ {tol:.3e}")
    assert band.sum() == 320 and wrong_plain >= 50
    assert wrong_new == 0
    assert err <= tol
    fg, _ = DU.two_layer_interiors(S["A"], S["H"], S["W"], S["radius"], box=OU.BOX)
    assert np.all(k[fg] == OU.K_FG)
    # subset against the restatement: at most a quarter of the interior may be left out, and the band is an occlusion edge
    left_out = check_subset(r.subset, r.index, o, tol, "scene", where=OU.interior())
    assert left_out <= 0.25
    assert float((r.subset.cpu().numpy()[band] != 0).mean()) >= 0.9
    # quadrants, other margins and the pass-through of the keyword
    for occ in ("quadrants", dict(margin=4.0), dict(margin=8.0)):
        kq = Dm.disparity(g, OU.SLOPES, interp=S["interp"], radius=S["radius"], occlusion=occ).index.cpu().numpy()
        print(f"{occ}: wrong at {int((kq[band] != OU.K_BG).sum())} band pixels")
    same = Dm.disparity_error(g, g, OU.SLOPES, interp=S["interp"], radius=S["radius"], occlusion="halves", min_confidence=0.0)
    assert same == (0.0, 1.0)
    loo = V.leave_one_out(g, OU.SLOPES, positions=[(2, 2), (0, 0)], radius=S["radius"], occlusion="halves")
    assert len(loo) == 2 and all(np.isfinite(s) for s in loo), loo


def test_regularize_runs_on_the_new_cost():
    S = OU.SCENE
    L, _, _, _ = scene()
    g = torch.from_numpy(L).to(DEV)
    swept = Dm.disparity(g, OU.SLOPES, interp=S["interp"], radius=S["radius"], cost_volume=True, occlusion="halves")
    p1, p2 = Dm.penalties_from_cost(swept.cost)
    how = dict(p1=p1, p2=p2, paths=8)
    r = Dm.disparity(g, OU.SLOPES, interp=S["interp"], radius=S["radius"], all_in_focus=True, aif_dtype=torch.float32, cost_volume=True,
                     regularize=how, occlusion="halves")
    stack = R.refocus(g, OU.SLOPES, interp=S["interp"], out_dtype=torch.float32)
    want = Dm.regularize(swept.cost, OU.SLOPES, stack=stack, aif_dtype=torch.float32, aggregated=True, **how)
    for name, x, y in zip(want._fields[:5], want[:5], r[:5]):
        assert torch.equal(x, y), name
    vol = Dm.occlusion_volume(g, OU.SLOPES, interp=S["interp"], occlusion="halves")
    assert r.subsets_kept == (0, 1, 2, 3) and torch.equal(r.subset, vol.gather(0, r.index.long()[None])[0])
    # without occlusion the regularized result has no subset
    assert Dm.disparity(g, OU.SLOPES, interp=S["interp"], radius=S["radius"], regularize=how).subset is None


def test_tool_writes_the_occlusion_map(golden_dir, tmp_path):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import disparity as tool
    from lft_amd import png, prepare
    A = 3
    mat = os.path.join(golden_dir, "prepare_lf_v73.mat")
    lf = prepare.to_device(prepare.load_lf(mat), A, DEV)             # [3, 3, 9, 7, 3] uint8
    slopes = [-1.0, -0.5, 0.0, 0.5, 1.0]
    names = ["disparity.png", "confidence.png", "all_in_focus.png", "disparity.npy", "occlusion.png"]
    for flags, occ in ((["--occlusion"], dict(subsets="halves", margin=2.0, min_views=2)),
                       (["--occlusion", "quadrants", "--margin", "1.0", "--min_views", "3"], dict(subsets="quadrants", margin=1.0, min_views=3))):
        out_dir = str(tmp_path / "_".join(flags).strip("-"))
        paths = tool.main(["--lf", mat, "--angRes", str(A), "--out_dir", out_dir, "--slopes=-1:1:5", "--radius", "1"] + flags)
        assert [os.path.basename(p) for p in paths] == names and sorted(os.listdir(out_dir)) == sorted(names)
        want = Dm.disparity(lf, slopes, radius=1, occlusion=occ)
        assert np.array_equal(np.load(os.path.join(out_dir, "disparity.npy")), want.disparity.cpu().numpy())
        grey = (want.subset.cpu().numpy() * 63)[..., None].repeat(3, axis=2)
        assert np.array_equal(png.read_png(os.path.join(out_dir, "occlusion.png")), grey)
