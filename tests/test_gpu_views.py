"""GPU tests of view synthesis (lft_view_render / k_view_splat + k_view_render, lft_amd.views) against the numpy restatement of its
definition (tests/views_util.py): the target map and the holes bit for bit against the float32 restatement, the views against the
fp64 one within the derived bound tol_render (3.2e-6 for 24 views, linear, 8.4e-6 for 25 views, cubic, on [0, 1] data)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import views as V
from lft_amd._lib import LftError

import disparity_util as DU
import refocus_util as RU
import views_util as VU

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H, W, T = 37, 45, 3                                     # one past a 32 x 32 splat tile and a 32 x 8 render tile in either direction
RANGE = (-1.5, 2.0)


def field(A, h, w, C, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (A, A, h, w, C)).astype(np.uint8)
    return rng.random((A, A, h, w, C)).astype(np.float32)


def disparity_map(h, w, seed, bad=0.03):
    """Random in (-1.6, 2.1): one pixel in twenty outside RANGE (clamped: no more, because a clamped value times half a view
    step is a dyadic fraction, and a single view sampled there has exact byte ties); the share `bad` NaN, two inf (skipped)."""
    rng = np.random.default_rng(seed)
    d = (rng.random((h, w)) * 3.7 - 1.6).astype(np.float32)
    d[rng.random((h, w)) < bad] = np.nan
    d[3, 5], d[h - 2, w - 1] = np.inf, -np.inf
    return d


def targets_of(A):
    """Inside the grid, on its edge, half a view step outside it."""
    return [(0.37 * (A - 1), 0.81 * (A - 1)), (A - 1.0, 0.25 * (A - 1)), (-0.5, A - 0.5)]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("A", [1, 2, 3, 5])
def test_parity(A, interp):
    taps = V.TAPS[interp]
    tg = targets_of(A)
    rec = V.record_table(A, tg, V.blend_weights(A, tg, "gaussian"))
    deltas = V.target_deltas(A, tg)
    n = 0
    for C in (1, 3, 4):
        for dtype in (np.uint8, np.float32):
            for near in ("larger", "smaller"):
                lf, Dr = field(A, H, W, C, dtype, seed=n), disparity_map(H, W, seed=100 + n)
                got = V.render(torch.from_numpy(lf).to(DEV), torch.from_numpy(Dr).to(DEV), tg, RANGE, blend="gaussian", interp=interp, near=near,
                               out_dtype=torch.float32)
                assert tuple(got.views.shape) == (T, H, W, C) and got.views.dtype == torch.float32
                assert tuple(got.disparity.shape) == (T, H, W) and got.holes.dtype == torch.uint8
                as8 = V.render(torch.from_numpy(lf).to(DEV), torch.from_numpy(Dr).to(DEV), tg, RANGE, blend="gaussian", interp=interp, near=near,
                               out_dtype=torch.uint8).views.cpu().numpy() if dtype == np.uint8 else None
                for t in range(T):
                    Dt, holes = VU.fill_np(VU.splat_np(Dr, deltas[t], RANGE, near), Dr, RANGE, near)
                    what = f"A={A} {interp} C={C} {np.dtype(dtype).name} near={near} target {tg[t]}"
                    assert np.array_equal(bits(got.disparity[t].cpu().numpy()), bits(Dt)), what
                    assert np.array_equal(got.holes[t].cpu().numpy(), holes), what
                    ref = VU.render_np(lf, Dt, rec[t], taps)
                    tol = VU.tol_render(int((rec[t]["skip"] == 0).sum()), taps, 1.0)
                    err = float(np.abs(got.views[t].cpu().numpy().astype(np.float64) - ref).max())
                    print(f"{what}: holes {float(holes.mean()):.3f}, max error {err:.3e}, tol {tol:.3e}")
                    assert err <= tol, what
                    if as8 is not None:
                        tie = RU.tie_distance(ref) <= 255 * tol
                        assert tie.mean() <= 0.01, (what, float(tie.mean()))                # on the reference alone
                        diff = np.abs(as8[t].astype(np.int64) - RU.quantise(ref).astype(np.int64))
                        assert diff[~tie].max(initial=0) == 0 and diff.max() <= 1, what
                n += 1


def test_clamp_range_and_holes_are_exercised():
    """The parity inputs do reach what they are meant to: clamped values, skipped pixels, holes of either kind."""
    Dr = disparity_map(H, W, seed=100)
    assert (Dr[np.isfinite(Dr)] > RANGE[1]).any() and (Dr[np.isfinite(Dr)] < RANGE[0]).any() and (~np.isfinite(Dr)).sum() > 20
    delta = V.target_deltas(5, targets_of(5))
    for t in range(T):
        Dt0 = VU.splat_np(Dr, delta[t], RANGE)
        assert 0.01 < np.isnan(Dt0).mean() < 0.5
        Dt, holes = VU.fill_np(Dt0, Dr, RANGE, fill=0)                  # no search: the holes fall back to Dr, or to the far end
        assert np.array_equal(holes, np.isnan(Dt0)) and (Dt[np.isnan(Dt0) & ~np.isfinite(Dr)] == np.float32(RANGE[0])).all()
    assert V.splat_reach(RANGE, delta) == 6


@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_identity_at_integer_targets(dtype, interp):
    A, C = 3, 3
    lf = field(A, H, W, C, dtype, seed=3)
    if dtype == np.float32:
        lf = (lf * 4 - 2).astype(np.float32)                 # outside [0, 1]: fp32 output is not clipped
    tg = [(u, v) for u in range(A) for v in range(A)]
    g = torch.from_numpy(lf).to(DEV)
    for Dr in (disparity_map(H, W, seed=4), np.zeros((H, W), np.float32)):
        got = V.render(g, torch.from_numpy(Dr).to(DEV), tg, RANGE, interp=interp)
        assert got.views.dtype == g.dtype
        for k, (u, v) in enumerate(tg):
            assert torch.equal(got.views[k], g[u, v]), (u, v)


@pytest.mark.parametrize("d0", [0.6, -1.3])
def test_geometry(d0):
    """A plane of slope d0 rendered at a fractional target is f displaced by d0 * (target - centre), within the interpolation
    bound max|f_yy| / 8 + max|f_xx| / 8 = (0.45^2 + 0.37^2) / 16 = 0.0213 (the fp64 restatement reaches 0.0168:
    tests/test_views_host.py); a wrong sign fails by an order of magnitude."""
    A, h, w = 5, 40, 44
    L, _ = RU.plane(A, h, w, d0)
    f = lambda y, x: 0.5 + 0.5 * np.sin(0.45 * y + 0.3) * np.cos(0.37 * x - 0.2)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    tg = [(1.5, 2.25), (0.3, 3.9)]
    got = V.render(torch.from_numpy(L).to(DEV), torch.full((h, w), d0, device=DEV), tg, (-2, 2), blend="quad", interp="linear")
    assert tuple(got.views.shape) == (2, h, w) and bool((got.disparity == float(np.float32(d0))).all())
    assert int(got.holes[:, 4:h - 4, 4:w - 4].sum()) == 0            # a constant shift leaves holes along the border only
    for k, t in enumerate(tg):
        want = f(y - d0 * (t[0] - 2), x - d0 * (t[1] - 2))
        err = float(np.abs(got.views[k].cpu().numpy().astype(np.float64) - want)[4:h - 4, 4:w - 4].max())
        print(f"d0={d0} target {t}: |render - f| {err:.4f} (bound 0.0213)")
        assert err <= 0.0213


def test_occlusion():
    """The two-layer scene: the foreground wins the splat, the holes it leaves take the background, and the held-out view comes
    back to rounding wherever every view agrees.  Inside the 9-pixel ring around the box the views disagree (no per-view
    visibility test) and the fp64 restatement itself is off by up to 0.5: the mask is the claim."""
    A, h, w = 5, 72, 64
    L, _ = DU.two_layer(A, h, w)
    y0, y1, x0, x1 = DU.FG_BOX
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    Dr = np.where((yy >= y0) & (yy < y1) & (xx >= x0) & (xx < x1), 1.0, -1.0).astype(np.float32)
    g, d = torch.from_numpy(L).to(DEV), torch.from_numpy(Dr).to(DEV)
    tol = VU.tol_render(A * A - 1, 2, 1.0)
    for t in ((0, 1), (4, 4), (1, 3), (2, 2)):
        ex = np.zeros((A, A), bool)
        ex[t] = True
        got = V.render(g, d, [t], (-1, 1), blend="gaussian", exclude=ex)
        want, b5, held, fg = VU.occlusion_masks(t, h, w)
        assert np.array_equal(got.disparity[0].cpu().numpy()[b5], want[b5]), t
        assert held.mean() >= 0.25 and (held & fg).sum() == 676
        err = np.abs(got.views[0, ..., 0].cpu().numpy().astype(np.float64) - L[t[0], t[1], ..., 0].astype(np.float64))
        print(f"target {t}: holes {int(got.holes.sum())}, max error on the mask {float(err[held].max()):.3e} (tol {tol:.3e}), off it {float(err[~held].max()):.3f}")
        assert float(err[held].max()) <= tol, t


def test_layouts_give_identical_bits():
    A, h, w = 3, 21, 34
    tg = [(0.5, 1.25), (2, 0.75), (1, 1)]
    for dtype in (np.float32, np.uint8):
        v = torch.from_numpy(field(A, h, w, 1, dtype, 4)[..., 0]).to(DEV)                  # [A, A, H, W]
        d = torch.from_numpy(disparity_map(h, w, seed=5)).to(DEV)
        mosaic = v.permute(0, 2, 1, 3).reshape(A * h, A * w).contiguous()
        strided = v.permute(2, 3, 0, 1).contiguous().permute(2, 3, 0, 1)
        assert not strided.is_contiguous() and torch.equal(strided, v)
        want = V.render(v, d, tg, RANGE, out_dtype=torch.float32)
        assert tuple(want.views.shape) == (3, h, w)

        def same(r, views):
            return torch.equal(views, want.views) and torch.equal(bits_t(r.disparity), bits_t(want.disparity)) and torch.equal(r.holes, want.holes)

        r = V.render(v[..., None], d, tg, RANGE, out_dtype=torch.float32)
        assert tuple(r.views.shape) == (3, h, w, 1) and same(r, r.views[..., 0])
        for lf, kw in ((v, dict(angRes=A)), (mosaic, dict(angRes=A)), (strided, {})):
            r = V.render(lf, d, tg, RANGE, out_dtype=torch.float32, **kw)
            assert same(r, r.views)
        b = V.render(mosaic[None, None], d[None], tg, RANGE, angRes=A, out_dtype=torch.float32)
        assert tuple(b.views.shape) == (1, 3, h, w) and tuple(b.disparity.shape) == (1, 3, h, w)
        assert torch.equal(b.views[0], want.views) and torch.equal(b.holes[0], want.holes)
        assert V.render(v, d, tg, RANGE).views.dtype == v.dtype                            # out_dtype defaults to the input's
        assert torch.equal(V.render(v, d.t().contiguous().t(), tg, RANGE, out_dtype=torch.float32).views, want.views)      # a strided map
    batch = torch.from_numpy(np.random.default_rng(6).random((2, 1, A * h, A * w)).astype(np.float32)).to(DEV)
    maps = torch.from_numpy(np.stack([disparity_map(h, w, seed=7), disparity_map(h, w, seed=8)])).to(DEV)
    got = V.render(batch, maps, tg, RANGE, angRes=A, interp="cubic")
    for k in range(2):
        one = V.render(batch[k, 0], maps[k], tg, RANGE, angRes=A, interp="cubic")
        assert torch.equal(got.views[k], one.views) and torch.equal(got.holes[k], one.holes)
    for bad in (lambda: V.render(batch, maps[0], tg, RANGE, angRes=A), lambda: V.render(batch, maps.cpu(), tg, RANGE, angRes=A),
                lambda: V.render(batch[0, 0], maps[0], tg, RANGE), lambda: V.render(batch[0, 0], maps[0, :-1], tg, RANGE, angRes=A)):
        with pytest.raises(LftError):
            bad()


def bits_t(x):
    return x.contiguous().view(torch.int32)


def test_tile_independence():
    """A pixel's results depend on its coordinates, its splat sources, its fill search and its taps only: a crop agrees with the
    whole image on the pixels that keep all of them, reach + fill + the largest tap shift + 2 from the crop's border.  A crop at
    the origin keeps every pixel's coordinates and agrees bit for bit, in other tiles.  A crop elsewhere moves the coordinates, and
    the definition's fp32 sample positions fl(y + fl(d*du)) round differently at another y: each position is within half an ulp,
    2^-18 below 128, of the exact one, so the two differ by at most 2^-17 an axis, and a linear sample of data in [0, 1] is
    1-Lipschitz in each: 2 * 2^-17, plus tol_render for each side's filtering.  The maps and holes still agree bit for bit."""
    A, h, w, fill = 3, 70, 75, 3
    tg = [(0.5, 1.25), (1.5, 0.25)]
    d_range = (-1.25, 1.25)
    lf = torch.from_numpy(field(A, h, w, 1, np.float32, 6)[..., 0]).to(DEV)
    d = torch.from_numpy(disparity_map(h, w, seed=9, bad=0.5)).to(DEV)     # half the sources missing: holes of every kind
    full = V.render(lf, d, tg, d_range, fill=fill)
    again = V.render(lf, d, tg, d_range, fill=fill)
    assert torch.equal(again.views, full.views) and torch.equal(bits_t(again.disparity), bits_t(full.disparity)) and torch.equal(again.holes, full.holes)
    assert 0.02 < float(full.holes.float().mean()) < 0.6
    none = V.render(lf, d, tg, d_range, fill=0)                      # no search: every hole takes Dr or the far end
    assert torch.equal(none.holes, full.holes) and not torch.equal(bits_t(none.disparity), bits_t(full.disparity))
    reach = V.splat_reach(d_range, V.target_deltas(A, tg))
    m = reach + fill + int(np.ceil(1.25 * 1.75)) + 2
    assert reach == 2 and m == 10
    moved = 2 * 2.0 ** -17 + 2 * VU.tol_render(4, 2, 1.0)
    for y0, x0 in ((0, 0), (13, 7), (1, 33)):
        crop = V.render(lf[:, :, y0:y0 + 40, x0:x0 + 41], d[y0:y0 + 40, x0:x0 + 41], tg, d_range, fill=fill)
        assert tuple(crop.views.shape) == (2, 40, 41)
        lo_y, lo_x = (m if y0 else 0), (m if x0 else 0)              # at the origin the image's own border is the crop's
        inner = (slice(None), slice(lo_y, 40 - m), slice(lo_x, 41 - m))
        outer = (slice(None), slice(y0 + lo_y, y0 + 40 - m), slice(x0 + lo_x, x0 + 41 - m))
        assert torch.equal(crop.holes[inner], full.holes[outer]) and torch.equal(bits_t(crop.disparity[inner]), bits_t(full.disparity[outer]))
        if (y0, x0) == (0, 0):
            assert torch.equal(crop.views[inner], full.views[outer])
        else:
            err = float((crop.views[inner].double() - full.views[outer].double()).abs().max())
            print(f"crop at ({y0}, {x0}): max difference {err:.3e} (bound {moved:.3e})")
            assert err <= moved
        assert not torch.equal(crop.views, full.views[:, y0:y0 + 40, x0:x0 + 41])          # the border does differ


def test_capture_and_replay():
    from lft_amd import train as Tr
    A = 3
    tg = [(0.5, 1.25), (2, 0.75), (1, 1)]
    lf = torch.from_numpy(field(A, 33, 40, 3, np.uint8, 15)).to(DEV)
    d = torch.from_numpy(disparity_map(33, 40, seed=16)).to(DEV)
    want = V.render(lf, d, tg, RANGE, interp="cubic")                # eager; tables and scratch are on the device from here on
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side, capture_error_mode=Tr.CAPTURE_MODE):
            got = V.render(lf, d, tg, RANGE, interp="cubic")
        got.views.fill_(9)
        got.disparity.fill_(9)
        got.holes.fill_(9)
        graph.replay()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(got.views, want.views) and torch.equal(bits_t(got.disparity), bits_t(want.disparity)) and torch.equal(got.holes, want.holes)


def _net(A, s, seed):
    from lft_amd.params import deterministic_state
    from model import LFT
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, s, seed=seed).items()})
    return net.to(DEV).eval()


def test_densify_and_leave_one_out(golden_dir):
    from lft_amd import disparity as Dm, prepare
    A = 3
    lf = prepare.to_device(prepare.load_lf(os.path.join(golden_dir, "prepare_lf_v73.mat")), A, DEV)      # [3, 3, 9, 7, 3] uint8, strided
    slopes = [-1.0, -0.5, 0.0, 0.5, 1.0]
    dr = Dm.disparity(lf, slopes, radius=1).disparity
    dense = V.densify(lf, dr, 2, (-1, 1))
    assert tuple(dense.shape) == (5, 5, 9, 7, 3) and dense.dtype == torch.uint8
    assert torch.equal(dense[::2, ::2], lf)                                                # the given views, bit for bit
    g = V.grid_targets(A, 2)
    new = [(i, j) for i in range(5) for j in range(5) if i % 2 or j % 2]
    r = V.render(lf, dr, [g[i, j] for i, j in new], (-1, 1))
    assert all(torch.equal(dense[i, j], r.views[k]) for k, (i, j) in enumerate(new))
    assert torch.equal(V.render(lf, dr, [(u, v) for u in range(A) for v in range(A)], (-1, 1)).views.reshape(A, A, 9, 7, 3), lf)
    f32 = V.densify(lf, dr, 2, (-1, 1), out_dtype=torch.float32)
    assert f32.dtype == torch.float32 and torch.equal(f32[::2, ::2], lf.float() / 255)
    assert tuple(V.densify(lf[..., 0], dr, 3, (-1, 1), interp="cubic").shape) == (7, 7, 9, 7)
    loo = V.leave_one_out(lf, slopes, radius=1)
    assert len(loo) == 9 and all(np.isfinite(p) and p > 0 for p in loo)
    # the plane: the true map predicts a held-out view better than a map that is off by one pixel per view step
    L, _ = RU.plane(5, 40, 44, 0.6)
    P = torch.from_numpy(L).to(DEV)
    sweep = list(np.linspace(-2.0, 2.0, 9))
    pos = [(2, 2), (0, 1), (3, 4)]
    true = V.leave_one_out(P, sweep, pos, disparity=torch.full((40, 44), 0.6, device=DEV))
    off = V.leave_one_out(P, sweep, pos, disparity=torch.full((40, 44), 1.6, device=DEV))
    swept = V.leave_one_out(P, sweep, pos)
    shuffled = V.leave_one_out(P.flip(0), sweep, pos)                                     # every view as good as before, the field inconsistent
    print(f"leave-one-out PSNR on the plane: true map {true}, map + 1 {off}, swept {swept}, rows of views reversed {shuffled}")
    assert all(a > b + 10 for a, b in zip(true, off))
    assert all(a > b for a, b in zip(swept, shuffled))


def test_tool_writes_frames_and_the_json_line(golden_dir, tmp_path, capsys):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import view_path as tool
    from lft_amd import disparity as Dm, png, prepare, trainer
    A, s = 3, 2
    mat = os.path.join(golden_dir, "prepare_lf_v73.mat")
    lf = prepare.to_device(prepare.load_lf(mat), A, DEV)
    out_dir = str(tmp_path / "line")
    paths = tool.main(["--lf", mat, "--angRes", str(A), "--out_dir", out_dir, "--slopes=-1:1:5", "--path", "line", "--frames", "3", "--radius", "1"])
    names = ["frame_0.png", "frame_1.png", "frame_2.png"]
    assert [os.path.basename(p) for p in paths] == names and sorted(os.listdir(out_dir)) == names
    for k in range(3):                                                                    # the ends and the middle of the centre row: the views themselves
        assert np.array_equal(png.read_png(paths[k]), lf[1, k].cpu().numpy())
    out_dir = str(tmp_path / "circle")
    paths = tool.main(["--lf", mat, "--angRes", str(A), "--out_dir", out_dir, "--slopes=-1:1:5", "--path", "circle", "--frames", "4", "--radius", "1"])
    slopes = [-1.0, -0.5, 0.0, 0.5, 1.0]
    dr = Dm.disparity(lf, slopes, interp="linear", radius=1).disparity
    want = V.render(lf, dr, tool.path_targets("circle", A, 4), (-1, 1)).views.cpu().numpy()
    assert len(paths) == 4 and all(np.array_equal(png.read_png(paths[k]), want[k]) for k in range(4))
    out_dir = str(tmp_path / "grid")
    paths = tool.main(["--lf", mat, "--angRes", str(A), "--out_dir", out_dir, "--slopes=-1:1:5", "--path", "grid:2", "--radius", "1"])
    assert len(paths) == 25 and sorted(os.listdir(out_dir)) == sorted(f"view_{i}_{j}.png" for i in range(5) for j in range(5))
    assert np.array_equal(png.read_png(os.path.join(out_dir, "view_2_4.png")), lf[1, 2].cpu().numpy())
    # super-resolved and bicubic views: frames of both, and the leave-one-out line
    net = _net(A, s, seed=12)
    ckpt = str(tmp_path / "net.pth.tar")
    trainer.save_checkpoint(net, ckpt, 1)
    out_dir = str(tmp_path / "sr")
    capsys.readouterr()
    paths = tool.main(["--lf", mat, "--angRes", str(A), "--out_dir", out_dir, "--slopes=-1:1:5", "--path", "line", "--frames", "2", "--radius", "1",
                       "--path_pre_pth", ckpt, "--scale_factor", str(s), "--bicubic", "--patch_size_for_test", "8", "--stride_for_test", "4"])
    assert sorted(os.listdir(out_dir)) == sorted(["frame_0.png", "frame_1.png", "bicubic_frame_0.png", "bicubic_frame_1.png"]) and len(paths) == 4
    assert png.read_png(paths[0]).shape == (s * 9, s * 7, 3)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert set(rec["leave_one_out_psnr"]) == {"sr", "bicubic"} and rec["views"] == 9 and rec["slopes"] == [-1.0, 1.0, 5]
    assert all(v > 0 for v in rec["leave_one_out_psnr"].values())
