"""GPU tests of view synthesis with the per-view visibility test (lft_view_render_visible / k_view_render_vis, lft_view_warp_disparity /
k_view_fill, lft_amd.views) against the numpy restatement of its definition (tests/visibility_util.py): the warped maps, the target
map, the holes and the count bit for bit, the views within views_util.tol_render of the fp64 render over the same classes."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from lft_amd import views as V

import refocus_util as RU
import views_util as VU
import visibility_util as XU
from test_gpu_views import RANGE, bits, bits_t, disparity_map, field, targets_of
from test_visibility_host import TWO_LAYER_TARGETS, border, two_layer_scene

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H, W, T = 37, 45, 3                                     # one past a 32 x 32 splat tile and a 32 x 8 render tile in either direction
TAU = 0.25


def dev(x):
    return torch.from_numpy(x).to(DEV)


@functools.lru_cache(maxsize=None)
def reference_maps(A, near):
    """(Dr, Dv, [(Dt, holes)] per target) of the parity inputs, computed once per (A, near) and left unchanged."""
    Dr = disparity_map(H, W, seed=100 + (near == "smaller"))
    deltas = V.target_deltas(A, targets_of(A))
    at = V.target_deltas(A, [(u, v) for u in range(A) for v in range(A)])
    warped = [VU.fill_np(VU.splat_np(Dr, d, RANGE, near), Dr, RANGE, near) for d in at]
    Dv = np.stack([m for m, _ in warped]).reshape(A, A, H, W)
    Hv = np.stack([h for _, h in warped])
    return Dr, Dv, Hv, [VU.fill_np(VU.splat_np(Dr, deltas[t], RANGE, near), Dr, RANGE, near) for t in range(T)]


@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("A", [1, 2, 3, 5])
def test_parity(A, interp):
    taps = V.TAPS[interp]
    tg = targets_of(A)
    rec = V.record_table(A, tg, V.blend_weights(A, tg, "gaussian"))
    n = 0
    for near in ("larger", "smaller"):
        Dr, Dv, Hv, Dts = reference_maps(A, near)
        d = dev(Dr)
        maps, holes = V.warp_disparity(d, [(u, v) for u in range(A) for v in range(A)], RANGE, ((A - 1) / 2, (A - 1) / 2), near=near)
        assert tuple(maps.shape) == (A * A, H, W) and maps.dtype == torch.float32 and holes.dtype == torch.uint8
        assert np.array_equal(bits(maps.cpu().numpy()), bits(Dv.reshape(A * A, H, W))) and np.array_equal(holes.cpu().numpy(), Hv), (A, near)
        for C in (1, 3, 4):
            for dtype in (np.uint8, np.float32):
                lf = field(A, H, W, C, dtype, seed=n)
                kw = dict(blend="gaussian", interp=interp, near=near, visibility=dict(tau=TAU))
                got = V.render(dev(lf), d, tg, RANGE, out_dtype=torch.float32, **kw)
                plain = V.render(dev(lf), d, tg, RANGE, blend="gaussian", interp=interp, near=near, out_dtype=torch.float32)
                assert isinstance(got, V.VisibleRenderResult) and tuple(got.views.shape) == (T, H, W, C) and got.views.dtype == torch.float32
                assert tuple(got.visible.shape) == (T, H, W) and got.visible.dtype == torch.uint8
                assert torch.equal(bits_t(got.disparity), bits_t(plain.disparity)) and torch.equal(got.holes, plain.holes)
                as8 = V.render(dev(lf), d, tg, RANGE, out_dtype=torch.uint8, **kw).views.cpu().numpy() if dtype == np.uint8 else None
                for t in range(T):
                    Dt, hl = Dts[t]
                    what = f"A={A} {interp} C={C} {np.dtype(dtype).name} near={near} target {tg[t]}"
                    assert np.array_equal(bits(got.disparity[t].cpu().numpy()), bits(Dt)) and np.array_equal(got.holes[t].cpu().numpy(), hl), what
                    ref, count, cls = XU.render_np(lf, Dt, rec[t], taps, Dv, TAU, near)
                    assert np.array_equal(got.visible[t].cpu().numpy(), count), what
                    tol = VU.tol_render(int((rec[t]["skip"] == 0).sum()), taps, 1.0)
                    err = float(np.abs(got.views[t].cpu().numpy().astype(np.float64) - ref).max())
                    print(f"{what}: classes {np.bincount(cls.ravel(), minlength=3).tolist()}, max error {err:.3e}, tol {tol:.3e}")
                    assert err <= tol, what
                    if as8 is not None:
                        tie = RU.tie_distance(ref) <= 255 * tol
                        assert tie.mean() <= 0.01, (what, float(tie.mean()))                # on the reference alone
                        diff = np.abs(as8[t].astype(np.int64) - RU.quantise(ref).astype(np.int64))
                        assert diff[~tie].max(initial=0) == 0 and diff.max() <= 1, what
                n += 1


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_nothing_occluded_is_the_plain_render(interp):
    """tau above hi - lo, or maps that are nowhere finite above the threshold: the views are the plain call's bits, the count the
    inside views.  A caller's maps equal to the warped ones give the default's bits."""
    A = 3
    tg = targets_of(A)
    rec = V.record_table(A, tg, V.blend_weights(A, tg, "gaussian"))
    for near in ("larger", "smaller"):
        Dr, Dv, _, Dts = reference_maps(A, near)
        d = dev(Dr)
        for dtype in (np.uint8, np.float32):
            lf = dev(field(A, H, W, 3, dtype, seed=5))
            kw = dict(blend="gaussian", interp=interp, near=near)
            plain = V.render(lf, d, tg, RANGE, **kw)
            inside = np.stack([XU.classes_np(Dts[t][0], rec[t], Dv, TAU, near)[1].sum(0) for t in range(T)]).astype(np.uint8)
            never = -np.inf if near == "larger" else np.inf
            for vis in (dict(tau=3.6), dict(tau=0.0, view_disparity=torch.full((A, A, H, W), float("nan"), device=DEV)),
                        dict(tau=0.0, view_disparity=torch.full((A, A, H, W), never, device=DEV))):
                got = V.render(lf, d, tg, RANGE, visibility=vis, **kw)
                assert torch.equal(got.views, plain.views) and got.views.dtype == plain.views.dtype, (near, dtype, vis["tau"])
                assert np.array_equal(got.visible.cpu().numpy(), inside)
            default = V.render(lf, d, tg, RANGE, visibility=dict(tau=TAU), **kw)
            given = V.render(lf, d, tg, RANGE, visibility=dict(tau=TAU, view_disparity=dev(Dv)), **kw)
            assert not torch.equal(default.views, plain.views)
            assert torch.equal(given.views, default.views) and torch.equal(given.visible, default.visible) and torch.equal(given.holes, default.holes)


@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_identity_at_integer_targets(dtype, interp):
    """One view of non-zero weight: whatever Dv says, it is the only member of the class that is chosen."""
    A, C = 3, 3
    lf = field(A, H, W, C, dtype, seed=3)
    if dtype == np.float32:
        lf = (lf * 4 - 2).astype(np.float32)                 # outside [0, 1]: fp32 output is not clipped
    tg = [(u, v) for u in range(A) for v in range(A)]
    g = dev(lf)
    d = dev(disparity_map(H, W, seed=4))
    rng = np.random.default_rng(8)
    for maps in (None, torch.full((A, A, H, W), 5.0, device=DEV), dev((rng.random((A, A, H, W)) * 8 - 4).astype(np.float32))):
        got = V.render(g, d, tg, RANGE, interp=interp, visibility=dict(tau=0.0, view_disparity=maps))
        assert got.views.dtype == g.dtype and int(got.visible.max()) <= 1
        for k, (u, v) in enumerate(tg):
            assert torch.equal(got.views[k], g[u, v]), (u, v)


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_two_layers(interp):
    """The test that shows the feature: with the visibility test the held-out view of the two-layer scene comes back within the
    render's rounding bound on every pixel >= 9 from the border, the 9-pixel ring around the foreground box included; the plain
    render of the same call misses that bound in the ring."""
    A, taps = 5, V.TAPS[interp]
    L, Dr = two_layer_scene()
    g, d = dev(L), dev(Dr)
    b9 = border(9)
    tol = VU.tol_render(A * A - 1, taps, 1.0)
    for t in TWO_LAYER_TARGETS:
        ex = np.zeros((A, A), bool)
        ex[t] = True
        kw = dict(blend="gaussian", exclude=ex, interp=interp)
        got = V.render(g, d, [t], (-1, 1), visibility=dict(tau=0.5), **kw)
        plain = V.render(g, d, [t], (-1, 1), **kw)
        _, _, held, _ = VU.occlusion_masks(t)
        truth = L[t[0], t[1], ..., 0].astype(np.float64)
        err = np.abs(got.views[0, ..., 0].cpu().numpy().astype(np.float64) - truth)
        off = np.abs(plain.views[0, ..., 0].cpu().numpy().astype(np.float64) - truth)
        count = got.visible[0].cpu().numpy()
        ring = b9 & ~held
        print(f"target {t} {interp}: max error {float(err[b9].max()):.3e} (tol {tol:.3e}), fewest visible views {int(count[b9].min())}, "
              f"plain: {int((off[ring] > tol).sum())} ring pixels above the bound, up to {float(off[ring].max()):.3f}")
        assert float(err[b9].max()) <= tol, t
        assert int(count[b9].min()) >= 1 and (count[held] == 24).all(), t
        assert float(off[ring].max()) > tol and int((off[ring] > 1e-3).sum()) >= 200, t


def test_occlusion_map():
    """Rendered at the reference with nothing excluded, `visible` counts the views that see each pixel of the centre view."""
    A = 5
    L, Dr = two_layer_scene()
    got = V.render(dev(L), dev(Dr), [(2, 2)], (-1, 1), blend="gaussian", visibility=dict(tau=0.5))
    _, _, held, _ = VU.occlusion_masks((2, 2))
    count = got.visible[0].cpu().numpy()
    assert (count[held] == 25).all() and (count[border(9) & ~held] < 25).any()
    rec = V.record_table(A, [(2, 2)], V.blend_weights(A, [(2, 2)], "gaussian"))[0]
    Dt, _ = VU.fill_np(VU.splat_np(Dr, (0, 0), (-1, 1)), Dr, (-1, 1))
    assert np.array_equal(count, XU.classes_np(Dt, rec, XU.warp_np(Dr, A, (-1, 1)), 0.5)[3])


def same(r, want, views=None):
    views = r.views if views is None else views
    return (torch.equal(views, want.views) and torch.equal(bits_t(r.disparity), bits_t(want.disparity)) and torch.equal(r.holes, want.holes)
            and torch.equal(r.visible, want.visible))


def test_layouts_give_identical_bits():
    A, h, w = 3, 21, 34
    tg = [(0.5, 1.25), (2, 0.75), (1, 1)]
    vis = dict(tau=TAU)
    for dtype in (np.float32, np.uint8):
        v = dev(field(A, h, w, 1, dtype, 4)[..., 0])                                      # [A, A, H, W]
        d = dev(disparity_map(h, w, seed=5))
        mosaic = v.permute(0, 2, 1, 3).reshape(A * h, A * w).contiguous()
        strided = v.permute(2, 3, 0, 1).contiguous().permute(2, 3, 0, 1)
        want = V.render(v, d, tg, RANGE, out_dtype=torch.float32, visibility=vis)
        assert tuple(want.views.shape) == (3, h, w) and tuple(want.visible.shape) == (3, h, w) and int(want.visible.max()) >= 1
        r = V.render(v[..., None], d, tg, RANGE, out_dtype=torch.float32, visibility=vis)
        assert tuple(r.views.shape) == (3, h, w, 1) and same(r, want, r.views[..., 0])
        for lf, kw in ((v, dict(angRes=A)), (mosaic, dict(angRes=A)), (strided, {})):
            assert same(V.render(lf, d, tg, RANGE, out_dtype=torch.float32, visibility=vis, **kw), want)
        maps = V.warp_disparity(d, [(u, c) for u in range(A) for c in range(A)], RANGE, (1, 1))[0].reshape(A, A, h, w)
        wide = torch.zeros(A, A, h, w + 3, device=DEV)
        wide[..., :w] = maps
        assert same(V.render(v, d, tg, RANGE, out_dtype=torch.float32, visibility=dict(tau=TAU, view_disparity=wide[..., :w])), want)   # strided maps
        b = V.render(mosaic[None, None], d[None], tg, RANGE, angRes=A, out_dtype=torch.float32, visibility=vis)
        assert tuple(b.visible.shape) == (1, 3, h, w) and torch.equal(b.views[0], want.views) and torch.equal(b.visible[0], want.visible)
    batch = dev(np.random.default_rng(6).random((2, 1, A * h, A * w)).astype(np.float32))
    maps = dev(np.stack([disparity_map(h, w, seed=7), disparity_map(h, w, seed=8)]))
    got = V.render(batch, maps, tg, RANGE, angRes=A, interp="cubic", visibility=vis)
    both = V.warp_disparity(maps, [(0, 2), (1.5, 0.5)], RANGE, (1, 1))
    assert tuple(both[0].shape) == (2, 2, h, w)
    for k in range(2):
        one = V.render(batch[k, 0], maps[k], tg, RANGE, angRes=A, interp="cubic", visibility=vis)
        assert torch.equal(got.views[k], one.views) and torch.equal(got.visible[k], one.visible) and torch.equal(got.holes[k], one.holes)
        alone = V.warp_disparity(maps[k], [(0, 2), (1.5, 0.5)], RANGE, (1, 1))
        assert torch.equal(bits_t(both[0][k]), bits_t(alone[0])) and torch.equal(both[1][k], alone[1])
    for bad in (lambda: V.render(batch, maps, tg, RANGE, angRes=A, visibility=dict(tau=TAU, view_disparity=torch.zeros(A, A, h, w, device=DEV))),
                lambda: V.render(batch[0, 0], maps[0], tg, RANGE, angRes=A, visibility=dict(tau=TAU, view_disparity=torch.zeros(A, A, h, w))),
                lambda: V.render(batch[0, 0], maps[0], tg, RANGE, angRes=A, visibility=dict(tau=TAU, view_disparity=torch.zeros(A, A, h, w - 1, device=DEV)))):
        with pytest.raises(V.LftError, match="view_disparity"):
            bad()


def test_a_crop_at_the_origin_agrees_bit_for_bit():
    """As tests/test_gpu_views.py::test_tile_independence: a pixel's results depend on its coordinates, its splat sources, its fill
    search, its taps and now its footprints in the warped maps, which have splat sources and fill searches of their own: twice the
    reach and fill of the plain margin, from the crop's far borders."""
    A, h, w, fill = 3, 70, 75, 3
    tg = [(0.5, 1.25), (1.5, 0.25)]
    d_range = (-1.25, 1.25)
    lf = dev(field(A, h, w, 1, np.float32, 6)[..., 0])
    d = dev(disparity_map(h, w, seed=9, bad=0.5))
    vis = dict(tau=TAU)
    full = V.render(lf, d, tg, d_range, fill=fill, visibility=vis)
    reach = max(V.splat_reach(d_range, V.target_deltas(A, tg)), V.splat_reach(d_range, V.target_deltas(A, [(0, 0)])))
    m = 2 * (reach + fill) + int(np.ceil(1.25 * 1.75)) + 2
    assert reach == 3 and m == 17
    crop = V.render(lf[:, :, :48, :51], d[:48, :51], tg, d_range, fill=fill, visibility=vis)
    inner = (slice(None), slice(0, 48 - m), slice(0, 51 - m))
    assert torch.equal(crop.views[inner], full.views[inner]) and torch.equal(crop.visible[inner], full.visible[inner])
    assert torch.equal(crop.holes[inner], full.holes[inner]) and torch.equal(bits_t(crop.disparity[inner]), bits_t(full.disparity[inner]))
    assert bool((full.visible[inner] < full.visible[inner].max()).any())                     # the test does decide something there
    assert not torch.equal(crop.views, full.views[:, :48, :51])                              # the border does differ


def test_capture_and_replay():
    from lft_amd import train as Tr
    A = 3
    tg = [(0.5, 1.25), (2, 0.75), (1, 1)]
    lf = dev(field(A, 33, 40, 3, np.uint8, 15))
    d = dev(disparity_map(33, 40, seed=16))
    vis = dict(tau=TAU)
    want = V.render(lf, d, tg, RANGE, interp="cubic", visibility=vis)      # eager; tables and scratch are on the device from here on
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side, capture_error_mode=Tr.CAPTURE_MODE):
            got = V.render(lf, d, tg, RANGE, interp="cubic", visibility=vis)
        for out in got:
            out.fill_(9)
        graph.replay()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert same(got, want)


def test_empty_shapes():
    A = 3
    tg = [(0.5, 1.25), (1, 1)]
    vis = dict(tau=TAU)
    for h, w in ((0, 5), (5, 0)):
        got = V.render(torch.zeros(A, A, h, w, device=DEV), torch.zeros(h, w, device=DEV), tg, RANGE, visibility=vis)
        assert tuple(got.views.shape) == (2, h, w) and tuple(got.visible.shape) == (2, h, w) and got.visible.dtype == torch.uint8
        maps, holes = V.warp_disparity(torch.zeros(h, w, device=DEV), tg, RANGE, (1, 1))
        assert tuple(maps.shape) == (2, h, w) and tuple(holes.shape) == (2, h, w)
    got = V.render(torch.zeros(0, 1, A * 4, A * 4, device=DEV), torch.zeros(0, 4, 4, device=DEV), tg, RANGE, angRes=A, visibility=vis)
    assert tuple(got.views.shape) == (0, 2, 4, 4) and tuple(got.visible.shape) == (0, 2, 4, 4)
    assert tuple(V.warp_disparity(torch.zeros(0, 4, 4, device=DEV), tg, RANGE, (1, 1))[0].shape) == (0, 2, 4, 4)


def test_leave_one_out_and_densify_pass_visibility_through():
    L, Dr = two_layer_scene()
    g, d = dev(L), dev(Dr)
    pos = [(0, 0), (2, 2), (1, 3)]
    sweep = [-1.0, -0.5, 0.0, 0.5, 1.0]
    plain = V.leave_one_out(g, sweep, pos, disparity=d)
    seen = V.leave_one_out(g, sweep, pos, disparity=d, visibility=dict(tau=0.5))
    print(f"leave-one-out PSNR on the two layers: plain {plain}, with the visibility test {seen}")
    assert all(a > b for a, b in zip(seen, plain))
    dense = V.densify(g, d, 2, (-1, 1), visibility=dict(tau=0.5))
    new = [(i, j) for i in range(9) for j in range(9) if i % 2 or j % 2]
    gt = V.grid_targets(5, 2)
    r = V.render(g, d, [gt[i, j] for i, j in new], (-1, 1), visibility=dict(tau=0.5))
    assert tuple(dense.shape) == (9, 9, 72, 64, 1) and torch.equal(dense[::2, ::2], g)
    assert all(torch.equal(dense[i, j], r.views[k]) for k, (i, j) in enumerate(new))
    assert not torch.equal(dense, V.densify(g, d, 2, (-1, 1)))


def test_tool_writes_frames_and_the_json_line(golden_dir, tmp_path, capsys):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import view_path as tool
    from lft_amd import disparity as Dm, png, prepare, trainer
    from test_gpu_views import _net
    A, s = 3, 2
    mat = os.path.join(golden_dir, "prepare_lf_v73.mat")
    lf = prepare.to_device(prepare.load_lf(mat), A, DEV)
    slopes = [-1.0, -0.5, 0.0, 0.5, 1.0]
    dr = Dm.disparity(lf, slopes, interp="linear", radius=1).disparity
    for flag, tau in ((["--visibility"], 0.5), (["--visibility", "0.125"], 0.125)):          # the default: the sweep's largest slope step
        out_dir = str(tmp_path / f"circle{tau}")
        paths = tool.main(["--lf", mat, "--angRes", str(A), "--out_dir", out_dir, "--slopes=-1:1:5", "--path", "circle", "--frames", "4", "--radius", "1"] + flag)
        want = V.render(lf, dr, tool.path_targets("circle", A, 4), (-1, 1), visibility=dict(tau=tau)).views.cpu().numpy()
        assert len(paths) == 4 and all(np.array_equal(png.read_png(paths[k]), want[k]) for k in range(4))
    net = _net(A, s, seed=12)
    ckpt = str(tmp_path / "net.pth.tar")
    trainer.save_checkpoint(net, ckpt, 1)
    out_dir = str(tmp_path / "sr")
    capsys.readouterr()
    paths = tool.main(["--lf", mat, "--angRes", str(A), "--out_dir", out_dir, "--slopes=-1:1:5", "--path", "line", "--frames", "2", "--radius", "1", "--visibility",
                       "--path_pre_pth", ckpt, "--scale_factor", str(s), "--bicubic", "--patch_size_for_test", "8", "--stride_for_test", "4"])
    assert sorted(os.listdir(out_dir)) == sorted(["frame_0.png", "frame_1.png", "bicubic_frame_0.png", "bicubic_frame_1.png"]) and len(paths) == 4
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert set(rec["leave_one_out_psnr"]) == {"sr", "bicubic"} and set(rec["leave_one_out_psnr_visible"]) == {"sr", "bicubic"}
    assert rec["visibility_tau"] == 0.5 and all(v > 0 for v in rec["leave_one_out_psnr_visible"].values())
