"""GPU tests of the disparity sweep (lft_disparity: k_sweep_cost + k_disparity_pick, lft_amd.disparity) against the fp64 numpy
restatement of its definition (tests/disparity_util.py), which takes the same fp32-rounded table.

The aggregated cost E is held to the derived bound tol_E = C (3 A^2 + 66 + (2r+1)^2) 2^-23 S^4 X^2 (1.5e-4 for A = 5, C = 3, r = 2,
cubic, data in [0, 1]).  Index, disparity and confidence are then checked from the GPU's own E with the selection steps restated
in numpy float32 (``pick_np``), so no near-tie allowance is needed: index exactly, disparity within 4 * 2^-23 * max|slope|,
confidence within (D + 4) * 2^-23.

On the two-layer scene "disparity exact to 1e-5" is taken against the oracle's disparity, not against the layer's slope: the
parabola through three costs of a random texture is not symmetric (the oracle itself is up to 0.14 of a slope step from the layer,
tests/test_disparity_host.py prints it), and what the GPU owes is the definition's value."""
import json
import os

import numpy as np
import pytest
import torch

from lft_amd import disparity as Dm, refocus as R

import disparity_util as DU
import refocus_util as RU

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ULP = 2.0 ** -23
SHAPES = [(24, 20), (9, 37), (5, 3), (33, 65)]          # below the tap span and the window, one past a tile in either direction
INTERPS = ["nearest", "linear", "cubic"]
RADII = [0, 1, 3]


def views(A, H, W, C, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (A, A, H, W, C)).astype(np.uint8)
    return rng.random((A, A, H, W, C)).astype(np.float32)


def apertures(A, seed):
    # the default disk radius uc reaches no view of A = 2 (refused, tests/test_refocus_host.py): A = 2 takes the radius of its views
    disk = R.aperture_weights(A, "disk", radius=0.75) if A == 2 else "disk"
    return {"full": "full", "disk": disk, "user": RU.user_aperture(A, seed)}


def sweep(lf, slopes, **kw):
    return Dm.disparity(torch.from_numpy(lf).to(DEV) if isinstance(lf, np.ndarray) else lf, slopes, **kw)


def check_selection(r, slopes, what):
    """index, disparity and confidence of a result against steps 4-6 applied to its own cost volume."""
    E = r.cost.cpu().numpy()
    k, disp, conf = DU.pick_np(E, slopes)
    assert r.index.dtype == torch.int32 and np.array_equal(r.index.cpu().numpy(), np.argmin(E, 0)), what
    assert np.array_equal(k, np.argmin(E, 0))
    d_err = float(np.abs(r.disparity.cpu().numpy().astype(np.float64) - disp).max(initial=0))
    c_err = float(np.abs(r.confidence.cpu().numpy().astype(np.float64) - conf).max(initial=0))
    assert d_err <= 4 * ULP * float(np.abs(slopes).max()), (what, d_err)
    assert c_err <= (len(slopes) + 4) * ULP, (what, c_err)
    return d_err, c_err


def check_parity(lf, A, slopes, aperture, interp, what, radii=RADII):
    """E for every radius against the oracle (one pass over the views for all radii), and the selection from the GPU's E."""
    table = R.shift_table(A, slopes, aperture, interp)
    taps = R.TAPS[interp]
    m, q = DU.moments_np(lf, table, taps)
    V = np.maximum(q - m * m, 0.0).sum(-1)
    worst = 0.0
    for radius in radii:
        r = sweep(lf, slopes, aperture=aperture, interp=interp, radius=radius, cost_volume=True)
        assert r.cost.dtype == torch.float32 and tuple(r.cost.shape) == V.shape and r.all_in_focus is None
        tol = DU.tol_E(A, lf.shape[-1], radius, table, taps, 1.0)
        err = float(np.abs(r.cost.cpu().numpy().astype(np.float64) - DU.aggregate_np(V, radius)).max())
        d_err, c_err = check_selection(r, slopes, what)
        print(f"{what} r={radius}: max error of E {err:.3e}, tol_E {tol:.3e}; disparity {d_err:.2e}, confidence {c_err:.2e} from pick_np")
        assert err <= tol, (what, radius)
        worst = max(worst, err / tol)
    return worst


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("A", [1, 2, 3, 5])
def test_cost_volume_parity_and_selection(A, interp):
    n = 0
    for H, W in SHAPES:
        for C in (1, 3):
            for dtype in (np.uint8, np.float32):
                lf = views(A, H, W, C, dtype, seed=n)
                for name, ap in apertures(A, seed=n).items():
                    check_parity(lf, A, RU.SLOPES, ap, interp, f"A={A} {interp} {H}x{W}x{C} {np.dtype(dtype).name} {name}")
                n += 1


def test_cost_volume_parity_81_views_and_other_channel_counts():
    check_parity(views(9, 8, 8, 3, np.uint8, 1), 9, RU.SLOPES, "full", "cubic", "A=9 8x8x3 cubic")
    for C in (2, 4):
        for interp in INTERPS:
            check_parity(views(3, 33, 34, C, np.float32, C), 3, RU.SLOPES, "gaussian", interp, f"A=3 33x34x{C} {interp} gaussian")
    # the largest radius, on a view smaller than the window and on one of several tiles
    check_parity(views(3, 5, 3, 1, np.float32, 7), 3, RU.SLOPES, "full", "linear", "A=3 5x3x1 linear", radii=[8])
    check_parity(views(2, 33, 65, 3, np.uint8, 8), 2, RU.SLOPES, "full", "linear", "A=2 33x65x3 linear", radii=[8])


def test_ties_go_to_the_lowest_index():
    """A = 2, nearest: the offsets +-d/2 round to the same taps for |d| < 1 and for 1 <= |d| < 3, so the slopes below fall into
    three groups of identical records and costs."""
    slopes = [-1.4, -1.2, -0.9, -0.6, 0.0, 0.6, 0.9, 1.2, 1.4]
    table = R.shift_table(2, slopes, "full", "nearest")
    same = [k for k in range(1, len(slopes)) if table[k].tobytes() == table[k - 1].tobytes()]
    assert same == [1, 3, 4, 5, 6, 8]                                                # on the table alone
    lf = views(2, 33, 65, 3, np.uint8, 3)
    for radius in (0, 2):
        r = sweep(lf, slopes, interp="nearest", radius=radius, cost_volume=True)
        check_selection(r, slopes, f"ties r={radius}")
        E = r.cost
        for k in same:
            assert torch.equal(E[k], E[k - 1])
            assert not bool((r.index == k).any())                                    # never the later of two equal costs
        assert len(torch.unique(r.index)) == 3


@pytest.mark.parametrize("interp", INTERPS)
def test_all_in_focus_is_the_refocus_stack_at_the_index(interp):
    for A, (H, W), C, dtype in ((3, (33, 65), 3, np.uint8), (5, (24, 20), 1, np.float32), (2, (9, 37), 4, np.float32), (3, (5, 3), 2, np.uint8)):
        lf = torch.from_numpy(views(A, H, W, C, dtype, seed=A)).to(DEV)
        for ap in ("full", RU.user_aperture(A, 1)):
            r32 = sweep(lf, RU.SLOPES, aperture=ap, interp=interp, radius=1, all_in_focus=True, aif_dtype=torch.float32)
            r8 = sweep(lf, RU.SLOPES, aperture=ap, interp=interp, radius=1, all_in_focus=True, aif_dtype=torch.uint8)
            dflt = sweep(lf, RU.SLOPES, aperture=ap, interp=interp, radius=1, all_in_focus=True)
            assert torch.equal(r32.index, r8.index) and dflt.all_in_focus.dtype == lf.dtype
            gather = r32.index.long()[None, :, :, None].expand(1, H, W, C)
            for res, dt in ((r32, torch.float32), (r8, torch.uint8)):
                stack = R.refocus(lf, RU.SLOPES, aperture=ap, interp=interp, out_dtype=dt)
                assert res.all_in_focus.dtype == dt and tuple(res.all_in_focus.shape) == (H, W, C)
                assert torch.equal(res.all_in_focus, stack.gather(0, gather)[0]), (A, H, W, C, interp, dt)


@pytest.mark.parametrize("d0", [1.5, -0.6, 0.1])
@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_plane_comes_back_at_its_slope(d0, interp):
    A, n, radius = 5, 32, 2
    slopes = np.linspace(-2.0, 2.0, 17)
    L, _ = RU.plane(A, n, n, d0)
    table = R.shift_table(A, slopes, "full", interp)
    E, _ = DU.cost_np(L[..., None], table, R.TAPS[interp], radius)
    _, ref, _ = DU.pick_np(E, slopes, np.float64)
    m = radius + int(np.ceil(2.0 * (A - 1) / 2)) + 2
    inner = (slice(m, n - m), slice(m, n - m))
    gate = float(np.abs(ref[inner] - d0).max()) + 1e-4
    got = sweep(L, slopes, interp=interp, radius=radius).disparity.cpu().numpy().astype(np.float64)
    err = float(np.abs(got[inner] - d0).max())
    print(f"plane d0={d0} {interp}: |disparity - d0| {err:.3e}, gate {gate:.3e}")
    assert got.shape == (n, n) and err <= gate and gate < 0.02


@pytest.mark.parametrize("interp,radius,D", [("nearest", 0, 5), ("linear", 1, 9), ("cubic", 2, 17)])
def test_two_layer_scene(interp, radius, D):
    A, H, W = 5, 72, 64
    slopes = np.linspace(-2.0, 2.0, D)
    L, centre = DU.two_layer(A, H, W)
    table = R.shift_table(A, slopes, "full", interp)
    taps = R.TAPS[interp]
    E, _ = DU.cost_np(L, table, taps, radius)
    k, disp, conf = DU.pick_np(E, slopes, np.float64)
    fg, bg = DU.two_layer_interiors(A, H, W, radius)
    both = fg | bg
    r = sweep(L, slopes, interp=interp, radius=radius, all_in_focus=True, cost_volume=True)
    e_err = float(np.abs(r.cost.cpu().numpy() - E).max())
    assert np.array_equal(r.index.cpu().numpy()[both], k[both])
    assert np.all(slopes[k[fg]] == 1.0) and np.all(slopes[k[bg]] == -1.0)
    d_err = float(np.abs(r.disparity.cpu().numpy().astype(np.float64) - disp)[both].max())
    a_err = float(np.abs(r.all_in_focus[..., 0].cpu().numpy().astype(np.float64) - centre)[both].max())
    print(f"two layers {interp} r={radius} D={D}: E error {e_err:.3e}, disparity against the oracle {d_err:.3e}, aif against the "
          f"centre view {a_err:.3e}, min confidence {float(r.confidence.cpu().numpy()[both].min()):.6f}")
    assert d_err <= 1e-5
    assert a_err <= RU.tol(A, table, taps, 1.0) + 1e-7
    assert float(r.confidence.cpu().numpy()[both].min()) > 0.999


def test_edge_cases():
    rng = np.random.default_rng(11)
    # A = 1: one view has no variance
    one = (rng.random((1, 1, 33, 35, 3)) * 4 - 2).astype(np.float32)
    for interp in INTERPS:
        r = sweep(one, RU.SLOPES, interp=interp, radius=1, all_in_focus=True, cost_volume=True)
        assert not bool(r.cost.any()) and not bool(r.index.any()) and not bool(r.confidence.any())
        assert bool((r.disparity == np.float32(RU.SLOPES[0])).all())
        assert torch.equal(r.all_in_focus.cpu(), torch.from_numpy(one[0, 0]))
    # D = 1: the slope itself, confidence 0
    lf = views(3, 24, 37, 3, np.uint8, 12)
    r = sweep(lf, [0.7], radius=2, cost_volume=True)
    assert tuple(r.cost.shape) == (1, 24, 37) and not bool(r.index.any()) and not bool(r.confidence.any())
    assert bool((r.disparity == np.float32(0.7)).all()) and bool((r.cost > 0).all())
    # a constant light field.  Zero: every cost is exactly 0.  One half through four views of weight 1/4, nearest: every product
    # and sum is exact, the same.  Any constant: the costs are rounding residue below tol_E, and the selection follows them.
    for lf in (np.zeros((5, 5, 33, 40, 3), np.uint8), np.full((2, 2, 33, 40, 3), 0.5, np.float32)):
        r = sweep(lf, RU.SLOPES, interp="nearest", radius=1, cost_volume=True)
        assert not bool(r.cost.any()) and not bool(r.index.any()) and not bool(r.confidence.any())
        assert bool((r.disparity == np.float32(RU.SLOPES[0])).all())
    lf = np.full((5, 5, 33, 40, 3), 0.3, np.float32)
    r = sweep(lf, RU.SLOPES, interp="cubic", radius=1, cost_volume=True)
    assert float(r.cost.max()) <= DU.tol_E(5, 3, 1, R.shift_table(5, RU.SLOPES, "full", "cubic"), 4, 0.3)
    check_selection(r, np.array(RU.SLOPES), "constant 0.3")
    assert 0.0 <= float(r.confidence.min()) and float(r.confidence.max()) <= 1.0
    # empty results
    for shape, want in (((3, 3, 0, 7, 3), (0, 7)), ((3, 3, 6, 0, 3), (6, 0))):
        r = sweep(np.zeros(shape, np.float32), [0.0, 1.0], all_in_focus=True, cost_volume=True)
        assert tuple(r.disparity.shape) == want and tuple(r.index.shape) == want and tuple(r.confidence.shape) == want
        assert tuple(r.cost.shape) == (2,) + want and tuple(r.all_in_focus.shape) == want + (3,)
    r = Dm.disparity(torch.zeros(0, 1, 12, 15, device=DEV), [0.0, 1.0], angRes=3, all_in_focus=True, cost_volume=True)
    assert tuple(r.disparity.shape) == (0, 4, 5) and tuple(r.cost.shape) == (0, 2, 4, 5) and tuple(r.all_in_focus.shape) == (0, 4, 5)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_layouts_and_batch_give_identical_bits():
    A, H, W = 3, 21, 34
    slopes = [-1.25, 0.0, 0.5, 0.8]
    kw = dict(radius=1, all_in_focus=True, cost_volume=True)
    for dtype in (np.float32, np.uint8):
        v = torch.from_numpy(views(A, H, W, 1, dtype, 4)[..., 0]).to(DEV)                  # [A, A, H, W]
        mosaic = v.permute(0, 2, 1, 3).reshape(A * H, A * W).contiguous()
        strided = v.permute(2, 3, 0, 1).contiguous().permute(2, 3, 0, 1)
        assert not strided.is_contiguous() and torch.equal(strided, v)
        want = Dm.disparity(v, slopes, **kw)
        assert tuple(want.disparity.shape) == (H, W) and tuple(want.all_in_focus.shape) == (H, W) and tuple(want.cost.shape) == (4, H, W)
        assert want.all_in_focus.dtype == v.dtype and len(torch.unique(want.index)) > 1
        assert same(Dm.disparity(v, slopes, angRes=A, **kw), want)
        assert same(Dm.disparity(mosaic, slopes, angRes=A, **kw), want)
        assert same(Dm.disparity(strided, slopes, **kw), want)
        b1 = Dm.disparity(mosaic[None, None], slopes, angRes=A, **kw)
        assert tuple(b1.disparity.shape) == (1, H, W) and tuple(b1.cost.shape) == (1, 4, H, W) and same([x[0] for x in b1], want)
        v5 = Dm.disparity(v[..., None], slopes, **kw)
        assert tuple(v5.all_in_focus.shape) == (H, W, 1) and torch.equal(v5.all_in_focus[..., 0], want.all_in_focus)
        assert same(v5[:3], want[:3]) and torch.equal(v5.cost, want.cost)
        plain = Dm.disparity(v, slopes, radius=1)                                          # without the optional outputs: the same maps
        assert plain.all_in_focus is None and plain.cost is None and same(plain[:3], want[:3])
    batch = torch.from_numpy(np.random.default_rng(5).random((3, 1, A * H, A * W)).astype(np.float32)).to(DEV)
    got = Dm.disparity(batch, slopes, angRes=A, **kw)
    assert tuple(got.disparity.shape) == (3, H, W) and tuple(got.all_in_focus.shape) == (3, H, W) and tuple(got.cost.shape) == (3, 4, H, W)
    for b in range(3):
        assert same([x[b] for x in got], Dm.disparity(batch[b, 0], slopes, angRes=A, **kw))


def test_crop_interior_equals_the_full_image():
    A, H, W = 3, 70, 75
    slopes = [-1.25, -0.4, 0.5, 1.0]
    lf = torch.from_numpy(views(A, H, W, 3, np.float32, 6)).to(DEV)
    for radius, interp in ((2, "cubic"), (0, "linear")):
        kw = dict(radius=radius, interp=interp, all_in_focus=True, cost_volume=True)
        full = Dm.disparity(lf, slopes, **kw)
        assert same(Dm.disparity(lf, slopes, **kw), full)                                  # two runs, the same bits
        m = radius + int(np.ceil(1.25 * (A - 1) / 2)) + 2
        for y0, x0 in ((13, 7), (1, 33)):
            crop = Dm.disparity(lf[:, :, y0:y0 + 40, x0:x0 + 41], slopes, **kw)             # a strided view, other tiles
            for c, f in zip(crop[:4], full[:4]):
                assert torch.equal(c[m:40 - m, m:41 - m], f[y0 + m:y0 + 40 - m, x0 + m:x0 + 41 - m])
            assert torch.equal(crop.cost[:, m:40 - m, m:41 - m], full.cost[:, y0 + m:y0 + 40 - m, x0 + m:x0 + 41 - m])
            assert not torch.equal(crop.cost, full.cost[:, y0:y0 + 40, x0:x0 + 41])        # the border does differ: replicate


def test_capture_and_replay():
    from lft_amd import train as T
    A, slopes = 3, [-0.5, 0.25, 1.25]
    lf = torch.from_numpy(views(A, 33, 40, 3, np.uint8, 15)).to(DEV)
    kw = dict(radius=2, all_in_focus=True, cost_volume=True)
    want = Dm.disparity(lf, slopes, **kw)                           # eager; table, slopes and scratch are on the device from here on
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side, capture_error_mode=T.CAPTURE_MODE):
            got = Dm.disparity(lf, slopes, **kw)
        for x in got:
            x.fill_(9)
        graph.replay()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert same(got, want)


def test_disparity_error():
    """0 for identical inputs.  Against a copy whose foreground lies at slope 0.5 (smooth texture, so that half-pixel shifts are
    interpolated well): the foreground differs by 0.5, the background by nothing, over the pixels where the reference sweep is
    confident.  min_confidence 0.99 keeps the pixels whose window no occlusion touches (the oracle's interiors are above 0.9999,
    tests/test_disparity_host.py; one occluded view of 25 in one column of a 3 x 3 window already costs more than 0.01)."""
    A, H, W = 5, 72, 64
    slopes = np.linspace(-2.0, 2.0, 9)
    kw = dict(interp="linear", radius=1)
    b = torch.from_numpy(DU.two_layer(A, H, W)[0]).to(DEV)
    a = torch.from_numpy(DU.two_layer(A, H, W, d_fg=0.5, smooth_fg=True)[0]).to(DEV)
    err, share = Dm.disparity_error(b, b, slopes, **kw)
    assert err == 0.0 and 0.5 < share <= 1.0
    err, share = Dm.disparity_error(a, b, slopes, min_confidence=0.99, **kw)
    keep = (Dm.disparity(b, slopes, **kw).confidence >= 0.99).cpu().numpy()
    y0, y1, x0, x1 = DU.FG_BOX
    box = np.zeros((H, W), bool)
    box[y0:y1, x0:x1] = True
    fg_share = float((box & keep).sum()) / float(keep.sum())
    print(f"disparity_error {err:.6f}, foreground share x 0.5 = {0.5 * fg_share:.6f}, counted share {share:.4f}")
    assert abs(share - keep.mean()) < 1e-12 and 0.5 < share < 0.9 and fg_share > 0.1
    assert abs(err - 0.5 * fg_share) <= 1e-3
    # batches compare too, and nothing confident gives nan over a share of 0
    mosaic = torch.rand(2, 1, 3 * 12, 3 * 10, device=DEV)
    assert Dm.disparity_error(mosaic, mosaic, [-1.0, 0.0, 1.0], angRes=3, min_confidence=0.0) == (0.0, 1.0)
    err, share = Dm.disparity_error(mosaic, mosaic, [-1.0, 0.0, 1.0], angRes=3, min_confidence=2.0)
    assert np.isnan(err) and share == 0.0


def test_tool_writes_the_maps(golden_dir, tmp_path, capsys):
    import sys
    from types import SimpleNamespace
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import disparity as tool
    from lft_amd import colour, png, prepare, trainer
    from lft_amd.params import deterministic_state
    from model import LFT
    A, s = 3, 2
    mat = os.path.join(golden_dir, "prepare_lf_v73.mat")
    lf = prepare.to_device(prepare.load_lf(mat), A, DEV)             # [3, 3, 9, 7, 3] uint8 in the file's reversed memory order
    slopes = [-1.0, -0.5, 0.0, 0.5, 1.0]
    names = ["disparity.png", "confidence.png", "all_in_focus.png", "disparity.npy"]

    def check(out_dir, prefix, field, **kw):
        want = Dm.disparity(field, slopes, all_in_focus=True, aif_dtype=torch.uint8, **kw)
        d = want.disparity.cpu().numpy()
        assert np.array_equal(np.load(os.path.join(out_dir, prefix + "disparity.npy")), d)
        g = np.rint(np.clip((d - np.float32(-1.0)) * np.float32(255.0 / 2.0), 0, 255)).astype(np.uint8)
        assert np.array_equal(png.read_png(os.path.join(out_dir, prefix + "disparity.png")), np.repeat(g[..., None], 3, axis=2))
        c = np.rint(np.clip(want.confidence.cpu().numpy() * np.float32(255.0), 0, 255)).astype(np.uint8)
        assert np.array_equal(png.read_png(os.path.join(out_dir, prefix + "confidence.png")), np.repeat(c[..., None], 3, axis=2))
        assert np.array_equal(png.read_png(os.path.join(out_dir, prefix + "all_in_focus.png")), want.all_in_focus.cpu().numpy())

    out_dir = str(tmp_path / "raw")
    paths = tool.main(["--lf", mat, "--angRes", str(A), "--out_dir", out_dir, "--slopes=-1:1:5", "--radius", "1"])
    assert [os.path.basename(p) for p in paths] == names and sorted(os.listdir(out_dir)) == sorted(names)
    check(out_dir, "", lf, radius=1)
    capsys.readouterr()
    # super-resolved and bicubic views: slopes in HR pixels, and the figure between them
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, s, seed=12).items()})
    net = net.to(DEV).eval()
    ckpt = str(tmp_path / "net.pth.tar")
    trainer.save_checkpoint(net, ckpt, 1)
    out_dir = str(tmp_path / "sr")
    paths = tool.main(["--lf", mat, "--angRes", str(A), "--out_dir", out_dir, "--slopes=-1,-0.5,0,0.5,1", "--interp", "cubic", "--aperture", "disk",
                       "--radius", "2", "--min_confidence", "0.25", "--path_pre_pth", ckpt, "--scale_factor", str(s), "--bicubic",
                       "--patch_size_for_test", "8", "--stride_for_test", "4"])
    assert len(paths) == 8 and sorted(os.listdir(out_dir)) == sorted(names + ["bicubic_" + n for n in names])
    sr = colour.super_resolve_lf(net, lf, patch=8, stride=4)
    base = colour.bicubic_lf(lf, A, s)
    check(out_dir, "", sr, radius=2, interp="cubic", aperture="disk")
    check(out_dir, "bicubic_", base, radius=2, interp="cubic", aperture="disk")
    line = json.loads([text for text in capsys.readouterr().out.splitlines() if text.startswith("{")][0])
    err, share = Dm.disparity_error(sr, base, slopes, min_confidence=0.25, radius=2, interp="cubic", aperture="disk")
    assert line["confident_share"] == share and (line["disparity_error"] == err or (np.isnan(err) and np.isnan(line["disparity_error"])))
