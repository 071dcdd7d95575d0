"""GPU tests of the semi-global aggregation (lft_sgm: k_sgm_scan + k_sgm_pick, lft_amd.disparity.regularize) against the numpy
float32 restatement of its definition (tests/sgm_util.py).

The aggregated volume S is held to equality: the definition consists of min and +, every sum has a fixed order, and the restatement
rounds each operation once as the kernels do.  Index, disparity and confidence are then checked from the GPU's own S with the
selection steps restated in numpy float32 (``disparity_util.pick_np``) under the gates of tests/test_gpu_disparity.py: index
exactly, disparity within 4 * 2^-23 * max|slope|, confidence within (D + 4) * 2^-23."""
import os

import numpy as np
import pytest
import torch

from lft_amd import disparity as Dm, refocus as R

import disparity_util as DU
import sgm_util as SU

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ULP = 2.0 ** -23
F = np.float32
# below any strip, one past a wave or tile in each direction, taller than wide and wider than tall: diagonals enter through every edge
SHAPES = [(1, 1), (1, 37), (37, 1), (5, 3), (33, 65), (70, 29), (66, 130)]


def slopes_for(D):
    return np.linspace(-2.0, 2.0, D) if D > 1 else np.array([0.5])


def costs(D, H, W, quantised, seed):
    """Random costs >= 0: multiples of 1/8 (exact ties and exact zeros occur), or rng.random as it comes."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 9, (D, H, W)) / 8).astype(F) if quantised else rng.random((D, H, W)).astype(F)


def penalties(E, quantised):
    return (0.25, 1.0) if quantised else (0.1 * float(E.mean()), float(E.mean()))


def run(E, slopes, p1, p2, **kw):
    return Dm.regularize(torch.from_numpy(E).to(DEV) if isinstance(E, np.ndarray) else E, slopes, p1, p2, **kw)


def check_selection(r, slopes, what):
    """index, disparity and confidence of a result against steps 4-6 applied to its own aggregated volume."""
    S = r.cost.cpu().numpy()
    k, disp, conf = DU.pick_np(S, slopes)
    assert r.index.dtype == torch.int32 and np.array_equal(r.index.cpu().numpy(), np.argmin(S, 0)), what
    assert np.array_equal(k, np.argmin(S, 0))
    d_err = float(np.abs(r.disparity.cpu().numpy().astype(np.float64) - disp).max(initial=0))
    c_err = float(np.abs(r.confidence.cpu().numpy().astype(np.float64) - conf).max(initial=0))
    assert d_err <= 4 * ULP * float(np.abs(slopes).max()), (what, d_err)
    assert c_err <= (len(slopes) + 4) * ULP, (what, c_err)


def check_equal(E, slopes, p1, p2, paths, what, guide=None, gain=0.0):
    r = run(E, slopes, p1, p2, paths=paths, aggregated=True, guide=None if guide is None else torch.from_numpy(guide).to(DEV), edge_gain=gain)
    want = SU.sgm_np(E, p1, p2, paths, guide, gain)
    got = r.cost.cpu().numpy()
    assert got.dtype == F and got.shape == E.shape and r.all_in_focus is None
    differ = int((got != want).sum())
    if differ:
        at = np.argwhere(got != want)[0]
        print(f"{what}: {differ} of {want.size} differ, first at {tuple(at)}: {got[tuple(at)]!r} against {want[tuple(at)]!r}")
    assert np.array_equal(got, want), what
    check_selection(r, slopes, what)
    return r


@pytest.mark.parametrize("D", [1, 2, 3, 9, 33, 64, 65])
def test_aggregated_volume_bit_for_bit(D):
    sl = slopes_for(D)
    n = 0
    for H, W in SHAPES:
        for paths in (4, 8):
            for quantised in (True, False):
                E = costs(D, H, W, quantised, seed=100 * D + n)
                check_equal(E, sl, *penalties(E, quantised), paths, f"D={D} {H}x{W} paths={paths} quantised={quantised}")
                n += 1


def test_aggregated_volume_bit_for_bit_256_slopes():
    sl = slopes_for(256)
    for paths in (4, 8):
        for quantised in (True, False):
            E = costs(256, 7, 9, quantised, seed=paths + quantised)
            check_equal(E, sl, *penalties(E, quantised), paths, f"D=256 7x9 paths={paths} quantised={quantised}")
    E = costs(129, 9, 40, False, seed=3)                                # two slopes per lane of a row, past one chunk of it
    check_equal(E, slopes_for(129), *penalties(E, False), 8, "D=129 9x40")
    # the register counts of a line's segment the D of the other tests do not reach: 5 .. 8 (D = 17 .. 32); D = 17 leaves the
    # last segment two of its five slopes
    for D in (17, 20, 32):
        E = costs(D, 33, 65, D % 2 == 0, seed=D)
        check_equal(E, slopes_for(D), *penalties(E, D % 2 == 0), 8, f"D={D} 33x65")


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_aggregated_volume_of_the_sweeps_own_cost(dtype):
    A, sl = 3, np.linspace(-1.5, 1.5, 9)
    rng = np.random.default_rng(5)
    for H, W in ((33, 65), (70, 29)):
        lf = rng.integers(0, 256, (A, A, H, W, 3)).astype(np.uint8) if dtype == np.uint8 else rng.random((A, A, H, W, 3)).astype(F)
        E = Dm.disparity(torch.from_numpy(lf).to(DEV), sl, interp="cubic", radius=1, cost_volume=True).cost.cpu().numpy()
        assert float(E.min()) >= 0.0 and float(E.max()) > 0.0
        for paths in (4, 8):
            check_equal(E, sl, *penalties(E, False), paths, f"sweep {np.dtype(dtype).name} {H}x{W} paths={paths}")


def test_guide():
    rng = np.random.default_rng(6)
    for (D, H, W), quantised in (((9, 33, 65), False), ((5, 70, 29), True), ((3, 1, 37), False), ((2, 37, 1), True)):
        E = costs(D, H, W, quantised, seed=D)
        p1, p2 = penalties(E, quantised)
        g = rng.random((H, W)).astype(F)
        gain = 2.0 * (p2 - p1)                                          # the clamp at P1 bites where |dg| > 1/2
        for r in SU.DIRECTIONS:
            low, high = SU.clamp_bites(g, r, p1, p2, gain)
            if (r[0] == 0 or H > 1) and (r[1] == 0 or W > 1):
                assert low > 0 and high > 0, (r, low, high)
        for paths in (4, 8):
            with_guide = check_equal(E, slopes_for(D), p1, p2, paths, f"guide D={D} {H}x{W} paths={paths}", g, gain)
            plain = run(E, slopes_for(D), p1, p2, paths=paths, aggregated=True)
            # with two slopes the jump is the step of one slope: min(L_k, L_other + P1) <= M + P1 <= c, and P2' never decides
            assert torch.equal(with_guide.cost, plain.cost) == (D < 3)
            # a gain of 0 is no guide
            zero = run(E, slopes_for(D), p1, p2, paths=paths, aggregated=True, guide=torch.from_numpy(g).to(DEV))
            assert torch.equal(zero.cost, plain.cost)


def same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def test_ties_go_to_the_lowest_index():
    """A constant light field: every cost is exactly 0, so is every L_r and S; index 0 and confidence 0 everywhere."""
    sl = np.linspace(-2.0, 2.0, 9)
    how = dict(p1=0.1, p2=1.0)
    for lf in (np.zeros((5, 5, 33, 40, 3), np.uint8), np.full((2, 2, 33, 40, 3), 0.5, F)):
        r = Dm.disparity(torch.from_numpy(lf).to(DEV), sl, interp="nearest", radius=1, cost_volume=True, regularize=how)
        assert not bool(r.cost.any()) and not bool(r.index.any()) and not bool(r.confidence.any())
        assert bool((r.disparity == F(sl[0])).all())
    # equal costs in every slice: S has them too, and the lowest index wins
    E = np.repeat(costs(1, 33, 65, True, 1), 5, axis=0)
    r = check_equal(E, slopes_for(5), 0.25, 1.0, 8, "equal slices")
    assert not bool(r.index.any()) and not bool(r.confidence.any())


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_all_in_focus_is_the_refocus_stack_at_the_index(interp):
    rng = np.random.default_rng(7)
    sl = np.linspace(-1.5, 1.5, 7)
    for A, (H, W), C, dtype in ((3, (33, 65), 3, np.uint8), (2, (9, 37), 4, np.float32), (3, (24, 20), 1, np.float32)):
        lf = rng.integers(0, 256, (A, A, H, W, C)).astype(np.uint8) if dtype == np.uint8 else rng.random((A, A, H, W, C)).astype(F)
        lf = torch.from_numpy(lf).to(DEV)
        E = Dm.disparity(lf, sl, interp=interp, radius=1, cost_volume=True).cost
        how = dict(zip(("p1", "p2"), Dm.penalties_from_cost(E)), paths=8)
        r32 = Dm.disparity(lf, sl, interp=interp, radius=1, all_in_focus=True, aif_dtype=torch.float32, regularize=how)
        r8 = Dm.disparity(lf, sl, interp=interp, radius=1, all_in_focus=True, aif_dtype=torch.uint8, regularize=how)
        dflt = Dm.disparity(lf, sl, interp=interp, radius=1, all_in_focus=True, regularize=how)
        assert torch.equal(r32.index, r8.index) and dflt.all_in_focus.dtype == lf.dtype and r32.cost is None
        assert torch.equal(r32.index, Dm.regularize(E, sl, **how).index)
        gather = r32.index.long()[None, :, :, None].expand(1, H, W, C)
        for res, dt in ((r32, torch.float32), (r8, torch.uint8)):
            stack = R.refocus(lf, sl, interp=interp, out_dtype=dt)
            assert res.all_in_focus.dtype == dt and tuple(res.all_in_focus.shape) == (H, W, C)
            assert torch.equal(res.all_in_focus, stack.gather(0, gather)[0]), (A, H, W, C, interp, dt)
        # views without a channel axis: the stack and the image have none either
        if C == 1:
            flat = Dm.disparity(lf[..., 0], sl, interp=interp, radius=1, all_in_focus=True, aif_dtype=torch.float32, regularize=how)
            assert tuple(flat.all_in_focus.shape) == (H, W) and torch.equal(flat.all_in_focus, r32.all_in_focus[..., 0])


def test_horizontal_flip_with_four_paths():
    for D, H, W, quantised in ((9, 33, 65, False), (33, 70, 29, True)):
        E = costs(D, H, W, quantised, seed=W)
        p1, p2 = penalties(E, quantised)
        S = run(E, slopes_for(D), p1, p2, paths=4, aggregated=True).cost
        flipped = run(np.ascontiguousarray(E[:, :, ::-1]), slopes_for(D), p1, p2, paths=4, aggregated=True).cost
        assert torch.equal(flipped, S.flip(2))


def test_batches_and_layouts_give_identical_bits():
    B, D, H, W, C = 3, 9, 33, 40, 2
    rng = np.random.default_rng(8)
    E = torch.from_numpy(rng.random((B, D, H, W)).astype(F)).to(DEV)
    g = torch.from_numpy(rng.random((B, H, W)).astype(F)).to(DEV)
    stack = torch.from_numpy(rng.random((B, D, H, W, C)).astype(F)).to(DEV)
    sl = slopes_for(D)
    kw = dict(p1=0.05, p2=0.6, edge_gain=1.0, aggregated=True)
    for paths in (4, 8):
        got = Dm.regularize(E, sl, paths=paths, guide=g, stack=stack, **kw)
        assert tuple(got.disparity.shape) == (B, H, W) and tuple(got.cost.shape) == (B, D, H, W) and tuple(got.all_in_focus.shape) == (B, H, W, C)
        assert got.all_in_focus.dtype == torch.float32 and len(torch.unique(got.index)) > 1
        for b in range(B):
            one = Dm.regularize(E[b], sl, paths=paths, guide=g[b], stack=stack[b], **kw)
            assert tuple(one.disparity.shape) == (H, W) and tuple(one.cost.shape) == (D, H, W) and tuple(one.all_in_focus.shape) == (H, W, C)
            assert same([x[b] for x in got], one)
            assert same([x[0] for x in Dm.regularize(E[b][None], sl, paths=paths, guide=g[b][None], stack=stack[b][None], **kw)], one)
        # a stack without a channel axis, a strided cost
        flat = Dm.regularize(E, sl, paths=paths, guide=g, stack=stack[..., 0].contiguous(), aif_dtype=torch.uint8, **kw)
        assert tuple(flat.all_in_focus.shape) == (B, H, W) and flat.all_in_focus.dtype == torch.uint8 and same(flat[:3], got[:3])
        strided = E.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert not strided.is_contiguous() and same(Dm.regularize(strided, sl, paths=paths, guide=g, stack=stack, **kw), got)
        plain = Dm.regularize(E, sl, paths=paths, guide=g, p1=0.05, p2=0.6, edge_gain=1.0)
        assert plain.cost is None and plain.all_in_focus is None and same(plain[:3], got[:3])


def test_two_runs_and_capture_and_replay():
    from lft_amd import train as T
    D, H, W = 33, 66, 130
    E = torch.from_numpy(costs(D, H, W, False, 9)).to(DEV)
    g = torch.from_numpy(np.random.default_rng(9).random((H, W)).astype(F)).to(DEV)
    stack = torch.rand(D, H, W, 3, device=DEV)
    sl = slopes_for(D)
    kw = dict(p1=0.05, p2=0.5, paths=8, guide=g, edge_gain=0.7, stack=stack, aif_dtype=torch.uint8, aggregated=True)
    want = Dm.regularize(E, sl, **kw)                                # eager; slopes and scratch are on the device from here on
    assert same(Dm.regularize(E, sl, **kw), want)                    # two runs, the same bits
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side, capture_error_mode=T.CAPTURE_MODE):
            got = Dm.regularize(E, sl, **kw)
        for x in got:
            x.fill_(9)
        graph.replay()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert same(got, want)


def test_constant_patch_scene():
    """Winner-take-all never finds the plane inside the patch (slopes 0.5, 1 and 1.5 tie at cost 0 there and the lowest wins); with
    regularize the index is the restatement's from the sweep's own E everywhere, and the plane's on both interiors."""
    L = torch.from_numpy(SU.patch_scene()).to(DEV)
    kw = dict(interp="linear", radius=1)
    plain = Dm.disparity(L, SU.SLOPES, cost_volume=True, **kw)
    E = plain.cost.cpu().numpy()
    wta = plain.index.cpu().numpy()
    assert not np.any(wta[SU.PATCH_INTERIOR] == SU.K_PLANE) and np.all(wta[20:28, 20:28] < SU.K_PLANE)
    mean = float(E.mean())
    for paths in (4, 8):
        for a, b in SU.PENALTIES:
            r = Dm.disparity(L, SU.SLOPES, regularize=dict(p1=a * mean, p2=b * mean, paths=paths), **kw)
            k = r.index.cpu().numpy()
            assert np.array_equal(k, np.argmin(SU.sgm_np(E, a * mean, b * mean, paths), 0)), (paths, a, b)
            assert np.all(k[SU.PATCH_INTERIOR] == SU.K_PLANE) and np.all(k[SU.TEXTURE_INTERIOR] == SU.K_PLANE), (paths, a, b)
    assert same(Dm.disparity(L, SU.SLOPES, cost_volume=True, **kw), plain)


def test_unchanged_path_and_empty_shapes(monkeypatch):
    rng = np.random.default_rng(10)
    lf = torch.from_numpy(rng.integers(0, 256, (3, 3, 21, 34, 3)).astype(np.uint8)).to(DEV)
    sl = [-1.25, 0.0, 0.5, 0.8]
    kw = dict(radius=1, all_in_focus=True, cost_volume=True)
    assert same(Dm.disparity(lf, sl, regularize=None, **kw), Dm.disparity(lf, sl, **kw))
    how = dict(p1=0.01, p2=0.1)
    for shape, want in (((3, 3, 0, 7, 3), (0, 7)), ((3, 3, 6, 0, 3), (6, 0))):
        r = Dm.disparity(torch.zeros(shape, device=DEV), [0.0, 1.0], regularize=how, **kw)
        assert tuple(r.disparity.shape) == want and tuple(r.index.shape) == want and tuple(r.confidence.shape) == want
        assert tuple(r.cost.shape) == (2,) + want and tuple(r.all_in_focus.shape) == want + (3,)
    r = Dm.disparity(torch.zeros(0, 1, 12, 15, device=DEV), [0.0, 1.0], angRes=3, regularize=how, **kw)
    assert tuple(r.disparity.shape) == (0, 4, 5) and tuple(r.cost.shape) == (0, 2, 4, 5) and tuple(r.all_in_focus.shape) == (0, 4, 5)
    r = Dm.regularize(torch.zeros(0, 3, 4, 5, device=DEV), [0.0, 0.5, 1.0], 0.1, 1.0, aggregated=True, stack=torch.zeros(0, 3, 4, 5, 2, device=DEV))
    assert tuple(r.index.shape) == (0, 4, 5) and tuple(r.cost.shape) == (0, 3, 4, 5) and tuple(r.all_in_focus.shape) == (0, 4, 5, 2)
    # a batch through disparity: element b equals the single light field
    batch = torch.from_numpy(rng.random((2, 1, 3 * 21, 3 * 34)).astype(F)).to(DEV)
    got = Dm.disparity(batch, sl, angRes=3, regularize=how, **kw)
    assert tuple(got.disparity.shape) == (2, 21, 34) and tuple(got.all_in_focus.shape) == (2, 21, 34) and tuple(got.cost.shape) == (2, 4, 21, 34)
    for b in range(2):
        assert same([x[b] for x in got], Dm.disparity(batch[b, 0], sl, angRes=3, regularize=how, **kw))
    # leave_one_out hands the argument to its sweeps
    from lft_amd import views as V
    views = torch.from_numpy(DU.two_layer(5, 40, 40, box=(12, 28, 12, 28))[0]).to(DEV)
    slopes = np.linspace(-2.0, 2.0, 9)
    seen, sweep = [], Dm.disparity
    monkeypatch.setattr(Dm, "disparity", lambda *a, **k: (seen.append(k.get("regularize")), sweep(*a, **k))[1])
    how = dict(p1=1e-3, p2=1e-2, paths=4)
    scores = V.leave_one_out(views, slopes, positions=[(2, 2), (0, 4)], radius=1, regularize=how)
    assert [s for s in seen if s is not None] == [how, how] and len(scores) == 2 and all(s > 0 for s in scores)     # None: the sweep inside
    del seen[:]
    assert V.leave_one_out(views, slopes, positions=[(2, 2)], radius=1, regularize=None) == V.leave_one_out(views, slopes, positions=[(2, 2)], radius=1)
    assert seen == [None, None]


def test_tool_writes_the_regularized_maps(golden_dir, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import disparity as tool
    from lft_amd import png, prepare
    A = 3
    mat = os.path.join(golden_dir, "prepare_lf_v73.mat")
    lf = prepare.to_device(prepare.load_lf(mat), A, DEV)             # [3, 3, 9, 7, 3] uint8 in the file's reversed memory order
    slopes = [-1.0, -0.5, 0.0, 0.5, 1.0]
    names = ["disparity.png", "confidence.png", "all_in_focus.png", "disparity.npy"]
    wta = Dm.disparity(lf, slopes, radius=1, all_in_focus=True, aif_dtype=torch.float32, cost_volume=True)
    p1, p2 = Dm.penalties_from_cost(wta.cost)

    def check(out_dir, want):
        assert sorted(os.listdir(out_dir)) == sorted(names)
        d = want.disparity.cpu().numpy()
        assert np.array_equal(np.load(os.path.join(out_dir, "disparity.npy")), d)
        g = np.rint(np.clip((d - F(-1.0)) * F(255.0 / 2.0), 0, 255)).astype(np.uint8)
        assert np.array_equal(png.read_png(os.path.join(out_dir, "disparity.png")), np.repeat(g[..., None], 3, axis=2))
        c = np.rint(np.clip(want.confidence.cpu().numpy() * F(255.0), 0, 255)).astype(np.uint8)
        assert np.array_equal(png.read_png(os.path.join(out_dir, "confidence.png")), np.repeat(c[..., None], 3, axis=2))
        assert np.array_equal(png.read_png(os.path.join(out_dir, "all_in_focus.png")), want.all_in_focus.cpu().numpy())

    base = ["--lf", mat, "--angRes", str(A), "--slopes=-1:1:5", "--radius", "1"]
    kw = dict(radius=1, all_in_focus=True, aif_dtype=torch.uint8)
    out_dir = str(tmp_path / "default")
    paths = tool.main(base + ["--out_dir", out_dir, "--regularize"])
    assert [os.path.basename(p) for p in paths] == names
    check(out_dir, Dm.disparity(lf, slopes, regularize=dict(p1=p1, p2=p2, paths=8), **kw))
    out_dir = str(tmp_path / "guided")
    tool.main(base + ["--out_dir", out_dir, "--regularize", "--p1", "0.001", "--p2", "0.02", "--paths", "4", "--edge_gain", "0.05"])
    guided = Dm.disparity(lf, slopes, regularize=dict(p1=0.001, p2=0.02, paths=4, guide=wta.all_in_focus.mean(-1), edge_gain=0.05), **kw)
    check(out_dir, guided)
    # without the new flags: the file list and bytes of the existing tool test
    out_dir = str(tmp_path / "raw")
    paths = tool.main(base + ["--out_dir", out_dir])
    assert [os.path.basename(p) for p in paths] == names
    check(out_dir, Dm.disparity(lf, slopes, **kw))
