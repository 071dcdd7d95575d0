"""GPU tests of the synthetic refocus (lft_refocus / k_refocus, lft_amd.refocus) against the fp64 numpy restatement of its definition
(tests/refocus_util.py), which takes the same fp32-rounded table: only fp32 accumulation separates the two, and the tolerance is the
derived bound tol = (A^2 + 16) * 2^-23 * S^2 * max|x| (7.6e-6 for A = 5, cubic, data in [0, 1])."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import colour, refocus as R
from lft_amd._lib import LftError

import refocus_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(24, 20), (9, 37), (5, 3), (33, 65)]          # below the tap span, one past a tile in either direction
INTERPS = ["nearest", "linear", "cubic"]


def views(A, H, W, C, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (A, A, H, W, C)).astype(np.uint8)
    return rng.random((A, A, H, W, C)).astype(np.float32)


def apertures(A, seed):
    # the default disk radius uc reaches no view of A = 2 (refused, tests/test_refocus_host.py): A = 2 takes the radius of its views
    disk = R.aperture_weights(A, "disk", radius=0.75) if A == 2 else "disk"
    return {"full": "full", "disk": disk, "user": U.user_aperture(A, seed)}


def check_parity(lf, A, slopes, aperture, interp, what):
    table = R.shift_table(A, slopes, aperture, interp)
    taps = R.TAPS[interp]
    ref = U.refocus_np(lf, table, taps)
    got = R.refocus(torch.from_numpy(lf).to(DEV), slopes, aperture=aperture, interp=interp, out_dtype=torch.float32)
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape
    tol = U.tol(A, table, taps, 1.0)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
    print(f"{what}: max error {err:.3e}, tol {tol:.3e}")
    assert err <= tol, what


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("A", [1, 2, 3, 5])
def test_oracle_parity(A, interp):
    n = 0
    for H, W in SHAPES:
        for C in (1, 3):
            for dtype in (np.uint8, np.float32):
                lf = views(A, H, W, C, dtype, seed=n)
                for name, ap in apertures(A, seed=n).items():
                    check_parity(lf, A, U.SLOPES, ap, interp, f"A={A} {interp} {H}x{W}x{C} {np.dtype(dtype).name} {name}")
                n += 1


def test_oracle_parity_81_views_and_other_channel_counts():
    check_parity(views(9, 8, 8, 3, np.uint8, 1), 9, U.SLOPES, "full", "cubic", "A=9 8x8x3 cubic")
    for C in (2, 4):
        for interp in INTERPS:
            check_parity(views(3, 33, 34, C, np.float32, C), 3, U.SLOPES, "gaussian", interp, f"A=3 33x34x{C} {interp} gaussian")


@pytest.mark.parametrize("d0,interp", [(2.0, "nearest"), (1.5, "cubic")])
def test_sign_and_geometry(d0, interp):
    """A Lambertian plane of slope d0 comes back as f at +d0, and does not at -d0."""
    A, n = 5, 32
    L, f = U.plane(A, n, n, d0)
    table = R.shift_table(A, [d0, -d0], "full", interp)
    got = R.refocus(torch.from_numpy(L).to(DEV), [d0, -d0], interp=interp).cpu().numpy().astype(np.float64)
    assert got.shape == (2, n, n)
    m = int(np.ceil(abs(d0) * (A - 1) / 2)) + 2
    inner = (slice(m, n - m), slice(m, n - m))
    tol = U.tol(A, table, R.TAPS[interp], 1.0)
    if interp == "nearest":      # integer shifts: every view holds f itself there, rounded to fp32
        gate = tol
    else:                        # the interpolation error of the oracle's own +d0 result, and the kernel's distance from the oracle
        ref = U.refocus_np(L[..., None], table, 4)[0, ..., 0]
        gate = float(np.abs(ref[inner] - f[inner]).max()) + tol
        assert gate < 2e-3
    err_p, err_m = float(np.abs(got[0][inner] - f[inner]).max()), float(np.abs(got[1][inner] - f[inner]).max())
    print(f"d0={d0} {interp}: |R(+d0) - f| {err_p:.3e} (gate {gate:.3e}), |R(-d0) - f| {err_m:.3e}")
    assert err_p <= gate and err_m > 0.1


def test_layouts_give_identical_bits():
    A, H, W = 3, 21, 34
    slopes = [-1.25, 0.0, 0.5]
    for dtype in (np.float32, np.uint8):
        v = torch.from_numpy(views(A, H, W, 1, dtype, 4)[..., 0]).to(DEV)                  # [A, A, H, W]
        mosaic = v.permute(0, 2, 1, 3).reshape(A * H, A * W).contiguous()
        hwaa = v.permute(2, 3, 0, 1).contiguous()                                          # [H, W, A, A]
        strided = hwaa.permute(2, 3, 0, 1)
        assert not strided.is_contiguous() and torch.equal(strided, v)
        want = R.refocus(v, slopes, out_dtype=torch.float32)
        assert tuple(want.shape) == (3, H, W)
        assert torch.equal(R.refocus(v, slopes, angRes=A, out_dtype=torch.float32), want)
        assert torch.equal(R.refocus(mosaic, slopes, angRes=A, out_dtype=torch.float32), want)
        b1 = R.refocus(mosaic[None, None], slopes, angRes=A, out_dtype=torch.float32)
        assert tuple(b1.shape) == (1, 3, H, W) and torch.equal(b1[0], want)
        assert torch.equal(R.refocus(strided, slopes, out_dtype=torch.float32), want)
        assert torch.equal(R.refocus(v[..., None], slopes, out_dtype=torch.float32), want[..., None])
        assert R.refocus(v, slopes).dtype == v.dtype                                       # out_dtype defaults to the input's
    batch = torch.from_numpy(np.random.default_rng(5).random((3, 1, A * H, A * W)).astype(np.float32)).to(DEV)
    got = R.refocus(batch, slopes, angRes=A)
    assert tuple(got.shape) == (3, 3, H, W)
    for b in range(3):
        assert torch.equal(got[b], R.refocus(batch[b, 0], slopes, angRes=A))
    for bad in (lambda: R.refocus(batch, slopes), lambda: R.refocus(batch[0, 0], slopes, angRes=4), lambda: R.refocus(batch[0, 0], slopes),
                lambda: R.refocus(batch.double(), slopes, angRes=A), lambda: R.refocus(batch, slopes, angRes=A, out_dtype=torch.float16),
                lambda: R.refocus(batch[0], slopes), lambda: R.refocus(torch.zeros(3, 3, 4, 4, 5, device=DEV), slopes),
                lambda: R.refocus(batch, slopes, angRes=A, interp="lanczos")):
        with pytest.raises(LftError):
            bad()


def test_tile_independence():
    A, H, W = 3, 70, 75
    slopes = [-1.25, 0.5]
    lf = torch.from_numpy(views(A, H, W, 1, np.float32, 6)[..., 0]).to(DEV)
    full = R.refocus(lf, slopes)
    assert torch.equal(R.refocus(lf, slopes), full)                                        # two runs, the same bits
    m = int(np.ceil(1.25 * (A - 1) / 2)) + 2
    for y0, x0 in ((13, 7), (1, 33)):
        crop = R.refocus(lf[:, :, y0:y0 + 40, x0:x0 + 41], slopes)                          # a strided view, other tiles
        assert tuple(crop.shape) == (2, 40, 41)
        assert torch.equal(crop[:, m:40 - m, m:41 - m], full[:, y0 + m:y0 + 40 - m, x0 + m:x0 + 41 - m])
        assert not torch.equal(crop, full[:, y0:y0 + 40, x0:x0 + 41])                      # the border does differ: replicate


@pytest.mark.parametrize("A", [3, 5])
def test_quantised_output(A):
    for H, W in SHAPES:
        for C in (1, 3):
            for interp in INTERPS:
                lf = views(A, H, W, C, np.uint8, seed=0)
                table = R.shift_table(A, U.SLOPES, "full", interp)
                taps = R.TAPS[interp]
                ref = U.refocus_np(lf, table, taps)
                tol = U.tol(A, table, taps, 1.0)
                near = U.tie_distance(ref) <= 255 * tol
                assert near.mean() <= 0.02, (H, W, C, interp, float(near.mean()))          # on the reference alone
                got = R.refocus(torch.from_numpy(lf).to(DEV), U.SLOPES, interp=interp)
                assert got.dtype == torch.uint8 and tuple(got.shape) == ref.shape
                diff = np.abs(got.cpu().numpy().astype(np.int64) - U.quantise(ref).astype(np.int64))
                print(f"A={A} {H}x{W}x{C} {interp}: {float(near.mean()):.4%} near ties, {int((diff != 0).sum())} of {diff.size} differ")
                assert diff[~near].max(initial=0) == 0 and diff.max() <= 1
    # values outside [0, 1] clip: float input in [-1, 2] through a small aperture
    lf = (views(A, 24, 20, 3, np.float32, 9) * 3.0 - 1.0).astype(np.float32)
    ap = R.aperture_weights(A, "disk", radius=1.0)
    table = R.shift_table(A, U.SLOPES, ap, "cubic")
    ref = U.refocus_np(lf, table, 4)
    assert ref.min() < -0.05 and ref.max() > 1.05
    near = U.tie_distance(ref) <= 255 * U.tol(A, table, 4, float(np.abs(lf).max()))
    got = R.refocus(torch.from_numpy(lf).to(DEV), U.SLOPES, aperture=ap, out_dtype=torch.uint8).cpu().numpy().astype(np.int64)
    diff = np.abs(got - U.quantise(ref).astype(np.int64))
    assert diff[~near].max(initial=0) == 0 and diff.max() <= 1 and near.mean() <= 0.02


def test_identities():
    rng = np.random.default_rng(8)
    # A = 1: the view itself for any slope and interpolation, exact for fp32 input
    one = torch.from_numpy((rng.random((1, 1, 33, 35, 3)) * 4 - 2).astype(np.float32)).to(DEV)
    for interp in INTERPS:
        got = R.refocus(one, U.SLOPES, interp=interp)
        assert all(torch.equal(got[k], one[0, 0]) for k in range(len(U.SLOPES))), interp
    # uint8 enters as x / 255, correctly rounded, for every byte
    ramp = torch.arange(256, dtype=torch.uint8, device=DEV).reshape(1, 1, 8, 32)
    exact = (np.arange(256, dtype=np.float32) / np.float32(255)).reshape(8, 32)           # IEEE division on the host
    got = R.refocus(ramp, [0.0, 3.0], out_dtype=torch.float32)[0].cpu().numpy()
    print(f"x / 255: {int((got != exact).sum())} of 256 bytes differ from the correctly rounded quotient")
    assert np.array_equal(got, exact)
    assert torch.equal(R.refocus(ramp, [0.0], interp="nearest")[0], ramp[0, 0])
    # slope 0: every interpolation gives the same bits
    lf = torch.from_numpy(views(5, 24, 37, 3, np.float32, 10)).to(DEV)
    for ap in ("full", "gaussian"):
        r = [R.refocus(lf, [0.0], aperture=ap, interp=i) for i in INTERPS]
        assert torch.equal(r[0], r[1]) and torch.equal(r[0], r[2])
    # a single view of the aperture, nearest: that view shifted by the integer offset, replicated at the border, exact
    A, H, W = 5, 24, 37
    for (u, v), d in (((0, 4), 1.5), ((3, 1), -3.0), ((2, 2), 7.0), ((4, 0), 40.0)):
        ap = np.zeros((A, A))
        ap[u, v] = 1.0
        got = R.refocus(lf, [d], aperture=ap, interp="nearest")[0]
        oy, ox = int(np.floor(d * (u - 2) + 0.5)), int(np.floor(d * (v - 2) + 0.5))
        ys = torch.arange(H, device=DEV).add(oy).clamp(0, H - 1)
        xs = torch.arange(W, device=DEV).add(ox).clamp(0, W - 1)
        assert torch.equal(got, lf[u, v][ys][:, xs]), (u, v, d)


def _net(A, s, seed):
    from lft_amd.params import deterministic_state
    from model import LFT
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, s, seed=seed).items()})
    return net.to(DEV).eval()


def test_pipeline_from_the_network(golden_dir):
    A, s = 3, 2
    slopes = [-1.0, 0.0, 0.6]
    net = _net(A, s, seed=13)
    lf = np.load(os.path.join(golden_dir, "colour_tiny.npz"))["lf"]                        # [5, 5, 3, 2, 3] uint8: its centre 3 x 3 views
    sr = colour.super_resolve_lf(net, lf, patch=4, stride=2)
    assert sr.dtype == torch.uint8 and tuple(sr.shape) == (A, A, s * lf.shape[2], s * lf.shape[3], 3)
    table = R.shift_table(A, slopes, "full", "cubic")
    got = R.refocus(sr, slopes, out_dtype=torch.float32)
    ref = U.refocus_np(sr.cpu().numpy(), table, 4)
    assert float(np.abs(got.cpu().numpy() - ref).max()) <= U.tol(A, table, 4, 1.0)
    assert R.refocus(sr, slopes).dtype == torch.uint8
    # the network's output mosaic [B, 1, A*s*h, A*s*w], as it comes: no copy in between
    lr = torch.from_numpy(np.random.default_rng(14).random((2, 1, A * 6, A * 5)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        y = net(lr)
    assert tuple(y.shape) == (2, 1, A * s * 6, A * s * 5)
    stack = R.refocus(y, slopes, angRes=A)
    assert tuple(stack.shape) == (2, 3, s * 6, s * 5) and stack.dtype == torch.float32
    yv = y.cpu().numpy().reshape(2, A, s * 6, A, s * 5).transpose(0, 1, 3, 2, 4)
    for b in range(2):
        ref = U.refocus_np(yv[b][..., None], table, 4)[..., 0]
        assert float(np.abs(stack[b].cpu().numpy() - ref).max()) <= U.tol(A, table, 4, float(np.abs(yv[b]).max()))


def test_capture_and_replay():
    from lft_amd import train as T
    A, slopes = 3, [-0.5, 1.25]
    lf = torch.from_numpy(views(A, 33, 40, 3, np.uint8, 15)).to(DEV)
    want = R.refocus(lf, slopes)                                     # eager; the table is on the device from here on
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side, capture_error_mode=T.CAPTURE_MODE):
            got = R.refocus(lf, slopes)
        got.fill_(9)
        graph.replay()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(got, want)


def test_tool_writes_focal_stack_and_epis(golden_dir, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import refocus as tool
    from lft_amd import png, prepare, trainer
    A, s = 3, 2
    mat = os.path.join(golden_dir, "prepare_lf_v73.mat")
    lf = prepare.to_device(prepare.load_lf(mat), A, DEV)             # [3, 3, 9, 7, 3] uint8 in the file's reversed memory order
    assert not lf.is_contiguous()
    slopes = [-1.0, 0.0, 1.0]
    # the raw views
    out_dir = str(tmp_path / "raw")
    paths = tool.main(["--lf", mat, "--angRes", str(A), "--out_dir", out_dir, "--slopes=-1:1:3", "--epi_row", "2", "--epi_zoom", "2"])
    names = ["focus_00_-1.000.png", "focus_01_+0.000.png", "focus_02_+1.000.png", "epi_h_2.png", "epi_v_3.png"]
    assert [os.path.basename(p) for p in paths] == names and sorted(os.listdir(out_dir)) == sorted(names)
    want = R.refocus(lf, slopes).cpu().numpy()
    for k in range(3):
        assert np.array_equal(png.read_png(paths[k]), want[k])
    v = lf.cpu().numpy()
    assert np.array_equal(png.read_png(paths[1]), U.quantise(U.refocus_np(v, R.shift_table(A, [0.0]), 4)[0]))    # slope 0: the mean view
    assert np.array_equal(png.read_png(paths[3]), np.repeat(v[1, :, 2], 2, axis=0))
    assert np.array_equal(png.read_png(paths[4]), np.repeat(v[:, 1, :, 3], 2, axis=0))
    # super-resolved and bicubic views: slopes in HR pixels
    net = _net(A, s, seed=12)
    ckpt = str(tmp_path / "net.pth.tar")
    trainer.save_checkpoint(net, ckpt, 1)
    out_dir = str(tmp_path / "sr")
    paths = tool.main(["--lf", mat, "--angRes", str(A), "--out_dir", out_dir, "--slopes=-1,0,1", "--interp", "linear", "--aperture", "disk",
                       "--path_pre_pth", ckpt, "--scale_factor", str(s), "--bicubic", "--patch_size_for_test", "8", "--stride_for_test", "4"])
    assert len(paths) == 10 and sorted(os.listdir(out_dir)) == sorted(os.path.basename(p) for p in paths)
    sr = colour.super_resolve_lf(net, lf, patch=8, stride=4)
    base = colour.bicubic_lf(lf, A, s)
    for prefix, field in (("", sr), ("bicubic_", base)):
        want = R.refocus(field, slopes, aperture="disk", interp="linear").cpu().numpy()
        for k, d in enumerate(slopes):
            assert np.array_equal(png.read_png(os.path.join(out_dir, f"{prefix}focus_{k:02d}_{d:+.3f}.png")), want[k])
        e = png.read_png(os.path.join(out_dir, f"{prefix}epi_h_{field.shape[2] // 2}.png"))
        assert np.array_equal(e, np.repeat(field[A // 2, :, field.shape[2] // 2].cpu().numpy(), 8, axis=0))
