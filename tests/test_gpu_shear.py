"""GPU tests of per-patch disparity compensation by integer shear (lft_scene_divide_shear, lft_scene_integrate_shear,
lft_shear_vote; lft_amd/scene.py has the definition) against the integer restatement of tests/shear_util.py: every comparison is
bit for bit."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import disparity as Dm, scene as S
from lft_amd.params import deterministic_state

import shear_util as SU

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# A, patch, stride, h0, w0, s; the last is a scene of exactly one patch per side
SHAPES = [(5, 16, 4, 13, 21, 2), (3, 8, 4, 9, 11, 4), (2, 8, 4, 7, 9, 2), (1, 8, 4, 9, 9, 2), (4, 12, 4, 10, 17, 2), (3, 8, 4, 4, 4, 2)]
DEEP = (3, 16, 4, 5, 6, 2)      # the border is deeper than the view: the sheared cut folds past one reflection (the plain pair is not defined there)


def gpu(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def case(A, patch, stride, h0, w0, s, seed):
    """(rng, scene, N, k): k random in [-kmax-1, kmax+1] per patch, so both clamps and fold past one reflection are exercised."""
    rng = np.random.default_rng([seed, A, h0, w0])
    scene = rng.random((A * h0, A * w0), dtype=np.float32)
    N = int(np.prod(SU.counts_np(h0, w0, patch, stride)))
    kmax = SU.kmax_np(A, patch, stride)
    k = rng.integers(-kmax - 1, kmax + 2, N).astype(np.int32)
    if N >= 2:
        k[0], k[-1] = -kmax - 1, kmax + 1
    return rng, scene, N, k


@pytest.mark.parametrize("A,patch,stride,h0,w0,s", SHAPES + [DEEP])
def test_divide_and_integrate_equal_the_restatement(A, patch, stride, h0, w0, s):
    rng, scene, N, k = case(A, patch, stride, h0, w0, s, 21)
    assert S.scene_counts(h0, w0, patch, stride) == SU.counts_np(h0, w0, patch, stride)
    got = S.divide(gpu(scene), A, patch, stride, shear=gpu(k)).cpu().numpy()
    assert got.shape == (N, 1, A * patch, A * patch)
    assert np.array_equal(got[:, 0], SU.divide_np(scene, A, patch, stride, k))
    sr = rng.random((N, 1, A * patch * s, A * patch * s), dtype=np.float32)
    back = S.integrate(gpu(sr), A, h0, w0, s, patch, stride, shear=gpu(k)).cpu().numpy()
    assert np.array_equal(back, SU.integrate_np(sr[:, 0], A, h0, w0, patch, stride, s, k))


@pytest.mark.parametrize("A,patch,stride,h0,w0,s", SHAPES)
def test_zero_shear_is_the_plain_pair(A, patch, stride, h0, w0, s):
    rng, scene, N, _ = case(A, patch, stride, h0, w0, s, 22)
    zero = torch.zeros(N, dtype=torch.int32, device=DEV)
    assert torch.equal(S.divide(gpu(scene), A, patch, stride, shear=zero), S.divide(gpu(scene), A, patch, stride))
    sr = gpu(rng.random((N, 1, A * patch * s, A * patch * s), dtype=np.float32))
    assert torch.equal(S.integrate(sr, A, h0, w0, s, patch, stride, shear=zero), S.integrate(sr, A, h0, w0, s, patch, stride))


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("A,patch,stride,h0,w0,_", SHAPES + [DEEP])
def test_round_trip_through_pixel_replication(A, patch, stride, h0, w0, _, s):
    _, scene, N, k = case(A, patch, stride, h0, w0, s, 23)
    cut = S.divide(gpu(scene), A, patch, stride, shear=gpu(k))
    rep = cut.repeat_interleave(s, dim=-2).repeat_interleave(s, dim=-1)
    back = S.integrate(rep, A, h0, w0, s, patch, stride, shear=gpu(k)).cpu().numpy()
    assert np.array_equal(back, SU.replicate(scene, s))


@pytest.mark.parametrize("d", [-2, 3])
@pytest.mark.parametrize("A,patch,stride,h0,w0", [(5, 16, 4, 13, 21), (3, 16, 8, 24, 40), (2, 16, 8, 17, 16)])
def test_the_true_shear_aligns_the_views(A, patch, stride, h0, w0, d):
    """Views that are whole-pixel translations of one image by d per view step, cut with k = d: in every patch every view equals
    the view (u0, u0) bit for bit at the pixels whose reads stayed inside the scene."""
    assert SU.kmax_np(A, patch, stride) >= abs(d)
    scene = SU.translated_scene(A, h0, w0, d)
    N = int(np.prod(SU.counts_np(h0, w0, patch, stride)))
    k = np.full(N, d, dtype=np.int32)
    views = SU.patch_views(S.divide(gpu(scene), A, patch, stride, shear=gpu(k)).cpu().numpy()[:, 0], A)[..., 0]
    ok = SU.patch_views(SU.inside_np(A, h0, w0, patch, stride, k), A)[..., 0]
    centre = np.broadcast_to(views[:, A // 2, A // 2][:, None, None], views.shape)
    assert ok.reshape(N, -1).any(1).all()
    assert np.array_equal(views[ok], centre[ok])


def test_estimate_shear_on_the_two_plane_scene():
    T = SU.TWO_PLANES
    A, patch, stride = T["A"], T["patch"], T["stride"]
    K, bdr = SU.kmax_np(A, patch, stride), (patch - stride) // 2
    scene = gpu(SU.two_plane_scene(**T))
    patches = S.divide(scene, A, patch, stride)
    got = S.estimate_shear(patches, A, stride=stride)
    assert got.dtype == torch.int32 and got.shape == (patches.shape[0],) and got.device == patches.device
    # the numpy vote over the GPU's own maps, exactly
    res = Dm.disparity(patches, [float(k) for k in range(-K, K + 1)], angRes=A, interp="nearest", radius=2, centre=(A // 2, A // 2))
    slopes = torch.arange(-K, K + 1, dtype=torch.int32, device=DEV)
    shear, counts = S.vote(res.index, res.confidence, slopes, bdr, 0.5)
    want_shear, want_counts = SU.vote_np(res.index.cpu().numpy(), res.confidence.cpu().numpy(), np.arange(-K, K + 1), bdr, 0.5)
    assert np.array_equal(counts.cpu().numpy(), want_counts) and np.array_equal(shear.cpu().numpy(), want_shear)
    assert torch.equal(got, shear)
    # every one-plane patch gets its plane's slope
    want = SU.one_plane_patches(**T)
    assert len(want) == 12
    for n, d in want.items():
        assert int(got[n]) == d, (n, got.tolist())
    # the vote's other rules on maps made for them: another margin and threshold, ties, wild indices, confidences that are not finite
    rng = np.random.default_rng(7)
    index = rng.integers(-2, 7, (6, 11, 12)).astype(np.int32)
    conf = rng.random((6, 11, 12)).astype(np.float32)
    conf[rng.random(conf.shape) < 0.1] = np.nan
    conf[rng.random(conf.shape) < 0.05] = np.inf
    index[4], index[5, :, :6], index[5, :, 6:] = 3, 0, 4                        # one slope only; an exact tie of -2 and 2 under every margin
    conf[5] = 1.0
    sl = np.array([-2, -1, 0, 1, 2], dtype=np.int32)
    for margin, thr in ((0, 0.5), (1, 0.0), (3, 0.9), (5, 2.0)):
        sh, ct = S.vote(gpu(index), gpu(conf), gpu(sl), margin, thr)
        ws, wc = SU.vote_np(index, conf, sl, margin, thr)
        assert np.array_equal(ct.cpu().numpy(), wc) and np.array_equal(sh.cpu().numpy(), ws), (margin, thr)
    assert ws.tolist() == [0] * 6 and SU.vote_np(index, conf, sl, 1, 0.0)[0][5] == -2
    # a constant scene: every confidence is 0, every count is 0, so the result is 0
    flat = S.divide(torch.full_like(scene, 0.25), A, patch, stride)
    assert not S.estimate_shear(flat, A, stride=stride).any()


def test_whole_scene_with_shear():
    """fp32, random weights: super_resolve_scene(shear=k) is the same network on the same input bits as the restatement's cut, put
    back by the restatement."""
    from model import LFT
    A, s, patch, stride, h0, w0 = 3, 2, 16, 8, 24, 24
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s), precision="fp32")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, s, seed=1, flavor="stress").items()})
    net = net.to(DEV).eval()
    _, scene, N, k = case(A, patch, stride, h0, w0, s, 26)
    with torch.no_grad():
        got = S.super_resolve_scene(net, gpu(scene), patch, stride, shear=gpu(k))
        out = net(gpu(SU.divide_np(scene, A, patch, stride, k)[:, None]))
    want = SU.integrate_np(out.cpu().numpy()[:, 0], A, h0, w0, patch, stride, s, k)
    assert got.shape == (A * h0 * s, A * w0 * s) and np.array_equal(got.cpu().numpy(), want)
    plain = S.super_resolve_scene(net, gpu(scene), patch, stride)
    assert torch.equal(S.super_resolve_scene(net, gpu(scene), patch, stride, shear=0), plain)
    assert not torch.equal(got, plain)
    one = S.super_resolve_scene(net, gpu(scene), patch, stride, shear=-2)
    assert torch.equal(one, S.super_resolve_scene(net, gpu(scene), patch, stride, shear=torch.full((N,), -2, dtype=torch.int32, device=DEV)))
    # auto is estimate_shear on the unsheared patches; on a scene with parallax it finds a shear
    lf = gpu(SU.translated_scene(A, h0, w0, 2, seed=4))
    est = S.estimate_shear(S.divide(lf, A, patch, stride), A, stride=stride)
    assert (est == 2).all()
    assert torch.equal(S.super_resolve_scene(net, lf, patch, stride, shear="auto"), S.super_resolve_scene(net, lf, patch, stride, shear=est))


def test_shear_sets_tool_over_an_h5_tree(tmp_path):
    """tools/shear_sets.py end to end on a test tree of the h5py-written fixture: its figures are evaluate.test_scene's with the
    same shear, --shear none gives the plain figures, and a shear moves them."""
    import os
    import shutil
    import sys
    from lft_amd import evaluate
    from model import LFT as MODEL
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import shear_sets
    h5 = os.path.join(root, "tests", "golden", "h5")
    os.makedirs(tmp_path / "data_for_test" / "SR_2x2_2x" / "SetA")
    shutil.copy(os.path.join(h5, "scene_a2_2x.h5"), tmp_path / "data_for_test" / "SR_2x2_2x" / "SetA" / "s1.h5")
    exp = np.load(os.path.join(h5, "expected.npz"))
    lr, hr = (torch.from_numpy(exp["scene_a2_2x.h5:" + name].T.copy()) for name in ("Lr_SAI_y", "Hr_SAI_y"))
    argv = ["--angRes", "2", "--scale_factor", "2", "--path_for_test", str(tmp_path / "data_for_test") + "/"]
    args = SimpleNamespace(angRes=2, scale_factor=2, channels=64)
    got = {}
    for shear in ("none", "3", "auto"):
        torch.manual_seed(0)
        got[shear] = shear_sets.main(argv + ["--shear", shear])["SetA"]
        torch.manual_seed(0)
        net = MODEL.get_model(args).to(DEV)
        net.apply(MODEL.weights_init)
        p, s, _ = evaluate.test_scene(net, lr, hr, shear={"none": None, "3": 3, "auto": "auto"}[shear])
        assert abs(got[shear][0] - p) < 1e-4 and abs(got[shear][1] - s) < 1e-6, (shear, got[shear], p, s)
    assert got["3"] != got["none"]
