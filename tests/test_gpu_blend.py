"""GPU tests of windowed blending of overlapping SR patches (lft_scene_integrate_blend; lft_amd/scene.py has the definition)
against the float32 restatement of tests/blend_util.py.

Shapes: A = 2 and 3, s = 2 and 4, LR views of 9 x 14, (patch, stride) from (8, 4), (8, 6), (8, 8), with and without a random int32
shear: the smallest with more than one patch per axis, an overhanging last patch, a non-integer pz/S, and a single-term pixel.
Parity is bit for bit; the quotient is __fdiv_rn, and no 1-ulp gate was needed."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import colour, ensemble as E, png, prepare, scene as S, trainer
from lft_amd.params import deterministic_state

import blend_util as BU
import shear_util as SU

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
H0, W0 = 9, 14
CASES = [(A, s, patch, stride, sheared) for A, s in ((2, 2), (3, 4), (2, 4), (3, 2)) for patch, stride in ((8, 4), (8, 6), (8, 8)) for sheared in (False, True)]
# (8, 4), (8, 6) and (8, 8) have 3, 2 and 1 candidate patches per axis, which the kernel has written out; (8, 2) has 7 and takes its loop
LOOP = [(2, 2, 8, 2, False), (3, 2, 8, 2, True)]


def gpu(x):
    return torch.from_numpy(np.array(x)).to(DEV)         # a copy: the shared cases are read-only


def bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x).view(np.int32)


@functools.lru_cache(maxsize=None)
def case(A, s, patch, stride, sheared):
    """(sr [N, A*pz, A*pz] random, k int32 [N] or None): k random in [-kmax-1, kmax+1] per patch, so both clamps are exercised.
    Made once and shared."""
    rng = np.random.default_rng([51, A, s, patch, stride, sheared])
    N = int(np.prod(SU.counts_np(H0, W0, patch, stride)))
    assert S.scene_counts(H0, W0, patch, stride) == SU.counts_np(H0, W0, patch, stride)
    sr = rng.random((N, A * patch * s, A * patch * s), dtype=np.float32)
    kmax = SU.kmax_np(A, patch, stride)
    k = rng.integers(-kmax - 1, kmax + 2, N).astype(np.int32) if sheared else None
    if sheared:
        k[0], k[-1] = -kmax - 1, kmax + 1
    sr.setflags(write=False)
    return sr, k


def net_of(A, s, seed=1):
    from model import LFT
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s), precision="fp32")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, s, seed=seed, flavor="stress").items()})
    return net.to(DEV).eval()


# ---- 1. parity ----
@pytest.mark.parametrize("A,s,patch,stride,sheared", CASES + LOOP)
def test_blend_equals_the_restatement_bit_for_bit(A, s, patch, stride, sheared):
    sr, k = case(A, s, patch, stride, sheared)
    pz = patch * s
    custom = (np.random.default_rng([52, pz]).random(pz, dtype=np.float32) + np.float32(0.01))
    x, kk = gpu(sr[:, None]), None if k is None else gpu(k)
    for blend, w in (("hann", BU.window_np("hann", pz)), ("linear", BU.window_np("linear", pz)), ("flat", BU.window_np("flat", pz)), (gpu(custom), custom)):
        got = S.integrate(x, A, H0, W0, s, patch, stride, shear=kk, blend=blend)
        want, terms = BU.blend_np(sr, A, H0, W0, patch, stride, s, w, k)
        assert got.shape == want.shape and got.dtype == torch.float32
        diff = bits(got) != bits(want)
        assert not diff.any(), (blend if isinstance(blend, str) else "custom", int(diff.sum()), int(terms.max()))
    assert np.array_equal(S.blend_window("hann", pz, DEV).cpu().numpy(), BU.window_np("hann", pz))
    assert S.blend_window("hann", pz, DEV) is S.blend_window("hann", pz, torch.device(DEV))       # made once per device and kept


# ---- 2. reproduction ----
@pytest.mark.parametrize("A,s,patch,stride,sheared", CASES + LOOP)
def test_a_perfect_networks_patches_blend_back_to_the_scene(A, s, patch, stride, sheared):
    _, k = case(A, s, patch, stride, sheared)
    rng = np.random.default_rng([53, A, s, patch, stride, sheared])
    G = rng.random((A * H0 * s, A * W0 * s), dtype=np.float32)
    kmax = SU.kmax_np(A, patch, stride)
    sk = None if k is None else gpu((s * np.clip(k, -kmax, kmax)).astype(np.int32))       # the cut at SR size, with s*k
    cut = S.divide(gpu(G), A, patch * s, stride * s, shear=sk)
    assert np.array_equal(cut.cpu().numpy()[:, 0], BU.cut_np(G, A, patch, stride, s, k))
    T = (-(-patch // stride)) ** 2 if k is None else int(BU.blend_np(cut.cpu().numpy()[:, 0], A, H0, W0, patch, stride, s, BU.window_np("flat", patch * s), k)[1].max())
    bound = (T + 2) * BU.EPS * float(np.abs(G).max())
    for kind in BU.WINDOWS:
        got = S.integrate(cut, A, H0, W0, s, patch, stride, shear=None if k is None else gpu(k), blend=kind).cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - G).max())
        print(f"{kind}: T = {T}, error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (kind, T, err, bound)


# ---- 3. seams: fails without the blend, and the crop fails its bound ----
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_no_seams_where_the_crop_has_them(seed):
    A, s, h0, w0, patch, stride = (BU.SEAM[k] for k in ("A", "s", "h0", "w0", "patch", "stride"))
    G, patches, c = BU.seam_case(seed)
    on_gpu = S.divide(gpu(G), A, patch * s, stride * s) + gpu(c)[:, None, None, None]     # cut and biased on the device: the same bits
    assert np.array_equal(on_gpu.cpu().numpy()[:, 0], patches)
    out = S.integrate(on_gpu, A, h0, w0, s, patch, stride, blend="hann").cpu().numpy()
    worst, bound = BU.seam_excess(out, G, c, patches)
    crop, _ = BU.seam_excess(S.integrate(on_gpu, A, h0, w0, s, patch, stride).cpu().numpy(), G, c, patches)
    print(f"seed {seed}: blend {worst:.4f}, crop {crop:.4f}, bound {bound:.4f}")
    assert worst <= bound
    assert crop > bound                                 # the same patches through the crop jump by |c_n - c_m| at region borders


# ---- 4. equalities ----
@pytest.mark.parametrize("A,s,patch,stride,sheared", [c for c in CASES if c[:2] in ((2, 2), (3, 4))])
def test_blend_none_is_todays_integrate(A, s, patch, stride, sheared):
    sr, k = case(A, s, patch, stride, sheared)
    x = gpu(sr[:, None])
    if k is None:
        want = SU.integrate_plain_np(sr, A, H0, W0, patch, stride, s)
        got = S.integrate(x, A, H0, W0, s, patch, stride, blend=None)
    else:
        want = SU.integrate_np(sr, A, H0, W0, patch, stride, s, k)
        got = S.integrate(x, A, H0, W0, s, patch, stride, shear=gpu(k), blend=None)
    assert np.array_equal(bits(got), bits(want))
    if stride == patch:                                  # one term per pixel under a flat window: (1*x)/1, the crop's bits
        assert torch.equal(S.integrate(x, A, H0, W0, s, patch, stride, shear=None if k is None else gpu(k), blend="flat"), got)


def test_layouts_give_identical_bits():
    from lft_amd import train as T
    A, s, patch, stride = 3, 2, 8, 4
    sr, k = case(A, s, patch, stride, True)
    x, kk = gpu(sr[:, None]), gpu(k)
    w = gpu(np.random.default_rng(54).random(patch * s, dtype=np.float32) + np.float32(0.5))
    run = lambda x_, w_: S.integrate(x_, A, H0, W0, s, patch, stride, shear=kk, blend=w_)
    want = run(x, w)                                    # eager
    # non-contiguous patches and window
    wide = torch.zeros(x.shape[0], 2, x.shape[2], x.shape[3] + 3, device=DEV)
    wide[:, 1:2, :, 3:] = x
    w2 = torch.zeros(2 * patch * s, device=DEV)
    w2[::2] = w
    assert not wide[:, 1:2, :, 3:].is_contiguous() and not w2[::2].is_contiguous()
    assert torch.equal(run(wide[:, 1:2, :, 3:], w2[::2]), want)
    assert torch.equal(run(x.transpose(2, 3).contiguous().transpose(2, 3), w), want)
    # captured and replayed
    want_hann = S.integrate(x, A, H0, W0, s, patch, stride, shear=kk, blend="hann")       # the table is on the device from here on
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side, capture_error_mode=T.CAPTURE_MODE):
            got = run(x, w)
            got_hann = S.integrate(x, A, H0, W0, s, patch, stride, shear=kk, blend="hann")
        got.fill_(9)
        got_hann.fill_(9)
        graph.replay()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(got, want) and torch.equal(got_hann, want_hann)


def test_whole_scene_with_blend():
    """fp32, random weights: super_resolve_scene(blend=) is the same network on the same patches, put together by the blended
    integrate -- plain, with a shear, and with the ensemble through lft_amd.ensemble.merge."""
    A, s, patch, stride, h0, w0 = 2, 2, 8, 4, 13, 18
    net = net_of(A, s)
    rng = np.random.default_rng(55)
    scene = gpu(rng.random((A * h0, A * w0), dtype=np.float32))
    N = int(np.prod(S.scene_counts(h0, w0, patch, stride)))
    k = gpu(rng.integers(-2, 3, N).astype(np.int32))
    with torch.no_grad():
        crop = S.super_resolve_scene(net, scene, patch, stride)
        out = net(S.divide(scene, A, patch, stride))
        assert torch.equal(crop, S.integrate(out, A, h0, w0, s, patch, stride))
        assert torch.equal(S.super_resolve_scene(net, scene, patch, stride, blend=None), crop)
        got = S.super_resolve_scene(net, scene, patch, stride, blend="hann")
        assert torch.equal(got, S.integrate(out, A, h0, w0, s, patch, stride, blend="hann")) and not torch.equal(got, crop)
        assert np.array_equal(bits(got), bits(BU.blend_np(out.cpu().numpy()[:, 0], A, h0, w0, patch, stride, s, BU.window_np("hann", patch * s))[0]))
        # with a shear
        outk = net(S.divide(scene, A, patch, stride, shear=k))
        assert torch.equal(S.super_resolve_scene(net, scene, patch, stride, shear=k, blend="linear"),
                           S.integrate(outk, A, h0, w0, s, patch, stride, shear=k, blend="linear"))
        # with the ensemble: merge, then the blended integrate
        mask = E.mask_of("flips")
        variants = net(E.expand(S.divide(scene, A, patch, stride), mask))
        want = S.integrate(E.merge(variants, mask), A, h0, w0, s, patch, stride, blend="hann")
        assert torch.equal(S.super_resolve_scene(net, scene, patch, stride, blend="hann", ensemble="flips"), want)
        assert torch.equal(S.super_resolve_scene(net, scene, patch, stride, max_batch=8, blend="hann", ensemble="flips"), want)


# ---- 5. the tool ----
def test_tool_writes_the_blended_views(golden_dir, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import super_resolve
    A, s = 3, 2
    net = net_of(A, s, seed=12)
    ckpt = str(tmp_path / "net.pth.tar")
    trainer.save_checkpoint(net, ckpt, 1)
    mat = os.path.join(golden_dir, "prepare_lf_v73.mat")
    out_dir = str(tmp_path / "png")
    paths = super_resolve.main(["--angRes", str(A), "--scale_factor", str(s), "--path_pre_pth", ckpt, "--lf", mat, "--out_dir", out_dir,
                                "--patch_size_for_test", "8", "--stride_for_test", "4", "--blend", "hann"])
    lf = prepare.load_lf(mat)
    want = colour.super_resolve_lf(net, lf, patch=8, stride=4, blend="hann")
    assert sorted(os.listdir(out_dir)) == sorted(os.path.basename(p) for p in paths) and len(paths) == A * A
    for u in range(A):
        for v in range(A):
            assert np.array_equal(png.read_png(os.path.join(out_dir, f"view_{u}_{v}.png")), want[u, v].cpu().numpy())
    # the blend is in the picture: the unquantised views differ from the crop's
    f32 = lambda **kw: colour.super_resolve_lf(net, lf, patch=8, stride=4, out_dtype=torch.float32, **kw)
    assert not torch.equal(f32(blend="hann"), f32())
