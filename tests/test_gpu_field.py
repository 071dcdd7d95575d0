"""GPU tests of angular tiling (lft_field_divide, lft_field_integrate; lft_amd/field.py has the definition) against the float32
restatement of tests/field_util.py.

Shapes: LR views of 9 x 14, (patch, stride) from (8, 4), (8, 6), (8, 8), s = 2 and 4, with and without a random int32 shear in
[-kmax-1, kmax+1] per batch element.  Angular cases (U, V, A, astride): (4, 5, 2, 1); (5, 3, 3, 2), one window along v; (4, 4, 3, 2),
the clamped origin 1; (5, 5, 2, 2), the extra-multiplicity view; (3, 3, 3, 3), a single window -- the smallest with an overhanging
patch, a clamped window, views in one and in several windows, and U != V.  All of these have at most 2 windows per axis, which the
kernel has written out for the crop; LOOP holds a view in 3 windows per axis ((5, 4, 3, 1)), where the crop takes the kernel's loop
as every blend does, and 7 spatial candidates per axis ((8, 2)).  Both forms are compared bit for bit with the one restatement, so
they agree with each other.  Parity is bit for bit; the quotient is __fdiv_rn."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import colour, ensemble as E, field as F, png, prepare, scene as S, trainer
from lft_amd.params import deterministic_state

import blend_util as BU
import field_util as FU
import shear_util as SU

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
H0, W0 = 9, 14
ANGULAR = [(4, 5, 2, 1), (5, 3, 3, 2), (4, 4, 3, 2), (5, 5, 2, 2), (3, 3, 3, 3)]
CASES = [(*ang, s, patch, stride, sheared) for ang in ANGULAR for s in (2, 4) for patch, stride in ((8, 4), (8, 6), (8, 8)) for sheared in (False, True)]
LOOP = [(5, 4, 3, 1, 2, 8, 4, True), (5, 4, 3, 1, 2, 8, 8, False), (4, 5, 2, 1, 2, 8, 2, True), (5, 4, 3, 1, 2, 8, 2, False)]
SPATIAL = (None, "hann", "linear", "flat", "random")
ANGLES = ("flat", "linear", "random")


def gpu(x):
    return torch.from_numpy(np.array(x)).to(DEV)         # a copy: the shared cases are read-only


def bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x).view(np.int32)


@functools.lru_cache(maxsize=None)
def case(U, V, A, astride, s, patch, stride, sheared):
    """(field [U*h0, V*w0], sr [B, A*pz, A*pz], k int32 [B] or None), random; k in [-kmax-1, kmax+1] per batch element, so both
    clamps are exercised.  Made once and shared."""
    rng = np.random.default_rng([71, U, V, A, astride, s, patch, stride, sheared])
    N = int(np.prod(SU.counts_np(H0, W0, patch, stride)))
    mu, mv = len(FU.origins_np(U, A, astride)), len(FU.origins_np(V, A, astride))
    assert F.counts(U, V, A, astride) == (mu, mv) and S.scene_counts(H0, W0, patch, stride) == SU.counts_np(H0, W0, patch, stride)
    B = mu * mv * N
    field = rng.random((U * H0, V * W0), dtype=np.float32)
    sr = rng.random((B, A * patch * s, A * patch * s), dtype=np.float32)
    k = None
    if sheared:
        kmax = SU.kmax_np(A, patch, stride)
        k = rng.integers(-kmax - 1, kmax + 2, B).astype(np.int32)
        k[0], k[-1] = -kmax - 1, kmax + 1
    field.setflags(write=False)
    sr.setflags(write=False)
    return field, sr, k


def table(kind, n, seed):
    """A spatial ([pz]) or angular ([A]) table: a window's name, or random positive weights."""
    if kind == "random":
        return np.random.default_rng([72, n, seed]).random(n, dtype=np.float32) + np.float32(0.01)
    return BU.window_np(kind, n)


@functools.lru_cache(maxsize=None)
def restated(key, spatial, angular):
    """(the restatement's SR field, T) of a case; computed once and shared among the tests."""
    U, V, A, astride, s, patch, stride, _ = key
    _, sr, k = case(*key)
    win = None if spatial is None else table(spatial, patch * s, 0)
    out, T = FU.integrate_np(sr, U, V, A, astride, H0, W0, patch, stride, s, table(angular, A, 1), win, k)
    out.setflags(write=False)
    T.setflags(write=False)
    return out, T


def on_gpu(kind, n, seed):
    return kind if kind is None or kind != "random" else gpu(table(kind, n, seed))


def net_of(A, s, seed=1):
    from model import LFT
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s), precision="fp32")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, s, seed=seed, flavor="stress").items()})
    return net.to(DEV).eval()


# ---- 1. divide ----
@pytest.mark.parametrize("U,V,A,astride,s,patch,stride,sheared", [c for c in CASES + LOOP if c[4] == 2])      # s plays no part in the LR cut
def test_divide_equals_the_restatement_and_the_per_window_divide(U, V, A, astride, s, patch, stride, sheared):
    field, _, k = case(U, V, A, astride, s, patch, stride, sheared)
    x, kk = gpu(field), None if k is None else gpu(k)
    got = F.divide(x, U, V, A, patch, stride, astride, shear=kk)
    want = FU.divide_np(field, U, V, A, astride, patch, stride, k)
    assert got.shape == (want.shape[0], 1, A * patch, A * patch) and got.dtype == torch.float32
    assert np.array_equal(bits(got[:, 0]), bits(want))
    # scene.divide of each window's sub-mosaic, built by indexing on the device
    N = int(np.prod(SU.counts_np(H0, W0, patch, stride)))
    views = x.reshape(U, H0, V, W0)
    for w, o_u, o_v in FU.windows_np(U, V, A, astride):
        sub = views[o_u:o_u + A, :, o_v:o_v + A, :].reshape(A * H0, A * W0).contiguous()
        assert torch.equal(got[w * N:(w + 1) * N], S.divide(sub, A, patch, stride, shear=None if kk is None else kk[w * N:(w + 1) * N].contiguous())), w


# ---- 2. integrate ----
@pytest.mark.parametrize("U,V,A,astride,s,patch,stride,sheared", CASES + LOOP)
def test_integrate_equals_the_restatement_bit_for_bit(U, V, A, astride, s, patch, stride, sheared):
    key = (U, V, A, astride, s, patch, stride, sheared)
    _, sr, k = case(*key)
    x, kk = gpu(sr[:, None]), None if k is None else gpu(k)
    for spatial in SPATIAL:
        for angular in ANGLES:
            got = F.integrate(x, U, V, A, H0, W0, s, patch, stride, astride, shear=kk, blend=on_gpu(spatial, patch * s, 0), angular=on_gpu(angular, A, 1))
            want, T = restated(key, spatial, angular)
            assert got.shape == want.shape and got.dtype == torch.float32
            diff = bits(got) != bits(want)
            assert not diff.any(), (spatial, angular, int(diff.sum()), int(T.max()))
    assert F.angular_table("linear", A, DEV) is F.angular_table("linear", A, torch.device(DEV))      # made once per device and kept
    assert np.array_equal(F.angular_table("hann", A, DEV).cpu().numpy(), BU.window_np("hann", A))


def test_the_cases_fall_on_both_sides_of_the_unroll_limit():
    mult = lambda c: max(max(sum(1 for o in FU.origins_np(L, c[2], c[3]) if o <= p < o + c[2]) for p in range(L)) for L in c[:2])
    nc = lambda c: (2 * c[5] + c[6] - 1) // c[6] - 1
    # the crop: the windows written out up to 2 per axis, the loop beyond; every blend loops, over 1, 2, 3 and 7 candidates per axis
    assert {mult(c) for c in CASES} == {1, 2} and {nc(c) for c in CASES} == {1, 2, 3}
    assert {mult(c) for c in LOOP} == {2, 3} and {nc(c) for c in LOOP} == {1, 3, 7}
    assert FU.origins_np(5, 3, 1) == [0, 1, 2] and FU.origins_np(5, 2, 2) == [0, 2, 3] and FU.origins_np(4, 3, 2) == [0, 1]


# ---- 3. the consequences ----
@pytest.mark.parametrize("A,s,patch,stride", [(A, s, patch, stride) for A in (2, 3) for s in (2, 4) for patch, stride in ((8, 4), (8, 6), (8, 8))])
def test_one_window_with_a_flat_table_is_the_scene_integrate(A, s, patch, stride):
    for sheared in (False, True):
        _, sr, k = case(A, A, A, A, s, patch, stride, sheared)
        x, kk = gpu(sr[:, None]), None if k is None else gpu(k)
        assert torch.equal(F.integrate(x, A, A, A, H0, W0, s, patch, stride, shear=kk), S.integrate(x, A, H0, W0, s, patch, stride, shear=kk))
        for blend in ("hann", "linear", "flat"):
            assert torch.equal(F.integrate(x, A, A, A, H0, W0, s, patch, stride, shear=kk, blend=blend),
                               S.integrate(x, A, H0, W0, s, patch, stride, shear=kk, blend=blend)), blend


@pytest.mark.parametrize("U,V,A,astride,s,patch,stride,sheared", CASES + LOOP)
def test_flat_crop_is_the_mean_of_the_per_window_integrates(U, V, A, astride, s, patch, stride, sheared):
    _, sr, k = case(U, V, A, astride, s, patch, stride, sheared)
    x, kk = gpu(sr[:, None]), None if k is None else gpu(k)
    N = int(np.prod(SU.counts_np(H0, W0, patch, stride)))
    H, W = H0 * s, W0 * s
    acc, cnt = np.zeros((U, H, V, W), np.float32), np.zeros((U, H, V, W), np.float32)
    for w, o_u, o_v in FU.windows_np(U, V, A, astride):                 # window order; today's kernels per window
        r = S.integrate(x[w * N:(w + 1) * N], A, H0, W0, s, patch, stride, shear=None if kk is None else kk[w * N:(w + 1) * N].contiguous())
        acc[o_u:o_u + A, :, o_v:o_v + A, :] += r.cpu().numpy().reshape(A, H, A, W)
        cnt[o_u:o_u + A, :, o_v:o_v + A, :] += np.float32(1)
    want = (acc / cnt).reshape(U * H, V * W)
    got = F.integrate(x, U, V, A, H0, W0, s, patch, stride, astride, shear=kk)
    assert np.array_equal(bits(got), bits(want))


# ---- 4. reproduction ----
@pytest.mark.parametrize("U,V,A,astride,s,patch,stride,sheared", CASES + LOOP)
def test_a_perfect_network_reproduces_the_field(U, V, A, astride, s, patch, stride, sheared):
    """|out - G| <= (2T+1) * 2^-24 * max|G|: the weight of a term is one value used in both sums and cancels; num carries T roundings
    of products and T-1 of sums beyond what den carries, and the quotient adds one."""
    key = (U, V, A, astride, s, patch, stride, sheared)
    _, _, k = case(*key)
    rng = np.random.default_rng([73, *key])
    G = rng.random((U * H0 * s, V * W0 * s), dtype=np.float32)
    kmax = SU.kmax_np(A, patch, stride)
    sk = None if k is None else gpu((s * np.clip(k, -kmax, kmax)).astype(np.int32))       # the cut at SR size, with s*k
    cut = F.divide(gpu(G), U, V, A, patch * s, stride * s, astride, shear=sk)
    kk = None if k is None else gpu(k)
    for spatial in (None, "hann", "flat"):
        T = int(restated(key, spatial, "flat")[1].max())
        bound = (2 * T + 1) * FU.EPS * float(np.abs(G).max())
        for angular in ("flat", "hann", "random"):
            got = F.integrate(cut, U, V, A, H0, W0, s, patch, stride, astride, shear=kk, blend=spatial, angular=on_gpu(angular, A, 1)).cpu().numpy()
            err = float(np.abs(got.astype(np.float64) - G).max())
            print(f"{spatial} / {angular}: T = {T}, error {err:.3e}, bound {bound:.3e}")
            assert err <= bound, (spatial, angular, T, err, bound)


# ---- 5. layouts ----
def test_layouts_give_identical_bits():
    from lft_amd import train as T
    U, V, A, astride, s, patch, stride = 4, 5, 2, 1, 2, 8, 4
    _, sr, k = case(U, V, A, astride, s, patch, stride, True)
    x, kk = gpu(sr[:, None]), gpu(k)
    w = gpu(table("random", patch * s, 2))
    g = gpu(table("random", A, 3))
    run = lambda x_, w_, g_: F.integrate(x_, U, V, A, H0, W0, s, patch, stride, astride, shear=kk, blend=w_, angular=g_)
    want = run(x, w, g)                                 # eager
    # non-contiguous patches and tables
    wide = torch.zeros(x.shape[0], 2, x.shape[2], x.shape[3] + 3, device=DEV)
    wide[:, 1:2, :, 3:] = x
    w2, g2 = torch.zeros(2 * patch * s, device=DEV), torch.zeros(3 * A, device=DEV)
    w2[::2], g2[::3] = w, g
    assert not wide[:, 1:2, :, 3:].is_contiguous() and not w2[::2].is_contiguous() and not g2[::3].is_contiguous()
    assert torch.equal(run(wide[:, 1:2, :, 3:], w2[::2], g2[::3]), want)
    assert torch.equal(run(x.transpose(2, 3).contiguous().transpose(2, 3), w, g), want)
    field = gpu(case(U, V, A, astride, s, patch, stride, True)[0])
    cut = F.divide(field, U, V, A, patch, stride, astride, shear=kk)
    assert torch.equal(F.divide(field.t().contiguous().t(), U, V, A, patch, stride, astride, shear=kk), cut)
    # captured and replayed
    want_crop = F.integrate(x, U, V, A, H0, W0, s, patch, stride, astride, shear=kk, angular="hann")      # the table is on the device from here on
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side, capture_error_mode=T.CAPTURE_MODE):
            got = run(x, w, g)
            got_crop = F.integrate(x, U, V, A, H0, W0, s, patch, stride, astride, shear=kk, angular="hann")
            got_cut = F.divide(field, U, V, A, patch, stride, astride, shear=kk)
        got.fill_(9)
        got_crop.fill_(9)
        got_cut.fill_(9)
        graph.replay()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(got, want) and torch.equal(got_crop, want_crop) and torch.equal(got_cut, cut)


# ---- 6. the whole field ----
def test_whole_field_is_divide_network_integrate():
    """fp32, random weights: super_resolve_field is the same network on the same patches, put together by the field integrate --
    plain, blended, with a shear, with the ensemble, in chunks; and with U = V = A it is super_resolve_scene."""
    A, s, patch, stride, h0, w0, U, V = 2, 2, 8, 4, 13, 18, 4, 3
    net = net_of(A, s)
    rng = np.random.default_rng(75)
    field = gpu(rng.random((U * h0, V * w0), dtype=np.float32))
    N = int(np.prod(S.scene_counts(h0, w0, patch, stride)))
    mu, mv = F.counts(U, V, A)
    assert (mu, mv) == (2, 2)
    k = gpu(rng.integers(-2, 3, mu * mv * N).astype(np.int32))
    with torch.no_grad():
        out = net(F.divide(field, U, V, A, patch, stride))
        plain = F.super_resolve_field(net, field, U, V, patch, stride)
        assert plain.shape == (U * h0 * s, V * w0 * s)
        assert torch.equal(plain, F.integrate(out, U, V, A, h0, w0, s, patch, stride))
        got = F.super_resolve_field(net, field, U, V, patch, stride, blend="hann")
        assert torch.equal(got, F.integrate(out, U, V, A, h0, w0, s, patch, stride, blend="hann")) and not torch.equal(got, plain)
        assert np.array_equal(bits(got), bits(FU.integrate_np(out.cpu().numpy()[:, 0], U, V, A, A, h0, w0, patch, stride, s, np.ones(A, np.float32),
                                                              BU.window_np("hann", patch * s))[0]))
        # overlapping windows with weights
        out1 = net(F.divide(field, U, V, A, patch, stride, astride=1))
        assert torch.equal(F.super_resolve_field(net, field, U, V, patch, stride, astride=1, angular="hann"),
                           F.integrate(out1, U, V, A, h0, w0, s, patch, stride, astride=1, angular="hann"))
        # with a shear tensor
        outk = net(F.divide(field, U, V, A, patch, stride, shear=k))
        assert torch.equal(F.super_resolve_field(net, field, U, V, patch, stride, shear=k), F.integrate(outk, U, V, A, h0, w0, s, patch, stride, shear=k))
        # with the ensemble: merge, then the field integrate
        mask = E.mask_of("flips")
        want = F.integrate(E.merge(net(E.expand(F.divide(field, U, V, A, patch, stride), mask)), mask), U, V, A, h0, w0, s, patch, stride)
        assert torch.equal(F.super_resolve_field(net, field, U, V, patch, stride, ensemble="flips"), want)
        assert torch.equal(F.super_resolve_field(net, field, U, V, patch, stride, max_batch=8, ensemble="flips"), want)
        assert torch.equal(F.super_resolve_field(net, field, U, V, patch, stride, max_batch=8), plain)
        # U = V = A: the scene path, bit for bit
        scene = field[:A * h0, :A * w0].contiguous()
        assert torch.equal(F.super_resolve_field(net, scene, A, A, patch, stride), S.super_resolve_scene(net, scene, patch, stride))
        assert torch.equal(F.super_resolve_field(net, scene, A, A, patch, stride, blend="linear", shear=1),
                           S.super_resolve_scene(net, scene, patch, stride, blend="linear", shear=1))


# ---- 7. the tool ----
def test_tool_writes_every_view(golden_dir, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import super_resolve
    A, s = 3, 2
    net = net_of(A, s, seed=12)
    ckpt = str(tmp_path / "net.pth.tar")
    trainer.save_checkpoint(net, ckpt, 1)
    mat = os.path.join(golden_dir, "prepare_lf_v73.mat")
    lf = prepare.load_lf(mat)
    assert lf.shape[:4] == (5, 5, 9, 7) and lf.dtype == np.uint8
    base = ["--angRes", str(A), "--scale_factor", str(s), "--path_pre_pth", ckpt, "--lf", mat, "--patch_size_for_test", "8", "--stride_for_test", "4"]
    out_dir = str(tmp_path / "all")
    paths = super_resolve.main(base + ["--out_dir", out_dir, "--views", "all", "--angular_stride", "2"])
    want = colour.super_resolve_lf(net, lf, patch=8, stride=4, views="all", astride=2)
    assert want.shape == (5, 5, 9 * s, 7 * s, 3)
    assert sorted(os.listdir(out_dir)) == sorted(os.path.basename(p) for p in paths) and len(paths) == 25
    for p in range(5):
        for q in range(5):
            assert np.array_equal(png.read_png(os.path.join(out_dir, f"view_{p}_{q}.png")), want[p, q].cpu().numpy())
    # without --views: the centre views, today's call
    out_dir = str(tmp_path / "centre")
    paths = super_resolve.main(base + ["--out_dir", out_dir])
    centre = colour.super_resolve_lf(net, lf, patch=8, stride=4)
    assert sorted(os.listdir(out_dir)) == sorted(os.path.basename(p) for p in paths) and len(paths) == A * A
    for u in range(A):
        for v in range(A):
            assert np.array_equal(png.read_png(os.path.join(out_dir, f"view_{u}_{v}.png")), centre[u, v].cpu().numpy())
    # the tiled field's luma, unquantised, is field.super_resolve_field of the whole luma mosaic
    t = prepare.to_device(lf, 5, DEV)
    y = F.super_resolve_field(net, colour.luma(t, 5), 5, 5, 8, 4, astride=2)
    assert torch.equal(colour.merge(t, y, 5, s), want)
