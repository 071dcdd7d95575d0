"""GPU tests of the dihedral light-field transforms and the self-ensemble built on them (lft_amd/csrc/lft_ensemble.cuh, C ABI
lft_dihedral_batch / _expand / _merge / lft_scene_integrate_ens, lft_amd/ensemble.py).

The gather kernels are pinned to the bit against their torch definition: T_t = flip(-1), flip(-2), transpose(-1, -2), each if its
bit of t is set; T_t^-1 = the same steps in reverse order; merge = first variant, += the others in ascending code order, one
multiplication by float32(1) / E.  The composition with the network is pinned to the reference through the CPU oracle: eight
oracle forwards of the transformed input, mapped back and averaged."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gpu_util as G
from lft_amd import _lib
from lft_amd import ensemble as E
from lft_amd import scene as S
from lft_amd.params import deterministic_state, synthetic_lr
from oracle import lft_oracle as O

pytestmark = pytest.mark.gpu
DEV = G.DEV


# ---------------------------------------------------------------------------------------------- the contract, in torch
def T(x, t):
    if t & 1:
        x = x.flip(-1)
    if t & 2:
        x = x.flip(-2)
    if t & 4:
        x = x.transpose(-1, -2)
    return x


def Tinv(y, t):
    if t & 4:
        y = y.transpose(-1, -2)
    if t & 2:
        y = y.flip(-2)
    if t & 1:
        y = y.flip(-1)
    return y


def codes_of(mask):
    return [t for t in range(8) if mask >> t & 1]


def merge_torch(variants, mask):
    """variants[k]: any [..., ., .] tensor holding variant k of the same images; the sequential fp32 sum of the contract."""
    codes = codes_of(mask)
    acc = Tinv(variants[0], codes[0]).contiguous()
    for y, t in zip(variants[1:], codes[1:]):
        acc = acc + Tinv(y, t)
    return acc * (torch.tensor(1.0, dtype=torch.float32) / len(codes))


def expand_torch(x, mask):
    """[B,1,H,W] (square, or a mask of one shape) -> [B*E,1,.,.] with the variants of an image adjacent."""
    return torch.stack([T(x, t) for t in codes_of(mask)], dim=1).reshape(-1, 1, *T(x, codes_of(mask)[0]).shape[-2:]).contiguous()


def merge_batch_torch(y, mask):
    """[B*E,1,.,.] -> [B,1,H,W]."""
    e = len(codes_of(mask))
    y = y.reshape(-1, e, *y.shape[1:])
    return merge_torch([y[:, k] for k in range(e)], mask)


def rand(shape, *seed):
    return torch.from_numpy(np.random.Generator(np.random.PCG64([7, *seed])).standard_normal(shape, dtype=np.float32))


def call(name, *args):
    _lib.call(name, *args, G.stream())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 1. lft_dihedral_batch
@pytest.mark.parametrize("H,W", [(10, 10), (6, 14), (70, 33)])
def test_dihedral_batch_bit_exact(H, W):
    """One code per image, all eight and a repeated 5; 70x33 is several tiles with ragged edges.  Images of different codes have
    different shapes for H != W, so the output is compared image by image as flat H*W runs."""
    codes = list(range(8)) + [5]
    x = rand((9, H, W), H, W)
    xd = x.to(DEV)
    outs = []
    for cs in (codes, codes[:8] + [13]):                                   # only the low three bits count: 13 behaves as 5
        buf, out = G.guarded((9, H * W), torch.float32)
        call("lft_dihedral_batch", xd.data_ptr(), out.data_ptr(), torch.tensor(cs, dtype=torch.int32, device=DEV).data_ptr(), 9, H, W)
        assert G.guard_intact(buf)
        outs.append(out.cpu())
    for b, t in enumerate(codes):
        assert torch.equal(outs[0][b], T(x[b], t).reshape(-1)), (b, t)
    assert torch.equal(outs[1], outs[0])
    if H == W:                                                             # the Python layer: shapes, and one batch = one shape
        assert torch.equal(E.dihedral_batch(xd[:, None], codes).cpu(), torch.stack([T(x[b], t) for b, t in enumerate(codes)])[:, None])
    else:
        assert torch.equal(E.dihedral_batch(xd[:, None], [4, 5, 6, 7, 7, 6, 5, 4, 4]).cpu()[3], T(x[3], 7)[None])
        with pytest.raises(ValueError, match="flips"):
            E.dihedral_batch(xd[:, None], codes)


# ---------------------------------------------------------------------------------------------- 2. expand / merge
@pytest.mark.parametrize("H,W", [(12, 12), (9, 20), (40, 33)])
@pytest.mark.parametrize("mask", [0xFF, 0x0F, 0x01, 0xA5])
def test_expand_and_merge_bit_exact(mask, H, W):
    B, codes = 3, codes_of(mask)
    e = len(codes)
    x = rand((B, H, W), mask, H, W)
    xd = x.to(DEV)
    buf, ex = G.guarded((B * e, H * W), torch.float32)
    call("lft_dihedral_expand", xd.data_ptr(), ex.data_ptr(), mask, B, H, W)
    assert G.guard_intact(buf)
    for b in range(B):
        for k, t in enumerate(codes):
            assert torch.equal(ex[b * e + k].cpu(), T(x[b], t).reshape(-1)), (b, k, t)
    # merge of INDEPENDENT random variants (each stored in the shape its code gives it) against the sequential torch sum
    y = rand((B, e, H * W), mask, H, W, 1)
    ref = merge_torch([y[:, k].reshape(B, W, H) if t & 4 else y[:, k].reshape(B, H, W) for k, t in enumerate(codes)], mask)
    buf, out = G.guarded((B, H, W), torch.float32)
    call("lft_dihedral_merge", y.to(DEV).data_ptr(), out.data_ptr(), mask, B, H, W)
    assert G.guard_intact(buf)
    assert torch.equal(out.cpu(), ref)
    # merge(expand(x)) == x.  The sequential sum x + x + ... of E equal numbers is exact in fp32 for E = 2 and 4 whatever x is, but for
    # E = 8 only while every partial sum k*x, k <= 7, fits 24 significant bits: on full-mantissa data x*5, x*6 and x*7 round (44 % of
    # normally distributed numbers do not come back, in torch as in the kernel).  The round trip is a statement about the geometry, so
    # it runs on data with 21 significant bits, for which every partial sum is exact and x must come back to the bit.
    if e & (e - 1) == 0:
        x21 = (x * 2.0 ** 18).round() * 2.0 ** -18                         # |x| < 8: at most 21 significant bits
        x21d = x21.to(DEV)
        call("lft_dihedral_expand", x21d.data_ptr(), ex.data_ptr(), mask, B, H, W)
        call("lft_dihedral_merge", ex.data_ptr(), out.data_ptr(), mask, B, H, W)
        assert torch.equal(out.cpu(), x21)
    # the Python layer on what may be one batch; the rest is refused with a pointer to "flips"
    if H == W or not (mask & 0xF0 and mask & 0x0F):
        got = E.expand(xd[:, None], mask)
        assert torch.equal(got.cpu(), expand_torch(x[:, None], mask))
        assert torch.equal(E.merge(got, mask).cpu(), merge_batch_torch(got.cpu(), mask))
    else:
        with pytest.raises(ValueError, match="flips"):
            E.expand(xd[:, None], mask)


# ---------------------------------------------------------------------------------------------- 3. lft_scene_integrate_ens
@pytest.mark.parametrize("A,h0,w0,patch,stride,s,mask", [(2, 20, 23, 8, 4, 2, 0xFF), (3, 19, 32, 16, 8, 4, 0x0F), (3, 19, 32, 16, 8, 4, 0xFF)])
def test_scene_integrate_ens_bit_exact(A, h0, w0, patch, stride, s, mask):
    nu, nv = O.lf_divide_counts(h0, w0, patch, stride)
    e, P = len(codes_of(mask)), A * patch * s
    y = rand((nu * nv * e, 1, P, P), A, h0, w0, mask)
    merged = merge_batch_torch(y, mask)
    ref = O.views_to_scene_mosaic(O.lf_integrate(merged.reshape(nu, nv, P, P), A, patch * s, stride * s, h0 * s, w0 * s))
    buf, out = G.guarded((A * h0 * s, A * w0 * s), torch.float32)
    call("lft_scene_integrate_ens", y.to(DEV).data_ptr(), out.data_ptr(), mask, A, h0, w0, patch, stride, s)
    assert G.guard_intact(buf)
    assert torch.equal(out.cpu(), ref)
    assert torch.equal(S.integrate_ensemble(y.to(DEV), mask, A, h0, w0, s, patch, stride).cpu(), ref)


# ---------------------------------------------------------------------------------------------- 4. end to end against the oracle
def make_net(A, s, precision="fp32"):
    from model import LFT
    sd = deterministic_state(64, s, seed=1, flavor="stress")
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s), precision=precision)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(DEV).eval(), O.state_from_numpy(sd)


def oracle_ensemble(osd, lr, A, s, mask):
    return merge_torch([O.forward(osd, T(lr, t).contiguous(), A, s) for t in codes_of(mask)], mask)


@pytest.mark.parametrize("A,s,B,h,w,mode", [(2, 2, 2, 6, 6, "dihedral"), (3, 4, 1, 5, 5, "dihedral"), (2, 2, 1, 5, 7, "flips")])
def test_self_ensemble_matches_oracle_fp32(A, s, B, h, w, mode):
    net, osd = make_net(A, s)
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0))
    ref = oracle_ensemble(osd, lr, A, s, E.MASKS[mode])
    got = net.self_ensemble(lr.to(DEV), mode).cpu()
    with torch.no_grad():
        plain = net(lr.to(DEV)).cpu()
    assert got.shape == ref.shape == plain.shape
    rel, apart = G.rel_max(got, ref), G.rel_max(plain, ref)
    print(f"self_ensemble {mode} A{A} s{s} B{B} {h}x{w}: rel max err {rel:.3e}, plain forward is {apart:.3e} away")
    assert rel <= 1e-4, G.err_report(got, ref)
    assert apart > 1e-2                      # an ensemble that silently returns the identity variant would pass the line above


def test_dihedral_on_non_square_views_is_refused():
    net, _ = make_net(2, 2)
    lr = torch.from_numpy(synthetic_lr(1, 2, 5, 7, seed=0)).to(DEV)
    with pytest.raises(ValueError, match="flips"):
        net.self_ensemble(lr, "dihedral")


# ---------------------------------------------------------------------------------------------- 5. the 16-bit paths
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_self_ensemble_16bit_is_the_same_composition(precision):
    """The same network batch (16 inputs in one call) between torch's transforms: bit-identical, the forward being bitwise
    repeatable (tests/test_gpu_determinism.py)."""
    A, s, B, h, w = 2, 2, 2, 6, 6
    net, _ = make_net(A, s, precision)
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0)).to(DEV)
    got = net.self_ensemble(lr, "dihedral", max_batch=16)
    with torch.no_grad():
        ref = merge_batch_torch(net(expand_torch(lr, 0xFF)), 0xFF)
    assert torch.equal(got, ref)


# ---------------------------------------------------------------------------------------------- 6. scenes
def test_scene_ensemble_matches_oracle_pipeline():
    from lft_amd import evaluate, metrics
    A, s, patch, stride, h0, w0 = 2, 2, 8, 4, 10, 9
    net, osd = make_net(A, s)
    rng = np.random.Generator(np.random.PCG64([13, A, h0, w0]))
    scene = torch.from_numpy(rng.random((A * h0, A * w0), dtype=np.float32))
    hr = torch.from_numpy(rng.random((A * h0 * s, A * w0 * s), dtype=np.float32))
    sd = scene.to(DEV)
    got = S.super_resolve_scene(net, sd, patch, stride, max_batch=20, ensemble="dihedral").cpu()    # 2 patches per chunk, 9 patches
    sub = O.lf_divide(scene, A, patch, stride)
    nu, nv = sub.shape[:2]
    assert nu * nv == 9
    outs = oracle_ensemble(osd, sub.reshape(nu * nv, 1, A * patch, A * patch), A, s, 0xFF)
    ref = O.views_to_scene_mosaic(O.lf_integrate(outs.reshape(nu, nv, A * patch * s, A * patch * s), A, patch * s, stride * s, h0 * s, w0 * s))
    assert got.shape == ref.shape == (A * h0 * s, A * w0 * s)
    rel = G.rel_max(got, ref)
    print(f"scene ensemble: rel max err {rel:.3e}")
    assert rel <= 1e-4, G.err_report(got, ref)
    # ensemble=None is today's path, to the bit
    assert torch.equal(S.super_resolve_scene(net, sd, patch, stride, max_batch=20, ensemble=None), S.super_resolve_scene(net, sd, patch, stride, max_batch=20))
    # evaluate.test_scene passes the mode on: the same mosaic as the default max_batch gives, and the metrics of that mosaic
    psnr, ssim, sr = evaluate.test_scene(net, scene, hr, patch=patch, stride=stride, ensemble="dihedral")
    assert torch.equal(sr, S.super_resolve_scene(net, sd, patch, stride, ensemble="dihedral"))
    assert G.rel_max(sr.cpu(), ref) <= 1e-4
    assert (psnr, ssim) == metrics.cal_metrics(net, hr.to(DEV), sr)


# ---------------------------------------------------------------------------------------------- 7. training augmentation
def test_augment_gpu_equals_augment():
    from lft_amd import trainer
    A, p, s, B = 2, 4, 2, 8
    seen = set()
    for seed in range(3):
        lr, hr = rand((B, 1, A * p, A * p), seed).to(DEV), rand((B, 1, A * p * s, A * p * s), seed, 1).to(DEV)
        a0, b0 = trainer.augment(lr, hr, np.random.Generator(np.random.PCG64(seed)))
        a1, b1 = trainer.augment_gpu(lr, hr, np.random.Generator(np.random.PCG64(seed)))
        assert torch.equal(a0, a1) and torch.equal(b0, b1)
        seen.add(bool(torch.equal(a0, lr)))
    assert False in seen                                                   # the draws did transform something


def test_fit_with_gpu_augment():
    from lft_amd import trainer
    A, s = 2, 2
    net, _ = make_net(A, s)
    net.train()
    src = trainer.SyntheticPatchSource(4, A, s, patch=8, seed=0)
    hist = trainer.fit(net, src, epochs=1, batch_size=2, gpu_augment=True, log=lambda *_: None)
    assert len(hist) == 1 and np.isfinite(hist[0])
