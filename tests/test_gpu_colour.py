"""GPU tests of the colour path: lft_lf_luma, lft_colour_merge, lft_amd.colour and tools/super_resolve.py, against the fixtures of
tools/gen_golden_colour.py (the reference's rgb2ycbcr / imresize / convertDouble2Byte, the exact inverse transform) and the numpy
restatement of tests/colour_util.py."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import _lib, colour, png, prepare, scene, trainer
from lft_amd._lib import LftError

from colour_util import CASES, colour_np, load_case, tie_distance, ulp_diff

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
_cache = {}


def case(golden_dir, name):
    """(fixture arrays, baseline restatement, light field on the device) of one case, made once."""
    if name not in _cache:
        g = load_case(golden_dir, name)
        A, s, v73 = (int(x) for x in g["meta"])
        if v73:     # the file's own order: a [C, W, H, V, U] array seen through reversed strides
            t = torch.from_numpy(np.ascontiguousarray(g["lf"].transpose(4, 3, 2, 1, 0))).to(DEV).permute(4, 3, 2, 1, 0)
            assert not t.is_contiguous()
        else:
            t = torch.from_numpy(g["lf"]).to(DEV)
        _cache[name] = (g, colour_np(g["lf"], A, s, None), t)
    return _cache[name]


def _net(A, s, seed):
    from lft_amd.params import deterministic_state
    from model import LFT
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, s, seed=seed).items()})
    return net.to(DEV).eval()


@pytest.mark.parametrize("name", sorted(CASES))
def test_luma(golden_dir, name):
    g, _, t = case(golden_dir, name)
    A, s, _ = (int(x) for x in g["meta"])
    y = colour.luma(t, A)
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and tuple(y.shape) == g["lr_y"].shape
    d = ulp_diff(y.cpu().numpy(), g["lr_y"])
    print(f"{name}: luma max {int(d.max())} ulp, {float((d == 0).mean()):.6f} bit-identical")
    assert d.max() <= 1
    if t.dtype != torch.uint8:      # floats enter lft_lf_prepare as they enter here: the same Y, bit for bit
        hr, _ = prepare.lf_prepare(t, A, s, [(0, 0)], int(t.shape[2]), int(t.shape[3]))
        assert torch.equal(hr[0], y)


@pytest.mark.parametrize("name", sorted(CASES))
def test_merge(golden_dir, name):
    g, base, t = case(golden_dir, name)
    A, s, _ = (int(x) for x in g["meta"])
    sr = torch.from_numpy(g["sr_y"]).to(DEV)
    out = colour.merge(t, sr, A, s)
    rgb = colour.merge(t, sr, A, s, torch.float32)
    out_b = colour.bicubic_lf(t, A, s)
    rgb_b = colour.merge(t, None, A, s, torch.float32)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and tuple(out.shape) == g["out"].shape and rgb.dtype == torch.float32
    d, db = ulp_diff(rgb.cpu().numpy(), g["rgb"]), ulp_diff(rgb_b.cpu().numpy(), base["rgb"].astype(np.float32))
    ne, neb = int((out.cpu().numpy() != g["out"]).sum()), int((out_b.cpu().numpy() != g["out_base"]).sum())
    print(f"{name}: uint8 differs in {ne} (sr_y) / {neb} (baseline) of {g['out'].size}; fp32 max {int(d.max())} / {int(db.max())} ulp")
    assert ne == 0 and neb == 0                                    # no tie in the fixtures: equal, no tolerance
    assert d.max() <= 1 and db.max() <= 1


def test_merge_strided_input_gives_the_same_bits(golden_dir):
    g, _, t = case(golden_dir, "v73_s2_u8")
    A, s, _ = (int(x) for x in g["meta"])
    sr = torch.from_numpy(g["sr_y"]).to(DEV)
    dense = t.contiguous()
    assert dense.stride() != t.stride()
    # views cut out of a larger field with a fourth channel: every stride differs from the dense one
    big = torch.zeros(7, 6, 11, 9, 4, dtype=torch.uint8, device=DEV)
    big[1:6, 0:5, 2:, 1:8, :3] = dense
    cut = big[1:6, 0:5, 2:, 1:8, :]
    for other in (t, cut):
        assert torch.equal(colour.luma(other, A), colour.luma(dense, A))
        for srr in (sr, None):
            for dt in (torch.uint8, torch.float32):
                assert torch.equal(colour.merge(other, srr, A, s, dt), colour.merge(dense, srr, A, s, dt))


def _merge_raw(t, angres, scale, sr_t, wh_t, ih_t, ww_t, iw_t, out_t, **kw):
    """lft_colour_merge with the caller's tables; kw overrides any argument of the call by name."""
    U, V, H, W, C = (int(d) for d in t.shape)
    a = dict(lf=t.data_ptr(), cls=prepare._CLASS[t.dtype], U=U, V=V, H=H, W=W, C=C, strides=(ctypes.c_longlong * 5)(*t.stride()),
             A=angres, s=scale, sr=sr_t.data_ptr() if sr_t is not None else None, wh=wh_t.data_ptr(), ih=ih_t.data_ptr(),
             ph=wh_t.shape[1], ww=ww_t.data_ptr(), iw=iw_t.data_ptr(), pw=ww_t.shape[1],
             minv=(ctypes.c_double * 9)(*colour.inverse_matrix().reshape(-1)), out=out_t.data_ptr(),
             out_cls=colour._OUT_CLASS[out_t.dtype])
    a.update(kw)
    _lib.enqueue("lft_colour_merge", DEV, a["lf"], a["cls"], a["U"], a["V"], a["H"], a["W"], a["C"], a["strides"], a["A"], a["s"], a["sr"],
                 a["wh"], a["ih"], a["ph"], a["ww"], a["iw"], a["pw"], a["minv"], a["out"], a["out_cls"])


def test_merge_fallback_path_gives_the_same_bits():
    """The true tables never span more than the staged region (at most 16 + 3 LR rows per 32 HR rows), so the fall-back is forced
    through the C ABI: a fifth tap of weight 0 that points to the far end of the view widens every tile's span past the region
    and adds w * v = 0 to each sum."""
    rng = np.random.default_rng(5)
    A, s, H, W = 2, 2, 40, 45
    t = torch.from_numpy(rng.integers(0, 256, (2, 2, H, W, 3)).astype(np.uint8)).to(DEV)
    sr = torch.from_numpy(rng.uniform(-0.05, 1.05, (A * s * H, A * s * W)).astype(np.float32)).to(DEV)

    def tables(L, far):
        w, i = colour.up_contributions(L, s)
        if far:
            w = np.concatenate([w, np.zeros((L * s, 1))], axis=1)
            i = np.concatenate([i, np.where(np.arange(L * s) < L, L - 1, 0).astype(np.int32)[:, None]], axis=1)
        return torch.from_numpy(np.ascontiguousarray(w)).to(DEV), torch.from_numpy(np.ascontiguousarray(i)).to(DEV)

    for dt in (torch.uint8, torch.float32):
        for srr in (sr, None):
            want = colour.merge(t, srr, A, s, dt)
            for far_h, far_w in ((True, True), (True, False), (False, True)):      # neither stage fits | rows only | columns only
                out = torch.zeros_like(want)
                _merge_raw(t, A, s, srr, *tables(H, far_h), *tables(W, far_w), out)
                assert torch.equal(out, want), (dt, srr is None, far_h, far_w)


def test_refusals_enqueue_nothing_and_calls_repeat():
    A, s, H, W = 3, 2, 6, 5
    t = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (5, 5, H, W, 3)).astype(np.uint8)).to(DEV)
    sr = torch.rand(A * s * H, A * s * W, device=DEV)
    wh, ih = colour._device_table(H, s, DEV)
    ww, iw = colour._device_table(W, s, DEV)
    out = torch.full((A, A, s * H, s * W, 3), 77, dtype=torch.uint8, device=DEV)
    outf = torch.full((A, A, s * H, s * W, 3), -7.0, device=DEV)
    y = torch.full((A * H, A * W), -7.0, device=DEV)
    st = (ctypes.c_longlong * 5)(*t.stride())
    neg = (ctypes.c_longlong * 5)(*[-x if k == 2 else x for k, x in enumerate(t.stride())])

    bad_lf = [dict(cls=3), dict(cls=-1), dict(C=2), dict(C=0), dict(A=0), dict(A=-1), dict(A=7), dict(A=4), dict(U=6), dict(V=4),
              dict(U=2), dict(H=0), dict(W=-3), dict(U=0), dict(lf=None), dict(strides=None), dict(strides=neg)]
    bad_merge = bad_lf + [dict(s=3), dict(s=1), dict(s=0), dict(s=8), dict(ph=0), dict(ph=7), dict(pw=0), dict(pw=7), dict(pw=-1),
                          dict(wh=None), dict(ih=None), dict(ww=None), dict(iw=None), dict(minv=None), dict(out=None),
                          dict(out_cls=_lib.LF_FLOAT64), dict(out_cls=-1)]
    for kw in bad_merge:
        for o in (out, outf):
            with pytest.raises(LftError, match="lft_colour_merge") as e:
                _merge_raw(t, A, s, sr, wh, ih, ww, iw, o, **kw)
            assert "(code -1)" in str(e.value) or "(code -2)" in str(e.value), (kw, str(e.value))

    def luma_raw(**kw):
        a = dict(lf=t.data_ptr(), cls=_lib.LF_UINT8, U=5, V=5, H=H, W=W, C=3, strides=st, A=A, y=y.data_ptr())
        a.update(kw)
        _lib.enqueue("lft_lf_luma", DEV, a["lf"], a["cls"], a["U"], a["V"], a["H"], a["W"], a["C"], a["strides"], a["A"], a["y"])

    for kw in bad_lf + [dict(y=None)]:
        with pytest.raises(LftError, match="lft_lf_luma") as e:
            luma_raw(**kw)
        assert "(code -1)" in str(e.value) or "(code -2)" in str(e.value), (kw, str(e.value))
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and bool((outf == -7.0).all()) and bool((y == -7.0).all())      # nothing ran
    for bad in (lambda: colour.merge(t, sr, A, 3), lambda: colour.merge(t, sr[1:], A, s), lambda: colour.merge(t, sr.cpu(), A, s),
                lambda: colour.merge(t, sr, A, s, torch.float64), lambda: colour.merge(t.to(torch.int16), sr, A, s),
                lambda: colour.luma(t.cpu(), A), lambda: colour.luma(t, 4), lambda: colour.luma(t, 0)):
        with pytest.raises(LftError):
            bad()
    # the good calls run, and a second call gives the same bits
    luma_raw()
    _merge_raw(t, A, s, sr, wh, ih, ww, iw, out)
    _merge_raw(t, A, s, sr, wh, ih, ww, iw, outf)
    torch.cuda.synchronize()
    ref = colour_np(t.cpu().numpy(), A, s, sr.cpu().numpy())
    assert ulp_diff(y.cpu().numpy(), ref["lr_y"]).max() <= 1 and ulp_diff(outf.cpu().numpy(), ref["rgb"].astype(np.float32)).max() <= 1
    free = tie_distance(ref["rgb"]) > 1e-6
    assert np.array_equal(out.cpu().numpy()[free], ref["out"][free])
    assert torch.equal(colour.merge(t, sr, A, s), out) and torch.equal(colour.merge(t, sr, A, s, torch.float32), outf)
    assert torch.equal(colour.luma(t, A), y)


@pytest.mark.parametrize("ensemble", [None, "flips"])
def test_super_resolve_lf_end_to_end(ensemble):
    A, s = 5, 2
    lf = np.random.default_rng(7).integers(0, 256, (7, 7, 16, 12, 3)).astype(np.uint8)
    net = _net(A, s, seed=11)
    t = prepare.to_device(lf, A, DEV)
    out = colour.super_resolve_lf(net, t, patch=8, stride=4, ensemble=ensemble)
    sr_y = scene.super_resolve_scene(net, colour.luma(t, A), 8, 4, 64, ensemble)        # the GPU's own luma
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and tuple(out.shape) == (A, A, 32, 24, 3) and tuple(sr_y.shape) == (A * 32, A * 24)
    ref = colour_np(lf, A, s, sr_y.cpu().numpy())
    got = out.cpu().numpy().astype(np.int64)
    free = tie_distance(ref["rgb"]) > 1e-6
    diff = np.abs(got - ref["out"].astype(np.int64))
    print(f"ensemble={ensemble}: {int((~free).sum())} of {free.size} values within 1e-6 of a tie; max difference {int(diff.max())}")
    assert diff[free].max() == 0 and diff.max() <= 1
    assert torch.equal(colour.super_resolve_lf(net, lf, patch=8, stride=4, ensemble=ensemble), out)    # a loaded array, same bits
    outf = colour.super_resolve_lf(net, t, patch=8, stride=4, ensemble=ensemble, out_dtype=torch.float32)
    assert ulp_diff(outf.cpu().numpy(), ref["rgb"].astype(np.float32)).max() <= 1


def test_luma_and_merge_capture_and_replay(golden_dir):
    from lft_amd import train as T
    g, _, t = case(golden_dir, "a5_s4_u8")
    A, s, _ = (int(x) for x in g["meta"])
    sr = torch.from_numpy(g["sr_y"]).to(DEV)
    y0, o0 = colour.luma(t, A), colour.merge(t, sr, A, s)            # eager; the tables are on the device from here on
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side, capture_error_mode=T.CAPTURE_MODE):
            y1 = colour.luma(t, A)
            o1 = colour.merge(t, sr, A, s)
        y1.fill_(-1.0)
        o1.fill_(9)
        graph.replay()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(y1, y0) and torch.equal(o1, o0)
    assert np.array_equal(o1.cpu().numpy(), g["out"])


def test_tool_writes_the_views(golden_dir, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import super_resolve
    A, s = 3, 2
    net = _net(A, s, seed=12)
    ckpt = str(tmp_path / "net.pth.tar")
    trainer.save_checkpoint(net, ckpt, 1)
    mat = os.path.join(golden_dir, "prepare_lf_v73.mat")
    out_dir = str(tmp_path / "png")
    paths = super_resolve.main(["--angRes", str(A), "--scale_factor", str(s), "--path_pre_pth", ckpt, "--lf", mat, "--out_dir", out_dir,
                                "--patch_size_for_test", "8", "--stride_for_test", "4", "--bicubic", "--mosaic"])
    lf = prepare.load_lf(mat)
    want = colour.super_resolve_lf(net, lf, patch=8, stride=4).cpu().numpy()
    base = colour.bicubic_lf(lf, A, s, device=DEV).cpu().numpy()
    assert want.shape == (A, A, s * lf.shape[2], s * lf.shape[3], 3)
    assert sorted(os.listdir(out_dir)) == sorted(os.path.basename(p) for p in paths) and len(paths) == 2 * (A * A + 1)
    for u in range(A):
        for v in range(A):
            assert np.array_equal(png.read_png(os.path.join(out_dir, f"view_{u}_{v}.png")), want[u, v])
            assert np.array_equal(png.read_png(os.path.join(out_dir, f"bicubic_{u}_{v}.png")), base[u, v])
    m = png.read_png(os.path.join(out_dir, "mosaic.png"))
    assert np.array_equal(m, want.transpose(0, 2, 1, 3, 4).reshape(A * want.shape[2], A * want.shape[3], 3))
    assert np.abs(want.astype(int) - base.astype(int)).max() > 0           # the network's luma is in the picture
