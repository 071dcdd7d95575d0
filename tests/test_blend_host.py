"""CPU: windowed blending of overlapping SR patches up to the device -- the windows, the new header and its binding, every refusal
of the entry point on the host, every Python refusal, every call site handing `blend` on in its place, and on the restatement alone
(tests/blend_util.py): a perfect network's patches blend back to the scene, and the seam bound of tests/test_gpu_blend.py holds for
the seeds it uses while the crop breaks it."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import _lib, scene as S
from lft_amd._lib import LftError

import blend_util as BU
import shear_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = -1, -2
P, Q, T, W = 1 << 20, 2 << 20, 3 << 20, 4 << 20        # addresses that are never dereferenced
NAME = "lft_scene_integrate_blend"


# ---- 1. the windows ----
@pytest.mark.parametrize("pz", [1, 2, 7, 16, 24, 32, 64, 128])
@pytest.mark.parametrize("kind", BU.WINDOWS)
def test_windows_are_positive_and_symmetric(kind, pz):
    w = S.window_table(kind, pz)
    assert w.dtype == np.float32 and w.shape == (pz,) and np.array_equal(w, BU.window_np(kind, pz))
    assert (w > 0).all() and np.isfinite(w).all() and np.array_equal(w, w[::-1]) and w.max() <= 1
    if kind == "flat":
        assert (w == 1).all()


@pytest.mark.parametrize("S_", [1, 4, 8, 16, 32, 64])
def test_hann_halves_sum_to_one(S_):
    w = S.window_table("hann", 2 * S_).astype(np.float64)
    assert np.abs(w[:S_] + w[S_:] - 1.0).max() <= 2.0 ** -23
    lin = S.window_table("linear", 2 * S_).astype(np.float64)      # so do the linear ones, which is why both blend without a ripple
    assert np.abs(lin[:S_] + lin[S_:] - 1.0).max() <= 2.0 ** -23


def test_window_refusals():
    for bad in ("Hann", "cosine", "", "none"):
        with pytest.raises(LftError, match="blend must be None, one of hann, linear, flat"):
            S.window_table(bad, 16)
    for bad in (0, -4, 1.5, True, _lib.BLEND_MAX_PZ + 1):
        with pytest.raises(LftError, match="a window of"):
            S.window_table("hann", bad)
    with pytest.raises(LftError, match="blend must be None"):
        S.blend_window("box", 16)                       # refused before the device is asked for
    assert S.parse_blend(None) is None and S.parse_blend("none") is None and S.parse_blend("linear") == "linear"
    with pytest.raises(LftError, match="--blend takes none, hann, linear, flat"):
        S.parse_blend("auto")


# ---- 2. the header and its binding ----
def test_header_declares_the_export_and_the_binding_holds_it():
    hdr = open(os.path.join(ROOT, "include", "lft_hip_blend.h")).read()
    assert tuple(re.findall(r"^int\s+(lft_\w+)\s*\(", hdr, flags=re.M)) == (NAME,)
    assert "Added beside ABI 5; lft_version unchanged" in hdr and "#define LFT_BLEND_MAX_PZ 8192" in hdr
    assert _lib.BLEND_EXPORTS == (NAME,) and _lib.ADDON_HEADERS["lft_hip_blend.h"] == "BLEND_" and _lib.BLEND_MAX_PZ == 8192
    assert NAME in _lib.ADDON_STREAM_LAST and NAME in _lib.OPTIONAL_EXPORTS and NAME not in _lib.EXPORTS and len(_lib.UNITS) == 3
    from ctypes import c_int, c_void_p
    assert _lib._ADDON_SIGS[NAME] == (c_int, [c_void_p] * 4 + [c_int] * 6 + [c_void_p])
    # the prototype's words: sub, shear, window, out, A, h0, w0, patch, stride, s, stream
    params = re.search(NAME + r"\s*\(([^)]*)\)\s*;", hdr).group(1).split(",")
    assert [p.split()[-1].lstrip("*") for p in params] == ["sr_patches", "shear", "window", "sr_scene", "A", "h0", "w0", "patch", "stride", "s", "stream"]
    assert "lft_blend.cuh" in _lib.SOURCES
    assert [u for u in _lib.UNITS if '"lft_blend.cuh"' in open(os.path.join(_lib.CSRC, u + ".hip")).read()] == ["lft_lightfield"]
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, NAME) and _lib.lib().lft_version() == 5
    kernel = open(os.path.join(_lib.CSRC, "lft_blend.cuh")).read()
    assert "k_scene_integrate_blend" in kernel and "#pragma clang fp contract(off)" in kernel and "__fdiv_rn" in kernel
    # the definition's sentences stand in the header, the kernel file's comment and the module docstring
    for text in (hdr, kernel, S.__doc__):
        flat = " ".join(re.sub(r"^\s*(//|\*|-)\s?", "", line).replace("`", "").strip() for line in text.splitlines())
        flat = flat.replace("−", "-").replace("≥", ">=").replace("≤", "<=").replace("·", "*").replace(" // ", " / ")
        for words in ("Y = ku*S + a - bdr + sk_n*(u - u0)", "X = kv*S + b - bdr + sk_n*(v - u0)", "read backwards",
                      "no zero-filled position ever contributes", "in ascending ku, then kv", "one rounded fp32 operation", "correctly rounded"):
            assert words in flat, words


# ---- 3. every refusal of the entry point is answered on the host ----
def test_every_c_refusal_comes_before_any_device_work():
    _lib.build()
    L = _lib.lib()

    def refused(args, rc, words):
        L.lft_scene_counts(1, 1, 1, 1, None, None)      # leaves another call's message behind
        assert getattr(L, NAME)(*args) == rc, args
        msg = L.lft_last_error().decode()
        assert words in msg, (args, msg)
        return msg

    keys = ("sub", "shear", "window", "out", "A", "h0", "w0", "patch", "stride", "s", "stream")
    good = dict(zip(keys, (P, Q, W, T, 5, 64, 64, 32, 16, 2, None)))
    change = lambda **kw: [kw.get(k, v) for k, v in good.items()]
    for k in ("sub", "window", "out"):
        assert refused(change(**{k: None}), ERR_ARG, "null pointer").startswith(NAME + ":")
    refused(change(A=0), ERR_ARG, NAME + ": angRes 0")
    for s in (0, 1, 3, 8, -2):
        refused(change(s=s), ERR_ARG, NAME + f": scale factor {s}")
    # lft_scene_divide's tilings, with its words: stride > patch among them
    for kw, words in ((dict(stride=33), "bad scene tiling"), (dict(stride=0), "bad scene tiling"), (dict(h0=0), "bad scene tiling"),
                      (dict(patch=0), "bad scene tiling"), (dict(h0=8), "smaller than one patch")):
        L.lft_scene_counts(1, 1, 1, 1, None, None)
        a = change(**kw)
        assert L.lft_scene_divide(P, T, *a[4:9], None) == ERR_SHAPE
        want = L.lft_last_error().decode()
        assert words in want and refused(a, ERR_SHAPE, words) == want
    refused(change(patch=31), ERR_SHAPE, NAME + ": patch - stride = 15 is odd")
    refused(change(stride=23), ERR_SHAPE, "patch - stride = 9 is odd")
    # the pointers come first, then the sizes
    refused(change(sub=None, stride=0), ERR_ARG, "null pointer")
    refused(change(window=None, s=3), ERR_ARG, "null pointer")
    # the launch: the window in LDS, the rows of the SR scene mosaic
    refused(change(patch=4096, stride=4096, h0=4096, w0=4096, s=4, A=1), ERR_SHAPE, "a window of 16384 entries (at most 8192)")
    refused(change(A=1, h0=30000, s=4), ERR_SHAPE, "an SR scene mosaic of 120000 rows needs more than 65535 blocks")
    refused(change(A=4096), ERR_SHAPE, "an SR scene mosaic of 524288 rows")


# ---- 4. Python refusals need no device ----
def test_python_refusals_need_no_device():
    A, patch, stride, s = 5, 32, 16, 2
    assert S.scene_counts(48, 64) == (3, 4)
    sr = torch.zeros(12, 1, A * patch * s, A * patch * s)
    for bad in ("box", 1, 1.0, True, [1.0] * 64, np.ones(64, np.float32), torch.ones(64, dtype=torch.float64), torch.ones(63), torch.ones(2, 32)):
        with pytest.raises(LftError, match="blend must be None, one of hann, linear, flat"):
            S.integrate(sr, A, 48, 64, s, patch, stride, blend=bad)
    with pytest.raises(LftError, match="blend: scale factor must be 2 or 4, got 3"):
        S.integrate(sr, A, 48, 64, 3, patch, stride, blend=torch.ones(96))
    with pytest.raises(LftError, match="is odd"):
        S.integrate(sr, A, 48, 64, s, patch, 15, blend="hann")
    with pytest.raises(LftError, match="shear_limit"):
        S.integrate(sr, A, 48, 64, s, patch, 40, blend="hann")
    with pytest.raises(LftError, match=r"sr_patches must be \[12, 1, 320, 320\] for this tiling"):
        S.integrate(sr[:11], A, 48, 64, s, patch, stride, blend="hann")
    with pytest.raises(LftError, match=r"sr_patches must be \[12, 1, 320, 320\]"):
        S.integrate(torch.zeros(12, 1, 8, 8), A, 48, 64, s, patch, stride, blend="flat")
    with pytest.raises(LftError, match=r"shear must be an int32 tensor of shape \[12\]"):
        S.integrate(sr, A, 48, 64, s, patch, stride, shear=torch.zeros(12), blend="hann")
    with pytest.raises(LftError, match="blend is on meta, the patches on cpu"):
        S.integrate(sr, A, 48, 64, s, patch, stride, blend=torch.ones(64, device="meta"))
    # everything right: the device is asked for last
    for blend in ("hann", "linear", "flat", torch.ones(64)):
        with pytest.raises(LftError, match="on a HIP device"):
            S.integrate(sr, A, 48, 64, s, patch, stride, blend=blend)
        with pytest.raises(LftError, match="on a HIP device"):
            S.integrate(sr, A, 48, 64, s, patch, stride, shear=torch.zeros(12, dtype=torch.int32), blend=blend)
    # the whole scene: judged before the scene is cut
    net = SimpleNamespace(angRes=A, factor=s)
    scene = torch.zeros(A * 48, A * 64)
    with pytest.raises(LftError, match="blend must be None"):
        S.super_resolve_scene(net, scene, blend="cosine")
    with pytest.raises(LftError, match="is odd"):
        S.super_resolve_scene(net, scene, stride=17, blend="hann")
    with pytest.raises(LftError, match="scale factor must be 2 or 4"):
        S.super_resolve_scene(SimpleNamespace(angRes=A, factor=3), scene, blend="hann")
    with pytest.raises(LftError, match="shear together with ensemble is not supported"):
        S.super_resolve_scene(net, scene, shear=1, ensemble="flips", blend="hann")
    for kw in (dict(blend="hann"), dict(blend="linear", stride=24), dict(blend="flat", shear=2), dict(blend=torch.ones(64), ensemble="flips")):
        with pytest.raises(LftError, match="on a HIP device"):
            S.super_resolve_scene(net, scene, **kw)


# ---- 5. every call site hands `blend` on, in its own place, and calls the crop as it always did ----
def test_call_sites_pass_blend_through(monkeypatch):
    import sys
    from lft_amd import colour, datasets, evaluate, metrics
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import blend_sets
    import super_resolve
    seen = []

    def fake_scene(net, scene, patch=32, stride=16, max_batch=64, ensemble=None, shear=None, blend=None):
        seen.append(dict(patch=patch, stride=stride, max_batch=max_batch, ensemble=ensemble, shear=shear, blend=blend))
        return torch.zeros(4, 4)

    monkeypatch.setattr(S, "super_resolve_scene", fake_scene)
    monkeypatch.setattr(metrics, "cal_metrics", lambda net, hr, sr, ssim_range=2.0: (30.0, 0.9))
    net = torch.nn.Linear(1, 1)
    net.angRes, net.factor = 2, 2
    lr, hr = torch.zeros(4, 4), torch.zeros(8, 8)
    want = dict(patch=16, stride=8, max_batch=64, ensemble=None, shear=None, blend="hann")
    evaluate.test_scene(net, lr, hr, 16, 8, blend="hann")
    assert seen.pop() == want
    evaluate.test(net, [(lr, hr)], 16, 8, shear=3, blend="linear", sharded=False)
    assert seen.pop() == dict(want, shear=3, blend="linear")
    monkeypatch.setattr(datasets, "MultiTestSetDataLoader", lambda args: (["SetA"], [[(lr[None], hr[None])]], 1))
    args = SimpleNamespace(patch_size_for_test=16, stride_for_test=8)
    w = torch.ones(32)
    assert evaluate.test_sets(net, args, log=lambda *_: None, blend=w) == {"SetA": (30.0, 0.9)}
    assert seen.pop()["blend"] is w and not seen
    evaluate.test_sets(net, args, log=lambda *_: None, ensemble="flips", blend="flat")
    assert seen.pop() == dict(want, ensemble="flips", blend="flat")
    evaluate.test_sets(net, args, log=lambda *_: None)
    assert seen.pop() == dict(want, blend=None)
    # the colour path
    monkeypatch.setattr(colour, "_field", lambda lf, A, dev: lf)
    monkeypatch.setattr(colour, "luma", lambda t, A: lr)
    monkeypatch.setattr(colour, "merge", lambda t, sr_y, A, s, out_dtype: sr_y)
    colour.super_resolve_lf(net, torch.zeros(2, 2, 2, 2, 3), 16, 8, blend="hann", shear=-2)
    assert seen.pop() == dict(want, shear=-2)
    colour.super_resolve_lf(net, torch.zeros(2, 2, 2, 2, 3), 16, 8, 7, "flips")
    assert seen.pop() == dict(want, max_batch=7, ensemble="flips", blend=None)
    # the crop reaches a super_resolve_scene that has never heard of blend with the arguments it always got
    old = []
    monkeypatch.setattr(S, "super_resolve_scene", lambda net, scene, patch=32, stride=16, max_batch=64, ensemble=None, shear=None:
                        old.append((patch, stride, ensemble, shear)) or torch.zeros(4, 4))
    evaluate.test_scene(net, lr, hr, 16, 8)
    colour.super_resolve_lf(net, torch.zeros(2, 2, 2, 2, 3), 16, 8)
    assert old == [(16, 8, None, None)] * 2
    # tools/super_resolve.py: the option is judged before the model is loaded, then handed to colour.super_resolve_lf
    got = {}
    monkeypatch.setattr(super_resolve, "load_model", lambda a, dev: got.setdefault("loaded", True) and net)
    monkeypatch.setattr(super_resolve, "load_field", lambda path, A, dev: "lf")
    monkeypatch.setattr(super_resolve, "write_views", lambda *a, **kw: [])
    monkeypatch.setattr(colour, "super_resolve_lf", lambda net, lf, patch, stride, ensemble=None, shear=None, blend=None:
                        got.update(patch=patch, stride=stride, shear=shear, blend=blend) or torch.zeros(2, 2, 4, 4, 3))
    base = ["--path_pre_pth", "x", "--lf", "y", "--out_dir", "unused", "--angRes", "5", "--scale_factor", "2"]
    with pytest.raises(LftError, match="--blend takes none, hann, linear, flat"):
        super_resolve.main(base + ["--blend", "some"])
    with pytest.raises(LftError, match="is odd"):
        super_resolve.main(base + ["--blend", "hann", "--stride_for_test", "21"])
    assert not got
    # tools/blend_sets.py: the same, for the test sets
    assert blend_sets.parse([])[1] == "hann" and blend_sets.parse(["--blend", "none"])[1] is None
    a, b = blend_sets.parse(["--blend", "linear", "--stride_for_test", "24"])
    assert b == "linear" and a.stride_for_test == 24 and a.patch_size_for_test == 32
    with pytest.raises(LftError, match="is odd"):
        blend_sets.parse(["--stride_for_test", "23"])
    assert blend_sets.parse(["--blend", "none", "--stride_for_test", "23"])[1] is None       # the crop takes it, as tools/test_sets.py does
    with pytest.raises(LftError, match="--blend takes"):
        blend_sets.parse(["--blend", "hamming"])


# ---- 6. the restatement alone ----
@pytest.mark.parametrize("A,s", [(2, 2), (3, 4)])
@pytest.mark.parametrize("patch,stride", [(8, 4), (8, 6), (8, 8)])
@pytest.mark.parametrize("sheared", [False, True])
def test_a_perfect_networks_patches_blend_back_to_the_scene(A, s, patch, stride, sheared):
    h0, w0 = 9, 14
    rng = np.random.default_rng([42, A, s, patch, stride, sheared])
    G = rng.random((A * h0 * s, A * w0 * s), dtype=np.float32)
    N = int(np.prod(SU.counts_np(h0, w0, patch, stride)))
    kmax = SU.kmax_np(A, patch, stride)
    k = rng.integers(-kmax, kmax + 1, N) if sheared else None
    cut = BU.cut_np(G, A, patch, stride, s, k)
    for kind in BU.WINDOWS:
        out, terms = BU.blend_np(cut, A, h0, w0, patch, stride, s, BU.window_np(kind, patch * s), k)
        assert np.abs(out.astype(np.float64) - G).max() <= BU.reproduction_slack(terms, G), (kind, terms.max())
    # the shapes hold what they were chosen for: more than one patch per axis, a single-term pixel, and without shear T = ceil(pz/S)^2
    assert min(SU.counts_np(h0, w0, patch, stride)) > 1 and terms.min() == 1
    if not sheared:
        assert terms.max() == (-(-patch // stride)) ** 2
    # a flat window over one term is the crop's pixel, and where patches are the crop's own the flat blend of stride == patch is the crop
    if stride == patch:
        assert np.array_equal(out, SU.integrate_plain_np(cut, A, h0, w0, patch, stride, s))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_seam_bound_holds_for_the_blend_and_not_for_the_crop(seed):
    A, s, h0, w0, patch, stride = (BU.SEAM[k] for k in ("A", "s", "h0", "w0", "patch", "stride"))
    G, patches, c = BU.seam_case(seed)
    out, terms = BU.blend_np(patches, A, h0, w0, patch, stride, s, BU.window_np("hann", patch * s))
    worst, bound = BU.seam_excess(out, G, c, patches, int(terms.max()))
    crop, _ = BU.seam_excess(SU.integrate_plain_np(patches, A, h0, w0, patch, stride, s), G, c, patches)
    print(f"seed {seed}: blend {worst:.4f}, crop {crop:.4f}, bound {bound:.4f}, bias range {float(c.max() - c.min()):.4f}")
    assert terms.max() == 4 and worst <= bound < crop
