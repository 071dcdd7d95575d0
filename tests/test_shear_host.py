"""CPU: per-patch disparity compensation by integer shear up to the device -- the new header and its binding, shear_limit, every
refusal of the three entry points on the host, every Python refusal, and on the restatement alone (tests/shear_util.py): k = 0 is
today's rule, divide -> pixel replication -> integrate returns the replicated scene, and on the two-plane scene every patch whose
central region lies in one plane votes that plane's slope."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import _lib, refocus as R, scene as S
from lft_amd._lib import LftError

import disparity_util as DU
import shear_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = -1, -2
P, Q, T = 1 << 20, 2 << 20, 3 << 20                     # addresses that are never dereferenced
NAMES = ("lft_scene_divide_shear", "lft_scene_integrate_shear", "lft_shear_vote")
SHAPES = [(5, 16, 4, 13, 21, 2), (3, 8, 4, 9, 11, 4), (2, 8, 4, 7, 9, 2), (1, 8, 4, 9, 9, 2), (4, 12, 4, 10, 17, 2), (3, 8, 4, 4, 4, 2)]   # A, patch, stride, h0, w0, s


DEEP = (3, 16, 4, 5, 6, 2)                              # the border is deeper than the view: the sheared cut folds past one reflection


def random_shear(rng, A, patch, stride, N):
    kmax = SU.kmax_np(A, patch, stride)
    return rng.integers(-kmax - 1, kmax + 2, N)         # both clamps, and fold past one reflection


# ---- 1. the header and its binding ----
def test_header_declares_library_exports_and_binding_holds_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "lft_hip_shear.h")).read()
    assert tuple(re.findall(r"^int\s+(lft_\w+)\s*\(", hdr, flags=re.M)) == NAMES
    assert "Added beside ABI 5; lft_version unchanged" in hdr and "#define LFT_SHEAR_MAX 16" in hdr
    assert _lib.SHEAR_EXPORTS == NAMES and _lib.ADDON_HEADERS["lft_hip_shear.h"] == "SHEAR_" and _lib.SHEAR_MAX == 16 == SU.SHEAR_MAX
    assert list(_lib.ADDON_HEADERS)[-1] == "lft_hip_focal.h"
    assert set(NAMES) <= _lib.ADDON_STREAM_LAST and set(NAMES) <= _lib.OPTIONAL_EXPORTS
    assert len(_lib._SIGS) == 59 and not set(NAMES) & set(_lib.EXPORTS) and len(_lib.UNITS) == 3
    from ctypes import c_float, c_int, c_void_p
    assert _lib._ADDON_SIGS["lft_scene_divide_shear"] == (c_int, [c_void_p] * 3 + [c_int] * 5 + [c_void_p])
    assert _lib._ADDON_SIGS["lft_scene_integrate_shear"] == (c_int, [c_void_p] * 3 + [c_int] * 6 + [c_void_p])
    assert _lib._ADDON_SIGS["lft_shear_vote"] == (c_int, [c_void_p] * 3 + [c_int] * 5 + [c_float] + [c_void_p] * 3)
    assert "lft_shear.cuh" in _lib.SOURCES
    assert [u for u in _lib.UNITS if '"lft_shear.cuh"' in open(os.path.join(_lib.CSRC, u + ".hip")).read()] == ["lft_lightfield"]
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(L, n) for n in NAMES) and _lib.lib().lft_version() == 5
    # the definition's sentences stand in the header, the kernel file's comment and the module docstring
    kernel = open(os.path.join(_lib.CSRC, "lft_shear.cuh")).read()
    for text in (hdr, kernel, S.__doc__):
        flat = " ".join(re.sub(r"^\s*(//|\*|-)\s?", "", line).replace("`", "").replace("**", "").strip() for line in text.splitlines())
        flat = flat.replace("−", "-").replace("≥", ">=").replace("≤", "<=").replace("·", "*").replace("Δu", "du").replace("Δv", "dv").replace(" // ", " / ")
        for words in ("A shear by a whole number k of LR pixels per view step is lossless", "No pixel is interpolated on either side",
                      "kmax = LFT_SHEAR_MAX if R = 0, else min(LFT_SHEAR_MAX, bdr / R)", "Every kernel clamps k_n into [-kmax, kmax] itself",
                      "so k = d aligns the views", "ey = ku*stride + y, and ex likewise",
                      "today's test, on the unsheared coordinates",
                      "scene[u*h0 + fold(ey - bdr + k_n*du, h0), v*w0 + fold(ex - bdr + k_n*dv, w0)]",
                      "m = i mod 2n (non-negative), then m if m < n, else 2n-1-m", "This is reflect_idx continued to any integer",
                      "at row bdr*s + i - s*k_n*du and column bdr*s + j - s*k_n*dv", "they never touch a zero-filled pixel",
                      "clamped index equal to j, and confidence finite and >= min_confidence", "where j* has the largest count",
                      "On a tie the smallest |slope| wins, then the smaller slope", "If every count is 0 the result is 0",
                      "Counts are integers, so arrival order cannot matter"):
            assert words in flat, words


def test_shear_limit():
    assert [S.shear_limit(A) for A in range(1, 12)] == [16, 8, 8, 4, 4, 2, 2, 2, 2, 1, 1]
    for A in range(1, 12):
        for patch, stride in ((32, 16), (16, 4), (8, 4), (12, 4), (16, 8), (64, 2), (8, 8)):
            assert S.shear_limit(A, patch, stride) == SU.kmax_np(A, patch, stride), (A, patch, stride)
    assert S.shear_limit(5, 64, 2) == 15 and S.shear_limit(3, 64, 2) == 16 and S.shear_limit(5, 8, 8) == 0 and S.shear_limit(1, 8, 8) == 16
    for bad in ((0, 32, 16), (5, 16, 32), (5, 16, 0)):
        with pytest.raises(LftError, match="shear_limit"):
            S.shear_limit(*bad)


# ---- 2. every refusal of the three entry points is answered on the host ----
def test_every_c_refusal_comes_before_any_device_work():
    _lib.build()
    L = _lib.lib()

    def refused(name, args, rc, words):
        L.lft_scene_counts(1, 1, 1, 1, None, None)      # leaves another call's message behind
        assert getattr(L, name)(*args) == rc, (name, args)
        msg = L.lft_last_error().decode()
        assert words in msg, (name, args, msg)
        return msg

    good_d = [P, Q, T, 5, 64, 64, 32, 16, None]         # scene, shear, patches, A, h0, w0, patch, stride, stream
    good_i = [P, Q, T, 5, 64, 64, 32, 16, 2, None]      # ... s, stream
    for name, good in (("lft_scene_divide_shear", good_d), ("lft_scene_integrate_shear", good_i)):
        change = lambda **kw: [kw.get(k, v) for k, v in zip(("a", "b", "c", "A", "h0", "w0", "patch", "stride", "s" if len(good) == 10 else "st", "st"), good)]
        for k in "abc":
            assert refused(name, change(**{k: None}), ERR_ARG, "null pointer").startswith(name + ":")
        refused(name, change(A=0), ERR_ARG, name + ": angRes 0")
        # lft_scene_divide's tilings, with its words
        for kw, words in ((dict(stride=33), "bad scene tiling"), (dict(stride=0), "bad scene tiling"), (dict(h0=0), "bad scene tiling"),
                          (dict(patch=0), "bad scene tiling"), (dict(h0=8), "smaller than one patch")):
            want = refused("lft_scene_divide", [P, T] + change(**kw)[3:8] + [None], ERR_SHAPE, words)
            assert refused(name, change(**kw), ERR_SHAPE, words) == want
        refused(name, change(patch=31), ERR_SHAPE, name + ": patch - stride = 15 is odd")
        # the pointers come first, then the sizes
        refused(name, change(a=None, stride=0), ERR_ARG, "null pointer")
    refused("lft_scene_integrate_shear", good_i[:8] + [0, None], ERR_ARG, "scale factor 0")
    # each call is judged by its own launch: divide by the rows of a patch mosaic and the number of patches, integrate by the rows of
    # the SR scene mosaic -- a scene of many rows is refused for integrate alone
    refused("lft_scene_divide_shear", good_d[:3] + [4096, 64, 64, 32, 16, None], ERR_SHAPE, "patch mosaics of 131072 rows")
    refused("lft_scene_divide_shear", good_d[:3] + [5, 4800, 4800, 32, 16, None], ERR_SHAPE, "300 x 300 patches need more than 65535 blocks")
    refused("lft_scene_integrate_shear", good_i[:3] + [1, 30000, 64, 32, 16, 4, None], ERR_SHAPE, "an SR scene mosaic of 120000 rows needs more than 65535 blocks")
    refused("lft_scene_integrate_shear", good_i[:3] + [4096, 64, 64, 32, 16, 2, None], ERR_SHAPE, "an SR scene mosaic of 524288 rows")

    name = "lft_shear_vote"
    keys = ("index", "confidence", "slopes", "B", "H", "W", "D", "margin", "min_confidence", "counts", "shear", "stream")
    good = dict(zip(keys, (P, Q, T, 4, 32, 32, 9, 8, 0.5, P + (1 << 18), Q + (1 << 18), None)))
    change = lambda **kw: [kw.get(k, v) for k, v in good.items()]
    for k in ("index", "confidence", "slopes", "counts", "shear"):
        assert refused(name, change(**{k: None}), ERR_ARG, "null pointer").startswith(name + ":")
    for kw, words in ((dict(D=0), "0 slopes outside 1 .. 33"), (dict(D=34), "34 slopes outside 1 .. 33"), (dict(margin=-1), "margin -1"),
                      (dict(margin=16), "margin 16 leaves nothing"), (dict(margin=12, W=24), "margin 12 leaves nothing"),
                      (dict(margin=1 << 30), "leaves nothing"), (dict(B=-1), "B = -1"), (dict(H=0), "maps of 0 x 32"), (dict(W=-3), "maps of 32 x -3")):
        refused(name, change(**kw), ERR_SHAPE, words)
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(name, change(min_confidence=bad), ERR_ARG, "min_confidence")
    refused(name, change(index=None, D=0), ERR_ARG, "null pointer")
    # B = 0 is no error and no work; the other rules are still judged
    assert L.lft_shear_vote(*change(B=0)) == 0
    refused(name, change(B=0, D=40), ERR_SHAPE, "slopes outside")
    assert L.lft_shear_vote(*change(B=0, margin=15, D=33, min_confidence=-1.0)) == 0


# ---- 3. Python refusals need no device ----
def test_python_refusals_need_no_device():
    A, patch, stride = 5, 32, 16
    scene = torch.zeros(A * 48, A * 64)                 # 3 x 4 patches
    assert S.scene_counts(48, 64) == (3, 4)
    k = torch.zeros(12, dtype=torch.int32)
    bad_shears = (k.long(), k.float(), k[:11], k.reshape(3, 4), k.numpy(), [0] * 12)
    for bad in bad_shears:
        with pytest.raises(LftError, match=r"shear must be an int32 tensor of shape \[12\]"):
            S.divide(scene, A, patch, stride, shear=bad)
        with pytest.raises(LftError, match=r"shear must be an int32 tensor of shape \[12\]"):
            S.integrate(torch.zeros(12, 1, 8, 8), A, 48, 64, 2, patch, stride, shear=bad)
    with pytest.raises(LftError, match="shear is on meta, the scene on cpu"):
        S.divide(scene, A, patch, stride, shear=k.to("meta"))
    with pytest.raises(LftError, match="shear is on meta, the scene on cpu"):
        S.integrate(torch.zeros(12, 1, 8, 8), A, 48, 64, 2, patch, stride, shear=k.to("meta"))
    # everything right: the device is asked for last
    with pytest.raises(LftError, match="on a HIP device"):
        S.divide(scene, A, patch, stride, shear=k)
    with pytest.raises(LftError, match="on a HIP device"):
        S.integrate(torch.zeros(12, 1, 8, 8), A, 48, 64, 2, patch, stride, shear=k)
    with pytest.raises(LftError, match="on a HIP device"):
        S.divide(scene, A, patch, stride)
    # the whole scene
    net = SimpleNamespace(angRes=A, factor=2)
    with pytest.raises(LftError, match="shear together with ensemble is not supported"):
        S.super_resolve_scene(net, scene, shear=1, ensemble="flips")
    with pytest.raises(LftError, match="shear together with ensemble is not supported"):
        S.super_resolve_scene(net, scene, shear="auto", ensemble="dihedral")
    for bad in ("Auto", "2", 1.0, True, [1]):
        with pytest.raises(LftError, match="shear must be None, an integer, an int32 tensor or auto"):
            S.super_resolve_scene(net, scene, shear=bad)
    with pytest.raises(LftError, match=r"shear 5: kmax is 4 for angRes 5, patch 32, stride 16; a patch of at least 36 at this stride, or a stride of at most 12 "
                                       "at this patch, would allow it"):
        S.super_resolve_scene(net, scene, shear=5)
    with pytest.raises(LftError, match="shear -6: kmax is 4 .* a patch of at least 40 at this stride, or a stride of at most 8 at this patch"):
        S.super_resolve_scene(net, scene, shear=-6)
    assert S.shear_limit(5, 36, 16) == 5 == S.shear_limit(5, 32, 12) and S.shear_limit(5, 34, 16) == 4 == S.shear_limit(5, 32, 14)
    # where no stride could allow it, only the patch is offered
    with pytest.raises(LftError) as e:
        S.check_shear_limit(3, 5, 8, 4)
    assert "kmax is 1" in str(e.value) and "a patch of at least 16 at this stride would allow it" in str(e.value) and "or a stride" not in str(e.value)
    assert S.shear_limit(5, 16, 4) == 3
    # a tiling the sheared kernels refuse has no limit either
    for odd in ((5, 35, 16), (5, 32, 13)):
        with pytest.raises(LftError, match="is odd"):
            S.shear_limit(*odd)
    with pytest.raises(LftError, match="is odd"):
        S.super_resolve_scene(net, scene, patch=31, shear=0)
    with pytest.raises(LftError, match="shear 17: kmax is 4 .* no patch or stride allows more than 16"):
        S.super_resolve_scene(net, scene, shear=17)
    with pytest.raises(LftError, match=r"shear must be an int32 tensor of shape \[12\]"):
        S.super_resolve_scene(net, scene, shear=k.long())
    for good in (4, -4, 0, k, "auto"):
        with pytest.raises(LftError, match="on a HIP device"):
            S.super_resolve_scene(net, scene, shear=good)
    # the estimate
    for bad, ang in ((torch.zeros(12, 160, 160), 5), (torch.zeros(12, 1, 160, 150), 5), (torch.zeros(12, 1, 160, 160), 3), (torch.zeros(12, 2, 160, 160), 5), (None, 5)):
        with pytest.raises(LftError, match=r"patches must be a batch \[N, 1, A\*patch, A\*patch\]"):
            S.estimate_shear(bad, ang)
    patches = torch.zeros(12, 1, 160, 160)
    for kw, words in ((dict(max_shear=-1), "max_shear"), (dict(max_shear=1.5), "max_shear"), (dict(margin=16), "margin"), (dict(margin=-1), "margin"),
                      (dict(stride=40), "shear_limit"), (dict(radius=9), "radius")):
        with pytest.raises(LftError, match=words):
            S.estimate_shear(patches, 5, **kw)
    with pytest.raises(LftError, match="no CPU path"):
        S.estimate_shear(patches, 5)
    idx, conf, sl = torch.zeros(2, 8, 8, dtype=torch.int32), torch.zeros(2, 8, 8), torch.arange(-1, 2, dtype=torch.int32)
    for args, words in (((idx.long(), conf, sl), "the index must be"), ((idx, conf.double(), sl), "the confidence must be"), ((idx, conf, sl.float()), "the slopes must be"),
                        ((idx, conf[:1], sl), "do not vote together"), ((idx, conf.to("meta"), sl), "on one device"), ((idx, conf, sl), "no CPU path")):
        with pytest.raises(LftError, match=words):
            S.vote(*args, margin=2)
    # the tools' option
    assert S.parse_shear(None) is None and S.parse_shear("auto") == "auto" and S.parse_shear("-3") == -3
    with pytest.raises(LftError, match="--shear takes auto or a whole number"):
        S.parse_shear("2.5")
    with pytest.raises(LftError, match="kmax is 4"):
        S.check_shear_limit(5, 5, 32, 16)


# ---- 3b. every call site hands `shear` on, in its own place ----
def test_call_sites_pass_shear_through(monkeypatch):
    """evaluate.test_scene / test / test_sets, colour.super_resolve_lf and the two tools reach super_resolve_scene through chains of
    positional arguments: each is run with every step around it replaced, and what arrives is compared."""
    import sys
    from lft_amd import colour, datasets, evaluate, metrics
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shear_sets
    import super_resolve
    seen = []

    def fake_scene(net, scene, patch=32, stride=16, max_batch=64, ensemble=None, shear=None):
        seen.append(dict(patch=patch, stride=stride, max_batch=max_batch, ensemble=ensemble, shear=shear))
        return torch.zeros(4, 4)

    monkeypatch.setattr(S, "super_resolve_scene", fake_scene)
    monkeypatch.setattr(metrics, "cal_metrics", lambda net, hr, sr, ssim_range=2.0: (30.0, 0.9))
    net = torch.nn.Linear(1, 1)
    net.angRes, net.factor = 2, 2
    lr, hr = torch.zeros(4, 4), torch.zeros(8, 8)
    want = dict(patch=16, stride=8, max_batch=64, ensemble=None, shear="auto")
    evaluate.test_scene(net, lr, hr, 16, 8, shear="auto")
    assert seen.pop() == want
    evaluate.test(net, [(lr, hr)], 16, 8, shear=3, sharded=False)
    assert seen.pop() == dict(want, shear=3)
    monkeypatch.setattr(datasets, "MultiTestSetDataLoader", lambda args: (["SetA"], [[(lr[None], hr[None])]], 1))
    args = SimpleNamespace(patch_size_for_test=16, stride_for_test=8)
    k = torch.zeros(1, dtype=torch.int32)
    assert evaluate.test_sets(net, args, log=lambda *_: None, shear=k) == {"SetA": (30.0, 0.9)}
    assert seen.pop()["shear"] is k and not seen
    evaluate.test_sets(net, args, log=lambda *_: None, ensemble="flips")
    assert seen.pop() == dict(want, ensemble="flips", shear=None)
    # the colour path
    monkeypatch.setattr(colour, "_field", lambda lf, A, dev: lf)
    monkeypatch.setattr(colour, "luma", lambda t, A: lr)
    monkeypatch.setattr(colour, "merge", lambda t, sr_y, A, s, out_dtype: sr_y)
    colour.super_resolve_lf(net, torch.zeros(2, 2, 2, 2, 3), 16, 8, shear=-2)
    assert seen.pop() == dict(want, shear=-2)
    colour.super_resolve_lf(net, torch.zeros(2, 2, 2, 2, 3), 16, 8, 7, "flips")
    assert seen.pop() == dict(want, max_batch=7, ensemble="flips", shear=None)
    # tools/super_resolve.py: the option is judged before the model is loaded, then handed to colour.super_resolve_lf
    got = {}
    monkeypatch.setattr(super_resolve, "load_model", lambda a, dev: got.setdefault("loaded", True) and net)
    monkeypatch.setattr(super_resolve, "load_field", lambda path, A, dev: "lf")
    monkeypatch.setattr(super_resolve, "write_views", lambda *a, **kw: [])
    monkeypatch.setattr(colour, "super_resolve_lf", lambda net, lf, patch, stride, ensemble=None, shear=None: got.update(patch=patch, stride=stride, shear=shear)
                        or torch.zeros(2, 2, 4, 4, 3))
    base = ["--path_pre_pth", "x", "--lf", "y", "--out_dir", "unused", "--angRes", "5", "--scale_factor", "2"]
    with pytest.raises(LftError, match="kmax is 4"):
        super_resolve.main(base + ["--shear", "5"])
    with pytest.raises(LftError, match="--shear takes auto or a whole number"):
        super_resolve.main(base + ["--shear", "some"])
    assert not got
    # tools/shear_sets.py: the same, for the test sets
    assert shear_sets.parse([])[1] == "auto" and shear_sets.parse(["--shear", "none"])[1] is None and shear_sets.parse(["--shear", "-4"])[1] == -4
    assert shear_sets.parse(["--shear", "6", "--patch_size_for_test", "40"])[1] == 6
    with pytest.raises(LftError, match="kmax is 4"):
        shear_sets.parse(["--shear", "6"])
    with pytest.raises(LftError, match="--shear takes auto or a whole number"):
        shear_sets.parse(["--shear", "1.5"])


# ---- 4. the restatement alone ----
@pytest.mark.parametrize("A,patch,stride,h0,w0,s", SHAPES)
def test_k0_is_todays_rule(A, patch, stride, h0, w0, s):
    rng = np.random.default_rng([1, A, h0, w0])
    scene = rng.random((A * h0, A * w0), dtype=np.float32)
    N = int(np.prod(SU.counts_np(h0, w0, patch, stride)))
    assert np.array_equal(SU.divide_np(scene, A, patch, stride, np.zeros(N, int)), SU.divide_plain_np(scene, A, patch, stride))
    sr = rng.random((N, A * patch * s, A * patch * s), dtype=np.float32)
    assert np.array_equal(SU.integrate_np(sr, A, h0, w0, patch, stride, s, np.zeros(N, int)), SU.integrate_plain_np(sr, A, h0, w0, patch, stride, s))
    # fold continues reflect_idx
    for n in (1, 2, 7):
        i = np.arange(-n, 2 * n)
        assert np.array_equal(SU.fold(i, n), SU.reflect(i, n))
        far = np.arange(-9 * n, 9 * n)
        assert np.array_equal(SU.fold(far, n), SU.fold(far + 2 * n, n)) and SU.fold(far, n).min() == 0 and SU.fold(far, n).max() == n - 1


@pytest.mark.parametrize("A,patch,stride,h0,w0,s", SHAPES + [DEEP])
def test_round_trip_through_pixel_replication_is_exact(A, patch, stride, h0, w0, s):
    rng = np.random.default_rng([2, A, h0, w0])
    scene = rng.random((A * h0, A * w0), dtype=np.float32)
    N = int(np.prod(SU.counts_np(h0, w0, patch, stride)))
    for _ in range(3):
        k = random_shear(rng, A, patch, stride, N)
        back = SU.integrate_np(SU.replicate(SU.divide_np(scene, A, patch, stride, k), s), A, h0, w0, patch, stride, s, k)
        assert np.array_equal(back, SU.replicate(scene, s))
    if (A, patch, stride, h0, w0, s) == DEEP:
        assert 2 * ((patch - stride) // 2) > h0 and SU.fold(np.array([-12, 16]), h0).tolist() == [1, 3]
    # a shear beyond the limit is the limit's
    kmax = SU.kmax_np(A, patch, stride)
    assert np.array_equal(SU.divide_np(scene, A, patch, stride, np.full(N, kmax + 5)), SU.divide_np(scene, A, patch, stride, np.full(N, kmax)))


@pytest.mark.parametrize("d", [-2, 3])
def test_the_true_shear_aligns_the_views(d):
    A, patch, stride, h0, w0 = 5, 16, 4, 13, 21
    scene = SU.translated_scene(A, h0, w0, d)
    N = int(np.prod(SU.counts_np(h0, w0, patch, stride)))
    k = np.full(N, d)
    views = SU.patch_views(SU.divide_np(scene, A, patch, stride, k), A)[..., 0]
    ok = SU.patch_views(SU.inside_np(A, h0, w0, patch, stride, k), A)[..., 0]
    centre = np.broadcast_to(views[:, A // 2, A // 2][:, None, None], views.shape)
    assert ok.reshape(N, -1).any(1).all() and np.array_equal(views[ok], centre[ok])
    plain = SU.patch_views(SU.divide_np(scene, A, patch, stride, np.zeros(N, int)), A)[..., 0]
    assert not np.array_equal(plain[ok], centre[ok])


def two_plane_maps(patches, A, K, radius=2):
    """index and confidence [N, P, P] of the restated sweep (tests/disparity_util.py) over the whole-number slopes -K .. K, seen from
    the view (u0, u0) with nearest samples: what estimate_shear asks lft_disparity for."""
    slopes = [float(k) for k in range(-K, K + 1)]
    table = R.shift_table(A, slopes, "full", "nearest", (A // 2, A // 2))
    index, conf = [], []
    for views in SU.patch_views(patches, A):
        E, _ = DU.cost_np(views, table, R.TAPS["nearest"], radius)
        k, _, c = DU.pick_np(E, slopes, np.float64)
        index.append(k)
        conf.append(c.astype(np.float32))
    return np.stack(index), np.stack(conf)


def test_two_plane_scene_votes_each_planes_slope():
    T = SU.TWO_PLANES
    A, patch, stride = T["A"], T["patch"], T["stride"]
    scene = SU.two_plane_scene(**T)
    N = int(np.prod(SU.counts_np(T["h0"], T["w0"], patch, stride)))
    K = SU.kmax_np(A, patch, stride)
    assert (N, K) == (15, 4)
    index, conf = two_plane_maps(SU.divide_np(scene, A, patch, stride, np.zeros(N, int)), A, K)
    shear, counts = SU.vote_np(index, conf, np.arange(-K, K + 1), (patch - stride) // 2, 0.5)
    want = SU.one_plane_patches(**T)
    assert len(want) == 12 and sorted(set(want.values())) == [-1, 2]
    print("votes per patch:", shear.tolist(), "pixels that voted:", counts.sum(1).tolist())
    for n, d in want.items():
        assert shear[n] == d, (n, shear[n], d, counts[n])
        assert counts[n].sum() >= stride * stride // 2                       # the vote is no accident of a few pixels
    # the vote's rules: ties, an empty vote, a confidence that is not finite, an index outside the slopes
    idx = np.array([[[0, 2], [0, 2]], [[1, 1], [0, 0]], [[-5, 9], [9, 1]], [[1, 1], [1, 1]]], dtype=np.int32)
    cf = np.ones((4, 2, 2), dtype=np.float32)
    cf[3] = [[np.nan, np.inf], [0.25, -1.0]]
    sh, ct = SU.vote_np(idx, cf, np.array([-1, 0, 1]), 0, 0.5)
    assert sh.tolist() == [-1, 0, 1, 0] and ct.tolist() == [[2, 0, 2], [2, 2, 0], [1, 1, 2], [0, 0, 0]]
    assert SU.vote_np(idx, cf, np.array([-3, 1, 2]), 0, 0.5)[0].tolist() == [2, 1, 2, 0]
