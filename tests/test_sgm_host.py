"""CPU: semi-global aggregation up to the device -- the numpy float32 restatement (tests/sgm_util.py) and its own properties, the
new header and its binding beside the pinned older ones, every refusal of lft_sgm on the host, and the Python refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from lft_amd import _lib, disparity as Dm, refocus as R, views as V
from lft_amd._lib import LftError

import disparity_util as DU
import sgm_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = -1, -2
P, Q = 1 << 20, 2 << 20                                                       # addresses that are never dereferenced
F = np.float32


def pixel_loop(E, r, p1, p2, guide=None, gain=0.0):
    """L_r by the definition, one pixel and one slope at a time (tiny shapes only)."""
    D, H, W = E.shape
    dy, dx = r
    p1, p2, gain = F(p1), F(p2), F(gain)
    L = np.zeros_like(E)
    ys = range(H) if dy >= 0 else range(H - 1, -1, -1)
    xs = range(W) if dx >= 0 else range(W - 1, -1, -1)
    for y in ys:
        for x in xs:
            qy, qx = y - dy, x - dx
            if not (0 <= qy < H and 0 <= qx < W):
                L[:, y, x] = E[:, y, x]
                continue
            Lq = L[:, qy, qx]
            M = Lq.min()
            p2e = p2 if guide is None else max(p1, F(p2 - F(gain * abs(F(guide[y, x] - guide[qy, qx])))))
            c = F(M + p2e)
            for k in range(D):
                t = min(Lq[k], c)
                near = [Lq[j] for j in (k - 1, k + 1) if 0 <= j < D]
                if near:
                    t = min(t, F(min(near) + p1))
                L[k, y, x] = F(E[k, y, x] + F(t - M))
    return L


def test_restatement_equals_the_definition_pixel_by_pixel():
    rng = np.random.default_rng(0)
    for D, H, W in ((3, 4, 5), (1, 3, 3), (2, 5, 2), (4, 1, 6), (4, 6, 1)):
        E = (rng.integers(0, 9, (D, H, W)) / 8).astype(F) if D != 3 else rng.random((D, H, W)).astype(F)
        g = rng.random((H, W)).astype(F)
        for r in SU.DIRECTIONS:
            assert np.array_equal(SU.path_np(E, r, 0.25, 1.5), pixel_loop(E, r, 0.25, 1.5)), (D, H, W, r)
            assert np.array_equal(SU.path_np(E, r, 0.25, 1.5, g, 3.0), pixel_loop(E, r, 0.25, 1.5, g, 3.0)), (D, H, W, r)
        total = pixel_loop(E, SU.DIRECTIONS[0], 0.25, 1.5)
        for r in SU.DIRECTIONS[1:4]:
            total = total + pixel_loop(E, r, 0.25, 1.5)
        assert np.array_equal(SU.sgm_np(E, 0.25, 1.5, 4), total * F(0.25))


def test_one_slope_returns_the_cost():
    """D = 1: t = L(q) = M, every L_r is E, and S is E added R times in order, times 1/R."""
    E = np.random.default_rng(1).random((1, 9, 11)).astype(F)
    for paths in (4, 8):
        for r in SU.DIRECTIONS[:paths]:
            assert np.array_equal(SU.path_np(E, r, 0.3, 0.9), E)
        total = E.copy()
        for _ in range(paths - 1):
            total = total + E
        S = SU.sgm_np(E, 0.3, 0.9, paths)
        assert S.dtype == F and np.array_equal(S, total * F(1.0 / paths))
        assert float(np.abs(S.astype(np.float64) - E).max()) <= 2.0 ** -23 * float(E.max()) * paths


def test_horizontal_flip_with_four_paths():
    """Flipping E in x swaps L_0 and L_1 and flips L_2 and L_3; L_0 + L_1 commutes, so S flips bit for bit."""
    rng = np.random.default_rng(2)
    for E in (rng.random((5, 13, 17)).astype(F), (rng.integers(0, 9, (4, 9, 6)) / 8).astype(F)):
        mean = float(E.mean())
        assert np.array_equal(SU.sgm_np(E[:, :, ::-1], 0.1 * mean, mean, 4), SU.sgm_np(E, 0.1 * mean, mean, 4)[:, :, ::-1])


def test_constant_patch_scene():
    """Winner-take-all gets none of the patch interior, the restatement all of it and all of the textured interior, for both path
    counts and every penalty pair."""
    L = SU.patch_scene()
    table = R.shift_table(SU.A, SU.SLOPES, "full", "linear")
    E, _ = DU.cost_np(L, table, 2, 1)
    E = E.astype(F)
    wta = np.argmin(E, 0)
    assert SU.SLOPES[SU.K_PLANE] == SU.D_PLANE
    assert not np.any(wta[SU.PATCH_INTERIOR] == SU.K_PLANE)
    textured = SU.mask_of(SU.TEXTURE_INTERIOR) & ~SU.mask_of((slice(SU.PATCH[0] - 2, SU.PATCH[1] + 2),) * 2)
    assert np.all(wta[textured] == SU.K_PLANE)
    mean = float(E.mean())
    for paths in (4, 8):
        for a, b in SU.PENALTIES:
            k = np.argmin(SU.sgm_np(E, a * mean, b * mean, paths), 0)
            assert np.all(k[SU.PATCH_INTERIOR] == SU.K_PLANE), (paths, a, b)
            assert np.all(k[SU.TEXTURE_INTERIOR] == SU.K_PLANE), (paths, a, b)


def test_clamp_bites_counts_both_cases():
    g = np.array([[0.0, 0.1, 1.0], [0.0, 0.0, 0.0]], F)
    assert SU.clamp_bites(g, (0, 1), 0.5, 1.0, 1.0) == (1, 3) and SU.clamp_bites(g, (1, 0), 0.5, 1.0, 1.0) == (1, 2)
    assert SU.clamp_bites(g, (1, 1), 0.5, 1.0, 1.0) == (0, 2) and SU.clamp_bites(g, (-1, 1), 0.5, 1.0, 1.0) == (1, 1)


def test_header_declares_and_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "lft_hip_sgm.h")).read()
    declared = set(re.findall(r"^int\s+(lft_\w+)\s*\(", hdr, flags=re.M))
    assert _lib.SGM_EXPORTS == ("lft_sgm_scratch_bytes", "lft_sgm") and set(_lib.SGM_EXPORTS) == declared
    assert "added beside ABI 5; lft_version unchanged" in " ".join(hdr.split()).replace("Added", "added")
    assert _lib.SGM_MAX_D == 256 and "#define LFT_SGM_MAX_D 256" in hdr
    # the older headers keep their prototypes, and the tables bound from them their contents
    assert len(_lib._SIGS) == 59 and not set(_lib.SGM_EXPORTS) & set(_lib.EXPORTS) and not set(_lib.SGM_EXPORTS) & set(_lib.TEST_EXPORTS)
    assert _lib.VIEW_EXPORTS == ("lft_view_render_scratch_bytes", "lft_view_render") and _lib.VIEW_STREAM_LAST == {"lft_view_render"}
    views_hdr = open(os.path.join(ROOT, "include", "lft_hip_views.h")).read()
    assert set(re.findall(r"^int\s+(lft_\w+)\s*\(", views_hdr, flags=re.M)) == set(_lib.VIEW_EXPORTS)
    assert not set(_lib.SGM_EXPORTS) & set(_lib.STREAM_LAST) and set(_lib.SGM_EXPORTS) <= _lib.OPTIONAL_EXPORTS
    assert _lib.UNITS == ("lft_network", "lft_lightfield", "lft_objective") and "lft_sgm.cuh" in _lib.SOURCES
    for other in ("lft_hip.h", "lft_hip_test.h", "lft_hip_views.h"):
        assert "lft_sgm" not in open(os.path.join(ROOT, "include", other)).read()
    users = [u for u in _lib.UNITS if "lft_sgm.cuh" in open(os.path.join(_lib.CSRC, u + ".hip")).read()]
    assert users == ["lft_lightfield"]
    deps_line = [line for line in open(os.path.join(ROOT, "lft_amd", "_lib.py")) if line.lstrip().startswith("deps =")][0]
    assert "ADDON_HEADERS" in deps_line and "lft_hip_sgm.h" in _lib.ADDON_HEADERS
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in _lib.SGM_EXPORTS:
        assert hasattr(L, name), name
    assert _lib.lib().lft_version() == 5
    # the definition's sentences stand in the header, the kernels' comment and the module docstring
    kernels = open(os.path.join(_lib.CSRC, "lft_sgm.cuh")).read()
    for text in (hdr, kernels, Dm.__doc__):
        flat = " ".join(re.sub(r"^\s*(//|\*)\s?", "", line).replace("`", "").replace("**", "").strip() for line in text.splitlines())
        flat = flat.replace("−", "-").replace("≥", ">=").replace("≤", "<=").replace("·", "*").replace("∈", "in")
        for words in ("It must be finite", "The bit-for-bit promise is for costs >= +0", "each rounded once to fp32", "paths = 4 takes the first four",
                      "r0 = (0,+1), r1 = (0,-1), r2 = (+1,0), r3 = (-1,0)", "r4 = (+1,+1), r5 = (-1,-1), r6 = (+1,-1), r7 = (-1,+1)",
                      "one rounded operation per step, contraction off", "If q lies outside the image: L_r(p,k) = E(p,k)",
                      "over the neighbours that exist", "The scaling is exact for R = 4 and 8", "index: the lowest k on a tie",
                      "Nothing may depend on launch shape, tile or arrival order", "min has none to fix"):
            assert words in flat, words


def test_scratch_query():
    assert _lib.query("lft_sgm_scratch_bytes", 2, 9, 37, 45, 8) == 8 * 2 * 9 * 37 * 45 * 4
    assert _lib.query("lft_sgm_scratch_bytes", 2, 9, 37, 45, 4) == 4 * 2 * 9 * 37 * 45 * 4
    assert _lib.query("lft_sgm_scratch_bytes", 0, 9, 37, 45, 8) == 0 and _lib.query("lft_sgm_scratch_bytes", 1, 256, 3, 0, 4) == 0
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    for args, rc in (((1, 9, 4, 4, 5), ERR_ARG), ((1, 9, 4, 4, 0), ERR_ARG), ((1, 0, 4, 4, 8), ERR_ARG), ((1, 257, 4, 4, 8), ERR_ARG),
                     ((-1, 3, 4, 4, 8), ERR_SHAPE), ((1, 3, -4, 4, 8), ERR_SHAPE), ((1 << 20, 64, 1 << 10, 1 << 10, 8), ERR_SHAPE),
                     ((1, 1, 1 << 16, 1 << 16, 4), ERR_SHAPE)):
        assert L.lft_sgm_scratch_bytes(*args, ctypes.byref(n)) == rc, args
        assert L.lft_last_error().decode().startswith("lft_sgm:")
    assert L.lft_sgm_scratch_bytes(1, 3, 4, 4, 8, None) == ERR_ARG
    with pytest.raises(LftError, match=r"lft_sgm_scratch_bytes failed \(code -1\)"):
        _lib.query("lft_sgm_scratch_bytes", 1, 0, 4, 4, 8)
    with pytest.raises(LftError, match="does not take its stream last"):
        _lib.enqueue("lft_sgm_scratch_bytes", "cuda:0", 1, 1, 1, 1, 8)
    assert "lft_sgm" in _lib.ADDON_STREAM_LAST and "lft_view_render" in _lib.ADDON_STREAM_LAST


GOOD = dict(cost=P, B=1, D=9, H=10, W=12, C=3, slopes=P + 8192, paths=8, p1=0.1, p2=1.0, guide=None, gain=0.0, stack=None, scratch=Q,
            disparity=Q + (1 << 19), confidence=Q + (2 << 19), index=Q + (3 << 19), aggregated=None, aif=None, aif_class=_lib.LF_FLOAT32, stream=None)


def sgm_raw(**kw):
    unknown = set(kw) - set(GOOD)
    assert not unknown, unknown
    return _lib.lib().lft_sgm(*{**GOOD, **kw}.values())


def test_every_refusal_comes_before_any_device_work():
    """Each call is answered on the host (this runs without a GPU): its code, and a message that starts with the entry point."""
    L = _lib.lib()
    inf, nan = float("inf"), float("nan")
    cases = [
        (dict(paths=0), ERR_ARG, "0 paths"), (dict(paths=5), ERR_ARG, "5 paths"), (dict(paths=16), ERR_ARG, "16 paths"), (dict(paths=-4), ERR_ARG, "paths"),
        (dict(D=0), ERR_ARG, "0 slopes outside 1 .. 256"), (dict(D=257), ERR_ARG, "257 slopes outside 1 .. 256"), (dict(D=-1), ERR_ARG, "slopes"),
        (dict(C=0), ERR_ARG, "channels"), (dict(C=5), ERR_ARG, "channels"),
        (dict(p1=-0.5), ERR_ARG, "must be finite and >= 0"), (dict(p2=-1.0), ERR_ARG, "must be finite and >= 0"), (dict(gain=-1.0, guide=P), ERR_ARG, "must be finite and >= 0"),
        (dict(p1=nan), ERR_ARG, "must be finite"), (dict(p2=inf), ERR_ARG, "must be finite"), (dict(gain=nan, guide=P), ERR_ARG, "must be finite"),
        (dict(p1=inf, p2=inf), ERR_ARG, "must be finite"),
        (dict(p1=1.5), ERR_ARG, "p2 1 below p1 1.5"),
        (dict(gain=0.5), ERR_ARG, "without a guide"),
        (dict(aif=Q + (5 << 19)), ERR_ARG, "without a stack"),
        (dict(aif_class=_lib.LF_FLOAT64), ERR_ARG, "all-in-focus class"), (dict(aif_class=9), ERR_ARG, "all-in-focus class"),
        (dict(B=-1), ERR_SHAPE, "negative size"), (dict(H=-3), ERR_SHAPE, "negative size"), (dict(W=-4), ERR_SHAPE, "negative size"),
        (dict(cost=None), ERR_ARG, "null pointer"), (dict(slopes=None), ERR_ARG, "null pointer"), (dict(scratch=None), ERR_ARG, "null pointer"),
        (dict(disparity=None), ERR_ARG, "null pointer"), (dict(confidence=None), ERR_ARG, "null pointer"), (dict(index=None), ERR_ARG, "null pointer"),
        (dict(scratch=Q + 2), ERR_ARG, "scratch must be 4-byte aligned"), (dict(scratch=Q + 2, paths=3), ERR_ARG, "paths"),
        (dict(B=1 << 20, H=1 << 10, W=1 << 10), ERR_SHAPE, "2^40"), (dict(D=1, H=1 << 16, W=1 << 16), ERR_SHAPE, "2^31 pixels"),
    ]
    for kw, rc, words in cases:
        L.lft_refocus(None, 99, 1, 1, 1, 1, 1, None, None, 1, 1, None, 0, None)              # leaves another call's message behind
        assert sgm_raw(**kw) == rc, kw
        msg = L.lft_last_error().decode()
        assert msg.startswith("lft_sgm:") and words in msg and "99" not in msg, (kw, msg)
    # the ends of the ranges are accepted: what refuses these calls is the misaligned scratch behind them
    for kw in (dict(D=256), dict(D=1), dict(paths=4), dict(p1=0.0, p2=0.0), dict(p1=1.0, p2=1.0), dict(C=1), dict(C=4), dict(gain=2.0, guide=P),
               dict(aif=P, stack=P), dict(aif_class=_lib.LF_UINT8)):
        assert sgm_raw(scratch=Q + 2, **kw) == ERR_ARG and b"scratch" in L.lft_last_error(), kw
    # empty shapes are no error and no work, null pointers included; the values are still judged
    for kw in (dict(B=0), dict(H=0), dict(W=0)):
        assert sgm_raw(cost=None, slopes=None, scratch=None, disparity=None, confidence=None, index=None, **kw) == 0, kw
        assert sgm_raw(paths=6, **kw) == ERR_ARG and sgm_raw(p1=2.0, **kw) == ERR_ARG, kw


def test_python_refusals_need_no_device():
    cost, sl = torch.zeros(3, 6, 7), [-1.0, 0.0, 1.0]
    with pytest.raises(LftError, match="no CPU path"):
        Dm.regularize(cost, sl, 0.1, 1.0)
    with pytest.raises(LftError, match="torch tensor"):
        Dm.regularize(np.zeros((3, 6, 7), np.float32), sl, 0.1, 1.0)
    for bad in (cost.double(), torch.zeros(6, 7), torch.zeros(1, 1, 3, 6, 7), torch.zeros(0, 6, 7)):
        with pytest.raises(LftError, match="cost"):
            Dm.regularize(bad, sl, 0.1, 1.0)
    for kw, words in ((dict(paths=5), "paths"), (dict(paths=True), "paths"), (dict(paths=8.5), "paths"), (dict(p1=-0.1), "p1"), (dict(p1=float("nan")), "p1"),
                      (dict(p2=float("inf")), "p2"), (dict(p2=1e39), "p2"), (dict(p1=2.0), "below p1"), (dict(p1="a"), "p1"), (dict(edge_gain=-1.0), "edge_gain"),
                      (dict(edge_gain=0.5), "needs a guide"), (dict(aif_dtype=torch.uint8), "without a stack"),
                      (dict(aif_dtype=torch.float16, stack=torch.zeros(3, 6, 7)), "aif_dtype"), (dict(guide=torch.zeros(7, 6)), "guide"),
                      (dict(guide=torch.zeros(6, 7).double()), "guide"), (dict(guide=np.zeros((6, 7), np.float32)), "guide"),
                      (dict(stack=torch.zeros(3, 6, 7, 5)), "stack"), (dict(stack=torch.zeros(2, 6, 7)), "stack"), (dict(stack=torch.zeros(3, 6, 7, dtype=torch.uint8)), "stack")):
        with pytest.raises(LftError, match=words):
            Dm.regularize(cost, sl, **{**dict(p1=0.1, p2=1.0), **kw})
    for slopes in ([0.0, 1.0], [1.0, 0.0, 2.0], [], [0.0, np.nan, 1.0]):
        with pytest.raises(LftError, match="slopes"):
            Dm.regularize(cost, slopes, 0.1, 1.0)
    with pytest.raises(LftError, match="at most 256"):
        Dm.regularize(torch.zeros(257, 2, 2), np.arange(257.0), 0.1, 1.0)
    with pytest.raises(LftError, match="guide"):
        Dm.regularize(torch.zeros(2, 3, 6, 7), sl, 0.1, 1.0, guide=torch.zeros(6, 7))                 # a batch wants [B, H, W]
    # disparity(regularize=...): the dict and its values are judged before the light field leaves the host
    lf = torch.zeros(3, 3, 6, 6)
    for how, words in (("sgm", "regularize must be None or a dict"), (dict(p1=0.1), "regularize must be None or a dict"), (dict(p1=0.1, p2=1.0, path=4), "regularize must be None or a dict"),
                       (dict(p1=0.1, p2=1.0, paths=6), "paths"), (dict(p1=1.0, p2=0.1), "below p1"), (dict(p1=0.1, p2=1.0, edge_gain=1.0), "needs a guide")):
        with pytest.raises(LftError, match=words):
            Dm.disparity(lf, sl, regularize=how)
    with pytest.raises(LftError, match="no CPU path"):
        Dm.disparity(lf, sl, regularize=dict(p1=0.1, p2=1.0))
    with pytest.raises(LftError, match="radius"):
        Dm.disparity(lf, sl, radius=9, regularize=dict(p1=0.1, p2=1.0))
    with pytest.raises(LftError, match="no CPU path"):
        V.leave_one_out(lf, sl, regularize=dict(p1=0.1, p2=1.0))
    for bad in ((-0.1, 1.0), (2.0, 1.0), (0.1, float("nan"))):
        with pytest.raises(LftError, match="p1_rel"):
            Dm.penalties_from_cost(cost, *bad)
    with pytest.raises(LftError, match="torch tensor"):
        Dm.penalties_from_cost(np.zeros(3))
    assert Dm.penalties_from_cost(torch.full((2, 3, 4), 2.0)) == (0.2, 2.0) and Dm.penalties_from_cost(torch.zeros(0, 3), 0.5, 4.0) == (0.0, 0.0)
    Dm.clear_cache()
