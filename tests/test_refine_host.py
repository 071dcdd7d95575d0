"""CPU: the refinement of a disparity map up to the device -- the new header and its binding, every refusal of the three entry
points on the host, every Python refusal, the view positions, the weight table, and the restatements of tests/refine_util.py against
the definitions themselves."""
import ctypes
import os
import re
from ctypes import c_float, c_int, c_void_p

import numpy as np
import pytest
import torch

from lft_amd import _lib, refine as R
from lft_amd._lib import LftError

import refine_util as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = -1, -2
NAMES = ("lft_disp_check", "lft_disp_fill", "lft_disp_wmedian")
P = [n << 20 for n in range(1, 8)]                      # addresses that are never dereferenced


# ---- 1. the header and its binding ----
def test_header_declares_the_exports_and_the_binding_holds_them():
    hdr = open(os.path.join(ROOT, "include", "lft_hip_refine.h")).read()
    assert tuple(re.findall(r"^int\s+(lft_\w+)\s*\(", hdr, flags=re.M)) == NAMES
    assert "Added beside ABI 5; lft_version unchanged" in hdr
    assert _lib.REFINE_EXPORTS == NAMES and _lib.ADDON_HEADERS["lft_hip_refine.h"] == "REFINE_"
    for name, value in (("MAX_VIEWS", 128), ("MAX_RADIUS", 7), ("MAX_FILL", 64), ("TABLE", 1024)):
        assert getattr(_lib, "REFINE_" + name) == value and f"#define LFT_REFINE_{name} {value}" in hdr
    assert (R.MAX_VIEWS, R.MAX_RADIUS, R.MAX_FILL, R.TABLE) == (128, 7, 64, 1024)
    for name in NAMES:
        assert name in _lib.ADDON_STREAM_LAST and name in _lib.OPTIONAL_EXPORTS and name not in _lib.EXPORTS
    assert len(_lib._SIGS) == 59 and len(_lib.UNITS) == 3
    assert list(_lib.ADDON_HEADERS)[-1] == "lft_hip_focal.h" and list(_lib.ADDON_HEADERS)[-2] == "lft_hip_refine.h"
    v = c_void_p
    assert _lib._ADDON_SIGS["lft_disp_check"] == (c_int, [v, v, v, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_int, v, v, v, v])
    assert _lib._ADDON_SIGS["lft_disp_fill"] == (c_int, [v, v, c_int, c_int, c_int, c_int, c_int, v, v, v])
    assert _lib._ADDON_SIGS["lft_disp_wmedian"] == (c_int, [v, v, v, v, c_int, c_int, c_int, c_int, c_int, v, v, v])
    words = {name: [p.split()[-1].lstrip("*") for p in re.search(name + r"\s*\(([^)]*)\)\s*;", hdr).group(1).split(",")] for name in NAMES}
    assert words["lft_disp_check"] == ["disparity", "view_disparity", "deltas", "B", "N", "H", "W", "tau", "near", "min_agree", "max_conflict", "valid",
                                       "agree", "conflict", "stream"]
    assert words["lft_disp_fill"] == ["disparity", "valid", "B", "H", "W", "reach", "near", "out", "holes", "stream"]
    assert words["lft_disp_wmedian"] == ["disparity", "valid", "guide", "table", "B", "H", "W", "C", "radius", "out", "flags", "stream"]
    assert "lft_refine.cuh" in _lib.SOURCES
    assert [u for u in _lib.UNITS if '"lft_refine.cuh"' in open(os.path.join(_lib.CSRC, u + ".hip")).read()] == ["lft_lightfield"]
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(L, name) for name in NAMES) and _lib.lib().lft_version() == 5
    kernel = open(os.path.join(_lib.CSRC, "lft_refine.cuh")).read()
    for k in ("k_disp_check", "k_disp_fill", "k_disp_wmedian", "#pragma clang fp contract(off)", "vw_search"):
        assert k in kernel, k
    assert "vw_search" in open(os.path.join(_lib.CSRC, "lft_views.cuh")).read()     # the one search of both fills
    # the definitions' sentences stand in the header, the kernel file's comment and the module docstring
    for text in (hdr, kernel, R.__doc__):
        flat = " ".join(re.sub(r"^\s*(//|\*|-)\s?", "", line).replace("`", "").replace("*", "").strip() for line in text.splitlines())
        flat = re.sub(r"\s+", " ", flat.replace("−", "-").replace("≥", ">=").replace("≤", "<=").replace("·", "").replace("Δu", "Du").replace("∈", "in"))
        for said in ("py = fl(y + fl(dDu))", "dropped, not clamped", "falls in the first class that applies", "looks through the surface the map claims",
                     "A non-finite d gives 0, 0, 0", "passes through bit for bit", "A filled pixel never feeds another", "table[min(1023,",
                     "the lower weighted median", "either may come back"):
            assert said.lower() in flat.lower(), said


# ---- 2. every refusal of the entry points is answered on the host ----
def _refuser(name, keys, good):
    _lib.build()
    L = _lib.lib()

    def refused(rc, words, **kw):
        L.lft_scene_counts(1, 1, 1, 1, None, None)      # leaves another call's message behind
        args = [kw.get(k, v) for k, v in zip(keys, good)]
        assert getattr(L, name)(*args) == rc, kw
        msg = L.lft_last_error().decode()
        assert msg.startswith(name + ":") and words in msg, (kw, msg)

    def accepted(**kw):
        assert getattr(L, name)(*[kw.get(k, v) for k, v in zip(keys, good)]) == 0, (kw, L.lft_last_error())

    return refused, accepted


def test_check_refusals_come_before_any_device_work():
    keys = ("dr", "dv", "deltas", "B", "N", "H", "W", "tau", "near", "min_agree", "max_conflict", "valid", "agree", "conflict", "stream")
    refused, accepted = _refuser("lft_disp_check", keys, (P[0], P[1], P[2], 1, 4, 8, 8, 0.5, _lib.VIEW_NEAR_LARGER, 1, 0, P[3], P[4], P[5], None))
    for k in ("dr", "dv", "deltas", "valid", "agree", "conflict"):
        refused(ERR_ARG, "null pointer", **{k: None})
    for n in (0, -1, 129, 1 << 20):
        refused(ERR_ARG, f"{n} views outside 1 .. 128", N=n)
    for tau in (-0.5, float("nan"), float("inf"), -float("inf")):
        refused(ERR_ARG, "must be finite and >= 0", tau=tau)
    for near in (-1, 2, 7):
        refused(ERR_ARG, "near must be LFT_VIEW_NEAR_LARGER or LFT_VIEW_NEAR_SMALLER", near=near)
    refused(ERR_ARG, "must be >= 0", min_agree=-1)
    refused(ERR_ARG, "must be >= 0", max_conflict=-2)
    for k in ("B", "H", "W"):
        refused(ERR_SHAPE, "negative size", **{k: -1})
        accepted(**{k: 0})                              # nothing to do, whatever the pointers
        accepted(**{k: 0, "dr": None, "valid": None})
    refused(ERR_SHAPE, "at most 2^24", H=(1 << 24) + 1)
    refused(ERR_SHAPE, "more than 2^31 pixels", H=1 << 16, W=1 << 16)
    refused(ERR_ARG, "views outside", N=0, dr=None)     # the values come before the pointers


def test_fill_refusals_come_before_any_device_work():
    keys = ("d", "valid", "B", "H", "W", "reach", "near", "out", "holes", "stream")
    refused, accepted = _refuser("lft_disp_fill", keys, (P[0], P[1], 1, 8, 8, 32, _lib.VIEW_NEAR_SMALLER, P[2], P[3], None))
    for k in ("d", "out", "holes"):
        refused(ERR_ARG, "null pointer", **{k: None})
    for reach in (-1, 65, 1000):
        refused(ERR_ARG, f"reach {reach} outside 0 .. 64", reach=reach)
    refused(ERR_ARG, "near must be", near=3)
    refused(ERR_ARG, "in place", out=P[0])
    for k in ("B", "H", "W"):
        refused(ERR_SHAPE, "negative size", **{k: -3})
        accepted(**{k: 0, "d": None})
    refused(ERR_SHAPE, "at most 2^24", W=(1 << 24) + 1)


def test_wmedian_refusals_come_before_any_device_work():
    keys = ("d", "valid", "guide", "table", "B", "H", "W", "C", "radius", "out", "flags", "stream")
    refused, accepted = _refuser("lft_disp_wmedian", keys, (P[0], P[1], P[2], P[3], 1, 8, 8, 3, 3, P[4], P[5], None))
    for k in ("d", "guide", "table", "out", "flags"):
        refused(ERR_ARG, "null pointer", **{k: None})
    for c in (0, 5, -1):
        refused(ERR_ARG, f"{c} guide channels (1 .. 4)", C=c)
    for r in (-1, 8, 100):
        refused(ERR_ARG, f"radius {r} outside 0 .. 7", radius=r)
    refused(ERR_ARG, "in place", out=P[0])
    for k in ("B", "H", "W"):
        refused(ERR_SHAPE, "negative size", **{k: -1})
        accepted(**{k: 0, "guide": None})
    refused(ERR_SHAPE, "more than 2^31 pixels", H=1 << 15, W=1 << 16)


# ---- 3. Python: refusals need no device ----
def test_python_refusals_need_no_device():
    d, dv = torch.zeros(6, 7), torch.zeros(4, 6, 7)
    pos = R.view_positions(5, "cross")
    for kw, words in ((dict(near="nearer"), "near must be larger or smaller"), (dict(tau=-1.0), "tau must be finite"), (dict(tau=float("nan")), "tau must be finite"),
                      (dict(tau="wide"), "tau must be a number"), (dict(min_agree=-1), "min_agree must be an integer >= 0"),
                      (dict(max_conflict=1.5), "max_conflict must be an integer >= 0"), (dict(reference=(1, 2, 3)), "reference must be two finite")):
        with pytest.raises(LftError, match=words):
            R.consistency(d, dv, pos, **{"tau": 0.5, **kw})
    with pytest.raises(LftError, match="positions must be"):
        R.consistency(d, dv, [[0, 1, 2]], tau=0.5)
    with pytest.raises(LftError, match="129 positions: the check takes at most 128"):
        R.consistency(d, torch.zeros(129, 6, 7), np.zeros((129, 2)), tau=0.5)
    with pytest.raises(LftError, match=r"the view disparity must be a torch.float32 tensor of shape \[4, 6, 7\]"):
        R.consistency(d, dv[:3], pos, tau=0.5)
    with pytest.raises(LftError, match="the disparity map must be a torch.float32 tensor"):
        R.consistency(d.double(), dv, pos, tau=0.5)
    with pytest.raises(LftError, match="the view disparity is on meta"):
        R.consistency(d, dv.to("meta"), pos, tau=0.5)
    with pytest.raises(LftError, match="must be on the GPU"):
        R.consistency(d, dv, pos, tau=0.5)
    # fill
    for kw, words in ((dict(reach=65), "reach must be an integer in 0 .. 64"), (dict(reach=-1), "reach must be"), (dict(reach=True), "reach must be"),
                      (dict(near="far"), "near must be"), (dict(valid=torch.ones(6, 7)), "the valid mask must be a torch.uint8 tensor"),
                      (dict(valid=torch.ones(7, 6, dtype=torch.uint8)), r"of shape \[6, 7\]")):
        with pytest.raises(LftError, match=words):
            R.fill(d, **kw)
    with pytest.raises(LftError, match="the disparity map must be"):
        R.fill(torch.zeros(2, 2, 6, 7))
    with pytest.raises(LftError, match="must be on the GPU"):
        R.fill(d, torch.ones(6, 7, dtype=torch.uint8))
    # weighted median
    g = torch.zeros(6, 7, 3, dtype=torch.uint8)
    for kw, words in ((dict(radius=8), "radius must be an integer in 0 .. 7"), (dict(radius=1.0), "radius must be"), (dict(iterations=0), "iterations must be an integer >= 1"),
                      (dict(sigma=0.0), "sigma must be None or a finite number > 0"), (dict(sigma=float("inf")), "sigma must be"),
                      (dict(table=np.ones(1024, np.int32)), "table must be an np.uint16 array"), (dict(table=np.ones(512, np.uint16)), "table must be"),
                      (dict(valid=torch.ones(6, 7, dtype=torch.bool)), "the valid mask must be")):
        with pytest.raises(LftError, match=words):
            R.weighted_median(d, g, **kw)
    for bad in (torch.zeros(6, 7, 5, dtype=torch.uint8), torch.zeros(7, 6, dtype=torch.uint8), torch.zeros(6, 7, 3, dtype=torch.float64), np.zeros((6, 7), np.uint8)):
        with pytest.raises(LftError, match="the guide must be a uint8 or float32 tensor"):
            R.weighted_median(d, bad)
    with pytest.raises(LftError, match="the guide is on meta"):
        R.weighted_median(d, g.to("meta"))
    for guide in (g, torch.zeros(6, 7), torch.zeros(6, 7, 1)):
        with pytest.raises(LftError, match="must be on the GPU"):
            R.weighted_median(d, guide, table=np.ones(1024, np.uint16))
    # the chain: everything is judged before the first sweep asks for the device
    lf = torch.zeros(5, 5, 8, 9, 1)
    sl = [-1.0, 0.0, 1.0]
    for kw, words in ((dict(centre=(1, 1)), "centre cannot be given"), (dict(near="x"), "near must be"), (dict(radius=9), "radius must be"),
                      (dict(reach=99), "reach must be"), (dict(tau=-1), "tau must be finite"), (dict(sigma=-0.1), "sigma must be"),
                      (dict(positions="ring"), "positions must be cross, corners, all"), (dict(iterations=0), "iterations must be"),
                      (dict(min_agree=-1), "min_agree must be"), (dict(max_conflict=-1), "max_conflict must be")):
        with pytest.raises(LftError, match=words):
            R.refine(lf, sl, **kw)
    with pytest.raises(LftError, match="strictly increasing"):
        R.refine(lf, [0.0, 0.0])
    with pytest.raises(LftError, match="leave no position"):
        R.refine(torch.zeros(1, 1, 8, 9, 1), sl)
    with pytest.raises(LftError, match="must be on the GPU"):
        R.refine(lf, sl)
    with pytest.raises(LftError, match="centre is set per position"):
        R.disparity_views(lf, sl, pos, centre=(0, 0))
    with pytest.raises(LftError, match="must be on the GPU"):
        R.disparity_views(lf, sl, pos)


@pytest.mark.parametrize("A", range(1, 12))
def test_view_positions(A):
    uc = (A - 1) / 2
    # cross: the largest whole step from the centre that stays inside the array
    Rr = int(np.floor(uc))
    if Rr < 1:
        with pytest.raises(LftError, match="leave no position"):
            R.view_positions(A, "cross")
    else:
        p = R.view_positions(A, "cross")
        assert p.dtype == np.float64 and p.tolist() == [[uc - Rr, uc], [uc + Rr, uc], [uc, uc - Rr], [uc, uc + Rr]]
        assert p.min() >= 0 and p.max() <= A - 1 and (p.min() < 1 or p.max() > A - 2)
    if A == 1:
        for which in ("corners", "all"):
            with pytest.raises(LftError, match="leave no position"):
                R.view_positions(A, which)
    else:
        assert R.view_positions(A, "corners").tolist() == [[0, 0], [0, A - 1], [A - 1, 0], [A - 1, A - 1]]
        every = [[u, v] for u in range(A) for v in range(A) if (u, v) != (uc, uc)]
        assert R.view_positions(A, "all").tolist() == every and len(every) == A * A - A % 2
    # another reference: its own cross, and it leaves the other lists
    if A >= 3:
        assert R.view_positions(A, "cross", reference=(1, 1)).tolist() == [[0, 1], [2, 1], [1, 0], [1, 2]]
        assert [0, 0] not in R.view_positions(A, "corners", reference=(0, 0)).tolist()
        assert len(R.view_positions(A, "all", reference=(0, 0))) == A * A - 1
    given = np.array([[0.5, 1.25], [0, 0]])
    assert np.array_equal(R.view_positions(A, given), given) and np.array_equal(R.view_positions(A, given.tolist()), given)
    for bad in ("ring", [[1, 2, 3]], np.zeros((0, 2)), [[np.nan, 0]]):
        with pytest.raises(LftError, match="positions must be"):
            R.view_positions(A, bad)
    with pytest.raises(LftError, match="angRes must be an integer >= 1"):
        R.view_positions(0, "all")


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("sigma", [None, 0.02, 0.05, 0.1, 1.0, 50.0])
def test_range_table(sigma, channels):
    w = R.range_table(sigma, channels)
    assert w.dtype == np.uint16 and w.shape == (1024,) and np.array_equal(w, RU.range_table_np(sigma, channels))
    assert np.all(np.diff(w.astype(np.int64)) <= 0)
    assert w[0] == (1 if sigma is None else 4096)
    if sigma is None:
        assert (w == 1).all()
    for bad in (0, 5, 1.0, True):
        with pytest.raises(LftError, match="channels must be an integer in 1 .. 4"):
            R.range_table(0.1, bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "0.1", True):
        with pytest.raises(LftError, match="sigma must be"):
            R.range_table(bad, channels)


def test_quantise_guide_is_refocus_rule():
    g = torch.tensor([-1.0, 0.0, 0.5 / 255, 1.5 / 255, 2.5 / 255, 0.5, 1.0, 2.0])
    assert R.quantise_guide(g).tolist() == [0, 0, 0, 2, 2, 128, 255, 255]         # clip, x 255, round half to even
    b = torch.arange(6, dtype=torch.uint8)
    assert R.quantise_guide(b) is b


# ---- 4. the restatements against the definitions ----
@pytest.mark.parametrize("seed", range(6))
def test_wmedian_np_is_the_definition(seed):
    rng = np.random.default_rng([11, seed])
    B, H, W, C, r = 1, 7, 9, (1, 3, 4)[seed % 3], (1, 2, 3)[seed % 3]
    d = (rng.integers(-6, 7, (B, H, W)) / 4).astype(np.float32)      # ties, negative values, both zeros
    d[0, 1, 2] = -0.0
    d[0, 3, 3], d[0, 0, 0] = np.nan, np.inf
    valid = (rng.random((B, H, W)) < 0.7).astype(np.uint8)
    guide = rng.integers(0, 256, (B, H, W, C)).astype(np.uint8)
    table = (rng.integers(1, 4, 1024) * (rng.random(1024) < 0.05)).astype(np.uint16)          # mostly zero weights, w[0] among them: T = 0 occurs
    table[0] = 0
    out, flags = RU.wmedian_np(d, guide, table, r, valid)
    good = RU.good_np(d, valid)
    seen = set()
    for y in range(H):
        for x in range(W):
            vals, wts = [], []
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and good[0, yy, xx]:
                        s = min(1023, int(np.abs(guide[0, y, x].astype(int) - guide[0, yy, xx].astype(int)).sum()))
                        vals.append(float(d[0, yy, xx]))
                        wts.append(int(table[s]))
            want = RU.wmedian_brute(vals, wts)
            if want is None:
                assert flags[0, y, x] == 2 and out[0, y, x].tobytes() == d[0, y, x].tobytes()
            else:
                assert flags[0, y, x] == (0 if good[0, y, x] else 1) and out[0, y, x] == want and want in vals
            seen.add(int(flags[0, y, x]))
    assert seen == {0, 1, 2}


def test_wmedian_np_fixed_point_and_plain_median():
    rng = np.random.default_rng(5)
    guide = rng.integers(0, 256, (2, 9, 11, 3)).astype(np.uint8)
    const = np.full((2, 9, 11), 0.375, np.float32)
    for table in (RU.range_table_np(None, 3), RU.range_table_np(0.05, 3)):
        out, flags = RU.wmedian_np(const, guide, table, 2)
        assert np.array_equal(out, const) and not flags.any()        # a constant map is a fixed point
    d = rng.standard_normal((2, 9, 11)).astype(np.float32)
    r = 2
    out, flags = RU.wmedian_np(d, guide, RU.range_table_np(None, 3), r)
    for b in range(2):
        for y in range(9):
            for x in range(11):
                win = np.sort(d[b, max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1].reshape(-1))
                assert out[b, y, x] == win[(len(win) - 1) // 2]      # all-ones weights, everything valid: the lower median
    assert not flags.any()


def test_fill_np_and_check_np_on_cases_worked_by_hand():
    n = np.nan
    d = np.array([[[1, n, n, 5, n, n, n, 2]]], np.float32)
    out, holes = RU.fill_np(d, None, 1, "larger")
    assert RU.same_values(out, np.array([[[1, 1, 5, 5, 5, n, 2, 2]]], np.float32)) and holes.tolist() == [[[0, 1, 1, 0, 1, 2, 1, 0]]]
    out, holes = RU.fill_np(d, None, 2, "larger")                    # both sides found: the farther, which is the smaller
    assert RU.same_values(out, np.array([[[1, 1, 1, 5, 5, 2, 2, 2]]], np.float32)) and holes.tolist() == [[[0, 1, 1, 0, 1, 1, 1, 0]]]
    out, holes = RU.fill_np(d, None, 3, "smaller")
    assert RU.same_values(out, np.array([[[1, 5, 5, 5, 5, 5, 5, 2]]], np.float32)) and holes.max() == 1
    col = np.array([[[n, 7], [3, n], [n, n]]], np.float32)           # nothing in the row: the column
    out, holes = RU.fill_np(col, np.array([[[1, 1], [0, 1], [1, 1]]], np.uint8), 1, "larger")
    assert RU.same_values(out, np.array([[[7, 7], [3, 7], [n, n]]], np.float32)) and holes.tolist() == [[[1, 0], [2, 1], [2, 2]]]
    # the check: one view one step to the right in v, a map that is 1 everywhere: the pixel (y, x) looks at (y, x + 1)
    dr = np.ones((1, 2, 4), np.float32)
    dv = np.array([[[[1, 1.5, 0, n], [1, 1, 1, 1]]]], np.float32)
    valid, agree, conflict = RU.check_np(dr, dv, np.array([[0, 1]], np.float32), 0.25, "larger", 1, 0)
    assert agree.tolist() == [[[0, 0, 0, 0], [1, 1, 1, 0]]]          # 1.5 is nearer (occluded), 0 farther (conflict), NaN and outside unseen
    assert conflict.tolist() == [[[0, 1, 0, 0], [0, 0, 0, 0]]] and valid.tolist() == agree.tolist()
    valid, agree, conflict = RU.check_np(dr, dv, np.array([[0, 1]], np.float32), 0.25, "smaller", 0, 0)
    assert conflict.tolist() == [[[1, 0, 0, 0], [0, 0, 0, 0]]] and valid.tolist() == [[[0, 1, 1, 1], [1, 1, 1, 1]]]
    # a fractional position: both neighbours are read, and one of them agreeing is enough
    valid, agree, conflict = RU.check_np(dr, dv, np.array([[0, 0.5]], np.float32), 0.25, "larger", 1, 0)
    assert agree.tolist() == [[[1, 0, 0, 0], [1, 1, 1, 1]]] and conflict.tolist() == [[[0, 0, 1, 0], [0, 0, 0, 0]]]
