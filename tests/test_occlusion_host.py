"""CPU: the occlusion-aware sweep cost up to the device -- the subset tables of lft_amd.disparity.subset_table against the
restatement (tests/occlusion_util.py) and the definition's own properties, every Python refusal, the new header and its binding,
every refusal of lft_disparity_occ on the host, and the conditions the GPU tests lean on, checked on the restatement alone."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from lft_amd import _lib, disparity as Dm, refocus as R, views as V
from lft_amd._lib import LftError

import abi_refusals_util as U
import disparity_util as DU
import occlusion_util as OU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = -1, -2
P, Q = 1 << 20, 2 << 20                                                       # addresses that are never dereferenced


# ---- 1. subset tables ----
@pytest.mark.parametrize("mode", ["halves", "quadrants"])
@pytest.mark.parametrize("A", [1, 2, 3, 4, 5])
def test_tables_at_the_centre(A, mode):
    a, uc = R.aperture_weights(A), (A - 1) / 2
    if A == 1 or (A == 2 and mode == "quadrants"):                              # a quadrant of A = 2 is one view: no subset has two
        with pytest.raises(LftError, match="none of the 4 subsets"):
            Dm.subset_table(A, "full", None, mode)
        return
    table, kept = Dm.subset_table(A, "full", None, mode)
    want, want_kept = OU.subset_table_np(A, a, (uc, uc), mode)
    assert table.dtype == np.float32 and table.shape == (4, A * A) and kept == want_kept == (0, 1, 2, 3)
    assert np.array_equal(table, want)
    assert np.all(np.abs(table.astype(np.float64).sum(1) - 1.0) <= A * A * 2.0 ** -24)
    n = A * ((A + 1) // 2) if mode == "halves" else ((A + 1) // 2) ** 2       # an odd A has its middle row on both sides
    assert np.all((table > 0).sum(1) == n)
    first = table[0].reshape(A, A)
    assert np.all(first[int(np.floor(uc)) + 1:] == 0) and np.all(first[:int(np.floor(uc)) + 1] > 0) if mode == "halves" else first[0, 0] > 0


@pytest.mark.parametrize("A", [1, 2, 3, 4, 5])
def test_tables_at_a_corner_with_the_view_held_out(A):
    a = np.ones((A, A))
    a[0, 0] = 0
    if A == 1:
        with pytest.raises(LftError, match="aperture"):
            Dm.subset_table(A, a, (0, 0), "halves")
        return
    a64 = a / a.sum()
    for mode in ("halves", "quadrants"):
        want, want_kept = OU.subset_table_np(A, a64, (0.0, 0.0), mode)
        table, kept = Dm.subset_table(A, a, (0, 0), mode)
        assert kept == want_kept and np.array_equal(table, want)
        assert np.all(table[:, 0] == 0)                                        # the held-out view is in no row
        assert np.all(np.abs(table.astype(np.float64).sum(1) - 1.0) <= A * A * 2.0 ** -24)
    # du <= 0 is the row u = 0 without the held-out view: A - 1 views.  For A = 2 that is one view, and the half is dropped
    _, kept = Dm.subset_table(A, a, (0, 0), "halves")
    assert kept == ((1, 3) if A == 2 else (0, 1, 2, 3))
    # (<=,<=) is the held-out view alone; (<=,>=) and (>=,<=) are its row and column; (>=,>=) everything
    _, kept = Dm.subset_table(A, a, (0, 0), "quadrants")
    assert kept == ((3,) if A == 2 else (1, 2, 3))


def test_min_views_and_array_subsets():
    A = 3
    masks = np.zeros((3, A, A), bool)
    masks[0, 0, :2] = True                                                     # two views
    masks[1, 1, :] = True                                                      # three
    masks[2] = True                                                            # all nine
    a = R.aperture_weights(A, "gaussian")
    table, kept = Dm.subset_table(A, "gaussian", None, masks)
    want, want_kept = OU.subset_table_np(A, a, (1.0, 1.0), masks)
    assert kept == want_kept == (0, 1, 2) and np.array_equal(table, want)
    assert np.array_equal(table[2], a.reshape(-1).astype(np.float32))          # the whole aperture: W = 1
    assert np.array_equal(table[0] != 0, masks[0].reshape(-1))
    assert Dm.subset_table(A, "gaussian", None, masks, min_views=3)[1] == (1, 2)
    t4, k4 = Dm.subset_table(A, "gaussian", None, masks, min_views=4)
    assert k4 == (2,) and np.array_equal(t4[0], table[2])
    with pytest.raises(LftError, match="none of the 3 subsets has 10 views"):
        Dm.subset_table(A, "gaussian", None, masks, min_views=10)
    # a view of weight 0 does not count
    ap = np.ones((A, A))
    ap[0, 0] = 0
    assert Dm.subset_table(A, ap, None, masks)[1] == (1, 2)
    # torch arrays are taken too
    assert np.array_equal(Dm.subset_table(A, "gaussian", None, torch.from_numpy(masks))[0], table)


def test_python_refusals_need_no_device():
    A = 3
    ok = np.ones((1, A, A), bool)
    for bad in (np.ones((0, A, A), bool), np.ones((5, A, A), bool), np.ones((2, A, A + 1), bool), np.ones((A, A), bool), np.ones((1, A, A), np.float32)):
        with pytest.raises(LftError, match="boolean array"):
            Dm.subset_table(A, "full", None, bad)
    for mv in (1, 0, -2, 2.0, True, "2"):
        with pytest.raises(LftError, match="min_views"):
            Dm.subset_table(A, "full", None, ok, min_views=mv)
    with pytest.raises(LftError, match="subsets must be halves, quadrants"):
        Dm.subset_table(A, "full", None, "thirds")
    lf, sl = torch.zeros(3, 3, 6, 6), [-1.0, 0.0, 1.0]
    for margin in (0.5, 0.0, -2.0, float("nan"), float("inf"), 1e39, True, "2"):
        with pytest.raises(LftError, match="margin"):
            Dm.disparity(lf, sl, occlusion=dict(margin=margin))
    for occ, words in (("thirds", "subsets must be"), (3, "occlusion must be"), (dict(subset="halves"), "occlusion must be"), (dict(min_views=1), "min_views"),
                       (dict(subsets="halves", margin=0.99), "margin")):
        with pytest.raises(LftError, match=words):
            Dm.disparity(lf, sl, occlusion=occ)
        with pytest.raises(LftError, match=words):                             # judged before the sweep with regularize too
            Dm.disparity(lf, sl, occlusion=occ, regularize=dict(p1=0.1, p2=1.0))
    # the values are judged before the light field leaves the host, then the device is asked for
    for occ in ("halves", "quadrants", dict(subsets=ok, margin=1.0), dict(margin=8, min_views=3)):
        with pytest.raises(LftError, match="no CPU path"):
            Dm.disparity(lf, sl, occlusion=occ)
    with pytest.raises(LftError, match="radius"):
        Dm.disparity(lf, sl, radius=9, occlusion="halves")
    with pytest.raises(LftError, match="no CPU path"):
        Dm.occlusion_volume(lf, sl)
    with pytest.raises(LftError, match="no CPU path"):
        V.leave_one_out(lf, sl, occlusion="halves")
    with pytest.raises(LftError, match="no CPU path"):
        Dm.disparity_error(lf, lf, sl, occlusion="quadrants")
    with pytest.raises(LftError, match="no CPU path"):
        Dm.gather_choice(torch.zeros(4, 5, dtype=torch.int32), torch.zeros(3, 4, 5, dtype=torch.uint8))
    for index, choice in ((torch.zeros(4, 5), torch.zeros(3, 4, 5, dtype=torch.uint8)), (torch.zeros(4, 5, dtype=torch.int32), torch.zeros(3, 4, 6, dtype=torch.uint8)),
                          (torch.zeros(2, 4, 5, dtype=torch.int32), torch.zeros(3, 4, 5, dtype=torch.uint8))):
        with pytest.raises(LftError, match="index|choice"):
            Dm.gather_choice(index, choice)
    # the result type: the old fields in their order, the two new ones at the end; the plain result still unpacks into five and
    # answers None for both
    assert Dm.OcclusionDisparityResult._fields == Dm.DisparityResult._fields + ("subset", "subsets_kept")
    assert Dm.DisparityResult._fields == ("disparity", "confidence", "index", "all_in_focus", "cost")
    r = Dm.DisparityResult(1, 2, 3, 4, 5)
    assert r.subset is None and r.subsets_kept is None and len(r) == 5
    Dm.clear_cache()


# ---- 2. the header ----
def test_header_declares_and_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "lft_hip_occlusion.h")).read()
    declared = re.findall(r"^int\s+(lft_\w+)\s*\(", hdr, flags=re.M)
    names = ("lft_disparity_occ_scratch_bytes", "lft_disparity_occ", "lft_occ_gather")
    assert _lib.OCCLUSION_EXPORTS == names and tuple(declared) == names
    assert "added beside ABI 5; lft_version unchanged" in " ".join(hdr.split()).replace("Added", "added")
    assert _lib.ADDON_HEADERS["lft_hip_occlusion.h"] == "OCC_" and _lib.OCC_MAX_SUBSETS == 4 and "#define LFT_OCC_MAX_SUBSETS 4" in hdr
    from ctypes import POINTER, c_float, c_int, c_size_t, c_void_p
    S = _lib._ADDON_SIGS
    assert S["lft_disparity_occ_scratch_bytes"] == (c_int, [c_int] * 6 + [POINTER(c_size_t)])
    assert S["lft_disparity_occ"] == (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p,
                                              c_int, c_int, c_int] + [c_void_p] * 8 + [c_int, c_void_p])
    assert S["lft_occ_gather"] == (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p])
    # lft_disparity's parameters, with the table's companions behind `table` and the two outputs behind `index`
    params = lambda text, name: [p.split()[-1].lstrip("*") for p in re.search(r"int\s+%s\s*\(([^)]*)\)" % name, text, flags=re.S).group(1).split(",")]
    plain = params(open(os.path.join(ROOT, "include", "lft_hip.h")).read(), "lft_disparity")
    at, ix = plain.index("table") + 1, plain.index("index") + 1
    assert params(hdr, "lft_disparity_occ") == plain[:at] + ["subsets", "P", "beta"] + plain[at:ix] + ["subset", "choice"] + plain[ix:]
    assert {"lft_disparity_occ", "lft_occ_gather"} <= _lib.ADDON_STREAM_LAST and set(names) <= _lib.OPTIONAL_EXPORTS
    assert len(_lib._SIGS) == 59 and not set(names) & set(_lib.EXPORTS)       # the older headers keep their prototypes
    for other in ("lft_hip.h", "lft_hip_test.h", "lft_hip_views.h", "lft_hip_sgm.h", "lft_hip_visibility.h"):
        assert "_occ" not in open(os.path.join(ROOT, "include", other)).read()
    assert "lft_occlusion.cuh" in _lib.SOURCES
    assert [u for u in _lib.UNITS if "lft_occlusion.cuh" in open(os.path.join(_lib.CSRC, u + ".hip")).read()] == ["lft_lightfield"]
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    assert _lib.lib().lft_version() == 5
    # the definition's sentences stand in the header, the kernels' comment and the module docstring
    kernels = open(os.path.join(_lib.CSRC, "lft_occlusion.cuh")).read()
    for text in (hdr, kernels, Dm.__doc__):
        flat = " ".join(re.sub(r"^\s*(//|\*)\s?", "", line).replace("`", "").replace("**", "").replace("*kept*", "kept").strip() for line in text.splitlines())
        flat = flat.replace("−", "-").replace("≥", ">=").replace("≤", "<=").replace("·", "*").replace("δ", "d").replace("β", "beta").replace("Σ", "sum")
        for words in ("A subset is kept iff at least min_views of its views have a > 0", "Dropped subsets never reach the kernel",
                      "Subset ids in the outputs are positions in the kept list", "for members and 0 for the rest", "is the only place these weights are rounded",
                      "The full aperture is unchanged", "m_p = fma(b_p, s, m_p)", "q_p = fma(fl(b_p*s), s, q_p)", "with c = 0 first",
                      "V = min(V_full, U)", "else the lowest p (1-based) with V_p = t", "finite, >= 1, rounded once to fp32",
                      "through the existing k_disparity_pick unchanged", "0 where all views agree",
                      "No result may depend on the tile, the launch shape or the arrival order"):
            assert words in flat, words
    # the sweep is written once, in the plain sweep's file: both kernels are wrappers of that body, and the new file repeats none
    # of the window pipeline
    plain_src = open(os.path.join(_lib.CSRC, "lft_disparity.cuh")).read()
    assert plain_src.count("void sweep_cost(") == 1 and "void sweep_cost(" not in kernels
    assert "void k_sweep_cost(SweepArgs a) { sweep_cost<T, C, TAPS, false>(" in plain_src
    assert "void k_sweep_cost_occ(SweepOccArgs oa) { sweep_cost<T, C, TAPS, true>(" in kernels and "k_occ_gather" in kernels
    assert not any(step in kernels for step in ("next_active", "fetch(", "commit(", "__fmaf_rn"))


def test_scratch_query():
    q = lambda *a: _lib.query("lft_disparity_occ_scratch_bytes", *a)
    plain = lambda *a: _lib.query("lft_disparity_scratch_bytes", *a)
    assert q(2, 9, 37, 45, 3, 0) == plain(2, 9, 37, 45, 3, 0) + (2 * 9 * 37 * 45 + 3) // 4 * 4
    assert q(1, 3, 5, 5, 4, _lib.DISPARITY_AIF) == plain(1, 3, 5, 5, 4, _lib.DISPARITY_AIF) + 76 and q(1, 3, 5, 5, 4, _lib.DISPARITY_AIF) % 4 == 0
    assert q(0, 9, 37, 45, 1, 0) == 0 and q(1, 9, 0, 45, 1, 0) == 0
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    for args, rc in (((1, 3, 4, 4, 0, 0), ERR_ARG), ((1, 3, 4, 4, 5, 0), ERR_ARG), ((1, 0, 4, 4, 1, 0), ERR_ARG), ((1, 3, 4, 4, 1, 2), ERR_ARG),
                     ((-1, 3, 4, 4, 1, 0), ERR_SHAPE), ((1, 3, 4, -4, 1, 0), ERR_SHAPE), ((1 << 10, 384, 1 << 15, 1 << 15, 1, 0), ERR_SHAPE)):
        assert L.lft_disparity_occ_scratch_bytes(*args, ctypes.byref(n)) == rc, args
        assert L.lft_last_error().decode().startswith("lft_disparity_occ:")
    assert L.lft_disparity_occ_scratch_bytes(1, 3, 4, 4, 1, 0, None) == ERR_ARG


OCC_AT, OUT_AT = 9, 17                   # lft_disparity's arguments up to `table`, and up to `index`


def occ_args(args, subsets=Q + (1 << 18), n=4, beta=2.0, subset=None, choice=None):
    """lft_disparity's argument tuple as lft_disparity_occ's."""
    return tuple(args[:OCC_AT]) + (subsets, n, beta) + tuple(args[OCC_AT:OUT_AT]) + (subset, choice) + tuple(args[OUT_AT:])


def test_every_refusal_comes_before_any_device_work():
    """Each call is answered on the host (this runs without a GPU).  Every rule of lft_disparity: the recorded case table of
    tests/abi_refusals_util.py, answered with the same code and the same words under the new name."""
    _lib.build()
    L = _lib.lib()
    plain = [(case, args) for entry, case, args in U.cases() if entry == "lft_disparity"]
    assert len(plain) >= 40 and {"radius9", "null_slopes", "span_rows", "too_many_blocks", "volume", "scratch_misaligned", "empty_B"} <= {c for c, _ in plain}
    refused = 0
    for case, args in plain:
        rc = L.lft_disparity(*args)
        want = L.lft_last_error().decode() if rc else ""
        L.lft_refocus(None, 99, 1, 1, 1, 1, 1, None, None, 1, 1, None, 0, None)              # leaves another call's message behind
        assert L.lft_disparity_occ(*occ_args(args)) == rc, case
        if rc:
            got = L.lft_last_error().decode()
            assert got.startswith("lft_disparity_occ:") and got == want.replace("lft_disparity:", "lft_disparity_occ:", 1), (case, got, want)
            refused += 1
    assert refused >= 35
    good = next(args for case, args in plain if case == "scratch_misaligned")               # everything right but the scratch
    aligned = list(good)
    aligned[13] = Q
    inf, nan = float("inf"), float("nan")
    for kw, words in ((dict(n=0), "0 subsets outside 1 .. 4"), (dict(n=5), "5 subsets outside 1 .. 4"), (dict(n=-1), "subsets outside"),
                      (dict(subsets=None), "null pointer"), (dict(beta=0.5), "margin 0.5 must be finite and >= 1"), (dict(beta=0.0), "margin"),
                      (dict(beta=-3.0), "margin"), (dict(beta=nan), "margin"), (dict(beta=inf), "margin"), (dict(beta=-inf), "margin")):
        L.lft_refocus(None, 99, 1, 1, 1, 1, 1, None, None, 1, 1, None, 0, None)
        assert L.lft_disparity_occ(*occ_args(aligned, **kw)) == ERR_ARG, kw
        msg = L.lft_last_error().decode()
        assert msg.startswith("lft_disparity_occ:") and words in msg and "99" not in msg, (kw, msg)
    # the ends of the ranges are accepted: what refuses these calls is the misaligned scratch behind them
    for kw in (dict(n=1), dict(n=4), dict(beta=1.0), dict(beta=3.0e38), dict(subset=P), dict(choice=P), dict(subset=P, choice=P + 4096)):
        assert L.lft_disparity_occ(*occ_args(good, **kw)) == ERR_ARG and b"scratch must be 4-byte aligned" in L.lft_last_error(), kw
    # lft_disparity's rules come first, the subsets' before the sizes of the volume
    for i, kw, words in ((12, dict(n=0), "radius"), (10, dict(beta=0.5), "slopes")):
        bad = list(aligned)
        bad[i] = 99 if i == 12 else 0
        assert L.lft_disparity_occ(*occ_args(bad, **kw)) == ERR_ARG and words in L.lft_last_error().decode()
    # empty shapes are no error and no work, null pointers included; the values are still judged
    for i in (2, 4, 5):
        empty = list(aligned)
        empty[i] = 0
        empty[0] = empty[7] = empty[8] = empty[9] = empty[13] = None
        assert L.lft_disparity_occ(*occ_args(empty, subsets=None)) == 0, i
        assert L.lft_disparity_occ(*occ_args(empty, n=7)) == ERR_ARG and L.lft_disparity_occ(*occ_args(empty, beta=0.5)) == ERR_ARG, i
    # lft_occ_gather
    for args, rc, words in (((P, Q, 1, 0, 4, 4, P + 4096, None), ERR_ARG, "0 slopes"), ((P, Q, -1, 3, 4, 4, P + 4096, None), ERR_SHAPE, "negative size"),
                            ((P, Q, 1, 3, 4, -4, P + 4096, None), ERR_SHAPE, "negative size"), ((None, Q, 1, 3, 4, 4, P + 4096, None), ERR_ARG, "null pointer"),
                            ((P, None, 1, 3, 4, 4, P + 4096, None), ERR_ARG, "null pointer"), ((P, Q, 1, 3, 4, 4, None, None), ERR_ARG, "null pointer"),
                            ((P, Q, 1 << 20, 3, 1 << 20, 1 << 20, P + 4096, None), ERR_SHAPE, "2^31 blocks")):
        assert L.lft_occ_gather(*args) == rc, args
        msg = L.lft_last_error().decode()
        assert msg.startswith("lft_occ_gather:") and words in msg, msg
    assert L.lft_occ_gather(None, None, 0, 3, 4, 4, None, None) == 0 and L.lft_occ_gather(None, None, 2, 3, 4, 0, None, None) == 0


# ---- 3. the conditions the GPU tests lean on, on the restatement alone ----
@pytest.fixture(scope="module")
def scene():
    S = OU.SCENE
    L = OU.noisy_two_layer()
    table = R.shift_table(S["A"], OU.SLOPES, "full", S["interp"])
    btable, kept = Dm.subset_table(S["A"], "full", None, S["subsets"])
    o = OU.occ_cost_np(L, table, R.TAPS[S["interp"]], btable, S["beta"])
    tol = OU.tol_occ(S["A"], 1, S["radius"], table, R.TAPS[S["interp"]], float(np.abs(L).max()), S["beta"])
    return L, o, tol


def test_the_scene_separates_the_two_costs(scene):
    L, o, tol = scene
    r, band = OU.SCENE["radius"], OU.band()
    assert band.sum() == 320 and OU.SLOPES[OU.K_BG] == -1.0 and OU.SLOPES[OU.K_FG] == 1.0
    k_plain = np.argmin(DU.aggregate_np(o["V_full"], r), 0)
    E = DU.aggregate_np(o["V"], r)
    k_new = np.argmin(E, 0)
    wrong_plain, wrong_new = int((k_plain[band] != OU.K_BG).sum()), int((k_new[band] != OU.K_BG).sum())
    srt = np.sort(E, 0)
    gap = float((srt[1] - srt[0])[band].min())
    chosen = np.take_along_axis(o["choice"], k_new[None], 0)[0]
    share = float((chosen[band] != 0).mean())
    print(f"band: plain wrong at {wrong_plain} of 320, new at {wrong_new}; smallest gap of E {gap:.3e} against tol {tol:.3e}; choice != 0 at {share:.3f}")
    assert wrong_plain >= 50
    assert wrong_new == 0
    assert gap > 100 * tol
    assert share >= 0.9
    # the foreground's interior is found by both
    fg, _ = DU.two_layer_interiors(5, 40, 40, r, box=OU.BOX)
    assert np.all(k_new[fg] == OU.K_FG) and np.all(k_plain[fg] == OU.K_FG)


def test_the_choice_is_well_conditioned_on_most_of_the_interior(scene):
    L, o, tol = scene
    k_new = np.argmin(DU.aggregate_np(o["V"], OU.SCENE["radius"]), 0)
    ok = np.take_along_axis(OU.well_conditioned(o, tol), k_new[None], 0)[0]
    inner = OU.interior()
    left_out = 1.0 - float(ok[inner].mean())
    print(f"left out of the subset comparison: {left_out:.3f} of the interior")
    assert left_out <= 0.25


def test_restatement_properties():
    """V <= V_full; beta -> large gives V = V_full and choice 0; one all-true subset and beta = 1 gives V = V_full; a tie between
    two identical subsets goes to the lower one."""
    rng = np.random.default_rng(3)
    L = rng.random((3, 3, 6, 7, 2)).astype(np.float32)
    table = R.shift_table(3, [-1.0, 0.5], "full", "linear")
    bt, _ = Dm.subset_table(3, "full", None, "quadrants")
    o = OU.occ_cost_np(L, table, 2, bt, 2.0)
    assert np.all(o["V"] <= o["V_full"]) and o["choice"].max() <= 4 and (o["choice"] > 0).any()
    m, q = DU.moments_np(L, table, 2)
    assert np.allclose(o["V_full"], np.maximum(q - m * m, 0).sum(-1), rtol=0, atol=1e-15) and np.array_equal(o["m"], m)
    big = OU.occ_cost_np(L, table, 2, bt, 1e30)
    assert np.array_equal(big["V"], big["V_full"]) and not big["choice"].any()
    whole, _ = Dm.subset_table(3, "full", None, np.ones((1, 3, 3), bool))
    one = OU.occ_cost_np(L, table, 2, whole, 1.0)
    assert np.allclose(one["V"], one["V_full"], rtol=0, atol=1e-9)
    twice = OU.occ_cost_np(L, table, 2, np.stack([bt[2], bt[2], bt[0]]), 1.0)
    assert not (twice["choice"] == 2).any() and (twice["choice"] == 1).any()
