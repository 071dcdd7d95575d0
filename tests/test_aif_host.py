"""CPU: the all-in-focus image from the winning partial aperture up to the device -- the new header and its binding, every refusal
of lft_aif_at on the host, every Python refusal, the table identity the GPU anchors rest on (a subset's row b_p is the `a` column of
refocus's table for the masked aperture, bit for bit), the restatement's own properties (tests/aif_util.py), and the defect and
its repair on the two-layer scene, on the restatement alone."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from lft_amd import _lib, disparity as Dm, refocus as R
from lft_amd._lib import LftError

import abi_refusals_util as U
import aif_util as AU
import disparity_util as DU
import occlusion_util as OU
import refocus_util as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = -1, -2
P, Q = 1 << 20, 2 << 20                                                       # addresses that are never dereferenced
TAPS_AT = 10                             # lft_refocus's arguments up to `D`: (subsets, P, index, subset) go behind them


def aif_args(args, subsets=Q + (1 << 18), n=4, index=Q + (2 << 18), subset=None):
    """lft_refocus's argument tuple as lft_aif_at's: out / out_class are aif / aif_class."""
    return tuple(args[:TAPS_AT]) + (subsets, n, index, subset) + tuple(args[TAPS_AT:])


# ---- 1. the header and its binding ----
def test_header_declares_and_library_exports_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "lft_hip_aif.h")).read()
    assert re.findall(r"^int\s+(lft_\w+)\s*\(", hdr, flags=re.M) == ["lft_aif_at"]
    assert _lib.AIF_EXPORTS == ("lft_aif_at",) and _lib.ADDON_HEADERS["lft_hip_aif.h"] == "AIF_"
    assert "added beside ABI 5; lft_version unchanged" in " ".join(hdr.split()).replace("Added", "added")
    assert "lft_aif_at" in _lib.ADDON_STREAM_LAST and "lft_aif_at" in _lib.OPTIONAL_EXPORTS
    from ctypes import c_int, c_void_p
    assert _lib._ADDON_SIGS["lft_aif_at"] == (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                                      c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p])
    # lft_refocus's parameters, with the maps' four behind D and aif / aif_class in the place of out / out_class
    params = lambda text, name: [p.split()[-1].lstrip("*") for p in re.search(r"int\s+%s\s*\(([^)]*)\)" % name, text, flags=re.S).group(1).split(",")]
    plain = params(open(os.path.join(ROOT, "include", "lft_hip.h")).read(), "lft_refocus")
    at = plain.index("D") + 1
    assert at == TAPS_AT
    assert params(hdr, "lft_aif_at") == plain[:at] + ["subsets", "P", "index", "subset"] + [{"out": "aif", "out_class": "aif_class"}.get(p, p) for p in plain[at:]]
    # the 59 prototypes of the two older headers and the other add-on headers keep their contents
    assert len(_lib._SIGS) == 59 and "lft_aif_at" not in _lib.EXPORTS and "lft_aif_at" not in _lib.TEST_EXPORTS
    for other in ("lft_hip.h", "lft_hip_test.h", "lft_hip_views.h", "lft_hip_sgm.h", "lft_hip_visibility.h", "lft_hip_occlusion.h"):
        assert "aif_at" not in open(os.path.join(ROOT, "include", other)).read()
    assert (len(_lib.VIEW_EXPORTS), len(_lib.SGM_EXPORTS), len(_lib.VISIBILITY_EXPORTS), len(_lib.OCCLUSION_EXPORTS)) == (2, 2, 3, 3)
    assert "lft_aif.cuh" in _lib.SOURCES
    assert [u for u in _lib.UNITS if "lft_aif.cuh" in open(os.path.join(_lib.CSRC, u + ".hip")).read()] == ["lft_lightfield"]
    _lib.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "lft_aif_at")
    assert _lib.lib().lft_version() == 5
    # the definition's sentences stand in the header, the kernel's comment and the module docstring
    kernel = open(os.path.join(_lib.CSRC, "lft_aif.cuh")).read()
    for text in (hdr, kernel, Dm.__doc__):
        flat = " ".join(re.sub(r"^\s*(//|\*)\s?", "", line).replace("`", "").replace("**", "").strip() for line in text.splitlines())
        flat = flat.replace("−", "-").replace("≥", ">=").replace("≤", "<=").replace("·", "*").replace("∈", "in")
        for words in ("refocus table [D, A*A] of lft_refocus_record, taps in {1, 2, 4} and the centre are those of lft_refocus",
                      "subsets: DEVICE fp32 [P, A*A], the rows b_p of lft_disparity_occ", "0 <= P <= LFT_OCC_MAX_SUBSETS", "subsets is NULL iff P = 0",
                      "A value outside 0 .. D-1 is clamped into it, as in lft_occ_gather", "0 means the whole aperture", "p >= 1 means row p-1 of subsets",
                      "NULL and any id above P count as 0", "fp32 or uint8 by rf_byte", "Let k be the clamped index and p the id of the pixel",
                      "For p = 0 the weight is w_n = a of record (k, n), and the view is skipped iff the record's skip is set",
                      "For p >= 1 the weight is w_n = b_p[n], and the view is skipped iff b_p[n] == 0 or the record's skip is set",
                      "The row pass over wy comes first, then the column pass over wx",
                      "Every step after a sum's first product is one explicit FMA, with contraction off", "acc = fma(w_n, s, acc) from acc = 0",
                      "p = 0: the bits of lft_refocus's stack (fp32 and uint8) at k",
                      "p >= 1: the bits of lft_refocus run with a table whose a / skip columns are b_p / b_p == 0, at k",
                      "on its neighbours' k or p, or on which code path served it"):
            assert words in flat, words
    # the kernel shares refocus's input and output rules and the XCD-aware order, and needs no LDS
    assert "rf_x<T>(" in kernel and "rf_byte(" in kernel and "xcd_tile(" in kernel and "__shared__" not in kernel and "__syncthreads" not in kernel


# ---- 2. every refusal of lft_aif_at is answered on the host ----
def test_every_refusal_comes_before_any_device_work():
    """Each call is answered on the host (this runs without a GPU).  Every rule of lft_refocus: the recorded case table of
    tests/abi_refusals_util.py, answered with the same code and the same words under the new name; then the new rules."""
    _lib.build()
    L = _lib.lib()
    plain = [(case, args) for entry, case, args in U.cases() if entry == "lft_refocus"]
    assert len(plain) >= 40 and {"taps3", "D0", "null_out", "out_class_9", "span_rows", "too_many_blocks", "empty_B", "stride5_neg"} <= {c for c, _ in plain}
    refused = 0
    for case, args in plain:
        rc = L.lft_refocus(*args)
        want = L.lft_last_error().decode() if rc else ""
        L.lft_scene_counts(1, 1, 1, 1, None, None)                             # leaves another call's message behind
        assert L.lft_aif_at(*aif_args(args)) == rc, case
        if rc:
            got = L.lft_last_error().decode()
            assert got.startswith("lft_aif_at:") and got == want.replace("lft_refocus:", "lft_aif_at:", 1), (case, got, want)
            refused += 1
    assert refused >= 35
    st = U._ll(0, 500, 100, 10, 1, 0)
    good = (P, _lib.LF_UINT8, 1, 5, 10, 10, 1, st, Q, 3, 4, P + (1 << 18), _lib.LF_FLOAT32, None)       # lft_refocus's good case
    for kw, rc, words in ((dict(n=-1), ERR_ARG, "-1 subsets outside 0 .. 4"), (dict(n=5), ERR_ARG, "5 subsets outside 0 .. 4"),
                          (dict(subsets=None), ERR_ARG, "subsets table must be null exactly when P = 0"),
                          (dict(n=0), ERR_ARG, "subsets table must be null exactly when P = 0"),
                          (dict(index=None), ERR_ARG, "null pointer")):
        L.lft_scene_counts(1, 1, 1, 1, None, None)
        assert L.lft_aif_at(*aif_args(good, **kw)) == rc, kw
        msg = L.lft_last_error().decode()
        assert msg.startswith("lft_aif_at:") and words in msg, (kw, msg)
    # lft_refocus's rules come first; the subsets' before the null maps; the block count of the 32 x 8 tiles last
    for change, kw, words in (({10: 3}, dict(n=9), "3 taps"), ({9: 0}, dict(n=9), "0 slopes"), ({4: -1}, dict(n=9), "negative size"),
                              ({}, dict(n=9, index=None), "subsets outside"), ({}, dict(subsets=None, index=None), "subsets table"),
                              ({11: None}, dict(n=7), "subsets outside")):
        bad = list(good)
        for i, v in change.items():
            bad[i] = v
        assert L.lft_aif_at(*aif_args(bad, **kw)) in (ERR_ARG, ERR_SHAPE) and words in L.lft_last_error().decode(), (change, kw, L.lft_last_error())
    many = list(good)                                                          # 2^16 images of 2^14 square tiles (2^30), of 2^16 tiles of 32 x 8 (2^32)
    many[2], many[4], many[5], many[7], many[9] = 1 << 16, 1 << 12, 1 << 12, U._ll(0, 0, 0, 1 << 12, 1, 0), 1
    assert L.lft_aif_at(*aif_args(many)) == ERR_SHAPE and b"lft_aif_at: 65536 images of 4096 x 4096 need more than 2^31 blocks" in L.lft_last_error()
    # empty shapes are no error and no work, null pointers included; the subsets' two rules are still judged
    for i in (2, 4, 5):
        empty = list(good)
        empty[i] = 0
        empty[0] = empty[7] = empty[8] = empty[11] = None
        assert L.lft_aif_at(*aif_args(empty, index=None)) == 0, i
        assert L.lft_aif_at(*aif_args(empty, subsets=None, n=0, index=None)) == 0, i
        assert L.lft_aif_at(*aif_args(empty, n=7)) == ERR_ARG and L.lft_aif_at(*aif_args(empty, subsets=None)) == ERR_ARG, i


# ---- 3. Python refusals need no device ----
def test_python_refusals_need_no_device():
    lf, sl = torch.zeros(3, 3, 6, 7), [-1.0, 0.0, 1.0]
    index, subset = torch.zeros(6, 7, dtype=torch.int32), torch.zeros(6, 7, dtype=torch.uint8)
    with pytest.raises(LftError, match="all_in_focus = subset needs occlusion"):
        Dm.disparity(lf, sl, all_in_focus="subset")
    with pytest.raises(LftError, match="all_in_focus = subset needs occlusion"):
        Dm.disparity(lf, sl, all_in_focus="subset", regularize=dict(p1=0.1, p2=1.0))
    with pytest.raises(LftError, match="all_in_focus must be False, True or subset"):
        Dm.disparity(lf, sl, all_in_focus="subsets", occlusion="halves")
    with pytest.raises(LftError, match="a subset map needs occlusion"):
        Dm.all_in_focus_at(lf, sl, index, subset)
    for bad_index in (index.long(), index.float(), torch.zeros(7, 6, dtype=torch.int32), torch.zeros(1, 6, 7, dtype=torch.int32), index.numpy(), None):
        with pytest.raises(LftError, match="the index must be a torch.int32 tensor of shape \\[6, 7\\]"):
            Dm.all_in_focus_at(lf, sl, bad_index, occlusion="halves")
    for bad_subset in (subset.int(), subset.bool(), torch.zeros(6, 8, dtype=torch.uint8), torch.zeros(6, 7, 1, dtype=torch.uint8), subset.numpy()):
        with pytest.raises(LftError, match="the subset must be a torch.uint8 tensor of shape \\[6, 7\\]"):
            Dm.all_in_focus_at(lf, sl, index, bad_subset, occlusion="halves")
    # a batch of mosaics takes maps [B, H, W]
    batch = torch.zeros(2, 1, 18, 21)
    with pytest.raises(LftError, match="shape \\[2, 6, 7\\]"):
        Dm.all_in_focus_at(batch, sl, index, angRes=3)
    # devices that differ
    with pytest.raises(LftError, match="the index is on meta, the light field on cpu"):
        Dm.all_in_focus_at(lf, sl, index.to("meta"))
    with pytest.raises(LftError, match="the subset is on meta, the light field on cpu"):
        Dm.all_in_focus_at(lf, sl, index, subset.to("meta"), occlusion="quadrants")
    # the arguments of the sweep and of occlusion, with their own words
    for kw, words in ((dict(interp="sinc"), "interp"), (dict(occlusion="thirds"), "subsets must be"), (dict(occlusion=dict(min_views=1)), "min_views"),
                      (dict(out_dtype=torch.float64), "out_dtype")):
        with pytest.raises(LftError, match=words):
            Dm.all_in_focus_at(lf, sl, index, **kw)
    with pytest.raises(LftError, match="strictly increasing"):
        Dm.all_in_focus_at(lf, [0.0, 0.0], index)
    # everything right: the device is asked for last
    for kw in (dict(), dict(occlusion="halves"), dict(subset=subset, occlusion="quadrants"), dict(subset=subset, occlusion=dict(subsets=np.ones((1, 3, 3), bool)))):
        with pytest.raises(LftError, match="no CPU path"):
            Dm.all_in_focus_at(lf, sl, index, **kw)
    with pytest.raises(LftError, match="no CPU path"):
        Dm.disparity(lf, sl, all_in_focus="subset", occlusion="halves")
    with pytest.raises(LftError, match="no CPU path"):
        Dm.disparity(lf, sl, all_in_focus="subset", occlusion="halves", regularize=dict(p1=0.1, p2=1.0))
    Dm.clear_cache()


# ---- 4. the table identity the GPU anchors rest on ----
@pytest.mark.parametrize("centre", [None, (0, 0)])
@pytest.mark.parametrize("mode", ["halves", "quadrants"])
@pytest.mark.parametrize("aperture", ["full", "gaussian", "disk", "held_out"])
@pytest.mark.parametrize("A", [2, 3, 5])
def test_a_subset_row_is_the_masked_apertures_column(A, aperture, mode, centre):
    """Row b_p of subset_table equals the `a` column of shift_table run with the aperture a * mask_p, bit for bit, and its skip
    flags equal b_p == 0: "the mean of subset p at slope k" is what lft_refocus computes with that aperture."""
    if aperture == "disk" and A == 2:
        aperture = R.aperture_weights(2, "disk", radius=1.0)                    # the default radius of A = 2 keeps no view
    elif aperture == "held_out":                                               # the full aperture without the view (0, 0)
        aperture = np.ones((A, A))
        aperture[0, 0] = 0
    a = R._aperture(A, aperture)
    try:
        btable, kept = Dm.subset_table(A, aperture, centre, mode)
    except LftError:
        assert A == 2 and mode == "quadrants" and centre is None                # one view per quadrant: none is kept
        return
    masks = AU.subset_masks(A, centre, mode)
    assert len(kept) >= 1
    for row, p in enumerate(kept):
        for interp in ("nearest", "linear", "cubic"):
            t = R.shift_table(A, RU.SLOPES, a * masks[p], interp, centre)
            assert np.array_equal(t["a"].view(np.int32), np.broadcast_to(btable[row].view(np.int32), t["a"].shape)), (p, interp)
            assert np.array_equal(t["skip"] != 0, np.broadcast_to(btable[row] == 0, t["skip"].shape))
            whole = R.shift_table(A, RU.SLOPES, aperture, interp, centre)
            want = AU.masked_table(whole, btable[row])
            assert t.tobytes() == want.tobytes()                                # nothing else of a record depends on the aperture


# ---- 5. the restatement's own properties ----
def test_restatement_properties():
    rng = np.random.default_rng(5)
    A, H, W, C = 3, 6, 7, 2
    L = rng.random((A, A, H, W, C)).astype(np.float32)
    slopes = [-1.0, 0.5, 2.0]
    table = R.shift_table(A, slopes, "gaussian", "linear")
    bt, _ = Dm.subset_table(A, "gaussian", None, "quadrants")
    stack = RU.refocus_np(L, table, 2)
    index = rng.integers(0, 3, (H, W)).astype(np.int32)
    take = lambda st, k: np.take_along_axis(st, k[None, :, :, None].astype(np.int64).repeat(C, 3), 0)[0]
    # subset all 0 (or None) gives refocus_np at the index, with and without a table of subsets
    for btable, subset in ((None, None), (bt, None), (bt, np.zeros((H, W), np.uint8))):
        assert np.allclose(AU.aif_at_np(L, table, 2, btable, index, subset), take(stack, index), rtol=0, atol=1e-15)
    # ids above P count as 0
    ids = rng.integers(0, 5, (H, W)).astype(np.uint8)
    over = np.where(ids == 0, 9, ids).astype(np.uint8)
    assert np.array_equal(AU.aif_at_np(L, table, 2, bt, index, over), AU.aif_at_np(L, table, 2, bt, index, ids))
    assert np.array_equal(AU.aif_at_np(L, table, 2, bt[:2], index, ids), AU.aif_at_np(L, table, 2, bt[:2], index, np.where(ids > 2, 0, ids)))
    assert np.array_equal(AU.aif_at_np(L, table, 2, None, index, ids), AU.aif_at_np(L, table, 2, None, index, None))
    # the index is clamped
    wild = index.copy()
    wild[0], wild[1] = -7, 11
    assert np.array_equal(AU.aif_at_np(L, table, 2, bt, wild, ids), AU.aif_at_np(L, table, 2, bt, np.clip(wild, 0, 2), ids))
    # p >= 1 is refocus_np with the masked table, pixel by pixel
    got = AU.aif_at_np(L, table, 2, bt, index, ids)
    for p in range(1, 5):
        want = take(RU.refocus_np(L, AU.masked_table(table, bt[p - 1]), 2), index)
        assert (ids == p).any() and np.allclose(got[ids == p], want[ids == p], rtol=0, atol=1e-15)
    # a record's skip holds for a subset too: a view of weight 0 in the table stays out even where b_p names it
    held = table.copy()
    held["skip"][:, 0] = 1
    assert not np.array_equal(AU.aif_at_np(L, held, 2, bt, index, ids)[ids == 1], got[ids == 1])


# ---- 6. the defect and its repair on the two-layer scene, on the restatement alone ----
def scene_images(L, subsets, unrounded=False):
    """(today's image: m gathered at the occlusion-aware index; the new image: the winning subset's mean there), fp64 [H, W].
    unrounded: the new image with the rows a / W_p as fp64, before their one rounding to fp32 (their sum is then 1 to 2^-52)."""
    S = OU.SCENE
    taps = R.TAPS[S["interp"]]
    table = R.shift_table(S["A"], OU.SLOPES, "full", S["interp"])
    btable, kept = Dm.subset_table(S["A"], "full", None, subsets)
    o = OU.occ_cost_np(L, table, taps, btable, S["beta"])
    k = np.argmin(DU.aggregate_np(o["V"], S["radius"]), 0)
    chosen = np.take_along_axis(o["choice"], k[None], 0)[0]
    today = np.take_along_axis(o["m"][..., 0], k[None], 0)[0]
    if unrounded:
        rows = R.aperture_weights(S["A"]).reshape(-1) * AU.subset_masks(S["A"], None, subsets)[list(kept)].reshape(len(kept), -1)
        btable = rows / rows.sum(1, keepdims=True)
    return today, AU.aif_at_np(L, table, taps, btable, k.astype(np.int32), chosen)[..., 0]


@pytest.mark.parametrize("subsets", ["halves", "quadrants"])
def test_the_scene_shows_the_ghost_and_the_new_image_has_none(subsets):
    band = OU.band()
    clean, centre = DU.two_layer(5, 40, 40, box=OU.BOX)
    centre = centre.astype(np.float64)
    today, new = scene_images(OU.noisy_two_layer(), subsets)
    off_today, off_new = np.abs(today - centre)[band], np.abs(new - centre)[band]
    print(f"{subsets}, noisy: today off by > 0.05 at {int((off_today > 0.05).sum())} of {int(band.sum())} band pixels (max {off_today.max():.4f}), "
          f"the winning subset's mean at {int((off_new > 0.05).sum())} (max {off_new.max():.4f})")
    assert band.sum() == 320
    assert int((off_today > 0.05).sum()) >= 100
    assert int((off_new > 0.05).sum()) == 0
    # Clean: every view of the winning subset sees the centre view's value, so the mean is that value times the sum of the weights.
    # With the rows as fp64 that sum is 1 and the image is the centre view within 1e-12; each fp32-rounded b_p is off by at most
    # 2^-24 of itself, so their sum by at most 2^-24, and the image by that times the largest value (< 1).
    _, new_clean = scene_images(clean, subsets, unrounded=True)
    err = float(np.abs(new_clean - centre)[band].max())
    _, new_rounded = scene_images(clean, subsets)
    err_rounded = float(np.abs(new_rounded - centre)[band].max())
    print(f"{subsets}, clean: the winning subset's mean is within {err:.2e} of the centre view on the band, {err_rounded:.2e} with the fp32-rounded rows")
    assert err <= 1e-12
    assert err_rounded <= 2.0 ** -24 + 1e-12
