"""GPU parity tests (run on the MI355X box with -m gpu): every stage of the HIP path, called through
the C ABI of liblft_hip.so, against the CPU oracle on the same seeded inputs, and the whole forward
against the fixtures captured from the real reference.

Tolerances (BASELINE.json north_star: 1e-3 relative fp32):
  fp32 path : max|err| <= 1e-4 * max|ref| per stage (observed ~1e-6), <= 1e-3 * max|ref| required end to end
  fp16 path : rms err <= 2e-3 * rms(ref) per stage; <= 1e-3 * max|ref| required end to end (observed ~2e-4: the bf16 kernels with
              IEEE-half operands and tensors -- the fast path that meets north_star)
  bf16 path : rms err <= 1e-2 * rms(ref) per stage; end to end bounded at 2.5e-3 * max|ref| (observed 1.5e-3 .. 1.9e-3: bf16 operand
              rounding, tests/diag_precision_study.py -- this path does NOT meet the 1e-3 of north_star; the fp32 and fp16 paths do)
  fp16 and bf16 stages additionally: the LOCALIZED gates of tests/parity_gates.py -- the kernel's error against the error of the rounding
              model of that precision (oracle/lft_oracle_lp.py) on the same input, in max norm, per token, image position, view, channel
              and batch element, each within M = 2 of the model.  A global rms cannot see one wrong token or column; these can
              (tests/test_parity_gates.py).  Every stage test prints its six ratios.
  VIEW_CASES (one shape per angular-attention code path: V = 1, 16, 49, 64, 100, 121) and test_ang_block_many_positions, fp32
              additionally: max|err| <= 1e-4 * max|ref| VIEW BY VIEW, over each view's own maximum -- a wrong view of the last key
              tile cannot hide behind a larger one.
  SPA_CLASS   one view size per class of the spatial path's shape-dependent dispatch (partial and mid-row 128-token tiles, ragged
              k_spa_b query tiles, either hand-off layout, either ring chunk of k_spa1); each case asserts its class from
              tests/spa_classes.py, fills its outputs with NaN in front of 64 guard elements, holds fp32 view by view and requires a
              clean status word.  Their forward additionally passes the localized gates on the residual branch (CHAIN_GATES).
              test_init_features_widest_view / test_too_wide_view_is_refused: the width limit (75 columns fp32, 347 in 16 bit).
"""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from lft_amd import _lib
from lft_amd.params import deterministic_state, synthetic_lr
from oracle import lft_oracle as O
from oracle import lft_oracle_lp as LP

import gpu_util as G
import parity_gates as PG
import spa_classes as S

pytestmark = pytest.mark.gpu

FP32_STAGE_TOL = 1e-4
BF16_STAGE_RMS = 1e-2
FP16_STAGE_RMS = 2e-3
END_TO_END = {"fp32": 1e-3, "fp16": 1e-3, "bf16": 2.5e-3}
ALL_PRECS = ["fp32", "fp16", "bf16"]
LFT_ERR_SHAPE = -2                  # include/lft_hip.h


def per_view_rel_max(got, ref, layout="act", A=None, s=None):
    """(worst max|err| / max|ref| over the views, each over its own maximum; that view's index)."""
    keep = PG._dims(layout)["view"]
    e, r = PG._shape(got - ref, layout, A, s).abs(), PG._shape(ref, layout, A, s).abs()
    red = tuple(d for d in range(e.dim()) if d not in keep)
    rel = (e.amax(dim=red) / r.amax(dim=red)).reshape(-1)
    return float(rel.max()), int(rel.argmax())


# A CHAIN of stages (the forward, the tail) against the model of the same chain: the kernel and the model round an intermediate
# tensor differently here and there (a value next to a rounding boundary), so their errors agree as distributions, no longer element
# by element.  A slice-wise rms comparison then needs slices with enough samples; in the "image" layout a `pos` slice holds B * A^2 of
# them (4 at A 2), and a second correct implementation of the policy (the model accumulated in fp64) reads 2 .. 8 in `pos` at every
# shape of SPA_CLASS while its other five gates stay below 1.05.  The chain checks assert those five.
CHAIN_GATES = tuple(g for g in PG.GATES if g != "pos")


def check(got, ref, prec, what, model=None, layout="act", A=None, s=None, per_view=False, gates=PG.GATES):
    """`model` (16-bit precisions): () -> the rounding model's output for the input the kernel saw.
    `per_view` (fp32): the 1e-4 of the stage also view by view.  `gates`: the localized gates that are asserted (all are printed)."""
    msg = f"{what} [{prec}]: " + G.err_report(got, ref)
    assert not torch.isnan(got).any(), msg
    if prec == "fp32":
        assert G.rel_max(got, ref) <= FP32_STAGE_TOL, msg
        if per_view:
            worst, view = per_view_rel_max(got, ref, layout, A, s)
            msg += f" per-view rel_max {worst:.3e} (view {view})"
            assert worst <= FP32_STAGE_TOL, msg
    else:
        assert G.rel_rms(got, ref) <= (FP16_STAGE_RMS if prec == "fp16" else BF16_STAGE_RMS), msg
        with torch.no_grad():
            ratios, text = PG.gate_report(got, ref, model(), layout, A, s)
        msg += f"\n{what} [{prec}] gates: {text}"
        print(msg)
        assert not [g for g in PG.failed(ratios) if g in gates], msg
        return
    print(msg)


@pytest.mark.parametrize("prec", ALL_PRECS)
def test_mfma_fragment_layout(prec):
    """C = A B and D = W2 C with asymmetric small-integer data (exact in bf16 and fp32)."""
    rng = np.random.default_rng(0)
    Am = torch.from_numpy(rng.integers(-3, 4, size=(32, 16)).astype(np.float32))
    Bm = torch.from_numpy(rng.integers(-3, 4, size=(16, 32)).astype(np.float32))
    W2 = torch.from_numpy(rng.integers(-2, 3, size=(32, 32)).astype(np.float32))
    C = torch.zeros(32, 32, device=G.DEV)
    D = torch.zeros(32, 32, device=G.DEV)
    a, b, w2 = Am.to(G.DEV), Bm.to(G.DEV), W2.to(G.DEV)
    _lib.call("lft_mfma_selftest", a.data_ptr(), b.data_ptr(), w2.data_ptr(), C.data_ptr(), D.data_ptr(), G.PRECS[prec], G.stream())
    torch.cuda.synchronize()
    Cref = Am @ Bm
    assert torch.equal(C.cpu(), Cref), "C = A*B layout wrong"
    if prec == "fp32":      # |C| can exceed bf16's exact-integer range, so D is only exact in fp32
        assert torch.equal(D.cpu(), W2 @ Cref), "acc-order operand re-use wrong"
    else:
        assert G.rel_max(D.cpu(), W2 @ Cref.to(G.ACT_DTYPE[prec]).float()) < 1e-6


@pytest.mark.parametrize("A,h,w,s", [(3, 7, 5, 2), (5, 8, 8, 4), (2, 4, 9, 4)])
def test_bicubic(A, h, w, s):
    lr = torch.from_numpy(synthetic_lr(2, A, h, w, seed=3))
    out = torch.empty(2, 1, A * h * s, A * w * s, device=G.DEV)
    x = lr.to(G.DEV)
    _lib.call("lft_bicubic_fwd", x.data_ptr(), out.data_ptr(), 2, A, h, w, s, G.stream())
    torch.cuda.synchronize()
    ref = O.bicubic_skip(lr, A, s)
    assert (out.cpu() - ref).abs().max() <= 2e-6, G.err_report(out.cpu(), ref)


CASES = [(5, 2, 2, 6, 6), (5, 4, 1, 8, 8), (3, 2, 1, 9, 7), (5, 2, 1, 32, 32), (9, 4, 1, 8, 8), (6, 2, 1, 6, 5),   # 81 views: 3 column tiles; 36: 2
         (2, 2, 1, 64, 64),                   # 64-wide views: two column tiles per row, wide-tile LDS path
         (2, 2, 1, 6, 12), (2, 2, 1, 36, 64)]  # h < w: queries with x - 2 >= h have an EMPTY window (LFT.py:155) -> attention output 0
# One shape per angular-attention code path that the cases above leave out, at the smallest views where every kernel still has work
# (12 .. 42 positions per batch element; four of the six with an odd B*h*w: the last two-position group of the 16-bit k_ang_multi is
# half empty): V = 1 and 16 (k_ang), 49 (17 rows in the last key tile), 64 (a full last tile), 100 and 121 (four key tiles).
VIEW_CASES = [(1, 2, 2, 6, 7), (4, 2, 1, 5, 5), (7, 2, 1, 3, 5), (8, 2, 1, 5, 3), (10, 4, 1, 3, 5), (11, 2, 1, 4, 3)]
CASES += VIEW_CASES

# ---------------------------------------------------------------------------------------------------- view-size classes
# Every case above has either h*w < 128 (one partial 128-token tile per view image, starting at token 0) or w in {32, 64} with
# h*w % 128 == 0 (every tile full and starting at column 0 of an image row).  The cases below are one view size per remaining class
# of the spatial path's dispatch -- front-end convolutions, k_spa1, k_spa_b / k_win_attn_lds + k_spa2, k_up + k_assemble_t.  The
# class a case was chosen for is asserted from tests/spa_classes.py (assert_class), so a changed constant cannot move it silently.
# h = w - 2 wherever attention matters: no query has an empty window (min(h, x + 3) empties columns x >= h + 2).
#   lm32 / lm16   lane-major hand-off k_spa1 -> part B (and last block -> k_up inside lft_forward) in fp32 / in the 16-bit precisions
#   ch32 / ch16   k_spa1's ring chunk
#   tiles, waves  128-token tiles per view image and the valid tokens of the LAST tile's four waves (store_tile's nvalid)
#   tx, ty, lc, lr  k_spa_b's 4 x 32 query tiles per image, columns / rows of the last one
#   straddle      h*w % 32 != 0: the flat 32-token tiles of k_spa2 / k_up straddle view images
Cls = namedtuple("Cls", "lm32 lm16 ch32 ch16 tiles waves tx ty lc lr straddle")
FULL = (32, 32, 32, 32)
SPA_CLASS = {
    (2, 2, 1, 13, 11): Cls(False, False, 16, 16, 2, (15, 0, 0, 0), 1, 4, 11, 1, True),     # 143 tokens: a second tile with p0 > 0, waves 1..3 empty
    (3, 2, 2, 17, 19): Cls(False, False, 16, 16, 3, (32, 32, 3, 0), 1, 5, 19, 1, True),    # a middle tile with neither clamp active; 18 images
    (2, 2, 1, 16, 24): Cls(True, False, 16, 16, 3, FULL, 1, 4, 24, 4, False),              # fp32 lane-major with tiles starting mid-row; columns 18..23: empty windows
    (2, 4, 1, 24, 16): Cls(True, False, 16, 16, 3, FULL, 1, 6, 16, 4, False),              # fp32 lane-major, row-aligned tiles; GT = 2 in k_up
    (2, 4, 1, 35, 37): Cls(False, False, 16, 16, 11, (15, 0, 0, 0), 2, 9, 5, 3, True),     # row-major k_spa_b with two column tiles, the second 5 wide
    (2, 2, 1, 31, 32): Cls(False, False, 16, 16, 8, (32, 32, 32, 0), 1, 8, 32, 3, False),  # w % 32 == 0 but h*w % 128 = 96: row-major, full column tile, 3-row last tile
    (2, 2, 1, 62, 64): Cls(True, True, 8, 8, 31, FULL, 2, 16, 32, 2, False),               # 16-bit lane-major with a 2-row last tile; CH 8; lane-major tail in the forward
    # launch_spa1's ring-chunk switch, each side of it in the precisions it is about
    (2, 2, 2, 53, 55): Cls(False, False, 16, 16, 23, (32, 32, 32, 3), 2, 14, 23, 1, True),   # 16 bit: the widest CH 16 (B 2: see below)
    (2, 2, 1, 54, 56): Cls(False, False, 16, 8, 24, (32, 32, 16, 0), 2, 14, 24, 2, True),    # 16 bit: the narrowest CH 8, row-major
    (2, 2, 1, 57, 59): Cls(False, False, 16, 8, 27, (32, 3, 0, 0), 2, 15, 27, 1, True),      # fp32: the widest CH 16, 163 072 B of LDS
    (2, 2, 1, 58, 60): Cls(False, False, 8, 8, 28, (24, 0, 0, 0), 2, 15, 28, 2, True),       # fp32: the narrowest CH 8
}
SPA_CASES = [c for c in SPA_CLASS if c[3] * c[4] < 2900]                                 # the full stage matrix
# Above 2900 tokens per view the oracle's forward takes most of a minute: init_features, spa_block 0 and 3, upsample and the forward
# only (the middle layers and the angular block do not depend on the view size), and only in the precisions the case is about.
# 53x55 has two batch elements: with one, the up-sampler's `pos` gate (B * A^2 = 4 samples per slice, 11 660 slices) reads 1.55 in fp16
# for the rounding model accumulated in fp64 -- above the 1.5 a case must leave to a second correct implementation; with two, 1.15.
BIG_PRECS = {(2, 2, 1, 62, 64): ALL_PRECS, (2, 2, 2, 53, 55): ["fp16", "bf16"], (2, 2, 1, 54, 56): ["fp16", "bf16"],
             (2, 2, 1, 57, 59): ["fp32"], (2, 2, 1, 58, 60): ["fp32"]}
assert set(SPA_CASES) | set(BIG_PRECS) == set(SPA_CLASS) and not set(SPA_CASES) & set(BIG_PRECS)
SHARED_WITH_TAIL = {(2, 2, 1, 16, 24), (2, 4, 1, 24, 16), (2, 2, 1, 62, 64)}               # tests/test_gpu_tail.py uses the same oracle run
CASES += SPA_CASES
CASE_ID = lambda c: "A%d_s%d_B%d_%dx%d" % c


def assert_class(shape, prec):
    A, s, B, h, w = shape
    want, got = SPA_CLASS[shape], S.classify(h, w, prec)
    f32 = prec == "fp32"
    assert (got.lane_major, got.chunk) == ((want.lm32, want.ch32) if f32 else (want.lm16, want.ch16)), (shape, prec, got)
    assert (got.tiles, S.wave_valid(h, w, got.tiles - 1), got.tiles_x, got.tiles_y, got.last_cols, got.last_rows, got.straddle) == \
        (want.tiles, want.waves, want.tx, want.ty, want.lc, want.lr, want.straddle), (shape, prec, got)
    assert got.last_tile == sum(want.waves) and LP.lane_major(h, w) == want.lm16


def make_case(shape):
    A, s, B, h, w = shape
    sd_np, sd, lr, taps, out = G.oracle_case(*shape, keep=shape in SHARED_WITH_TAIL)
    packs = {p: G.Packed(sd_np, A, h, w, s, p, B) for p in (BIG_PRECS.get(shape) or ALL_PRECS)}
    # strict (the view-size cases): the class table, the per-view fp32 bound, a clean status word after every call
    return dict(shape=shape, A=A, s=s, B=B, h=h, w=w, sd=sd, lr=lr, taps=taps, out=out, packs=packs, mask=O.window_mask(h, w),
                strict=shape in SPA_CLASS, per_view=shape in VIEW_CASES or shape in SPA_CLASS)


@pytest.fixture(scope="module", params=CASES, ids=CASE_ID)
def case(request):
    return make_case(request.param)


_BIG = {}


@pytest.fixture(scope="module", params=[(c, p) for c in BIG_PRECS for p in BIG_PRECS[c]], ids=lambda cp: CASE_ID(cp[0]) + "-" + cp[1])
def big(request):
    """(case, prec) of the reduced matrix; the case is built once for its precisions and dropped when the next one starts."""
    shape, prec = request.param
    if shape not in _BIG:
        _BIG.clear()
        _BIG[shape] = make_case(shape)
    return _BIG[shape], prec


def begin(case, prec):
    """The packed weights of a stage call; on a view-size case first the class it stands for, and a cleared status word."""
    pk = case["packs"][prec]
    if case["strict"]:
        assert_class(case["shape"], prec)
        G.status_reset(pk)
    return pk


def end(case, pk, buf, what):
    """After the call: nothing written behind the output; view-size cases: the clamped lanes of partial tiles raised no flag."""
    torch.cuda.synchronize()
    assert G.guard_intact(buf), f"{what}: the {G.GUARD} elements behind the output were written"
    if case["strict"]:
        assert G.status_flags(pk) == (0, 0), f"{what}: status word {G.status_flags(pk)} ({_lib.lib().lft_last_error().decode()})"


def run_init_features(case, prec):
    pk = begin(case, prec)
    lr = case["lr"].to(G.DEV)
    buf, act = G.guarded(pk.new_act().shape, G.ACT_DTYPE[prec])
    _lib.call("lft_init_features_fwd", pk.buf.data_ptr(), lr.data_ptr(), act.data_ptr(), pk.work.data_ptr(), *pk.dims(), G.stream())
    end(case, pk, buf, "init_features")
    check(G.from_act(act), case["taps"]["feat"], prec, "init_features",
          lambda: LP.init_features(case["sd"], O.mosaic_to_views(case["lr"], case["A"]), prec), per_view=case["per_view"])


def run_spa_block(case, prec, layer, with_skip):
    pk = begin(case, prec)
    xin = G.to_act(case["taps"][f"ang{layer}"], prec)
    skip = G.to_act(case["taps"]["feat"], prec) if with_skip else None
    ref = O.spa_block(case["sd"], layer, G.from_act(xin), case["mask"])
    if with_skip:
        ref = ref + G.from_act(skip)
    buf, act = G.guarded(pk.new_act().shape, G.ACT_DTYPE[prec])
    _lib.call("lft_spa_block_fwd", pk.buf.data_ptr(), layer, xin.data_ptr(), skip.data_ptr() if with_skip else None, act.data_ptr(),
              pk.work.data_ptr(), *pk.dims(), G.stream())
    end(case, pk, buf, f"spa_block{layer}")
    check(G.from_act(act), ref, prec, f"spa_block{layer}",
          lambda: LP.spa_block(case["sd"], layer, G.from_act(xin), prec, case["mask"], G.from_act(skip) if with_skip else None),
          per_view=case["per_view"])


def run_upsample(case, prec):
    pk = begin(case, prec)
    xin = G.to_act(case["taps"]["body"], prec)
    lr = case["lr"].to(G.DEV)
    A, s, B, h, w = case["shape"]
    buf, out = G.guarded((B, 1, A * h * s, A * w * s), torch.float32)
    _lib.call("lft_upsample_fwd", pk.buf.data_ptr(), xin.data_ptr(), lr.data_ptr(), out.data_ptr(), pk.work.data_ptr(), *pk.dims(), G.stream())
    end(case, pk, buf, "upsample")
    ref = O.upsample(case["sd"], O.views_to_mosaic(G.from_act(xin), A), s)
    skip = case["taps"]["skip"]
    check(out.cpu() - skip, ref, prec, "upsample(residual branch)",
          lambda: LP.upsample(case["sd"], O.views_to_mosaic(G.from_act(xin), A), s, prec), "image", A, s, per_view=case["per_view"])


def run_forward(case, prec):
    pk = begin(case, prec)
    lr = case["lr"].to(G.DEV)
    A, s, B, h, w = case["shape"]
    buf, out = G.guarded((B, 1, A * h * s, A * w * s), torch.float32)
    _lib.call("lft_forward", pk.buf.data_ptr(), lr.data_ptr(), out.data_ptr(), pk.work.data_ptr(), *pk.dims(), G.stream())
    end(case, pk, buf, "forward")
    got, ref = out.cpu(), case["out"]
    msg = f"forward [{prec}] " + G.err_report(got, ref) + f" psnr={O.psnr(got, ref):.2f}dB"
    print(msg)
    assert not torch.isnan(got).any(), msg
    assert G.rel_max(got, ref) <= END_TO_END[prec], msg
    res_got, res_ref = got - case["taps"]["skip"], case["taps"]["res"]
    assert G.rel_rms(res_got, res_ref) <= {"fp32": 1e-4, "fp16": 4e-3, "bf16": 2e-2}[prec], "residual branch: " + G.err_report(res_got, res_ref)
    if case["strict"] and prec != "fp32":
        # The max norm and the residual rms above are blind to one wrong token or column (a lane-major tail that misplaces a tile):
        # the localized gates on the residual branch, against the rounding model of the whole forward.
        with torch.no_grad():
            model = LP.forward(case["sd"], case["lr"], A, s, prec) - case["taps"]["skip"]
        ratios, text = PG.gate_report(res_got, res_ref, model, "image", A, s)
        print(f"forward [{prec}] gates: {text}")
        assert not [g for g in PG.failed(ratios) if g in CHAIN_GATES], text


@pytest.mark.parametrize("prec", ALL_PRECS)
def test_init_features(case, prec):
    run_init_features(case, prec)


@pytest.mark.parametrize("prec", ALL_PRECS)
@pytest.mark.parametrize("layer", [0, 1, 2, 3])
def test_ang_block(case, prec, layer):
    pk = begin(case, prec)
    x = case["taps"]["feat"] if layer == 0 else case["taps"][f"spa{layer - 1}"]
    xin = G.to_act(x, prec)
    ref = O.ang_block(case["sd"], layer, G.from_act(xin))       # oracle sees the same (possibly bf16-rounded) input
    buf, act = G.guarded(pk.new_act().shape, G.ACT_DTYPE[prec])
    _lib.call("lft_ang_block_fwd", pk.buf.data_ptr(), layer, xin.data_ptr(), act.data_ptr(), *pk.dims(), G.stream())
    torch.cuda.synchronize()
    assert G.guard_intact(buf), "ang_block: the elements behind the output were written"
    check(G.from_act(act), ref, prec, f"ang_block{layer}", lambda: LP.ang_block(case["sd"], layer, G.from_act(xin), prec),
          per_view=case["per_view"])


@pytest.mark.parametrize("prec", ALL_PRECS)
@pytest.mark.parametrize("layer,with_skip", [(0, False), (1, False), (2, False), (3, True)])
def test_spa_block(case, prec, layer, with_skip):
    run_spa_block(case, prec, layer, with_skip)


@pytest.mark.parametrize("prec", ALL_PRECS)
def test_upsample(case, prec):
    run_upsample(case, prec)


@pytest.mark.parametrize("prec", ALL_PRECS)
def test_forward_vs_oracle(case, prec):
    run_forward(case, prec)


# The reduced matrix of the view sizes above 2900 tokens (BIG_PRECS): the same stage checks, one test per (case, precision).
def test_init_features_big(big):
    run_init_features(*big)


@pytest.mark.parametrize("layer,with_skip", [(0, False), (3, True)])
def test_spa_block_big(big, layer, with_skip):
    run_spa_block(*big, layer, with_skip)


def test_upsample_big(big):
    run_upsample(*big)


def test_forward_vs_oracle_big(big):
    run_forward(*big)


# ---------------------------------------------------------------------------------------------------- the width limit
# The conv input tile in LDS grows with the view width; allow_lds (lft_host.cuh) refuses what no longer fits into the 160 KiB of a
# CU, on the host, before anything is launched.  Widest accepted view: 75 columns in fp32 (k_conv64), 347 in the 16-bit precisions
# (k_conv64_lr); k_spa1 accepts more (155 / 471: tests/test_spa_classes.py), so the weights still pack at these widths.
WIDE_H = 3


@pytest.mark.parametrize("prec", ALL_PRECS)
def test_init_features_widest_view(prec):
    """lft_init_features_fwd alone at the widest view the front end accepts (the conv oracle is cheap at any width): A 2, 2x, 3 rows."""
    A, s, B, h, w = 2, 2, 1, WIDE_H, S.front_end_w_max(prec)
    assert w == (75 if prec == "fp32" else 347) and S.lds_front_end(prec, w) <= S.K_MAX_LDS < S.lds_front_end(prec, w + 1)
    sd_np = deterministic_state(64, s, seed=1, flavor="stress")
    sd = O.state_from_numpy(sd_np)
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0))
    views = O.mosaic_to_views(lr, A)
    with torch.no_grad():
        ref = O.init_features(sd, views)
    pk = G.Packed(sd_np, A, h, w, s, prec, B)
    x = lr.to(G.DEV)
    buf, act = G.guarded(pk.new_act().shape, G.ACT_DTYPE[prec])
    _lib.call("lft_init_features_fwd", pk.buf.data_ptr(), x.data_ptr(), act.data_ptr(), pk.work.data_ptr(), *pk.dims(), G.stream())
    torch.cuda.synchronize()
    assert G.guard_intact(buf), "init_features: the elements behind the output were written"
    check(G.from_act(act), ref, prec, f"init_features {h}x{w}", lambda: LP.init_features(sd, views, prec), per_view=True)


@pytest.mark.parametrize("prec", ALL_PRECS)
def test_too_wide_view_is_refused(prec):
    """One column more: lft_init_features_fwd and lft_forward return LFT_ERR_SHAPE, say that it is the width, and write nothing."""
    A, s, B, h, w = 2, 2, 1, WIDE_H, S.front_end_w_max(prec) + 1
    assert w <= S.spa1_w_max(prec)                                   # k_spa1 is not what refuses: the weights pack
    pk = G.Packed(deterministic_state(64, s, seed=1, flavor="stress"), A, h, w, s, prec, B)
    x = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0)).to(G.DEV)
    buf, act = G.guarded(pk.new_act().shape, G.ACT_DTYPE[prec])
    obuf, out = G.guarded((B, 1, A * h * s, A * w * s), torch.float32)
    L = _lib.lib()
    for what, rc in (("lft_init_features_fwd", L.lft_init_features_fwd(pk.buf.data_ptr(), x.data_ptr(), act.data_ptr(), pk.work.data_ptr(), *pk.dims(), G.stream())),
                     ("lft_forward", L.lft_forward(pk.buf.data_ptr(), x.data_ptr(), out.data_ptr(), pk.work.data_ptr(), *pk.dims(), G.stream()))):
        msg = L.lft_last_error().decode()
        assert rc == LFT_ERR_SHAPE, (what, rc, msg)
        assert "width" in msg and "LDS" in msg, (what, msg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(act).all()) and bool(torch.isnan(out).all()), "a refused call wrote to its output"
    assert G.guard_intact(buf) and G.guard_intact(obuf)
    with pytest.raises(_lib.LftError, match="width"):
        _lib.call("lft_forward", pk.buf.data_ptr(), x.data_ptr(), out.data_ptr(), pk.work.data_ptr(), *pk.dims(), G.stream())


# ---------------------------------------------------------------------------------------------------- beyond the grid cap
def ang_positions_per_sweep(V, prec):
    """Positions one launch of the angular block covers before its workgroups loop: lft_network.hip, ang_block / ang_multi and lds_ang
    re-derived -- grid = min(ceil(positions / per workgroup), 256 * max(1, 160 KiB / LDS per workgroup))."""
    esz = 4 if prec == "fp32" else 2
    fb = 1024 * (2 if prec == "fp32" else 1)                 # bytes of one weight / K / V fragment
    tile_io = 16 * (64 * esz + 16)                           # TileIO<2, T>::BYTES
    if V <= 32:                                              # k_ang: 4 waves = 4 positions, the 64 weight fragments in LDS
        lds, per_wg = 64 * fb + 1024 + 4 * tile_io, 4
    else:                                                    # k_ang_multi<CT, NG>
        ct = 4 if V > 96 else 3 if V > 64 else 2
        per_wg = 2 if esz == 2 and ct <= 3 else 1            # NG
        lds = (64 * fb if esz == 2 else 0) + 1024 + per_wg * ct * 8 * fb + per_wg * ct * tile_io
    assert lds <= 160 * 1024
    return 256 * max(1, 160 * 1024 // lds) * per_wg


MANY_B, MANY_W = 3, 35


def many_positions_h(V, prec):
    h = 11
    while MANY_B * h * MANY_W <= ang_positions_per_sweep(V, prec):
        h += 2                                               # stays odd
    return h


_MANY_X = {}


@pytest.mark.parametrize("prec", ALL_PRECS)
@pytest.mark.parametrize("A", [1, 4, 6, 7, 8, 9, 10, 11])
def test_ang_block_many_positions(A, prec):
    """lft_ang_block_fwd alone (layer 0) on more positions than one sweep of the grid covers, so that workgroups take the
    grid-stride loop, with an odd position count: B 3, w 35, h 11 -> 1155 positions (h*w = 385 is odd too: groups of 2 or 4
    positions straddle batch elements, and the last two-position group of the 16-bit k_ang_multi is half empty).

    Positions per sweep (ang_positions_per_sweep):
        A (V)           kernel                  fp32    fp16 / bf16
        1, 4 (1, 16)    k_ang<13>               1024    2048  -> h = 21 there: 2205 positions
        6, 7 (36, 49)   k_ang_multi<2, LL 9>     768     512
        8 (64)          k_ang_multi<2, LL 16>    768     512
        9 (81)          k_ang_multi<3, LL 9>     512     512
        10 (100)        k_ang_multi<4, LL 9>     256     256
        11 (121)        k_ang_multi<4, LL 13>    256     256
    The input is a seeded normal tensor rounded to the activation type (no network in front: the oracle's other stages at
    140 k tokens are the slow part).  The output buffer is pre-filled with NaN, so check() also proves that every token was
    stored, and 64 elements behind it must stay as they were."""
    V, B, w, s = A * A, MANY_B, MANY_W, 2
    h = many_positions_h(V, prec)
    cap = ang_positions_per_sweep(V, prec)
    assert cap == {("k_ang", True): 1024, ("k_ang", False): 2048, (2, True): 768, (2, False): 512, (3, True): 512, (3, False): 512,
                   (4, True): 256, (4, False): 256}[("k_ang" if V <= 32 else (V + 31) // 32, prec == "fp32")]
    assert B * h * w > cap and (B * h * w) % 2 == 1 and h == (21 if V <= 32 and prec != "fp32" else 11)
    sd_np = deterministic_state(64, s, seed=1, flavor="stress")
    sd = O.state_from_numpy(sd_np)
    if (A, h) not in _MANY_X:
        _MANY_X[(A, h)] = torch.randn(B, 64, V, h, w, generator=torch.Generator().manual_seed(1000 + A))
    xin = G.to_act(_MANY_X[(A, h)], prec)
    pk = G.Packed(sd_np, A, h, w, s, prec, B, work=False)
    n = B * V * h * w * 64
    buf = torch.full((n + 64,), float("nan"), dtype=G.ACT_DTYPE[prec], device=G.DEV)
    buf[n:] = -7.0
    act = buf[:n].view(B, V, h, w, 64)
    with torch.no_grad():
        ref = O.ang_block(sd, 0, G.from_act(xin))
    _lib.call("lft_ang_block_fwd", pk.buf.data_ptr(), 0, xin.data_ptr(), act.data_ptr(), *pk.dims(), G.stream())
    torch.cuda.synchronize()
    assert bool((buf[n:].float() == -7.0).all()), "the 64 elements behind the output were written"
    check(G.from_act(act), ref, prec, f"ang_block0 A{A} {B}x{h}x{w}", lambda: LP.ang_block(sd, 0, G.from_act(xin), prec), per_view=True)
