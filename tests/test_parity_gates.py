"""CPU proof that the localized gates of the stage parity tests (tests/parity_gates.py) see what the rms assertion does not.

Nothing on the GPU is broken on purpose: the "kernel output" here is a second correct implementation of the rounding policy --
the model of oracle/lft_oracle_lp.py accumulated in fp64 instead of fp32, same rounding sites -- and corruptions of it of the
kinds this code base has had.  A5, 2x, 8x8 views (1 600 tokens per batch element), "stress" weights, one
`spa` and one `ang` block, input already rounded to the activation type, ref = the exact oracle of that block.

Found (ratio of the sharpest gate, spa / ang block; rms = the old assertion's rel_rms, whose gates are 1e-2 / 2e-3):
                                     bf16                                  fp16
  healthy candidate                  every gate <= 1.01                    every gate <= 1.04
  one token x1.05                    tok 8.6 / 11.7; rms 4.5e-3 / 2.9e-3   tok 63 / 90; rms 1.4e-3 / 1.1e-3   -- the rms assertion PASSES both
  8 channels of one view x1.03       max 2.8 / 5.0;  rms 4.6e-3 / 3.2e-3   max 23 / 36; rms 1.7e-3 / 1.7e-3   -- passes (fp16: by a hair, not asserted)
  last image column x1.02            pos 5.1 / 8.2;  rms 8.6e-3 / 7.7e-3   pos 41 / 62; rms 7.4e-3 / 7.2e-3   -- passes in bf16, fails in fp16
  last image row x1.02               pos 5.0 / 8.1;  rms 7.7e-3 / 7.7e-3   pos 38 / 63; rms 6.4e-3 / 7.1e-3   -- passes in bf16, fails in fp16
  one 32-token tile shifted by one token, one batch element swapped with the other in one view: errors of the size of the signal
  on 2 % / 4 % of the tokens, which the rms assertion sees as well (rel_rms 0.11 .. 0.15); every gate reads 24 and more.
"""
import pytest
import torch

from lft_amd.params import deterministic_state, synthetic_lr
from oracle import lft_oracle as O
from oracle import lft_oracle_lp as LP

import parity_gates as PG

A, S, H, W = 5, 2, 8, 8
DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}
OLD_RMS_GATE = {"bf16": 1e-2, "fp16": 2e-3}          # tests/test_gpu_parity.py: BF16_STAGE_RMS, FP16_STAGE_RMS
HEALTHY = 1.5


def rel_rms(got, ref):
    return float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


@pytest.fixture(scope="module")
def setup():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = O.state_from_numpy(deterministic_state(64, S, seed=1, flavor="stress"))
    taps = {}
    O.forward(sd, torch.from_numpy(synthetic_lr(2, A, H, W, seed=0)), A, S, taps)
    return sd, {k: v.double() for k, v in sd.items()}, taps


def block_outputs(setup, stage, prec, B):
    """(ref, model, healthy candidate) of one block for the first B batch elements."""
    sd, sd64, taps = setup
    fn, ofn, key = (LP.spa_block, O.spa_block, "ang0") if stage == "spa" else (LP.ang_block, O.ang_block, "feat")
    x = taps[key][:B].to(DTYPE[prec]).float()
    with torch.no_grad():
        return ofn(sd, 0, x), fn(sd, 0, x, prec), fn(sd64, 0, x.double(), prec).float()


def one_token(c):
    c[0, :, 7, 3, 5] *= 1.05


def eight_channels_of_a_view(c):
    c[0, 8:16, 12] *= 1.03


def last_column(c):
    c[0, :, :, :, W - 1] *= 1.02


def last_row(c):
    c[0, :, :, H - 1, :] *= 1.02


def tile_shifted_by_one_token(c):
    """Tokens 32 .. 63 of view 9 (image rows 4 .. 7) each receive their successor's value, the last one the first's."""
    t = c[0, :, 9].reshape(64, H * W)
    t[:, 32:64] = torch.roll(t[:, 32:64].clone(), -1, dims=1)
    c[0, :, 9] = t.reshape(64, H, W)


def batch_elements_swapped_in_a_view(c):
    a = c[0, :, 17].clone()
    c[0, :, 17] = c[1, :, 17]
    c[1, :, 17] = a


# (corruption, batch size, precisions in which the OLD rms assertion must still pass -- the gap on record)
CORRUPTIONS = [(one_token, 1, ("bf16", "fp16")), (eight_channels_of_a_view, 1, ("bf16",)), (last_column, 1, ("bf16",)),
               (last_row, 1, ("bf16",)), (tile_shifted_by_one_token, 1, ()), (batch_elements_swapped_in_a_view, 2, ())]


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("stage", ["spa", "ang"])
def test_gates_pass_a_second_implementation_and_catch_local_corruptions(setup, stage, prec):
    for B in (1, 2):
        ref, model, healthy = block_outputs(setup, stage, prec, B)
        ratios, text = PG.gate_report(healthy, ref, model)
        print(f"{stage} {prec} B={B} healthy: {text} | old rms {rel_rms(healthy, ref):.2e}")
        assert max(ratios.values()) <= HEALTHY, text
        assert rel_rms(healthy, ref) <= OLD_RMS_GATE[prec]
        for corrupt, cb, rms_passes in CORRUPTIONS:
            if cb != B:
                continue
            cand = healthy.clone()
            corrupt(cand)
            ratios, text = PG.gate_report(cand, ref, model)
            old = rel_rms(cand, ref)
            print(f"{stage} {prec} {corrupt.__name__}: {text} | old rms {old:.2e}")
            assert PG.failed(ratios), f"{corrupt.__name__} passes every gate: {text}"
            if prec in rms_passes:
                assert old <= OLD_RMS_GATE[prec], f"{corrupt.__name__}: the rms assertion was expected to miss this ({old:.2e})"


def test_gates_catch_a_wrong_last_view_at_121_views():
    """A 11, 2x, 4x3 views (121 views, 12 positions -- the smallest of the view-count cases of tests/test_gpu_parity.py): view
    V - 1, the last row of the last key tile of the angular attention, x1.02.  Global rel_max of that corruption: 1.5e-2.  Found:
    the healthy candidate <= 1.11 in every gate; the `view` gate reads 4.7 / 7.1 in bf16 and 36 / 57 in fp16 (spa / ang block)."""
    A_, B, h, w = 11, 1, 4, 3
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = O.state_from_numpy(deterministic_state(64, S, seed=1, flavor="stress"))
    taps = {}
    O.forward(sd, torch.from_numpy(synthetic_lr(B, A_, h, w, seed=0)), A_, S, taps)
    setup = (sd, {k: v.double() for k, v in sd.items()}, taps)
    for stage in ("spa", "ang"):
        for prec in ("bf16", "fp16"):
            ref, model, healthy = block_outputs(setup, stage, prec, B)
            ratios, text = PG.gate_report(healthy, ref, model)
            print(f"A11 {stage} {prec} healthy: {text}")
            assert max(ratios.values()) <= HEALTHY, text
            cand = healthy.clone()
            cand[:, :, A_ * A_ - 1] *= 1.02
            ratios, text = PG.gate_report(cand, ref, model)
            print(f"A11 {stage} {prec} last view x1.02: {text} | old rms {rel_rms(cand, ref):.2e}")
            assert "view" in PG.failed(ratios), f"a wrong last view passes the view gate: {text}"


def test_image_layout_slices():
    """The up-sampler's layout: a corruption of one sub-pixel phase, one view, one LR pixel's block lands in its own gate."""
    g = torch.Generator().manual_seed(0)
    A_, s, h, w = 2, 2, 3, 5
    ref = torch.randn(2, 1, A_ * h * s, A_ * w * s, generator=g)
    model = ref + 1e-3 * torch.randn(ref.shape, generator=g)
    base = model + 1e-4 * torch.randn(ref.shape, generator=g)       # a candidate that rounds where the model rounds
    r, _ = PG.gate_ratios(base, ref, model, "image", A_, s)
    assert max(r.values()) <= 1.2, r
    c = base.clone(); c[:, :, 1::2, 0::2] += 4e-3                     # phase (1, 0)
    r, wst = PG.gate_ratios(c, ref, model, "image", A_, s)
    assert r["chan"] > 2 and wst["chan"] == (1, 0), (r, wst)
    c = base.clone(); c[1, :, h * s:, :w * s] += 4e-3                  # view (1, 0) of batch element 1
    r, wst = PG.gate_ratios(c, ref, model, "image", A_, s)
    assert r["view"] > 2 and wst["view"] == (1, 0) and wst["patch"] == (1,), (r, wst)
    c = base.clone(); c[0, 0, 2 * s:3 * s, (w + 4) * s:(w + 5) * s] += 8e-3      # LR pixel (y 2, x 4) of view (0, 1)
    r, wst = PG.gate_ratios(c, ref, model, "image", A_, s)
    assert r["tok"] > 2 and wst["tok"] == (0, 0, 2, 1, 4), (r, wst)
    c = base.clone(); c[:, :, 1::h * s, :] += 6e-3                     # HR row 1 of every view
    r, wst = PG.gate_ratios(c, ref, model, "image", A_, s)
    assert r["pos"] > 2 and wst["pos"][:2] == (0, 1), (r, wst)
    c = base.clone(); c[0, 0, 3, 7] = float("nan")
    assert "max" in PG.failed(PG.gate_ratios(c, ref, model, "image", A_, s)[0])


def test_gates_on_a_ragged_view_and_on_a_chain_of_stages():
    """A 2, 2x, 13x11 views (143 tokens: the second 128-token tile of a view image holds 15), the smallest of the view-size cases of
    tests/test_gpu_parity.py.  Per stage (init_features, spa block, up-sampler, each on its own input) the healthy candidate stays
    below 1.5 in every gate, and the 15 tokens of one view's last tile x1.05 fail.  Over a CHAIN of stages (the whole forward; the
    residual branch in the "image" layout) the candidate and the model round some intermediate values differently, and a `pos` slice
    holds only B * A^2 = 4 samples: found at most 1.11 / 1.24 (bf16 / fp16) in the other five gates and 3.98 / 4.14 in `pos` -- the reason
    why the chain checks of the GPU tests assert CHAIN_GATES, the five gates without `pos`.  One LR row of one view moved by one
    pixel reads 10 and more in `tok` there."""
    A_, B, h, w = 2, 1, 13, 11
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = O.state_from_numpy(deterministic_state(64, S, seed=1, flavor="stress"))
    sd64 = {k: v.double() for k, v in sd.items()}
    lr = torch.from_numpy(synthetic_lr(B, A_, h, w, seed=0))
    taps = {}
    O.forward(sd, lr, A_, S, taps)
    views = O.mosaic_to_views(lr, A_)
    chain_gates = [g for g in PG.GATES if g != "pos"]
    for prec in ("bf16", "fp16"):
        with torch.no_grad():
            x = taps["ang0"].to(DTYPE[prec]).float()
            xm = O.views_to_mosaic(taps["body"].to(DTYPE[prec]).float(), A_)
            stages = {"init": (taps["feat"], LP.init_features(sd, views, prec), LP.init_features(sd64, views.double(), prec).float(), "act"),
                      "spa": (O.spa_block(sd, 0, x), LP.spa_block(sd, 0, x, prec), LP.spa_block(sd64, 0, x.double(), prec).float(), "act"),
                      "up": (O.upsample(sd, xm, S), LP.upsample(sd, xm, S, prec), LP.upsample(sd64, xm.double(), S, prec).float(), "image")}
            model = LP.forward(sd, lr, A_, S, prec) - taps["skip"]
            healthy = (LP.forward(sd64, lr.double(), A_, S, prec) - taps["skip"].double()).float()
        for name, (ref, mod, cand, layout) in stages.items():
            ratios, text = PG.gate_report(cand, ref, mod, layout, A_, S)
            print(f"13x11 {name} {prec} healthy: {text}")
            assert max(ratios.values()) <= HEALTHY, text
        ref, mod, cand, _ = stages["spa"]
        cand = cand.clone()
        t = cand[0, :, 1].reshape(64, h * w)
        t[:, 128:] *= 1.05                                            # the partial second tile of view 1
        cand[0, :, 1] = t.reshape(64, h, w)
        ratios, text = PG.gate_report(cand, ref, mod)
        print(f"13x11 spa {prec} last tile of a view x1.05: {text}")
        assert PG.failed(ratios), text
        ratios, text = PG.gate_report(healthy, taps["res"], model, "image", A_, S)
        print(f"13x11 forward {prec} healthy: {text}")
        assert max(ratios[g] for g in chain_gates) <= HEALTHY, text
        cand = healthy.clone()
        rows = slice(h * S + 4 * S, h * S + 5 * S)                    # LR row 4 of view (1, 0)
        cand[0, 0, rows, :w * S] = torch.roll(cand[0, 0, rows, :w * S].clone(), S, dims=-1)
        ratios, text = PG.gate_report(cand, taps["res"], model, "image", A_, S)
        print(f"13x11 forward {prec} one LR row of a view moved by one pixel: {text}")
        assert [g for g in PG.failed(ratios) if g in chain_gates], text
