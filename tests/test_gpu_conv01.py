"""GPU tests of the composed 16-bit front end (k_conv64_lr + k_conv64<T, 2>: conv_init0 folded into conv_init.0 and recomputed
for the residual) against the exact oracle, the rounding model and the front end it replaced (include/lft_hip_test.h).

Shapes (A, s, B, h, w): tiny views with all four borders inside one tile, B > 1 and A > 1 (view addressing inside the
mosaic), tiles that start mid-row with a partial last tile (5 x 37), h w < 128, and a 64-wide view."""
import pytest
import torch

from lft_amd import _lib
from lft_amd.params import deterministic_state, synthetic_lr
from oracle import lft_oracle as O
from oracle import lft_oracle_lp as LP

import gpu_util as G
import parity_gates as PG

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 2, 3, 2), (3, 2, 2, 6, 5), (2, 2, 2, 5, 37), (2, 4, 1, 12, 16), (2, 2, 1, 4, 64)]
STAGE_RMS = {"bf16": 1e-2, "fp16": 2e-3}          # tests/test_gpu_parity.py


@pytest.fixture(scope="module", params=SHAPES, ids=lambda c: "A%d_s%d_B%d_%dx%d" % c)
def case(request):
    A, s, B, h, w = request.param
    sd_np = deterministic_state(64, s, seed=1, flavor="stress")
    sd = O.state_from_numpy(sd_np)
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0))
    views = O.mosaic_to_views(lr, A)
    with torch.no_grad():
        feat = O.init_features(sd, views)
        model = {p: LP.init_features(sd, views, p) for p in STAGE_RMS}
    packs = {p: G.Packed(sd_np, A, h, w, s, p, B) for p in STAGE_RMS}
    return dict(A=A, sd=sd, lr=lr, feat=feat, model=model, packs=packs)


def run(case, prec, entry="lft_init_features_fwd"):
    pk = case["packs"][prec]
    lr = case["lr"].to(G.DEV)
    act = pk.new_act()
    _lib.check(getattr(_lib.lib(), entry)(pk.buf.data_ptr(), lr.data_ptr(), act.data_ptr(), pk.work.data_ptr(), *pk.dims(), G.stream()), entry)
    torch.cuda.synchronize()
    return act


def check(got, ref, model, prec, what):
    """The 16-bit branch of test_gpu_parity.check: global rms bound, then the localized gates at M = 2."""
    msg = f"{what} [{prec}]: " + G.err_report(got, ref)
    assert not torch.isnan(got).any(), msg
    assert G.rel_rms(got, ref) <= STAGE_RMS[prec], msg
    ratios, text = PG.gate_report(got, ref, model)
    msg += f"\n{what} [{prec}] gates: {text}"
    print(msg)
    assert not PG.failed(ratios), msg


@pytest.mark.parametrize("prec", list(STAGE_RMS))
def test_composed_front_end_against_oracle_and_model(case, prec):
    check(G.from_act(run(case, prec)), case["feat"], case["model"][prec], prec, "init_features")


@pytest.mark.parametrize("prec", list(STAGE_RMS))
def test_recomputed_x0_is_bit_identical_to_k_conv0(case, prec):
    pk = case["packs"][prec]
    lr = case["lr"].to(G.DEV)
    x0 = [pk.new_act().fill_(7.0) for _ in range(2)]
    for recomputed in (0, 1):
        _lib.call("lft_conv0_fwd", pk.buf.data_ptr(), lr.data_ptr(), x0[recomputed].data_ptr(), recomputed, *pk.dims(), G.stream())
    torch.cuda.synchronize()
    ref = G.from_act(x0[0])
    exact = O.conv_views(O.mosaic_to_views(case["lr"], case["A"]), case["sd"]["conv_init0.0.weight"])
    assert G.rel_max(ref, exact) <= (1e-2 if prec == "bf16" else 2e-3)        # the stand-alone kernel is conv_init0 (one rounding: 2^-9 / 2^-12)
    assert torch.equal(x0[0].view(torch.int16), x0[1].view(torch.int16)), G.err_report(G.from_act(x0[1]), ref)


@pytest.mark.parametrize("prec", list(STAGE_RMS))
def test_composed_front_end_against_the_one_it_replaced(case, prec):
    new = G.from_act(run(case, prec))
    old = G.from_act(run(case, prec, "lft_init_features_legacy_fwd"))
    check(old, case["feat"], case["model"][prec], prec, "init_features (legacy)")
    check(new, case["feat"], case["model"][prec], prec, "init_features (composed)")
    print(f"composed - legacy [{prec}]: max|d| = {float((new - old).abs().max()):.3e} of max|feat| = {float(case['feat'].abs().max()):.3e}")
    # the composed path's error against the legacy kernels' error (in the model's place), slice by slice
    check(new, case["feat"], old, prec, "init_features (composed, gated by legacy)")


@pytest.mark.parametrize("prec", list(STAGE_RMS))
def test_composed_front_end_is_bitwise_repeatable(case, prec):
    a, b = run(case, prec), run(case, prec)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
