"""CPU self-checks of the rounding model (oracle/lft_oracle_lp.py): with every hook off it is the exact oracle, stage by
stage, empty windows (h < w) included; with every hook on its end-to-end error sits where DESIGN.md section 2 says the 16-bit
paths sit."""
import pytest
import torch

from lft_amd.params import deterministic_state, synthetic_lr
from oracle import lft_oracle as O
from oracle import lft_oracle_lp as LP

EXACT_TOL = 2e-6            # of max|ref|: two fp32 evaluations of the same formula (exp2 with a folded scale against exp)


def rel_max(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("A,s,B,h,w", [(5, 2, 2, 8, 8), (2, 4, 1, 6, 12)], ids=["A5_s2_B2_8x8", "A2_s4_B1_6x12_empty_windows"])
def test_hooks_off_is_the_exact_oracle(A, s, B, h, w):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = O.state_from_numpy(deterministic_state(64, s, seed=1, flavor="stress"))
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0))
    taps = {}
    out = O.forward(sd, lr, A, s, taps)
    if h < w:                                                    # the shape must really contain queries without a key
        assert bool(torch.isinf(O.window_mask(h, w)).all(dim=-1).any())
    with torch.no_grad():
        got = {"init_features": (LP.init_features(sd, O.mosaic_to_views(lr, A)), taps["feat"]),
               "upsample": (LP.upsample(sd, O.views_to_mosaic(taps["body"], A), s), taps["res"]),
               "forward": (LP.forward(sd, lr, A, s), out)}
        for l in range(O.LAYERS):
            x = taps["feat"] if l == 0 else taps[f"spa{l - 1}"]
            got[f"ang_block{l}"] = (LP.ang_block(sd, l, x), taps[f"ang{l}"])
            got[f"spa_block{l}"] = (LP.spa_block(sd, l, taps[f"ang{l}"]), taps[f"spa{l}"])
        got["spa_block3+skip"] = (LP.spa_block(sd, 3, taps["ang3"], skip=taps["feat"]), taps["body"])
        got["forward(explicit exact policy)"] = (LP.forward(sd, lr, A, s, {k: "exact" for k in LP.SITES}), out)
    for name, (a, b) in got.items():
        assert not torch.isnan(a).any(), name
        r = rel_max(a, b)
        print(f"{name}: {r:.2e}")
        assert r <= EXACT_TOL, (name, r)


def test_policy_argument():
    assert LP.resolve(None) == {} and LP.resolve("exact") == {}
    assert LP.resolve("bf16") == {k: "bf16" for k in LP.SITES}
    assert LP.resolve({"ang.w": "x2", "up.w": "exact"}) == {"ang.w": "x2"}
    for bad in ("fp8", {"ang.weights": "bf16"}, {"ang.w": "bf8"}):
        with pytest.raises(ValueError):
            LP.resolve(bad)
    x = torch.tensor([1.0 + 2.0 ** -9, 3.0 + 2.0 ** -12])
    r = LP._Rounder({"ang.act": "bf16", "ang.w": "fp16", "ang.o": "x2"})
    assert torch.equal(r(x, "ang.act"), torch.tensor([1.0, 3.0]))
    assert torch.equal(r(x, "ang.w"), torch.tensor([1.0 + 2.0 ** -9, 3.0]))
    assert torch.equal(r(x, "ang.o"), x)                         # 16 mantissa bits hold both
    assert r(x, "spa.act") is x
    assert r(x.double(), "ang.act").dtype == torch.float64


# DESIGN.md section 2, first table, column "end-to-end error": what the 16-bit paths measure on the GPU against the
# reference fixtures; the study's own figures in the second table (bf16 1.71e-3 on this very input, fp16 1.8e-4 .. 2.4e-4) lie
# inside them.  Max-norm error over max|ref|.
BAND = {"bf16": (1.4e-3, 1.9e-3), "fp16": (1.6e-4, 2.4e-4)}


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_end_to_end_error_in_the_tabulated_band(prec):
    """A5, 4x, 32x32, the study's weights and input (tests/diag_precision_study.py defaults)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    A, s, h, w = 5, 4, 32, 32
    sd = O.state_from_numpy(deterministic_state(64, s, seed=1, flavor="default"))
    lr = torch.from_numpy(synthetic_lr(1, A, h, w, seed=0))
    ref = O.forward(sd, lr, A, s)
    out = LP.forward(sd, lr, A, s, prec)
    r = rel_max(out, ref)
    print(f"{prec}: model end to end {r:.3e}, band {BAND[prec]}")
    assert BAND[prec][0] <= r <= BAND[prec][1], (prec, r)
