"""Run-to-run determinism of the HIP path (GPU).  Every kernel is free of atomics and of data-dependent
scheduling, so repeated launches on the same input must be bit-identical.  This guards against
synchronisation bugs: a B-fragment read of the LDS-staged conv input issued before the barrier that
publishes the tile showed up as ~0.5 % of launches differing in 8 tokens of one image row (second-round
workgroups only), invisible to a single parity run."""
import pytest
import torch

from lft_amd import _lib
from lft_amd.params import deterministic_state, synthetic_lr

import gpu_util as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_forward_is_bitwise_repeatable(prec):
    A, s, B, h, w = 5, 4, 4, 32, 32                      # BASELINE configs[1]: more workgroups than fit at once
    pk = G.Packed(deterministic_state(64, s, seed=1, flavor="stress"), A, h, w, s, prec, B)
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0)).to(G.DEV)
    out = torch.empty(B, 1, A * h * s, A * w * s, device=G.DEV)
    reps = {"bf16": 400, "fp16": 200, "fp32": 60}[prec]
    outs = []
    for _ in range(reps):
        _lib.call("lft_forward", pk.buf.data_ptr(), lr.data_ptr(), out.data_ptr(), pk.work.data_ptr(), *pk.dims(), G.stream())
        torch.cuda.synchronize()
        outs.append(out.clone())
    ref = outs[-1]
    bad = [i for i, o in enumerate(outs) if not torch.equal(o, ref)]
    detail = [(i, int((outs[i] != ref).sum()), float((outs[i] - ref).abs().max())) for i in bad[:5]]
    assert not bad, f"{len(bad)} of {reps} repeated forwards differ from the last one: (run, #elements, max|d|) {detail}"


def test_init_features_is_bitwise_repeatable():
    A, s, B, h, w = 5, 4, 4, 32, 32
    pk = G.Packed(deterministic_state(64, s, seed=1, flavor="stress"), A, h, w, s, "bf16", B)
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0)).to(G.DEV)
    base, bad = None, 0
    for _ in range(1500):
        act = pk.new_act()
        _lib.call("lft_init_features_fwd", pk.buf.data_ptr(), lr.data_ptr(), act.data_ptr(), pk.work.data_ptr(), *pk.dims(), G.stream())
        torch.cuda.synchronize()
        if base is None:
            base = act.clone()
        elif not torch.equal(act, base):
            bad += 1
    assert bad == 0, f"{bad} of 1499 repeated launches differ"
