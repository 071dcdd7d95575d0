"""The tail of the forward -- SpaTrans of layer 3 with the global skip, then the up-sampler -- with the LANE-MAJOR hand-off between
the two (run on the MI355X box with -m gpu).

Inside lft_forward the last spatial block hands its output to k_up as lane-major 32-token tiles whenever the view size has the
lane-major property (tests/spa_classes.py: tok_lane_major); lft_spa_block_fwd and lft_upsample_fwd always use row-major tokens, so
the stage tests never run k_spa_b / k_spa2 with a lane-major output, nor k_up with a lane-major input.  The test-only entry
lft_tail_fwd (include/lft_hip_test.h) runs the two stages with either hand-off:
  * the two hand-offs differ in the layout of one store and one load, so the output images must agree BIT FOR BIT;
  * the lane-major one is also held against the oracle (O.spa_block + skip, O.upsample) and the rounding model of the same chain;
  * a view size without the property is refused with LFT_ERR_SHAPE before anything is launched.
Shapes: 8x32 (the smallest 16-bit lane-major view: 2 tiles), 32x32 at 4x (GT = 2 in k_up), 62x64 (2-row last query tile, CH 8) in
the three precisions; 16x24 (tiles start mid-row) and 24x16 at 4x in fp32, where the 16-bit kernels are row-major."""
import pytest
import torch

from lft_amd import _lib
from oracle import lft_oracle as O
from oracle import lft_oracle_lp as LP

import gpu_util as G
import spa_classes as S
from test_gpu_parity import ALL_PRECS, CHAIN_GATES, LFT_ERR_SHAPE, check

pytestmark = pytest.mark.gpu

TAIL = [((2, 2, 1, 8, 32), p) for p in ALL_PRECS] + [((2, 4, 1, 32, 32), p) for p in ALL_PRECS] + \
       [((2, 2, 1, 62, 64), p) for p in ALL_PRECS] + [((2, 2, 1, 16, 24), "fp32"), ((2, 4, 1, 24, 16), "fp32")]


def tail(pk, xin, skip, lr, out, handoff):
    return _lib.lib().lft_tail_fwd(pk.buf.data_ptr(), xin.data_ptr(), skip.data_ptr(), lr.data_ptr(), out.data_ptr(), pk.work.data_ptr(),
                                   *pk.dims(), handoff, G.stream())


@pytest.mark.parametrize("shape,prec", TAIL, ids=lambda v: v if isinstance(v, str) else "A%d_s%d_B%d_%dx%d" % v)
def test_lane_major_tail(shape, prec):
    A, s, B, h, w = shape
    assert S.tok_lane_major(h, w, prec)
    sd_np, sd, lr, taps, _ = G.oracle_case(*shape, keep=True)
    pk = G.Packed(sd_np, A, h, w, s, prec, B)
    xin, skip, x = G.to_act(taps["ang3"], prec), G.to_act(taps["feat"], prec), lr.to(G.DEV)
    outs = []
    for handoff in (0, 1):
        G.status_reset(pk)
        buf, out = G.guarded((B, 1, A * h * s, A * w * s), torch.float32)
        _lib.check(tail(pk, xin, skip, x, out, handoff), "lft_tail_fwd")
        torch.cuda.synchronize()
        assert G.guard_intact(buf), f"handoff {handoff}: the elements behind the output were written"
        assert G.status_flags(pk) == (0, 0), f"handoff {handoff}: status word {G.status_flags(pk)}"
        outs.append(out.cpu())
    assert not torch.isnan(outs[0]).any()
    diff = outs[0] != outs[1]
    assert not bool(diff.any()), (f"lane-major and row-major tails differ in {int(diff.sum())} of {diff.numel()} pixels, first at "
                                  f"{tuple(int(i) for i in diff.nonzero()[0])}; " + G.err_report(outs[1], outs[0]))
    mask = O.window_mask(h, w)
    chain = lambda pol: LP.upsample(sd, O.views_to_mosaic(LP.spa_block(sd, 3, G.from_act(xin), pol, mask, G.from_act(skip)), A), s, pol)
    with torch.no_grad():
        ref = O.upsample(sd, O.views_to_mosaic(O.spa_block(sd, 3, G.from_act(xin), mask) + G.from_act(skip), A), s)
    check(outs[1] - taps["skip"], ref, prec, f"tail {h}x{w}", lambda: chain(prec), "image", A, s, per_view=True, gates=CHAIN_GATES)


@pytest.mark.parametrize("shape,prec", [((2, 2, 1, 6, 6), "fp32"), ((2, 2, 1, 16, 24), "bf16"), ((2, 2, 1, 16, 24), "fp16"), ((2, 2, 1, 31, 32), "bf16"),
                                        ((2, 2, 1, 31, 32), "fp32")], ids=lambda v: v if isinstance(v, str) else "A%d_s%d_B%d_%dx%d" % v)
def test_lane_major_tail_is_refused_without_the_property(shape, prec):
    """handoff = 1 on a view size whose tiles are not lane-major: LFT_ERR_SHAPE, nothing launched, the output as it was.  (The inputs
    are never read, so they are not the oracle's.)"""
    A, s, B, h, w = shape
    assert not S.tok_lane_major(h, w, prec)
    from lft_amd.params import deterministic_state
    pk = G.Packed(deterministic_state(64, s, seed=1, flavor="stress"), A, h, w, s, prec, B)
    xin = torch.zeros(pk.new_act().shape, dtype=G.ACT_DTYPE[prec], device=G.DEV)
    lr = torch.zeros(B, 1, A * h, A * w, device=G.DEV)
    buf, out = G.guarded((B, 1, A * h * s, A * w * s), torch.float32)
    rc = tail(pk, xin, xin, lr, out, 1)
    msg = _lib.lib().lft_last_error().decode()
    torch.cuda.synchronize()
    assert rc == LFT_ERR_SHAPE and f"{h}x{w}" in msg, (rc, msg)
    assert bool(torch.isnan(out).all()) and G.guard_intact(buf), "a refused call wrote to its output"
    _lib.check(tail(pk, xin, xin, lr, out, 0), "lft_tail_fwd")         # the row-major tail runs on every view size
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and G.guard_intact(buf)
