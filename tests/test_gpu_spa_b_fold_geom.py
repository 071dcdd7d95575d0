"""k_spa_b with the 1x1x1 conv folded into the FFN's second Linear and its per-lane geometry read from the pack-time table
(16-bit precisions, lane-major view sizes; run on the MI355X box with -m gpu).

The tail of part B computes  y = Wl t + (Wl W2) relu(W1 LN(t))  with Wl W2 composed in fp32 when the weights are packed, where it
used to compute  y = Wl (t + W2 relu(W1 LN(t))).  That is other rounding, not other arithmetic, so the yardstick is the CPU oracle
under the gates of the existing spatial-block tests (tests/test_gpu_parity.py: check).  The DMA offsets, LDS read bases and window
masks of a workgroup come from k_spa_b_geom's table, indexed by the query tile: a wrong entry misplaces a halo token or opens a
window, which the localized gates see.  The smallest lane-major view sizes:

  A1 B1  4x32   one query tile; h < w, so the `min(h, x+3)` quirk of the window (reference LFT.py:155) and its empty windows are live
  A2 B1  8x32   two vertically adjacent tiles, the halo crosses the seam; four images
  A1 B2 12x32   interior, top and bottom tile rows of the table
  A1 B1  8x64   two tile columns: the table's entries of tx = 1, the halo crosses the vertical seam

each for a middle layer (lft_spa_block_fwd) and for the last one (global skip and lane-major output into the up-sampler:
lft_tail_fwd), in bf16 and fp16.  One more case keeps the overflow detector honest: an fp16 input large enough for the token
embedding to leave the fp16 range must raise the status word, not pass silently."""
import pytest
import torch

from lft_amd import _lib
from oracle import lft_oracle as O
from oracle import lft_oracle_lp as LP

import gpu_util as G
import spa_classes as S
from test_gpu_parity import CHAIN_GATES, check

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 1, 4, 32), (2, 2, 1, 8, 32), (1, 2, 2, 12, 32), (1, 2, 1, 8, 64)]
PRECS = ["bf16", "fp16"]
ID = lambda v: v if isinstance(v, str) else "A%d_s%d_B%d_%dx%d" % v

_CASES = {}


def case(shape, prec):
    """The oracle run of a shape (once per shape) and the packed weights of a precision."""
    A, s, B, h, w = shape
    assert S.tok_lane_major(h, w, prec)
    if shape not in _CASES:
        sd_np, sd, lr, taps, _ = G.oracle_case(*shape)
        _CASES[shape] = dict(sd_np=sd_np, sd=sd, lr=lr, taps=taps, mask=O.window_mask(h, w), packs={})
    c = _CASES[shape]
    if prec not in c["packs"]:
        c["packs"][prec] = G.Packed(c["sd_np"], A, h, w, s, prec, B)
    return c, c["packs"][prec]


def spa_block(pk, layer, xin, skip, out):
    return _lib.lib().lft_spa_block_fwd(pk.buf.data_ptr(), layer, xin.data_ptr(), skip.data_ptr() if skip is not None else None,
                                        out.data_ptr(), pk.work.data_ptr(), *pk.dims(), G.stream())


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", SHAPES, ids=ID)
def test_middle_layer(shape, prec):
    c, pk = case(shape, prec)
    layer = 1
    xin = G.to_act(c["taps"][f"ang{layer}"], prec)
    G.status_reset(pk)
    buf, act = G.guarded(pk.new_act().shape, G.ACT_DTYPE[prec])
    _lib.check(spa_block(pk, layer, xin, None, act), "lft_spa_block_fwd")
    torch.cuda.synchronize()
    assert G.guard_intact(buf), "the elements behind the output were written"
    assert G.status_flags(pk) == (0, 0), f"status word {G.status_flags(pk)}"
    with torch.no_grad():
        ref = O.spa_block(c["sd"], layer, G.from_act(xin), c["mask"])
    check(G.from_act(act), ref, prec, f"spa_block{layer} {shape[3]}x{shape[4]}",
          lambda: LP.spa_block(c["sd"], layer, G.from_act(xin), prec, c["mask"]))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", SHAPES, ids=ID)
def test_last_layer_into_the_upsampler(shape, prec):
    """Layer 3 with the global skip, its output handed to k_up as lane-major tiles (what lft_forward does at these view sizes)."""
    A, s, B, h, w = shape
    c, pk = case(shape, prec)
    sd, taps = c["sd"], c["taps"]
    xin, skip, lr = G.to_act(taps["ang3"], prec), G.to_act(taps["feat"], prec), c["lr"].to(G.DEV)
    G.status_reset(pk)
    buf, out = G.guarded((B, 1, A * h * s, A * w * s), torch.float32)
    _lib.call("lft_tail_fwd", pk.buf.data_ptr(), xin.data_ptr(), skip.data_ptr(), lr.data_ptr(), out.data_ptr(), pk.work.data_ptr(), *pk.dims(), 1,
              G.stream())
    torch.cuda.synchronize()
    assert G.guard_intact(buf), "the elements behind the output were written"
    assert G.status_flags(pk) == (0, 0), f"status word {G.status_flags(pk)}"
    chain = lambda pol: LP.upsample(sd, O.views_to_mosaic(LP.spa_block(sd, 3, G.from_act(xin), pol, c["mask"], G.from_act(skip)), A), s, pol)
    with torch.no_grad():
        ref = O.upsample(sd, O.views_to_mosaic(O.spa_block(sd, 3, G.from_act(xin), c["mask"]) + G.from_act(skip), A), s)
    check(out.cpu() - taps["skip"], ref, prec, f"tail {h}x{w}", lambda: chain(prec), "image", A, s, gates=CHAIN_GATES)


def test_fp16_token_overflow_still_raises_the_status_word():
    """The input scaled until the token embedding leaves the fp16 range: the stored tokens hold inf, the LayerNorm that makes Q sees
    a non-finite variance and the status word says so.  (Nothing faults: an overflow is a flag, and the output is simply not used.)"""
    shape, prec, layer = SHAPES[0], "fp16", 1
    A, s, B, h, w = shape
    c, _ = case(shape, prec)
    # the "stress" embedding attenuates (max|tok| = 0.54 max|x| on this input), so an fp16 input alone cannot overflow it: the
    # embedding weight is scaled by 8 as well (0.33 at most, and the position tokens stay near 1)
    key = f"altblock.{layer}.spa_trans.MLP.weight"
    sd_np = dict(c["sd_np"])
    sd_np[key] = sd_np[key] * 8.0
    pk = G.Packed(sd_np, A, h, w, s, prec, B)
    x = c["taps"][f"ang{layer}"]
    x = x * (60000.0 / float(x.abs().max()))                                # still finite as fp16 (65504)
    xin = G.to_act(x, prec)
    assert bool(torch.isfinite(xin).all())
    with torch.no_grad():
        tok = O.spa_tokens(G.from_act(xin), torch.from_numpy(sd_np[key]))
    assert float(tok.abs().max()) > 2 * 65504.0, "the scaled input does not overflow the token embedding: the case checks nothing"
    G.status_reset(pk)
    buf, act = G.guarded(pk.new_act().shape, G.ACT_DTYPE[prec])
    _lib.check(spa_block(pk, layer, xin, None, act), "lft_spa_block_fwd")
    torch.cuda.synchronize()
    assert G.guard_intact(buf)
    rc, flags = G.status_flags(pk)
    assert rc == _lib.STATUS_NONFINITE and flags != 0, (rc, flags)
    # and the same weights on the unscaled input afterwards: clean again
    G.status_reset(pk)
    _lib.check(spa_block(pk, layer, G.to_act(c["taps"][f"ang{layer}"], prec), None, act), "lft_spa_block_fwd")
    torch.cuda.synchronize()
    assert G.status_flags(pk) == (0, 0)
