"""ROUNDING MODEL of the 16-bit inference kernels -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The forward of oracle/lft_oracle.py restated with a rounding hook wherever the bf16 / fp16 instantiation of a HIP kernel
converts an fp32 value to its 16-bit operand type.  With every hook off it IS the exact oracle (tests/test_oracle_lp.py pins
that to 2e-6); with a policy it predicts, element by element, what a correct kernel of that precision may return for a given
input -- so `model - exact` is the error that precision alone explains, and the stage parity tests gate the kernels' error
against it per token, position, view, channel and batch element (tests/parity_gates.py) instead of only in a global rms.
tests/diag_precision_study.py switches groups of hooks on to price them.

Every function has the signature of its counterpart in lft_oracle.py plus `policy`:
  None / "exact"   every hook off
  "bf16" / "fp16"  every hook rounds to that type (what the kernels of that precision do)
  dict             site class -> "exact" | "bf16" | "fp16" | "x2" (split bf16, hi + lo: 16 mantissa bits); classes left out are exact
The model computes in the dtype of its inputs: handed float64 weights and activations it accumulates in fp64 and rounds at the
same sites -- a second, equally valid implementation of the policy (the "healthy candidate" of tests/test_parity_gates.py).

Rounding sites, per stage, with the kernel that owns each.  Not rounded in any mode, in kernels and model alike: LayerNorm
(statistics, scale, shift), scores, exponentials, softmax sums, residual adds, every accumulator, the LR input, conv_init0's
weight, LayerNorm parameters, the angular position table, the up-sampler's footprints G and the bicubic skip.

init_features
  store.x   conv_init0's output x0                                       k_conv0   (fp32 arithmetic on fp32 weights, 16-bit store)
  conv.w    the three conv_init weights                                  k_pack
  conv.act  their inputs (already 16-bit in memory: a no-op after store.x)
  store.x   lrelu(conv) of conv_init.0 / .2;  lrelu(conv_init.4) + x0    k_conv64  (x0 re-read as stored, added in fp32)
ang_block                                                                  k_ang / k_ang_multi (one kernel, nothing leaves registers)
  ang.w     Wq * (log2(e) / sqrt(8)) -- the scale is folded BEFORE the rounding -- Wk, Wv, Wo, W1, W2      k_pack
  ang.act   LN(x + PE) -> Q, K;  x -> V (a no-op: x is 16-bit);  LN(t) -> FFN;  relu(hidden) -> W2
  ang.qkv   the Q, K, V accumulators, re-used as MFMA operands
  ang.p     exp2(S - max), UNNORMALISED, as the operand of P.V; the denominator is the fp32 sum of the unrounded exponentials
  ang.o     (P.V) / sum, the operand of out_proj
  store.x   the block's output
spa_block
  spa.act   the input (no-op) and the position image (PE_h[y] + PE_w[x]) / 2, which the pack step stores in the activation type   k_pe_tables
  spa.w     MLP.weight, Wq * (log2(e) / 4) (folded before rounding), Wk, Wv, Wo, W1, W2, linear.0                k_pack
  store.tok the embedded tokens `tok` and the embedded position tokens (pack-time k_spa1<PE_ONLY> on the rounded image)    k_spa1
  spa.act   LN(tok32 + PEtok) -> K, where tok32 is the embedding's fp32 ACCUMULATOR, not the stored token     k_spa1
            Q: row-major hand-off -- from the same LN(tok32 + PEtok)                                       k_spa1
               lane-major hand-off (w % 32 == 0 and h w % 128 == 0) -- from LN(tok + PEtok), the STORED token     k_spa_b
            V: from the rounded token (the conversion to an operand is the store's rounding)
  spa.qkv   Q, K, V as stored / as operands
  spa.p     exp2(S - max), unnormalised; the denominator is the sum of the ROUNDED exponentials (all-ones MFMA),    k_spa_b
            0 for a query with an empty window (h < w, lft_oracle.mha)
  spa.o     (P.V) / sum, the operand of out_proj
  spa.act   LN(t) -> FFN; relu(hidden) -> W2; t2 -> linear.0.  The residuals tok + O Wo and t + FFN stay fp32 (tok as stored)
  store.x   the block's output, after the global skip (read as stored, added in fp32) where there is one
upsample
  up.act    the input (no-op); lrelu(Wu x), the operand of the overlap-add product                         k_up
  up.w      upsampling.0.weight; upsampling.3.weight (the overlap-add matrix holds its entries unchanged)       k_pack
  nothing   G = M lrelu(U) is written in fp32 and summed in fp32                                              k_up / k_assemble_t
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Union

import torch
import torch.nn.functional as F

from oracle import lft_oracle as O

SITES = ["store.x", "store.tok", "conv.act", "conv.w", "ang.act", "ang.w", "ang.qkv", "ang.p", "ang.o",
         "spa.act", "spa.w", "spa.qkv", "spa.p", "spa.o", "up.act", "up.w"]
MODES = ("exact", "bf16", "fp16", "x2")
LOG2E = 1.4426950408889634
Policy = Union[None, str, Dict[str, str]]


def resolve(policy: Policy) -> Dict[str, str]:
    """site class -> mode, for every class that is not exact."""
    if policy is None or policy == "exact":
        return {}
    if isinstance(policy, str):
        if policy not in ("bf16", "fp16"):
            raise ValueError(f"unknown policy {policy!r}")
        return {k: policy for k in SITES}
    for k, m in policy.items():
        if k not in SITES or m not in MODES:
            raise ValueError(f"unknown site class or mode: {k!r}: {m!r}")
    return {k: m for k, m in policy.items() if m != "exact"}


def lane_major(h: int, w: int) -> bool:
    """The 16-bit kernels' choice of the k_spa1 -> k_spa_b hand-off (lft_network.hip:tok_lane_major)."""
    return (h * w) % 128 == 0 and w % 32 == 0


class _Rounder:
    def __init__(self, policy: Policy):
        self.pol = resolve(policy)

    def __call__(self, x: torch.Tensor, cls: str) -> torch.Tensor:
        m = self.pol.get(cls, "exact")
        if m == "exact":
            return x
        if m == "fp16":
            return x.to(torch.float16).to(x.dtype)
        hi = x.to(torch.bfloat16).to(x.dtype)
        if m == "bf16":
            return hi
        return hi + (x - hi).to(torch.bfloat16).to(x.dtype)      # split bf16: hi + lo carries 16 mantissa bits

    def lin(self, a, w, blk):
        """a [.., K] activations, w [N, K] weights; operand rounding by block class."""
        return self(a, blk + ".act") @ self(w, blk + ".w").t()


def _attention(rnd: _Rounder, nq, nk, v_in, w_in, w_out, mask, blk: str, rounded_sum: bool):
    """MultiheadAttention(E, 8) as the kernels run it: nq / nk the normalised inputs of the Q / K projections, v_in of V.
    exp2 softmax with the scale folded into Wq, probabilities rounded unnormalised, normalisation after P.V."""
    L, N, E = nq.shape
    d = E // O.HEADS
    wq, wk, wv = w_in[:E] * (LOG2E / math.sqrt(d)), w_in[E:2 * E], w_in[2 * E:]
    q = rnd(rnd.lin(nq, wq, blk), blk + ".qkv").reshape(L, N, O.HEADS, d).permute(1, 2, 0, 3)      # [N,H,L,d]
    k = rnd(rnd.lin(nk, wk, blk), blk + ".qkv").reshape(L, N, O.HEADS, d).permute(1, 2, 0, 3)
    v = rnd(rnd.lin(v_in, wv, blk), blk + ".qkv").reshape(L, N, O.HEADS, d).permute(1, 2, 0, 3)
    o = torch.empty_like(q)
    # A masked key has probability exactly 0, so only the keys a query can see are gathered (a 5 x 5 window: W <= 25 of L = h w):
    # the [L, L] score matrix of the dense form would make this model cost several times the exact oracle at 64 x 64 views.
    idx = bias = None
    if mask is not None:
        seen = mask == 0
        W = max(1, int(seen.sum(dim=-1).max()))
        idx = seen.to(torch.int8).argsort(dim=-1, descending=True, stable=True)[:, :W]            # [L, W] keys of each query
        bias = mask.gather(1, idx)                                                                # 0 / -inf (fewer than W keys)
    step = max(1, (1 << 25) // (O.HEADS * L * (L if mask is None else idx.shape[1] * d)))       # bound the work block
    for n0 in range(0, N, step):
        qn, kn, vn = q[n0:n0 + step], k[n0:n0 + step], v[n0:n0 + step]
        if mask is None:
            s = qn @ kn.transpose(-1, -2)                                                         # [n, H, L, L]
        else:
            kn, vn = kn[:, :, idx], vn[:, :, idx]                                                 # [n, H, L, W, d]
            s = (qn.unsqueeze(-2) @ kn.transpose(-1, -2)).squeeze(-2) + bias                      # [n, H, L, W]
        m = s.amax(dim=-1, keepdim=True).clamp_min(-1.0e30)      # empty window: exp2(-inf - m) = 0, not NaN
        p = torch.exp2(s - m)
        pr = rnd(p, blk + ".p")
        den = (pr if rounded_sum else p).sum(dim=-1, keepdim=True)
        on = (pr @ vn if mask is None else (pr.unsqueeze(-2) @ vn).squeeze(-2)) / den.clamp_min(1e-30)
        o[n0:n0 + step] = torch.where(den > 0, on, torch.zeros((), dtype=on.dtype))
    o = o.permute(2, 0, 1, 3).reshape(L, N, E)
    return rnd.lin(rnd(o, blk + ".o"), w_out, blk)


def _ffn(rnd: _Rounder, t, lw, lb, w1, w2, blk: str):
    n = F.layer_norm(t, (t.shape[-1],), lw, lb, 1e-5)
    return rnd.lin(F.relu(rnd.lin(n, w1, blk)), w2, blk)


def _conv3(rnd: _Rounder, x, wgt, blk: str):
    return F.conv3d(rnd(x, blk + ".act"), rnd(wgt, blk + ".w"), padding=(0, 1, 1))


def init_features(sd, lr_views: torch.Tensor, policy: Policy = None) -> torch.Tensor:
    rnd = _Rounder(policy)
    f0 = rnd(F.conv3d(lr_views, sd["conv_init0.0.weight"], padding=(0, 1, 1)), "store.x")
    f = f0
    for i in (0, 2, 4):
        f = F.leaky_relu(_conv3(rnd, f, sd[f"conv_init.{i}.weight"], "conv"), 0.2)
        if i != 4:
            f = rnd(f, "store.x")
    return rnd(f + f0, "store.x")


def ang_block(sd, l: int, x: torch.Tensor, policy: Policy = None) -> torch.Tensor:
    rnd = _Rounder(policy)
    p = f"altblock.{l}.ang_trans."
    B, C, V, h, w = x.shape
    t = x.permute(2, 0, 3, 4, 1).reshape(V, B * h * w, C)
    pe = O.angular_pe(V, C).view(V, 1, C).to(x.dtype)
    n = F.layer_norm(t + pe, (C,), sd[p + "norm.weight"], sd[p + "norm.bias"], 1e-5)
    t = _attention(rnd, n, n, t, sd[p + "attention.in_proj_weight"], sd[p + "attention.out_proj.weight"], None, "ang", False) + t
    t = _ffn(rnd, t, sd[p + "feed_forward.0.weight"], sd[p + "feed_forward.0.bias"], sd[p + "feed_forward.1.weight"],
             sd[p + "feed_forward.4.weight"], "ang") + t
    return rnd(t.reshape(V, B, h, w, C).permute(1, 4, 0, 2, 3), "store.x")


def spa_block(sd, l: int, x: torch.Tensor, policy: Policy = None, mask: Optional[torch.Tensor] = None,
              skip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`skip`: the global skip of the last layer (lft_oracle._forward's `y + x`), which k_spa_b adds before its store."""
    rnd = _Rounder(policy)
    p = f"altblock.{l}.spa_trans."
    B, C, V, h, w = x.shape
    if mask is None:
        mask = O.window_mask(h, w)
    wm = rnd(sd[p + "MLP.weight"], "spa.w")
    tok32 = O.spa_tokens(rnd(x, "spa.act"), wm)                               # k_spa1's accumulators
    tok = rnd(tok32, "store.tok")
    pe_img = rnd(O.spatial_pe(h, w, C).to(x.dtype), "spa.act").view(1, C, 1, h, w)
    pe = rnd(O.spa_tokens(pe_img, wm), "store.tok")
    ln = lambda z: F.layer_norm(z, (2 * C,), sd[p + "norm.weight"], sd[p + "norm.bias"], 1e-5)
    nk = ln(tok32 + pe)
    nq = ln(tok + pe) if lane_major(h, w) else nk
    t = _attention(rnd, nq, nk, tok, sd[p + "attention.in_proj_weight"], sd[p + "attention.out_proj.weight"],
                   mask.to(x.dtype), "spa", True) + tok
    t = _ffn(rnd, t, sd[p + "feed_forward.0.weight"], sd[p + "feed_forward.0.bias"], sd[p + "feed_forward.1.weight"],
             sd[p + "feed_forward.4.weight"], "spa") + t
    t = rnd.lin(t, sd[p + "linear.0.weight"].reshape(C, 2 * C), "spa")
    y = t.reshape(h, w, B, V, C).permute(2, 4, 3, 0, 1)
    if skip is not None:
        y = y + skip
    return rnd(y, "store.x")


def upsample(sd, x_mosaic: torch.Tensor, s: int, policy: Policy = None) -> torch.Tensor:
    rnd = _Rounder(policy)
    u = F.conv2d(rnd(x_mosaic, "up.act"), rnd(sd["upsampling.0.weight"], "up.w"))
    u = F.pixel_shuffle(F.leaky_relu(u, 0.2), s)
    return F.conv2d(rnd(u, "up.act"), rnd(sd["upsampling.3.weight"], "up.w"), padding=1)


def forward(sd, lr: torch.Tensor, A: int, s: int, policy: Policy = None, taps: Optional[dict] = None) -> torch.Tensor:
    """lft_oracle.forward under a rounding policy; `taps` receives skip, feat, ang0..3, spa0..2, body and res."""
    with torch.no_grad():
        skip = O.bicubic_skip(lr.float(), A, s).to(lr.dtype)
        x = init_features(sd, O.mosaic_to_views(lr, A), policy)
        h, w = x.shape[-2:]
        mask = O.window_mask(h, w)
        if taps is not None:
            taps["skip"], taps["feat"] = skip, x
        y = x
        for l in range(O.LAYERS):
            y = ang_block(sd, l, y, policy)
            if taps is not None:
                taps[f"ang{l}"] = y
            y = spa_block(sd, l, y, policy, mask, x if l == O.LAYERS - 1 else None)
            if taps is not None:
                taps[f"spa{l}" if l < O.LAYERS - 1 else "body"] = y
        r = upsample(sd, O.views_to_mosaic(y, A), s, policy)
        if taps is not None:
            taps["res"] = r
        return r + skip
