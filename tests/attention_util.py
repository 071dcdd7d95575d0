"""Shared by the attention-map tests: the fixtures of tools/gen_golden_attention.py, and the maps recomputed on the CPU with
torch.nn.functional.multi_head_attention_forward(need_weights=True) on the oracle's taps (the reference's own operator, fed with
the block inputs of oracle.lft_oracle.forward)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from lft_amd.attention import compact_from_dense
from lft_amd.params import deterministic_state, synthetic_lr
from oracle import lft_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("attention_a3_s2_b1_6x6", "attention_a2_s2_b1_6x12")
FP32_STAGE_TOL = 1e-4          # the per-stage fp32 bound of tests/test_gpu_parity.py


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    A, s, B, h, w, wseed, iseed = (int(v) for v in z["meta"])
    sd = deterministic_state(64, s, seed=wseed, flavor=str(z["flavor"]))
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=iseed))
    return z, sd, lr, (A, s, B, h, w)


def _mha_weights(n, t, w_in, w_out, mask, per_head):
    E = n.shape[-1]
    return F.multi_head_attention_forward(n, n, t, E, O.HEADS, w_in, None, None, None, False, 0.0, w_out, None, training=False,
                                          need_weights=True, attn_mask=mask, average_attn_weights=not per_head)[1]


def functional_maps(sd_np, lr, A, s, per_head, blocks=None):
    """{"ang0": [B,h,w,(8,)V,V], "spa0": compact [B,V,(8,)h,w,5,5], ...} from torch's functional multi-head attention on the
    oracle's taps: block inputs are feat / spa{l-1} for the angular blocks and ang{l} for the spatial ones.  Rows of queries with
    an empty window are NaN, as torch returns them.  The spatial blocks go one view image at a time, so the dense [hw, hw] maps
    of a 64x64 view never exist for more than one image."""
    sd = O.state_from_numpy(sd_np)
    taps = {}
    with torch.no_grad():
        O.forward(sd, lr, A, s, taps)
        B, C, V, h, w = taps["feat"].shape
        H = (O.HEADS,) if per_head else ()
        out = {}
        mask = O.window_mask(h, w)
        for l in range(O.LAYERS):
            if blocks is None or f"ang{l}" in blocks:
                p = f"altblock.{l}.ang_trans."
                x = taps["feat"] if l == 0 else taps[f"spa{l - 1}"]
                t = x.permute(2, 0, 3, 4, 1).reshape(V, B * h * w, C)
                n = F.layer_norm(t + O.angular_pe(V, C).view(V, 1, C), (C,), sd[p + "norm.weight"], sd[p + "norm.bias"], 1e-5)
                m = _mha_weights(n, t, sd[p + "attention.in_proj_weight"], sd[p + "attention.out_proj.weight"], None, per_head)
                out[f"ang{l}"] = m.reshape(B, h, w, *H, V, V)
            if blocks is None or f"spa{l}" in blocks:
                p = f"altblock.{l}.spa_trans."
                x = taps[f"ang{l}"]
                t = O.spa_tokens(x, sd[p + "MLP.weight"])
                pe = O.spa_tokens(O.spatial_pe(h, w, C).view(1, C, 1, h, w), sd[p + "MLP.weight"])
                n = F.layer_norm(t + pe, (2 * C,), sd[p + "norm.weight"], sd[p + "norm.bias"], 1e-5)
                imgs = []
                for i in range(B * V):
                    m = _mha_weights(n[:, i:i + 1], t[:, i:i + 1], sd[p + "attention.in_proj_weight"], sd[p + "attention.out_proj.weight"],
                                     mask, per_head)
                    imgs.append(compact_from_dense(m[0], h, w))
                out[f"spa{l}"] = torch.stack(imgs).reshape(B, V, *H, h, w, 5, 5)
    return out


def empty_window_queries(h, w):
    """[h, w] bool: queries whose clamped window holds no key (x - 2 >= h, only for h < w)."""
    return torch.isinf(O.window_mask(h, w)).all(dim=-1).reshape(h, w)
