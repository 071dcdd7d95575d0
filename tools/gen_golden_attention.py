#!/usr/bin/env python3
"""Generate tests/golden/attention_*.npz: the REAL reference's attention weights (build container only).

For each case the reference's model/LFT.py (loaded from its checkout as tools/gen_golden.py does) is filled with the
deterministic weights of ``lft_amd.params.deterministic_state`` and run on ``synthetic_lr`` on the CPU.  A forward hook
(``with_kwargs=True``, guarded against recursion) on each of its eight ``nn.MultiheadAttention`` modules calls the module again
on the very arguments it was given, with ``need_weights=True`` and ``average_attn_weights`` False and True -- the one-word
change of LFT.py:183-187 / :230-233 without touching the reference.  The reference returns ``[B*h*w, 8, V, V]`` for the angular
blocks and ``[B*V, 8, hw, hw]`` for the spatial ones.

Written (data only -- no reference source leaves the container), per layer L:
  angL_mean  [B,h,w,V,V]        angL_heads  [B,h,w,8,V,V]       (the per-head maps of the case's `head_layers` only)
  spaL_mean  [B,V,h,w,5,5]      spaL_heads  [B,V,8,h,w,5,5]     compact, through lft_amd.attention.compact_from_dense
  spaL_mean_dense [B,V,hw,hw]   the head-averaged spatial maps as the reference returned them (small views only)
For h < w the reference's rows of queries with an empty window are NaN; they are stored as they come.  Before a spatial map is
stored compact, the script checks that nothing is lost: the dense map is exactly 0 outside the centred 5x5 taps.

Usage:  python tools/gen_golden_attention.py      (needs the reference checkout of tools/gen_golden.py; writes tests/golden/attention_*.npz)
"""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lft_amd.attention import compact_from_dense, dense_spatial  # noqa: E402
from lft_amd.params import deterministic_state, synthetic_lr  # noqa: E402
from gen_golden import load_reference  # noqa: E402

# (name, A, s, B, h, w, layers whose per-head maps are stored): one square case, one h < w case (the column clamp of LFT.py:155
# leaves queries with an empty window).  The square case keeps the per-head maps of the first and the last layer only: with all
# four the file would pass 1 MiB.
CASES = [("attention_a3_s2_b1_6x6", 3, 2, 1, 6, 6, (0, 3)), ("attention_a2_s2_b1_6x12", 2, 2, 1, 6, 12, (0, 1, 2, 3))]


def attention_case(ref, name, A, s, B, h, w, head_layers, wseed=1, iseed=0, flavor="stress"):
    net = ref.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s)).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, s, seed=wseed, flavor=flavor).items()})
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=iseed))
    got, busy = {}, [False]

    def hook(tag):
        def fn(mod, args, kwargs, _out):
            if busy[0]:
                return
            busy[0] = True
            try:
                for avg, key in ((False, "heads"), (True, "mean")):
                    kw = dict(kwargs, need_weights=True, average_attn_weights=avg)
                    got[f"{tag}_{key}"] = mod(*args, **kw)[1].detach().clone()
            finally:
                busy[0] = False
        return fn

    hooks = []
    for l, blk in enumerate(net.altblock):
        hooks.append(blk.ang_trans.attention.register_forward_hook(hook(f"ang{l}"), with_kwargs=True))
        hooks.append(blk.spa_trans.attention.register_forward_hook(hook(f"spa{l}"), with_kwargs=True))
    with torch.no_grad():
        net(lr)
    for x in hooks:
        x.remove()
    V, hw = A * A, h * w
    rec = {"meta": np.array([A, s, B, h, w, wseed, iseed], dtype=np.int64), "flavor": np.array(flavor)}
    nan_rows = 0
    for l in range(4):
        am, ah = got[f"ang{l}_mean"], got[f"ang{l}_heads"]
        assert tuple(am.shape) == (B * hw, V, V) and tuple(ah.shape) == (B * hw, 8, V, V), (am.shape, ah.shape)
        rec[f"ang{l}_mean"] = am.reshape(B, h, w, V, V).numpy()
        if l in head_layers:
            rec[f"ang{l}_heads"] = ah.reshape(B, h, w, 8, V, V).numpy()
        sm, sh = got[f"spa{l}_mean"], got[f"spa{l}_heads"]
        assert tuple(sm.shape) == (B * V, hw, hw) and tuple(sh.shape) == (B * V, 8, hw, hw), (sm.shape, sh.shape)
        for dense in (sm, sh):            # nothing outside the compact window
            z = torch.nan_to_num(dense)
            assert torch.equal(dense_spatial(torch.nan_to_num(compact_from_dense(dense, h, w)), h, w), z)
        nan_rows += int(torch.isnan(sm).all(dim=-1).sum())
        rec[f"spa{l}_mean"] = compact_from_dense(sm, h, w).reshape(B, V, h, w, 5, 5).numpy()
        if l in head_layers:
            rec[f"spa{l}_heads"] = compact_from_dense(sh, h, w).reshape(B, V, 8, h, w, 5, 5).numpy()
        rec[f"spa{l}_mean_dense"] = sm.reshape(B, V, hw, hw).numpy()
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **rec)
    print(f"{name}: ang max {max(float(rec[f'ang{l}_mean'].max()) for l in range(4)):.3f}, "
          f"spa max {max(float(np.nanmax(rec[f'spa{l}_mean'])) for l in range(4)):.3f}, NaN rows {nan_rows} "
          f"-> {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    torch.manual_seed(0)
    ref = load_reference()
    for case in CASES:
        attention_case(ref, *case)


if __name__ == "__main__":
    main()
