#!/usr/bin/env python3
"""Generate tests/golden/input_grad_*.npz: the REAL reference's gradient with respect to its INPUT (build container only).

For each case the reference (``/root/reference/model/LFT.py``, loaded as tools/gen_golden.py does) is filled with the
deterministic weights of ``lft_amd.params.deterministic_state`` and run on ``synthetic_lr``; a seeded ``dout`` is pulled back
through it with ``torch.autograd.grad(out, lr, dout)``.  Written: the seeds, d lr (whole for the small cases, a ``sub_indices``
sample and its statistics for every case) and the smallest |pre-activation| over the network's ReLU / LeakyReLU units, which
says how far the case sits from a kink.  Data only -- no reference source leaves the container.

Usage:  python tools/gen_golden_input_grad.py      (needs /root/reference; writes tests/golden/input_grad_*.npz)
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
from lft_amd.params import deterministic_state, synthetic_lr  # noqa: E402
from fixture_util import stats, sub_indices  # noqa: E402
from gen_golden import kink_tags, load_reference  # noqa: E402

# (name, A, s, B, h, w); d lr is stored whole up to FULL_MAX elements
CASES = [("input_grad_a3_s2_b2_6x6", 3, 2, 2, 6, 6), ("input_grad_a2_s4_b1_8x5", 2, 4, 1, 8, 5),
         ("input_grad_a5_s4_b1_8x8", 5, 4, 1, 8, 8), ("input_grad_a9_s2_b1_4x4", 9, 2, 1, 4, 4),
         ("input_grad_a5_s2_b1_16x16", 5, 2, 1, 16, 16)]
FULL_MAX = 2048


def dout_for(A, s, B, h, w, dseed=3) -> np.ndarray:
    """The seeded cotangent of the output (the tests regenerate it from the same seed)."""
    rng = np.random.Generator(np.random.PCG64([dseed, B, A, h, w, s]))
    return rng.standard_normal((B, 1, A * h * s, A * w * s), dtype=np.float32)


def input_grad_case(ref, name, A, s, B, h, w, wseed=1, iseed=0, dseed=3, flavor="stress"):
    net = ref.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s)).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, s, seed=wseed, flavor=flavor).items()})
    for p in net.parameters():
        p.requires_grad_(False)
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=iseed)).requires_grad_()
    pre = {}
    hooks = [mod.register_forward_hook(lambda _m, _i, o, tag=tag: pre.__setitem__(tag, o.detach().clone()))
             for tag, mod in kink_tags(net)]
    out = net(lr)
    for x in hooks:
        x.remove()
    dout = torch.from_numpy(dout_for(A, s, B, h, w, dseed))
    (g,) = torch.autograd.grad(out, lr, dout)
    a = g.numpy().astype(np.float32).ravel()
    rec = {"meta": np.array([A, s, B, h, w, wseed, iseed, dseed], dtype=np.int64), "flavor": np.array(flavor),
           "d_lr_sub": a[sub_indices(a.size)].copy(), "d_lr_stats": stats(a),
           "min_abs_pre": np.array(min(float(z.abs().min()) for z in pre.values()))}
    if a.size <= FULL_MAX:
        rec["d_lr_full"] = g.numpy().astype(np.float32)
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **rec)
    print(f"{name}: d lr {tuple(g.shape)} max|.| {float(g.abs().max()):.4e}, min |pre-activation| {float(rec['min_abs_pre']):.2e} "
          f"-> {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    torch.manual_seed(0)
    ref = load_reference()
    for case in CASES:
        input_grad_case(ref, *case)


if __name__ == "__main__":
    main()
