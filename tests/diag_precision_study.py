#!/usr/bin/env python3
"""Design study (CPU, not a test): which bf16 roundings of the throughput path cost how much end-to-end error.

TEST INFRASTRUCTURE: takes the restatement of the forward with a rounding hook at every GEMM operand and every
inter-kernel tensor (oracle/lft_oracle_lp.py, the model the stage parity tests gate the kernels against), checks it
against the oracle with all hooks off, then switches groups of hooks on.  The numbers decide the precision policy
of the HIP kernels.
usage: python tests/diag_precision_study.py [A s h w]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lft_amd.params import deterministic_state, synthetic_lr   # noqa: E402
from oracle import lft_oracle as O                              # noqa: E402
from oracle import lft_oracle_lp as LP                          # noqa: E402

ALL = LP.SITES


def main():
    A, s, h, w = (int(v) for v in sys.argv[1:5]) if len(sys.argv) >= 5 else (5, 4, 32, 32)
    flavor = sys.argv[5] if len(sys.argv) > 5 else "default"
    torch.set_num_threads(8)
    sd = O.state_from_numpy(deterministic_state(64, s, seed=1, flavor=flavor))
    lr = torch.from_numpy(synthetic_lr(1, A, h, w, seed=0))
    with torch.no_grad():
        ref = O.forward(sd, lr, A, s)
        base = LP.forward(sd, lr, A, s)
        print(f"self-check vs oracle (all exact): {float((base - ref).abs().max() / ref.abs().max()):.2e}")

        def run(name, pol):
            out = LP.forward(sd, lr, A, s, pol)
            e = (out - ref).abs()
            print(f"{name:58s} max {float(e.max() / ref.abs().max()):.2e}  rms {float(e.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()):.2e}", flush=True)

        allb = {k: "bf16" for k in ALL}
        run("everything bf16 (round-1 throughput path)", allb)
        for k in ALL:
            run(f"only {k} bf16", {k: "bf16"})
        for grp in ("store", "conv", "ang", "spa", "up"):
            run(f"all bf16 except {grp}.* exact", {k: v for k, v in allb.items() if not k.startswith(grp)})
        run("everything fp16 (operands and storage)", {k: "fp16" for k in ALL})
        run("all bf16, weights x2 (hi+lo)", {k: ("x2" if k.endswith(".w") else "bf16") for k in ALL})
        run("all bf16, activations x2, storage x2", {k: ("bf16" if k.endswith(".w") else "x2") for k in ALL})
        run("all bf16, store.x exact", {k: v for k, v in allb.items() if k != "store.x"})
        run("all bf16, store.x + store.tok exact", {k: v for k, v in allb.items() if not k.startswith("store")})
        run("all bf16, up.* x2", {k: ("x2" if k.startswith("up") else "bf16") for k in ALL})
        run("all bf16, up.* x2, store.x exact", {k: ("x2" if k.startswith("up") else "bf16") for k in ALL if k != "store.x"})
        run("all bf16, up.* + conv.* x2, store.x exact", {k: ("x2" if k[:2] in ("up", "co") else "bf16") for k in ALL if k != "store.x"})


if __name__ == "__main__":
    main()
