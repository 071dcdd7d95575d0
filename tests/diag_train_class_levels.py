"""Diagnostic (not a test): the figures behind the tight gate of tests/test_gpu_train_classes.py.  Run on the GPU box:
    python tests/diag_train_class_levels.py
For every size-class case, block and math mode: our kernels' worst per-tensor gradient error against the fp64 reference, and -- on
the fp32 tape's inputs and branches -- the reference's OWN fp32 noise (torch-fp32 autograd of the block against the fp64 one).
A case whose kernel error exceeds KINK_ALIGNED_LEVEL gets the level 4 x noise (x 6 for bf16x3) in LEVEL there."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import test_gpu_train_classes as M  # noqa: E402
import train_classes as C  # noqa: E402
import train_ref as R  # noqa: E402

if __name__ == "__main__":
    for shape, blocks in C.GPU_CASES:
        noise, kern = {}, {}
        for math in C.MATHS:
            case = M.get_case(shape, math)
            for kind in blocks:
                x, d_out, masks = M.block_inputs(case, kind)
                got = M.ours(case, kind, d_out)
                t0 = time.time()
                ref = M.reference(case, kind, x, d_out, masks)
                t1 = time.time()
                errs = R.rel_errors(got, ref)
                fwd = float((got["y"] - ref["y"]).abs().max() / ref["y"].abs().max())
                worst = max(errs, key=errs.get)
                kern[(math, kind)] = errs[worst]
                line = f"{M._ID(shape)} {math:7s} {kind:8s} forward {fwd:.2e}  worst gradient {errs[worst]:.2e} ({worst})  fp64 ref {t1 - t0:.1f} s"
                if math == "fp32":
                    n32 = R.rel_errors(R.block_reference(kind, case["sd"], M.BLOCK_OF[kind][1], x, case["lr"].cpu(), d_out, case["A"], case["s"], masks,
                                                         dtype=torch.float32), ref)
                    wn = max(n32, key=n32.get)
                    noise[kind] = n32[wn]
                    line += f"  | reference fp32 noise {n32[wn]:.2e} ({wn}), at our worst tensor {n32[worst]:.2e}"
                print(line, flush=True)
        print(f"== {M._ID(shape)}: fp32 noise {max(noise.values()):.2e}; kernels " +
              ", ".join(f"{m} {max(v for (mm, _), v in kern.items() if mm == m):.2e}" for m in C.MATHS), flush=True)
    M._live.clear()
