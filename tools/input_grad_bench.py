"""Cost of the input gradient: the fp32 training step (lft_train_forward + lft_train_backward[_input]) at the training shape,
with and without d lr, alternating in one process (GPU box).  Prints one JSON line: median step milliseconds of both and the
difference.  Under rocprofv3 --kernel-trace --stats, run with --steps 5 --warmup 1 for k_lr_grad's kernel time.

  python tools/input_grad_bench.py [--B 8] [--steps 30] [--warmup 3] [--math fp32]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from lft_amd import train as T  # noqa: E402
from lft_amd.params import deterministic_state, param_table, synthetic_lr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--A", type=int, default=5)
    ap.add_argument("--s", type=int, default=2)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--hw", type=int, default=32)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--math", default="fp32")
    a = ap.parse_args()
    A, s, B, h, w = a.A, a.s, a.B, a.hw, a.hw
    dev = torch.device("cuda", 0)
    sd = deterministic_state(64, s, seed=1, flavor="stress")
    ps = [torch.from_numpy(sd[n]).to(dev).contiguous() for n, _, _ in param_table(64, s)]
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0)).to(dev)
    dout = torch.randn(B, 1, A * h * s, A * w * s, generator=torch.Generator().manual_seed(5)).to(dev) * 1e-3
    tape = torch.empty(T.tape_bytes(B, A, h, w, s), dtype=torch.uint8, device=dev)
    grads = torch.empty(T.grad_floats(s), dtype=torch.float32, device=dev)
    d_lr = torch.empty_like(lr)

    def step(with_lr):
        T.train_forward(ps, lr, A, s, tape=tape, math=a.math)
        T.train_backward(ps, lr, tape, dout, A, s, grads=grads, math=a.math, d_lr=d_lr if with_lr else None)

    times = {False: [], True: []}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(2 * (a.warmup + a.steps)):
        with_lr = bool(i % 2)
        ev0.record()
        step(with_lr)
        ev1.record()
        ev1.synchronize()
        if i >= 2 * a.warmup:
            times[with_lr].append(ev0.elapsed_time(ev1))
    base, inp = statistics.median(times[False]), statistics.median(times[True])
    print(json.dumps({"shape": [A, s, B, h, w], "math": a.math, "steps": a.steps, "step_ms": round(base, 4),
                      "step_ms_with_d_lr": round(inp, 4), "delta_ms": round(inp - base, 4), "delta_pct": round(100 * (inp - base) / base, 3),
                      "spread_ms": [round(min(times[False]), 4), round(max(times[False]), 4)]}))


if __name__ == "__main__":
    main()
