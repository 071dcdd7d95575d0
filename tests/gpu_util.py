"""Helpers for the -m gpu parity tests: call liblft_hip.so's per-stage C-ABI entry points on torch
device tensors and bring results back in the oracle's [B,C,V,h,w] layout."""
import numpy as np
import torch

from lft_amd import _lib, module
from lft_amd.params import deterministic_state, param_table, synthetic_lr

DEV = "cuda:0"
PRECS = {"fp32": _lib.PREC_F32, "bf16": _lib.PREC_BF16, "fp16": _lib.PREC_F16}
ACT_DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def stream():
    return torch.cuda.current_stream().cuda_stream


class Packed:
    """Packed weights + workspace for one (state dict, A, h, w, s, prec, B)."""

    def __init__(self, sd_np, A, h, w, s, prec, B, work=True):
        self.A, self.h, self.w, self.s, self.B = A, h, w, s, B
        self.prec_name, self.prec = prec, PRECS[prec]
        names = [n for n, _, _ in param_table(64, s)]
        self.params = [torch.from_numpy(sd_np[n]).to(DEV).contiguous() for n in names]
        self.buf = module.pack_weights(self.params, A, h, w, s, self.prec, stream())
        # work=False: for the entry points that take no workspace (lft_ang_block_fwd) at sizes where it would be hundreds of MiB
        self.work = torch.empty(_lib.workspace_bytes(B, A, h, w, s, self.prec), dtype=torch.uint8, device=DEV) if work else None
        torch.cuda.synchronize()

    def dims(self):
        return (self.B, self.A, self.h, self.w, self.s, self.prec)

    def new_act(self):
        return torch.empty((self.B, self.A * self.A, self.h, self.w, 64), dtype=ACT_DTYPE[self.prec_name], device=DEV)


_ORACLE = {}


def oracle_case(A, s, B, h, w, keep=False):
    """(state dict as numpy, as torch, LR input, taps, output) of the CPU oracle's forward on the seeded "stress" weights and input
    every parity case uses.  keep: remember it for the next module that asks for the same shape (the oracle costs up to 45 s)."""
    from oracle import lft_oracle as O
    key = (A, s, B, h, w)
    if key not in _ORACLE:
        sd_np = deterministic_state(64, s, seed=1, flavor="stress")
        sd = O.state_from_numpy(sd_np)
        lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0))
        taps = {}
        got = (sd_np, sd, lr, taps, O.forward(sd, lr, A, s, taps))
        if not keep:
            return got
        _ORACLE[key] = got
    return _ORACLE[key]


GUARD = 64          # elements behind a guarded output that a kernel must leave alone


def guarded(shape, dtype):
    """(buffer, view of `shape`): the view is filled with NaN -- a token a partial tile fails to store stays NaN, which the checks
    refuse -- and GUARD elements of -7 follow it."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), float("nan"), dtype=dtype, device=DEV)
    buf[n:] = -7.0
    return buf, buf[:n].view(*shape)


def guard_intact(buf):
    return bool((buf[-GUARD:].float() == -7.0).all())


def status_reset(pk):
    module.status_reset(pk.work, *pk.dims(), stream())


def status_flags(pk):
    """(return code, flag word) of lft_status_read: (0, 0) unless a kernel saw a non-finite value since the reset."""
    return module.status_read(pk.work, *pk.dims(), stream())


def to_act(x_bcvhw: torch.Tensor, prec: str) -> torch.Tensor:
    """oracle layout [B,C,V,h,w] (cpu fp32) -> device channels-last [B,V,h,w,C] in the activation dtype."""
    return x_bcvhw.permute(0, 2, 3, 4, 1).contiguous().to(DEV).to(ACT_DTYPE[prec])


def from_act(a: torch.Tensor) -> torch.Tensor:
    return a.float().cpu().permute(0, 4, 1, 2, 3).contiguous()


def err_report(got: torch.Tensor, ref: torch.Tensor) -> str:
    e = (got - ref).abs()
    idx = np.unravel_index(int(e.argmax()), tuple(e.shape))
    return (f"max|err|={float(e.max()):.3e} at {idx} (got {float(got[idx]):.6f} ref {float(ref[idx]):.6f}) "
            f"rms err={float(e.pow(2).mean().sqrt()):.3e} ref rms={float(ref.pow(2).mean().sqrt()):.3e} "
            f"nan={int(torch.isnan(got).sum())}")


def rel_rms(got, ref):
    return float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


def rel_max(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())
