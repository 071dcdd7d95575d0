"""Training side of the plugin surface: what the reference gets from PyTorch autograd when ``train.py:89-107`` runs
``net(data) -> criterion -> loss.backward() -> optimizer.step()`` -- here the forward-with-tape and the backward of
the whole network are liblft_hip.so calls (fp32 kernels, lft_amd/csrc/lft_train*.cuh).

Two ways in:
  * ``get_model.forward`` under autograd returns a tensor whose ``grad_fn`` is :class:`LFTFunction`; ``loss.backward()``
    fills ``p.grad`` of the 78 parameters, so the reference's ``torch.optim.Adam`` loop works unchanged.
  * :class:`TrainStep` is the MI355X-first loop: parameters, gradients and Adam moments live in three flat fp32
    buffers (the module's parameters become views), the loss gradient, backward, ONE all-reduce over RCCL and the
    fused Adam update are five enqueues per step.  ``TrainStep(..., max_grad_norm=..., guard=True)`` swaps the update for
    the guarded one (lft_adam_step_guarded): gradient-norm clipping, a step with a non-finite gradient skipped, frozen
    (``requires_grad = False``) tensors left alone -- all decided on the device, no host round trip inside the step.
    ``TrainStep(..., ema_decay=...)`` keeps an exponential moving average of the weights in a fourth flat buffer (lft_ema_update,
    which obeys the guard); ``state_dict()`` / ``load_state_dict()`` carry moments, counters and the average across a restart.
    ``TrainStep(..., loss=LFLoss(...))`` minimises another objective (lft_amd.loss: MSE / Charbonnier, EPI-gradient term) with
    lft_lf_loss in the place of lft_l1_loss, inside the same captured step.
"""
from __future__ import annotations

import contextlib
import ctypes
import logging
from collections import OrderedDict
from typing import List, Optional

import torch

from . import _lib
from .params import param_table


def tape_bytes(B, A, h, w, s) -> int:
    return _lib.query("lft_train_tape_bytes", B, A, h, w, s)


def grad_floats(s) -> int:
    return _lib.query("lft_train_grad_floats", s)


def tape_view(tape: torch.Tensor, name: str, B, A, h, w, s, shape) -> torch.Tensor:
    """A saved activation of the last lft_train_forward as a tensor view (tests / debugging)."""
    off = _lib.query("lft_train_tape_offset", name.encode(), B, A, h, w, s)
    n = torch.Size(shape).numel()
    return tape.view(torch.float32)[off:off + n].view(*shape)


def _check_params(ps: List[torch.Tensor], dev) -> None:
    if len(ps) != _lib.NUM_PARAMS:
        raise _lib.LftError(f"expected {_lib.NUM_PARAMS} parameters, got {len(ps)}")
    for p in ps:
        if p.device != dev or p.dtype != torch.float32 or not p.is_contiguous():
            raise _lib.LftError(f"all parameters must be contiguous float32 tensors on {dev}; call net.to(device) first")


_ptr_array = _lib.ptr_array
MATH = {"fp32": _lib.MATH_F32, "bf16x3": _lib.MATH_BF16X3, "bf16x6": _lib.MATH_BF16X6}
# HIP-graph captures use the thread-local error mode: with a process group alive, torch's NCCL watchdog THREAD polls its work
# events (hipEventQuery) at any time; under the default global mode such a call from another thread while this thread captures
# invalidates the capture ("operation not permitted when stream is capturing" -- seen once in round 4 on the RCCL test, a race
# that had been there since the graphs were introduced).  Only calls of the capturing thread itself matter to these captures.
CAPTURE_MODE = "thread_local"


def train_forward(ps, lr, A, s, tape=None, math="fp32"):
    """lft_train_forward: returns (out, tape).  math: 'fp32' (exact fp32 MFMA), 'bf16x6' (fp32-class six-product split) or 'bf16x3' (split-bf16 products)."""
    B, _, H, W = lr.shape
    h, w = H // A, W // A
    dev = lr.device
    _check_params(ps, dev)
    if tape is None:
        tape = torch.empty(tape_bytes(B, A, h, w, s), dtype=torch.uint8, device=dev)
    out = torch.empty((B, 1, H * s, W * s), dtype=torch.float32, device=dev)
    _lib.enqueue("lft_train_forward", dev, _ptr_array(ps), len(ps), lr.data_ptr(), out.data_ptr(), tape.data_ptr(), B, A, h, w, s, MATH[math])
    return out, tape


def train_backward(ps, lr, tape, dout, A, s, grads=None, math="fp32", d_lr=None):
    """lft_train_backward: returns the flat gradient buffer (78 gradients back to back, state_dict order).
    d_lr (contiguous float32, lr's shape): also the gradient of the input, written there (lft_train_backward_input)."""
    B, _, H, W = lr.shape
    h, w = H // A, W // A
    dev = lr.device
    if grads is None:
        grads = torch.empty(grad_floats(s), dtype=torch.float32, device=dev)
    if d_lr is None:
        _lib.enqueue("lft_train_backward", dev, _ptr_array(ps), len(ps), lr.data_ptr(), tape.data_ptr(), dout.data_ptr(), grads.data_ptr(),
                     B, A, h, w, s, MATH[math])
    else:
        if d_lr.shape != lr.shape or d_lr.dtype != torch.float32 or not d_lr.is_contiguous() or d_lr.device != dev:
            raise _lib.LftError(f"d_lr must be a contiguous float32 tensor of shape {tuple(lr.shape)} on {dev}")
        _lib.enqueue("lft_train_backward_input", dev, _ptr_array(ps), len(ps), lr.data_ptr(), tape.data_ptr(), dout.data_ptr(),
                     grads.data_ptr(), d_lr.data_ptr(), B, A, h, w, s, MATH[math])
    return grads


def lr_grad_bwd(w0, dx0, dout, A, s, B, h, w):
    """lft_lr_grad_bwd: d lr = conv_init0^T(dx0) + bicubic^T(dout) as a new [B,1,A*h,A*w] tensor.  dx0 [B*A*A*h*w, 64] channels-last,
    w0 = conv_init0.0.weight; dout [B,1,A*h*s,A*w*s] or None (the conv term alone)."""
    dev = dx0.device
    d_lr = torch.empty((B, 1, A * h, A * w), dtype=torch.float32, device=dev)
    _lib.enqueue("lft_lr_grad_bwd", dev, w0.data_ptr(), dx0.data_ptr(), None if dout is None else dout.data_ptr(), d_lr.data_ptr(), B, A, h, w, s)
    return d_lr


def block_backward(ps, lr, tape, block, layer, d_out, A, s, grads, math="fp32"):
    """lft_train_block_backward: the backward pass of ONE block (include/lft_hip.h: LFT_BLOCK_*) against the tape of a full forward;
    returns the block's outgoing gradient [B, A*A, h, w, 64] (None for the feature extractor) and writes the block's parameter
    gradients into the flat buffer `grads`."""
    B, _, H, W = lr.shape
    h, w = H // A, W // A
    dev = lr.device
    d_in = None if block == _lib.BLOCK_INIT else torch.empty((B, A * A, h, w, 64), dtype=torch.float32, device=dev)
    _lib.enqueue("lft_train_block_backward", dev, _ptr_array(ps), len(ps), lr.data_ptr(), tape.data_ptr(), block, layer, d_out.data_ptr(),
                 None if d_in is None else d_in.data_ptr(), grads.data_ptr(), B, A, h, w, s, MATH[math])
    return d_in


def grad_bucket(s: int, bucket: int):
    """(first_float, n_floats) of gradient bucket `bucket` in the flat buffer (include/lft_hip.h: lft_train_grad_bucket)."""
    return _lib.query("lft_train_grad_bucket", s, bucket)


def train_backward_buckets(ps, lr, tape, dout, A, s, grads, on_bucket, math="fp32"):
    """lft_train_backward_buckets: the backward pass, calling on_bucket(bucket, first_float, n_floats) on the host each
    time a contiguous range of the flat gradient buffer is final (its last kernel enqueued on the current stream).
    An exception raised by on_bucket stops the pass at that boundary (the C call enqueues nothing further and returns
    LFT_ERR_CALLBACK) and is re-raised here."""
    B, _, H, W = lr.shape
    h, w = H // A, W // A
    err = []

    def trampoline(_user, bucket, first, count):
        try:
            on_bucket(int(bucket), int(first), int(count))
            return 0
        except BaseException as e:          # noqa: BLE001 -- must not propagate through the C frame
            err.append(e)
            return 1                        # tells lft_train_backward_buckets to stop: nothing further is enqueued

    cb = _lib.BUCKET_FN(trampoline)
    rc = _lib.lib().lft_train_backward_buckets(_ptr_array(ps), len(ps), lr.data_ptr(), tape.data_ptr(), dout.data_ptr(), grads.data_ptr(),
                                               B, A, h, w, s, MATH[math], _lib.stream_ptr(lr.device),
                                               ctypes.cast(cb, ctypes.c_void_p), None)
    if err:
        raise err[0]
    _lib.check(rc, "lft_train_backward_buckets")
    return grads


# ---------------------------------------------------------------------------------------------- guarded Adam step
def guard_bytes(nseg: int) -> int:
    return _lib.query("lft_guard_bytes", nseg)


def guard_init(guard: torch.Tensor, segments, n: int, steps_applied0: int = 0) -> None:
    """lft_guard_init on the current stream of the block's device; segments: (first, count, trainable) triples that tile [0, n) ascending."""
    segs = (_lib.GuardSegment * len(segments))(*[_lib.GuardSegment(int(f), int(c), int(bool(t))) for f, c, t in segments])
    _lib.enqueue("lft_guard_init", guard.device, guard.data_ptr(), segs, len(segments), n, steps_applied0)


def guard_new(segments, n: int, device, steps_applied0: int = 0) -> torch.Tensor:
    """A guard block (include/lft_hip.h: lft_guard_init) for a flat buffer of n floats.  Enqueued on the current stream of `device`."""
    guard = torch.empty(guard_bytes(len(segments)), dtype=torch.uint8, device=device)
    guard_init(guard, segments, n, steps_applied0)
    return guard


def adam_step_guarded(p, g, m, v, guard, lr, beta1=0.9, beta2=0.999, eps=1e-8, gscale=1.0, weight_decay=0.0, max_norm=None):
    """lft_adam_step_guarded on flat fp32 tensors; max_norm None (or <= 0, or inf): no clipping.  Only enqueues."""
    _lib.enqueue("lft_adam_step_guarded", p.device, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, beta1, beta2, eps,
                 gscale, weight_decay, 0.0 if max_norm is None else max_norm, guard.data_ptr())


def guard_read(guard: torch.Tensor) -> _lib.GuardReport:
    """lft_guard_read: the report of the last guarded step and the counters.  SYNCHRONISES the current stream."""
    rep = _lib.GuardReport()
    _lib.call("lft_guard_read", guard.data_ptr(), _lib.stream_ptr(guard.device), ctypes.byref(rep))
    return rep


# ---------------------------------------------------------------------------------------------- EMA of the weights
def ema_decay_at(decay: float, warmup: bool, t: int) -> float:
    """d_t of lft_ema_update as the kernel forms it: the decay crosses the C ABI as a float, the rest is double."""
    d = float(torch.tensor(decay, dtype=torch.float32))
    return min(d, (1.0 + t) / (10.0 + t)) if warmup else d


def ema_update(ema, p, decay, warmup=True, step=0, guard=None):
    """lft_ema_update on flat fp32 tensors: ema += (1 - d_t) * (p - ema).  With a guard block t is its steps_applied and a skipped
    step or a frozen segment leaves ema alone; without one t = step.  Only enqueues."""
    _lib.enqueue("lft_ema_update", p.device, ema.data_ptr(), p.data_ptr(), p.numel(), decay, int(bool(warmup)), int(step),
                 None if guard is None else guard.data_ptr())


# ---------------------------------------------------------------------------------------------- saved optimizer state
STATE_VERSION = 1
log = logging.getLogger(__name__)


class StateError(ValueError):
    """A saved training state that does not fit the TrainStep it is loaded into; the message names the field."""


def check_state(sd: dict, own: dict) -> List[str]:
    """Compare a saved state (TrainStep.state_dict()) with the description of the receiving step (the same keys, tensors left out:
    `ema` is True / False there).  Raises StateError, naming the field, for what cannot be continued; returns one line for every
    field the caller was free to change."""
    if not isinstance(sd, dict) or "version" not in sd:
        raise StateError("version: not a TrainStep state (no format version)")
    if int(sd["version"]) > STATE_VERSION:
        raise StateError(f"version: the state has format {sd['version']}, this build reads up to {STATE_VERSION}")
    missing = [k for k in ("m", "v", "ema", "t", "guard", "floats", "scale", "channels", "A", "trainable") if k not in sd]
    if missing:
        raise StateError(f"{missing[0]}: missing from the state")
    for k in ("floats", "scale", "channels"):
        if int(sd[k]) != int(own[k]):
            raise StateError(f"{k}: the state was saved with {sd[k]}, this step has {own[k]}")
    if [bool(x) for x in sd["trainable"]] != [bool(x) for x in own["trainable"]]:
        raise StateError("trainable: the state was saved with another set of frozen tensors")
    if (sd["ema"] is not None) != bool(own["ema"]):
        raise StateError("ema: " + ("the state holds averaged weights, this step keeps none" if sd["ema"] is not None
                                    else "this step keeps averaged weights, the state holds none"))
    if bool(sd["guard"]) != bool(own["guard"]):
        raise StateError("guard: " + ("a guarded state (Adam's step count is steps_applied) cannot continue an unguarded step"
                                      if sd["guard"] else "an unguarded state (Adam's step count is t) cannot continue a guarded step"))
    if sd["guard"]:
        for k in ("steps_applied", "steps_skipped", "steps_clipped"):
            if k not in sd:
                raise StateError(f"{k}: missing from a guarded state")
    for k in ("m", "v", "ema"):
        if sd[k] is not None and (tuple(sd[k].shape) != (int(own["floats"]),) or sd[k].dtype != torch.float32):
            raise StateError(f"{k}: expected {own['floats']} float32 values, got {tuple(sd[k].shape)} {sd[k].dtype}")
    return [f"{k}: saved with {sd.get(k)!r}, continuing with {own[k]!r}"
            for k in ("A", "math", "lr", "betas", "eps", "weight_decay", "max_grad_norm", "ema_decay", "ema_warmup")
            if k in sd and sd[k] != own[k]]


class LFTFunction(torch.autograd.Function):
    """autograd node of the whole network: forward saves the tape, backward returns the 78 parameter gradients (None for a
    parameter that does not need one) and, when the input needs one, the gradient of lr (lft_train_backward_input)."""

    @staticmethod
    def forward(ctx, lr, A, s, math, *params):
        ps = [p.detach() for p in params]
        out, tape = train_forward(ps, lr, A, s, math=math)
        ctx.A, ctx.s, ctx.tape, ctx.lr, ctx.math = A, s, tape, lr, math
        ctx.save_for_backward(*params)
        return out

    @staticmethod
    def backward(ctx, dout):
        ps = [p.detach() for p in ctx.saved_tensors]
        d_lr = torch.empty_like(ctx.lr) if ctx.needs_input_grad[0] else None
        flat = train_backward(ps, ctx.lr, ctx.tape, dout.contiguous().float(), ctx.A, ctx.s, math=ctx.math, d_lr=d_lr)
        ctx.tape = None
        grads, off = [], 0
        for i, p in enumerate(ps):
            grads.append(flat[off:off + p.numel()].view(p.shape) if ctx.needs_input_grad[4 + i] else None)
            off += p.numel()
        return (d_lr, None, None, None, *grads)


class TrainStep:
    """One data-parallel training step of the reference's loop (train.py:89-107) with flat buffers.

    net: lft_amd.module.get_model on a HIP device.  After construction the module's parameters are views into
    ``self.flat_params`` (state_dict / checkpoints keep working).  ``step(lr, hr)`` returns the loss tensor (device
    scalar, local shard).  With torch.distributed initialised, the flat gradient buffer is summed over the ranks in the three
    contiguous buckets in which the backward pass finishes it -- each bucket's all-reduce starts as soon as its last
    kernel is enqueued and runs beside the rest of the backward pass -- and averaged inside the Adam kernel (L1Loss is a
    mean over the local shard, shards are equal: SURVEY 8e).

    guard=True (implied by a finite max_grad_norm): the update is lft_adam_step_guarded.  The global gradient norm -- after the
    all-reduce and the 1/world scale, so every rank decides alike -- is clipped to max_grad_norm as torch.nn.utils.clip_grad_norm_
    would (the flat gradient buffer itself is NOT scaled: the clip is folded into the update); a step whose gradient holds a NaN or
    an inf leaves weights and moments untouched and does not advance Adam's step counter; parameters with
    ``requires_grad == False`` AT CONSTRUCTION are neither updated nor counted, as in the reference's
    ``[p for p in net.parameters() if p.requires_grad]``.  ``guard_report()`` reads what happened.
    """

    def __init__(self, net, lr: float = 2e-4, betas=(0.9, 0.999), eps: float = 1e-8, process_group=None, math: Optional[str] = None,
                 graph: bool = True, weight_decay: float = 0.0, max_grad_norm: Optional[float] = None, guard: bool = False,
                 ema_decay: Optional[float] = None, ema_warmup: bool = True, loss=None):
        self.net, self.lr, self.betas, self.eps = net, float(lr), betas, float(eps)
        if ema_decay is not None and not 0.0 <= ema_decay < 1.0:
            raise ValueError(f"ema_decay must lie in [0, 1), got {ema_decay}")
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        if max_grad_norm is not None and max_grad_norm != max_grad_norm:
            raise ValueError("max_grad_norm is NaN")
        clip = max_grad_norm is not None and 0.0 < max_grad_norm < float("inf")
        self.max_grad_norm = float(max_grad_norm) if clip else None
        self.guard = bool(guard) or clip
        self.weight_decay = float(weight_decay)                        # reference train.py:82 weight_decay=args.decay_rate (option.py default 0)
        self.math = math or getattr(net, "train_math", "fp32")
        # forward + loss + backward are ~450 kernel launches; for a fixed batch shape they are captured once into a HIP
        # graph and replayed (the kernels read the weights through the same flat buffer every step, and re-pack them
        # inside the graph).  The all-reduce and the Adam kernel (whose bias corrections change every step) stay eager.
        self.use_graph = bool(graph)
        self._graphs = {}
        self.group = process_group
        self.exchange = True               # False: skip the gradient exchange although a process group exists (bench.py times the step both ways)
        ps = net._params_in_order()
        dev = ps[0].device
        _check_params(ps, dev)
        self.s, self.A = net.factor, net.angRes
        n = grad_floats(self.s)
        assert n == sum(p.numel() for p in ps)
        self.flat_params = torch.empty(n, dtype=torch.float32, device=dev)
        self.flat_grads = torch.zeros(n, dtype=torch.float32, device=dev)
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        off = 0
        with torch.no_grad():
            for p in ps:
                k = p.numel()
                self.flat_params[off:off + k].copy_(p.reshape(-1))
                p.data = self.flat_params[off:off + k].view(p.shape)
                p.grad = self.flat_grads[off:off + k].view(p.shape)
                off += k
        self.params = ps
        self._guard = None
        self._segments, off = [], 0        # one segment per parameter tensor, state-dict order; trainable as of now
        for p in ps:
            self._segments.append((off, p.numel(), bool(p.requires_grad)))
            off += p.numel()
        self._counter0 = {"steps_skipped": 0, "steps_clipped": 0}      # what a loaded state adds to the block's own counters
        if self.guard:
            table = param_table(net.channels, self.s)
            assert [tuple(p.shape) for p in ps] == [tuple(sh) for _, sh, _ in table]
            self.segment_names = [name for name, _, _ in table]
            self._guard = guard_new(self._segments, n, dev)
        # Replicas must start from the same weights (the reference has no DP; torch's DDP broadcasts rank 0's
        # parameters at construction): a network built from scratch draws its weights from this process's own RNG.
        from .dp import broadcast_
        broadcast_(self.flat_params, src=0, group=self.group)
        self.ema = None if self.ema_decay is None else self.flat_params.clone()
        self.t = 0
        self._tape = None
        self.last_out = None               # [B,1,A*h*s,A*w*s]: what the network produced in the last step (before the update), for per-batch metrics
        self._scratch = torch.empty(1024 + 1, dtype=torch.float32, device=dev)
        # loss: None or 'l1' -- the reference's L1 through lft_l1_loss, the bits of every earlier version; an lft_amd.loss.LFLoss (or
        # its spec) other than pure L1 -- lft_lf_loss at the same place, (total, P, E) of the last step in last_loss_terms; with
        # ssim_weight > 0 lft_ssim_loss follows it, adds to the same dout and total, and leaves S in a fourth entry; with focal_weight > 0
        # lft_focal_loss follows both in the same way and leaves F in a fifth (the fourth is then 0 without the SSIM term)
        self.loss, self.last_loss_terms, self._loss_scratch, self._ssim_scratch, self._focal_scratch = None, None, {}, {}, {}
        if loss is not None and loss != "l1":
            from .loss import LFLoss
            loss = LFLoss.from_spec(loss)
            if loss.angRes is None:
                loss.angRes = int(self.A)
            if loss.angRes != self.A:
                raise ValueError(f"the loss was built for angRes {loss.angRes}, the network has {self.A}")
            if not loss.is_plain_l1():
                self.loss = loss
                self.last_loss_terms = torch.zeros(5 if loss.focal_weight > 0.0 else 4 if loss.ssim_weight > 0.0 else 3, dtype=torch.float32, device=dev)

    def _loss_scratch_for(self, hr):
        """Scratch of lft_lf_loss (and of lft_ssim_loss, and of lft_focal_loss with its device table) for this batch shape: allocated
        once, outside any capture."""
        key = tuple(hr.shape)
        B, _, R, C = hr.shape
        if self.loss.ssim_weight > 0.0 and (R // self.A < 11 or C // self.A < 11):      # before anything is allocated, enqueued or captured
            raise ValueError(f"the SSIM term needs HR views of at least 11x11 (its window), got views of {R // self.A}x{C // self.A}")
        if key not in self._loss_scratch:
            from .loss import scratch_bytes
            self._loss_scratch[key] = torch.empty(scratch_bytes(B, self.A, R // self.A, C // self.A), dtype=torch.uint8, device=hr.device)
        if self.loss.ssim_weight > 0.0 and key not in self._ssim_scratch:
            from .loss import ssim_scratch_bytes
            self._ssim_scratch[key] = torch.empty(ssim_scratch_bytes(B, self.A, R // self.A, C // self.A), dtype=torch.uint8, device=hr.device)
        if self.loss.focal_weight > 0.0 and key not in self._focal_scratch:
            from .loss import focal_scratch_bytes
            from .refocus import _device_table
            _device_table(self.A, self.loss.focal_slopes, "full", self.loss.focal_interp, hr.device)      # cached: the step finds it there
            self._focal_scratch[key] = torch.empty(focal_scratch_bytes(B, len(self.loss.focal_slopes), self.A, R // self.A, C // self.A),
                                                   dtype=torch.uint8, device=hr.device)
        return self._loss_scratch[key]

    def _fwd_loss_bwd(self, lr_in, hr, tape, dout, loss, on_bucket=None):
        out, _ = train_forward(self.params, lr_in, self.A, self.s, tape=tape, math=self.math)
        n = out.numel()
        if self.loss is None:
            _lib.enqueue("lft_l1_loss", lr_in.device, out.data_ptr(), hr.data_ptr(), n, dout.data_ptr(), 1.0 / n, loss.data_ptr(),
                         self._scratch.data_ptr())
        else:
            from .loss import focal_loss, lf_loss, ssim_loss
            lf = self.loss.has_lf_terms()
            if lf:
                lf_loss(out, hr, self.A, self.loss.penalty, self.loss.eps, self.loss.pixel_weight, self.loss.epi_weight, dsr=dout,
                        loss3=self.last_loss_terms, scratch=self._loss_scratch[tuple(hr.shape)])
            if self.loss.ssim_weight > 0.0:                    # P and E stay 0 in the pure structural objective
                ssim_loss(out, hr, self.A, self.loss.ssim_range, self.loss.ssim_weight, dsr=dout, accumulate=lf,
                          total=self.last_loss_terms[0:1], ssim_out=self.last_loss_terms[3:4], scratch=self._ssim_scratch[tuple(hr.shape)])
            if self.loss.focal_weight > 0.0:                   # S stays 0 without the SSIM term
                focal_loss(out, hr, self.A, self.loss.focal_slopes, self.loss.focal_interp, "full", self.loss.penalty, self.loss.eps,
                           self.loss.focal_weight, dsr=dout, accumulate=lf or self.loss.ssim_weight > 0.0, total=self.last_loss_terms[0:1],
                           focal_out=self.last_loss_terms[4:5], scratch=self._focal_scratch[tuple(hr.shape)])
        if on_bucket is None:
            train_backward(self.params, lr_in, tape, dout, self.A, self.s, grads=self.flat_grads, math=self.math)
        else:
            train_backward_buckets(self.params, lr_in, tape, dout, self.A, self.s, self.flat_grads, on_bucket, math=self.math)
        return out

    def _graph_for(self, lr_in, hr, bucketed=False):
        """Captured forward + loss + backward for this batch shape.  bucketed (data-parallel): one graph per gradient
        bucket -- the capture is ended and the next one begun at every bucket boundary the backward pass reports, so that
        step() can start a bucket's all-reduce between two replays."""
        key = (tuple(lr_in.shape), str(lr_in.device), bool(bucketed))
        g = self._graphs.get(key)
        if g is None:
            dev = lr_in.device
            B, _, H, W = lr_in.shape
            h, w = H // self.A, W // self.A
            g = {"lr": lr_in.clone(), "hr": hr.clone(), "dout": torch.empty_like(hr),
                 "tape": torch.empty(tape_bytes(B, self.A, h, w, self.s), dtype=torch.uint8, device=dev)}
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):                      # eager warm-up: sets kernel attributes, sizes nothing lazily later
                self._fwd_loss_bwd(g["lr"], g["hr"], g["tape"], g["dout"], self._scratch[1024:1025])
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            if not bucketed:
                g["graphs"] = [torch.cuda.CUDAGraph()]
                with torch.cuda.graph(g["graphs"][0], capture_error_mode=CAPTURE_MODE):
                    g["out"] = self._fwd_loss_bwd(g["lr"], g["hr"], g["tape"], g["dout"], self._scratch[1024:1025])
            else:
                graphs = [torch.cuda.CUDAGraph() for _ in range(_lib.GRAD_BUCKETS)]
                state = {"open": 0}

                def boundary(bucket, first, count):            # host callback between two kernels of the backward pass
                    assert bucket == state["open"], (bucket, state["open"])
                    graphs[bucket].capture_end()
                    state["open"] = bucket + 1
                    if bucket + 1 < len(graphs):
                        graphs[bucket + 1].capture_begin(pool=graphs[0].pool(), capture_error_mode=CAPTURE_MODE)

                with torch.cuda.stream(side):
                    graphs[0].capture_begin(capture_error_mode=CAPTURE_MODE)
                    try:
                        g["out"] = self._fwd_loss_bwd(g["lr"], g["hr"], g["tape"], g["dout"], self._scratch[1024:1025], on_bucket=boundary)
                    except BaseException as e:
                        # A failed capture must not leave a stream in capture mode: the backward pass has stopped at the failing
                        # boundary (nothing was enqueued after it), so end whatever capture is still open, drop every graph of this
                        # attempt and wait for the device before handing the error on (an error of the clean-up itself is chained).
                        try:
                            if state["open"] < len(graphs):
                                graphs[state["open"]].capture_end()
                        except BaseException as e2:            # noqa: BLE001
                            e.__context__ = e2
                        finally:
                            graphs.clear()
                            torch.cuda.synchronize(dev)
                        raise
                torch.cuda.current_stream(dev).wait_stream(side)
                g["graphs"] = graphs
            g["buckets"] = [grad_bucket(self.s, b) for b in range(_lib.GRAD_BUCKETS)]
            self._graphs[key] = g
        return g

    def step(self, lr_in: torch.Tensor, hr: torch.Tensor) -> torch.Tensor:
        from . import dp
        dev = lr_in.device
        B, _, H, W = lr_in.shape
        h, w = H // self.A, W // self.A
        exchange = self.exchange and dp.dp_active(self.group)
        handles = []

        def start_bucket(bucket, first, count):                # the all-reduce of a finished bucket, beside the rest of the backward
            handles.append(dp.sum_gradients_start_(self.flat_grads[first:first + count], self.group))

        with torch.cuda.device(dev):
            loss = self._scratch[1024:1025] if self.loss is None else self.last_loss_terms[:1]
            if self.loss is not None:
                self._loss_scratch_for(hr)
            if self.use_graph:
                g = self._graph_for(lr_in.contiguous().float(), hr.contiguous().float(), bucketed=exchange)
                g["lr"].copy_(lr_in)
                g["hr"].copy_(hr)
                for b, graph in enumerate(g["graphs"]):
                    graph.replay()
                    if exchange:
                        start_bucket(b, *g["buckets"][b])
                self.last_out = g["out"]                       # SR output of this step's forward (overwritten by the next step of this shape)
            else:
                nb = tape_bytes(B, self.A, h, w, self.s)
                if self._tape is None or self._tape.numel() != nb:
                    self._tape = torch.empty(nb, dtype=torch.uint8, device=dev)
                self.last_out = self._fwd_loss_bwd(lr_in.contiguous().float(), hr.contiguous().float(), self._tape, torch.empty_like(hr), loss,
                                                   on_bucket=start_bucket if exchange else None)
            dp.sum_gradients_finish(handles)                   # the Adam kernel is ordered after the collectives
            gscale = dp.grad_scale(self.group) if exchange else 1.0
            self.t += 1                    # calls of step(); with the guard Adam's own counter is steps_applied in the guard block
            if self._guard is None:
                _lib.enqueue("lft_adam_step", dev, self.flat_params.data_ptr(), self.flat_grads.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                             self.flat_params.numel(), self.lr, self.betas[0], self.betas[1], self.eps, self.t, gscale, self.weight_decay)
            else:
                adam_step_guarded(self.flat_params, self.flat_grads, self.m, self.v, self._guard, self.lr, self.betas[0], self.betas[1],
                                  self.eps, gscale, self.weight_decay, self.max_grad_norm)
            if self.ema is not None:
                ema_update(self.ema, self.flat_params, self.ema_decay, self.ema_warmup, self.t, self._guard)
        self.net._packed = None            # the inference path must re-pack the new weights
        return loss.clone()

    def guard_report(self) -> dict:
        """What the guarded update saw and did: ONE synchronising read of the guard block (never called from step()).
        grad_norm / clip_coef / skipped / nonfinite / bad_parameter describe the last step (bad_parameter: the first trainable
        parameter, in state-dict order, whose gradient held a NaN or an inf; None if none did); steps_applied / steps_skipped /
        steps_clipped count since construction; param_norms maps every parameter name, frozen ones included, to the norm of its
        gradient in the last step (non-finite elements left out)."""
        if self._guard is None:
            raise _lib.LftError("guard_report() needs TrainStep(..., guard=True) or a max_grad_norm")
        with torch.cuda.device(self._guard.device):
            r = guard_read(self._guard)
        return {"grad_norm": float(r.grad_norm), "clip_coef": float(r.clip_coef), "skipped": bool(r.skipped_last),
                "nonfinite": int(r.nonfinite_last), "bad_parameter": self.segment_names[r.bad_segment] if r.bad_segment >= 0 else None,
                "steps_applied": int(r.steps_applied), "steps_skipped": int(r.steps_skipped) + self._counter0["steps_skipped"],
                "steps_clipped": int(r.steps_clipped) + self._counter0["steps_clipped"],
                "param_norms": {name: float(r.seg_norm[i]) for i, name in enumerate(self.segment_names)}}

    # ------------------------------------------------------------------ averaged weights
    def _need_ema(self):
        if self.ema is None:
            raise _lib.LftError("no averaged weights: construct TrainStep(..., ema_decay=...)")

    def ema_state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """The averaged weights under the network's parameter names, CPU tensors: the 'state_dict' of a reference-format checkpoint."""
        self._need_ema()
        host = self.ema.cpu()
        return OrderedDict((name, host[first:first + count].view(p.shape).clone())
                           for name, p, (first, count, _) in zip(self.net._names, self.params, self._segments))

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the network runs with the averaged weights: the CONTENTS of flat_params and ema are exchanged in place
        (the parameters are views and captured graphs hold their addresses) and exchanged back on exit.  Do not step() inside."""
        self._need_ema()

        def exchange():
            with torch.no_grad():
                tmp = self.flat_params.clone()
                self.flat_params.copy_(self.ema)
                self.ema.copy_(tmp)
            self.net._packed = None

        exchange()
        try:
            yield self.net
        finally:
            exchange()

    # ------------------------------------------------------------------ saving and resuming
    def _describe(self) -> dict:
        """Everything of state_dict() but the tensors and the counters."""
        return {"version": STATE_VERSION, "lr": self.lr, "betas": tuple(float(b) for b in self.betas), "eps": self.eps,
                "weight_decay": self.weight_decay, "max_grad_norm": self.max_grad_norm, "guard": self.guard, "math": self.math,
                "ema_decay": self.ema_decay, "ema_warmup": self.ema_warmup, "A": int(self.A), "scale": int(self.s),
                "channels": int(self.net.channels), "floats": int(self.flat_params.numel()),
                "trainable": [bool(t) for _, _, t in self._segments]}

    def state_dict(self) -> dict:
        """What a restart needs beside the weights (those stay in the reference-format checkpoint): Adam's moments, the averaged
        weights, the step counters and the hyper-parameters, as CPU tensors and Python scalars.  With the guard: ONE synchronising
        read of the guard block."""
        sd = self._describe()
        sd.update(m=self.m.cpu(), v=self.v.cpu(), ema=None if self.ema is None else self.ema.cpu(), t=int(self.t))
        if self.guard:
            rep = self.guard_report()
            sd.update({k: rep[k] for k in ("steps_applied", "steps_skipped", "steps_clipped")})
        return sd

    def load_state_dict(self, sd: dict) -> None:
        """Continue from a state_dict(): m, v and ema are copied IN PLACE (captured graphs stay valid), t is set, the guard block is
        written again with the state's steps_applied and the other two counters go on from the state's.  StateError, naming the
        field, for a state of another network shape, another set of frozen tensors, a newer format, averaged weights on one side
        only, or a guarded state into an unguarded step (or the reverse); a different math, lr or max_grad_norm is logged."""
        own = self._describe()
        own["ema"] = self.ema is not None
        for line in check_state(sd, own):
            log.warning("training state: %s", line)
        with torch.no_grad():
            self.m.copy_(sd["m"])
            self.v.copy_(sd["v"])
            if self.ema is not None:
                self.ema.copy_(sd["ema"])
        self.t = int(sd["t"])
        if self.guard:
            guard_init(self._guard, self._segments, self.flat_params.numel(), int(sd["steps_applied"]))
            self._counter0 = {k: int(sd[k]) for k in ("steps_skipped", "steps_clipped")}


def names(channels: int = 64, scale: int = 2):
    return [n for n, _, _ in param_table(channels, scale)]
