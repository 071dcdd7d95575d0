"""Data-parallel training driver around the hot path: the loop of the reference's train.py (:74-132) -- Adam, StepLR
(step 15 epochs, gamma 0.5), per-epoch checkpoints in the reference's ``{'epoch', 'state_dict'}`` format -- with one
process per GPU, every global batch sharded over the ranks and one gradient all-reduce per step (lft_amd.train.TrainStep).
The per-batch skimage PSNR/SSIM of train.py:121-124 is not part of the step; an epoch reports the
mean loss and the PSNR of the last batch computed on the GPU.

Data comes from a *patch source*: anything with ``__len__`` and ``get(indices) -> (lr [n,1,A*p,A*p], hr [n,1,A*p*s,A*p*s])``
float32 tensors.  ``TensorPatchSource`` wraps arrays already in memory; ``lft_amd.datasets.H5PatchSource`` reads the reference's
``Lr_SAI_y`` / ``Hr_SAI_y`` .h5 training tree (own HDF5 reader);
``SyntheticPatchSource`` makes band-limited random light fields for rehearsals and benchmarks.
"""
from __future__ import annotations

import contextlib
import os
from collections import OrderedDict
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import dp


# ---------------------------------------------------------------------------------------------- checkpoints
def checkpoint_name(model_name: str, angRes: int, scale: int, epoch: int) -> str:
    """File name used by the reference (train.py:99-100)."""
    return "%s_%dx%d_%dx_epoch_%02d_model.pth" % (model_name, angRes, angRes, scale, epoch)


def save_checkpoint(net, path: str, epoch: int) -> None:
    """``{'epoch': int, 'state_dict': OrderedDict}`` with CPU tensors (reference train.py:101-105)."""
    save_weights(net.module.state_dict() if hasattr(net, "module") else net.state_dict(), path, epoch)


def load_checkpoint(net, path: str) -> int:
    """Load a reference-format checkpoint, with or without the ``module.`` prefix DataParallel adds (reference
    train.py:42-58, test.py:35-51).  Parameters are updated IN PLACE (they may be views of a flat buffer).
    Returns the stored epoch."""
    ckpt = torch.load(path, map_location="cpu")
    sd = ckpt["state_dict"] if isinstance(ckpt, dict) and "state_dict" in ckpt else ckpt
    clean = OrderedDict((k[len("module."):] if k.startswith("module.") else k, v) for k, v in sd.items())
    own = net.state_dict()
    missing = [k for k in own if k not in clean]
    extra = [k for k in clean if k not in own]
    if missing or extra:
        raise KeyError(f"checkpoint does not match the model: missing {missing[:3]}..., unexpected {extra[:3]}...")
    with torch.no_grad():
        for k, p in net.named_parameters():
            p.copy_(clean[k].to(p.device, p.dtype).reshape(p.shape))
    if hasattr(net, "_packed"):
        net._packed = None
    return int(ckpt.get("epoch", 0)) if isinstance(ckpt, dict) else 0


def save_weights(state_dict, path: str, epoch: int) -> None:
    """A reference-format checkpoint from a ready state dict (the averaged weights of TrainStep.ema_state_dict())."""
    state = {"epoch": int(epoch), "state_dict": OrderedDict((k, v.detach().cpu().clone()) for k, v in state_dict.items())}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(state, path)


def ema_checkpoint_name(model_name: str, angRes: int, scale: int, epoch: int) -> str:
    return "%s_%dx%d_%dx_epoch_%02d_ema_model.pth" % (model_name, angRes, angRes, scale, epoch)


def best_checkpoint_name(model_name: str, angRes: int, scale: int) -> str:
    return "%s_%dx%d_%dx_best_model.pth" % (model_name, angRes, angRes, scale)


# ---------------------------------------------------------------------------------------------- the training state file
STATE_FILE_VERSION = 1
_FOLLOWS = "<broadcast>"                    # stands for a tensor of the state on the ranks that do not read the file


def training_state_name(model_name: str, angRes: int, scale: int) -> str:
    """The ONE state file of a run, overwritten every epoch (the per-epoch model files are the history)."""
    return "%s_%dx%d_%dx_training_state.pth" % (model_name, angRes, angRes, scale)


def save_training_state(path: str, ts, epoch: int, extra: Optional[dict] = None) -> None:
    """Everything a restart needs beside the model checkpoint of `epoch`: TrainStep.state_dict(), the epoch and `extra` (fit puts
    the loss history, last_metrics / last_guard, seed, global batch, world size and the best validation score there).  Written to a
    temporary name in the same directory and moved into place: a process killed mid-save leaves the previous file intact."""
    state = dict(extra or {})
    for k in ("file_version", "epoch", "train_step"):
        if k in state:
            raise ValueError(f"extra must not hold the reserved key {k!r}")
    state.update(file_version=STATE_FILE_VERSION, epoch=int(epoch), train_step=ts.state_dict())
    path = os.path.abspath(path)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tmp = "%s.tmp.%d" % (path, os.getpid())
    try:
        torch.save(state, tmp)
        os.replace(tmp, path)
    except BaseException:
        with contextlib.suppress(OSError):
            os.remove(tmp)
        raise


def check_state_file(state) -> None:
    """StateError, naming the field, for what is not a training state file of this or an older format."""
    from .train import StateError
    if not isinstance(state, dict):
        raise StateError("file_version: not a training state file")
    for k in ("file_version", "epoch", "train_step"):
        if k not in state:
            raise StateError(f"{k}: missing from the training state file")
    if int(state["file_version"]) > STATE_FILE_VERSION:
        raise StateError(f"file_version: the file has format {state['file_version']}, this build reads up to {STATE_FILE_VERSION}")
    if not isinstance(state["train_step"], dict):
        raise StateError("train_step: not a TrainStep state")
    if int(state["epoch"]) < 0:
        raise StateError(f"epoch: {state['epoch']}")


def load_training_state(path: str, ts, model_name: Optional[str] = None, group=None) -> dict:
    """Read a file of save_training_state into the TrainStep `ts` and return its other fields ('epoch' and the extras).
    model_name: also load the reference-format model checkpoint of the state's epoch from the same directory (into ts.net, in place).
    Data parallel: ONLY RANK 0 READS -- no shared file system is assumed; the small fields travel as one object broadcast, then the
    weights, m, v and ema through dp.broadcast_.  An error on rank 0 is raised on every rank."""
    import torch.distributed as dist
    from .train import StateError
    multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    rank = dist.get_rank(group) if multi else 0
    state, err = None, None
    if rank == 0:
        try:
            state = torch.load(path, map_location="cpu")
            check_state_file(state)
            if model_name is not None:
                load_checkpoint(ts.net, os.path.join(os.path.dirname(os.path.abspath(path)),
                                                     checkpoint_name(model_name, ts.A, ts.s, int(state["epoch"]))))
        except Exception as e:                  # noqa: BLE001 -- handed to every rank below
            err = e
    if multi:
        box = [None]
        if rank == 0:
            if err is not None:
                box = [{"error": "%s: %s" % (type(err).__name__, err)}]
            else:
                lean = dict(state)
                lean["train_step"] = {k: (_FOLLOWS if torch.is_tensor(v) else v) for k, v in state["train_step"].items()}
                box = [lean]
        dist.broadcast_object_list(box, src=0, group=group)
        if rank != 0:
            if "error" in box[0]:
                raise StateError("rank 0 could not read the training state: " + box[0]["error"])
            state = box[0]
            own = {"m": ts.m, "v": ts.v, "ema": ts.ema if ts.ema is not None else torch.empty(0)}   # placeholders of the right kind
            state["train_step"] = {k: (own[k] if isinstance(v, str) and v == _FOLLOWS else v) for k, v in state["train_step"].items()}
    if err is not None:
        raise err
    ts.load_state_dict(state["train_step"])     # the same refusals on every rank, before any collective
    if multi:
        for buf in (ts.flat_params, ts.m, ts.v, ts.ema):
            if buf is not None:
                dp.broadcast_(buf, src=0, group=group)
        ts.net._packed = None
    return {k: v for k, v in state.items() if k != "train_step"}


# ---------------------------------------------------------------------------------------------- schedule / sampling
def step_lr(base_lr: float, epoch: int, n_steps: int = 15, gamma: float = 0.5) -> float:
    """torch.optim.lr_scheduler.StepLR as the reference uses it (train.py:84, stepped once per epoch)."""
    return base_lr * gamma ** (epoch // n_steps)


def epoch_batches(n_items: int, global_batch: int, epoch: int, seed: int, rank: int, world: int) -> List[np.ndarray]:
    """This rank's index batches for one epoch: a permutation seeded by (seed, epoch) -- identical on every rank --
    cut into global batches (the reference's DataLoader(shuffle=True, batch_size=--batch_size), train.py:26-27), each
    split contiguously over the ranks.  global_batch must divide by world; the tail wraps around so that all ranks
    always hold equal shards (the gradient average over ranks is then the global-batch gradient)."""
    if global_batch % world:
        raise ValueError(f"global batch {global_batch} is not divisible by the world size {world}")
    perm = np.random.Generator(np.random.PCG64([seed, epoch])).permutation(n_items)
    nb = (n_items + global_batch - 1) // global_batch
    idx = np.resize(perm, nb * global_batch)                       # wrap-around padding of the last batch
    per = global_batch // world
    return [idx[b * global_batch + rank * per: b * global_batch + (rank + 1) * per] for b in range(nb)]


def augment(lr: torch.Tensor, hr: torch.Tensor, rng: np.random.Generator) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reference's three augmentations (utils_datasets.py:123-135), decided per sample: mirror the whole mosaic
    left-right, up-down, and transpose it (each flips / swaps the angular and the spatial axes together)."""
    lo, ho = [], []
    for i in range(lr.shape[0]):
        a, b = lr[i], hr[i]
        if rng.random() < 0.5:
            a, b = a.flip(-1), b.flip(-1)
        if rng.random() < 0.5:
            a, b = a.flip(-2), b.flip(-2)
        if rng.random() < 0.5:
            a, b = a.transpose(-1, -2), b.transpose(-1, -2)
        lo.append(a)
        ho.append(b)
    return torch.stack(lo).contiguous(), torch.stack(ho).contiguous()


def augment_gpu(lr: torch.Tensor, hr: torch.Tensor, rng: np.random.Generator) -> Tuple[torch.Tensor, torch.Tensor]:
    """`augment` as two kernel launches: the same three rng.random() draws per sample, in the same order, become one dihedral code
    per sample (bit 0 left-right, bit 1 up-down, bit 2 transpose) and lft_dihedral_batch moves lr and hr; bit-identical to
    `augment` for equally seeded generators."""
    from . import ensemble
    codes = np.empty(lr.shape[0], dtype=np.int32)
    for i in range(lr.shape[0]):
        c = 1 if rng.random() < 0.5 else 0
        c |= 2 if rng.random() < 0.5 else 0
        c |= 4 if rng.random() < 0.5 else 0
        codes[i] = c
    codes_dev = torch.from_numpy(codes).to(lr.device)
    return ensemble.dihedral_batch(lr, codes_dev), ensemble.dihedral_batch(hr, codes_dev)


# ---------------------------------------------------------------------------------------------- patch sources
class TensorPatchSource:
    def __init__(self, lr: torch.Tensor, hr: torch.Tensor):
        if lr.dim() == 3:
            lr, hr = lr[:, None], hr[:, None]
        assert lr.shape[0] == hr.shape[0] and lr.dim() == 4 and hr.dim() == 4
        self.lr, self.hr = lr.float(), hr.float()

    def __len__(self):
        return self.lr.shape[0]

    def get(self, indices: Sequence[int]):
        ix = torch.as_tensor(np.asarray(indices), dtype=torch.long, device=self.lr.device)
        return self.lr[ix], self.hr[ix]


class SyntheticPatchSource(TensorPatchSource):
    """Smooth random light fields: HR views = a random low-frequency image shifted by a per-view disparity; LR = box
    down-sampling of each view.  Learnable (the network must undo the blur), deterministic in ``seed``."""

    def __init__(self, n: int, angRes: int, scale: int, patch: int = 32, seed: int = 0, device="cpu", fmax: float = 0.25):
        # fmax: highest spatial frequency of the scene in cycles per HR pixel (0.25 = the LR Nyquist limit at 2x: hard scenes,
        # bicubic ~24 dB; 0.06: smooth scenes on which a trained network reaches the PSNR range of the reference's tables)
        g = np.random.Generator(np.random.PCG64([seed, n, angRes, scale, patch]))
        P = patch * scale
        hr = np.empty((n, angRes * P, angRes * P), dtype=np.float32)
        yy, xx = np.meshgrid(np.arange(P, dtype=np.float32), np.arange(P, dtype=np.float32), indexing="ij")
        for i in range(n):
            k = 6
            fy, fx = g.uniform(0.02, fmax, k), g.uniform(0.02, fmax, k)
            ph, am = g.uniform(0, 2 * np.pi, k), g.uniform(0.2, 1.0, k)
            disp = g.uniform(-1.5, 1.5)
            for u in range(angRes):
                for v in range(angRes):
                    img = sum(am[j] * np.sin(2 * np.pi * (fy[j] * (yy + disp * u) + fx[j] * (xx + disp * v)) + ph[j]) for j in range(k))
                    hr[i, u * P:(u + 1) * P, v * P:(v + 1) * P] = 0.5 + 0.5 * img / am.sum()
        hr_t = torch.from_numpy(hr)
        lr_t = hr_t.reshape(n, angRes, patch, scale, angRes, patch, scale).mean(dim=(3, 6)).reshape(n, angRes * patch, angRes * patch)
        super().__init__(lr_t.to(device), hr_t.to(device))


# ---------------------------------------------------------------------------------------------- the loop
def psnr_gpu(sr: torch.Tensor, hr: torch.Tensor) -> float:
    mse = float(((sr - hr) ** 2).mean())
    return float("inf") if mse == 0 else 10.0 * float(np.log10(1.0 / mse))


def fit(net, source, epochs: int, batch_size: int, lr: float = 2e-4, n_steps: int = 15, gamma: float = 0.5,
        start_epoch: int = 0, ckpt_dir: Optional[str] = None, model_name: str = "LFT", seed: int = 0,
        use_augmentation: bool = True, log=print, max_batches_per_epoch: Optional[int] = None, decay_rate: float = 0.0,
        batch_metrics: bool = False, ssim_range: float = 2.0, gpu_augment: bool = False, max_grad_norm: Optional[float] = None,
        guard: bool = False, ema_decay: Optional[float] = None, ema_warmup: bool = True, save_state: bool = False,
        resume: Optional[str] = None, validate=None, val_weights: str = "live", loss=None):
    """Train ``net`` (lft_amd.module.get_model on this rank's GPU) like reference train.py:86-110.  ``batch_size`` is
    the GLOBAL batch (reference --batch_size).  Returns the list of per-epoch mean losses (global).
    batch_metrics: also compute the reference's per-batch ``cal_metrics(args, label, out)`` (train.py:121-124: per-view PSNR / SSIM of
    the step's own output, means over positive views, then the mean over the epoch's batches) -- on the GPU (lft_view_metrics), with
    no host synchronisation inside the epoch -- and log the reference's line ('... loss is: %.5f, psnr is %.5f, ssim is %.5f');
    ``fit.last_metrics`` then holds the per-epoch (psnr, ssim) pairs.
    gpu_augment: augment with `augment_gpu` (one lft_dihedral_batch launch per tensor) instead of `augment`'s per-sample torch ops;
    the batches are bit-identical.
    max_grad_norm / guard: the guarded update of TrainStep (gradient-norm clipping; a step with a non-finite gradient is skipped
    instead of destroying the weights).  The guard block is read ONCE per epoch and the epoch line gains
    'grad norm %.3g, clipped %d, skipped %d (first bad: <parameter>)' -- norm and parameter of the epoch's last step, counts of the
    epoch; an epoch in which every step was skipped is reported with a warning.  ``fit.last_guard`` holds the per-epoch reports.
    ema_decay / ema_warmup: TrainStep keeps an exponential moving average of the weights; with ckpt_dir every epoch also writes
    '..._epoch_%02d_ema_model.pth' in the reference's format.
    save_state: after every epoch (rank 0) the one training state file of ckpt_dir is rewritten (save_training_state).
    resume: path of such a file.  The model checkpoint of its epoch (same directory) and the state are loaded, training goes on at
    the state's epoch (``start_epoch`` is ignored) and the returned history covers all epochs.  The per-epoch RNG derives from (seed,
    epoch, rank) and the learning rate from the epoch, so for the same seed, world size and global batch the continued run equals
    the uninterrupted one bit for bit; if one of them differs training continues and the log says so.
    validate: callable(net) -> float (higher is better), called on rank 0 after each epoch -- inside TrainStep.ema_weights() with
    val_weights='ema'.  The score joins the epoch line; an improvement writes '..._best_model.pth' (the validated weights, reference
    format) and is remembered, with its epoch, in the state file (``fit.best``).
    loss: an lft_amd.loss.LFLoss, its spec (a dict) or a penalty name -- the objective of TrainStep(loss=...); None: the reference's L1.
    The components are summed on the device and the epoch line gains 'pix %.5f, epi %.5f' (the means of the pixel and the EPI term;
    not for a spec that is the plain L1, which runs the reference's kernel) and, with ssim_weight > 0, ', ssim %.5f', the epoch mean of
    the structural term's S, and with focal_weight > 0 ', focal %.5f', the epoch mean of the focal-stack term's F.  The spec goes into the state file; a resume with another
    one continues and says so."""
    import torch.distributed as dist
    from .train import TrainStep
    rank, _, world = dp.env_world()
    if not (dist.is_available() and dist.is_initialized()):
        rank, world = 0, 1
    dev = next(net.parameters()).device
    if val_weights not in ("live", "ema"):
        raise ValueError(f"val_weights must be 'live' or 'ema', got {val_weights!r}")
    if val_weights == "ema" and validate is not None and ema_decay is None:
        raise ValueError("val_weights='ema' needs an ema_decay")
    if save_state and not ckpt_dir:
        raise ValueError("save_state needs a ckpt_dir")
    ts = TrainStep(net, lr=lr, weight_decay=decay_rate,            # reference train.py:82 weight_decay=args.decay_rate
                   max_grad_norm=max_grad_norm, guard=guard, ema_decay=ema_decay, ema_warmup=ema_warmup, loss=loss)
    loss_spec = None
    if loss is not None:
        from .loss import LFLoss
        loss_spec = (ts.loss or LFLoss.from_spec(loss)).spec()
    history = []
    fit.last_metrics = []
    fit.last_guard = []
    fit.best = {"score": None, "epoch": None}
    seen = {"steps_clipped": 0, "steps_skipped": 0}
    if resume:
        state = load_training_state(resume, ts, model_name=model_name)
        start_epoch = int(state["epoch"])
        history = [float(x) for x in state.get("history", [])]
        fit.last_metrics = [tuple(x) for x in state.get("last_metrics", [])]
        fit.last_guard = list(state.get("last_guard", []))
        fit.best = dict(state.get("best") or fit.best)
        if ts.guard and fit.last_guard:
            seen = {k: fit.last_guard[-1][k] for k in seen}
        now = {"seed": seed, "global_batch": batch_size, "world": world, "loss": loss_spec}
        changed = ["%s %s (saved with %s)" % (k, v, state[k]) for k, v in now.items() if k in state and state[k] != v]
        if rank == 0:
            log("resuming after epoch %d from %s" % (start_epoch, resume))
            if changed:
                log("WARNING: continuing with " + ", ".join(changed) + ": this run will not reproduce the uninterrupted one")
    for epoch in range(start_epoch, epochs):
        ts.lr = step_lr(lr, epoch, n_steps, gamma)
        rng = np.random.Generator(np.random.PCG64([seed, epoch, rank, 17]))
        batches = epoch_batches(len(source), batch_size, epoch, seed, rank, world)
        if max_batches_per_epoch:
            batches = batches[:max_batches_per_epoch]
        total = torch.zeros(3 if batch_metrics else 1, device=dev)
        terms = torch.zeros(3 if ts.last_loss_terms is None else ts.last_loss_terms.numel(), device=dev)   # (total, P, E[, S[, F]]) of TrainStep(loss=...)
        last = None
        for ix in batches:
            a, b = source.get(ix)
            a, b = a.to(dev, non_blocking=True), b.to(dev, non_blocking=True)
            if use_augmentation:
                a, b = (augment_gpu if gpu_augment else augment)(a, b, rng)
            loss = ts.step(a, b)
            if ts.last_loss_terms is not None:
                terms += ts.last_loss_terms
            if batch_metrics:
                from . import metrics
                p, s = metrics.view_metrics(b, ts.last_out, net.angRes, ssim_range)
                total += torch.stack([loss[0], p.sum() / (p > 0).sum(), s.sum() / (s > 0).sum()])
            else:
                total += loss
            last = (a, b)
        mean = total / max(1, len(batches))
        if world > 1:
            host = mean.cpu() if dist.get_backend() == "gloo" else mean
            dist.all_reduce(host)
            mean = host.to(dev) / world
            if ts.last_loss_terms is not None:
                host = terms.cpu() if dist.get_backend() == "gloo" else terms
                dist.all_reduce(host)
                terms = host.to(dev) / world
        history.append(float(mean[0]))
        if batch_metrics:
            fit.last_metrics.append((float(mean[1]), float(mean[2])))
            msg = "The %dth Train, loss is: %.5f, psnr is %.5f, ssim is %.5f" % (epoch + 1, history[-1], *fit.last_metrics[-1])   # train.py:90-91
        else:
            msg = "The %dth Train, loss is: %.5f, lr %.3g" % (epoch + 1, history[-1], ts.lr)
        if ts.last_loss_terms is not None:
            pix, epi, *more = (terms[1:] / max(1, len(batches))).tolist()
            msg += ", pix %.5f, epi %.5f" % (pix, epi)
            if more and ts.loss.ssim_weight > 0.0:                 # the epoch mean of S, the structural term's SSIM
                msg += ", ssim %.5f" % more[0]
            if len(more) > 1:                                      # the epoch mean of F, the focal-stack term
                msg += ", focal %.5f" % more[1]
        if last is not None and not batch_metrics:
            with torch.no_grad():
                msg += ", psnr(last batch) %.3f" % psnr_gpu(net(last[0]), last[1])
        warn = None
        if ts.guard:
            rep = ts.guard_report()                                # the epoch's one synchronising read (every rank holds the same figures)
            clipped, skipped = (rep[k] - seen[k] for k in ("steps_clipped", "steps_skipped"))
            seen = {k: rep[k] for k in seen}
            fit.last_guard.append(rep)
            msg += ", grad norm %.3g, clipped %d, skipped %d (first bad: %s)" % (rep["grad_norm"], clipped, skipped, rep["bad_parameter"] or "-")
            if batches and skipped == len(batches):
                warn = ("WARNING: every step of epoch %d was skipped for non-finite gradients (last seen in %s): the weights did not move"
                        % (epoch + 1, rep["bad_parameter"]))
        if rank == 0:
            if validate is not None:
                with (ts.ema_weights() if val_weights == "ema" else contextlib.nullcontext()), torch.no_grad():
                    score = float(validate(net))
                    msg += ", val(%s) %.4f" % (val_weights, score)
                    if fit.best["score"] is None or score > fit.best["score"]:
                        fit.best = {"score": score, "epoch": epoch + 1}
                        if ckpt_dir:                                   # the weights that were validated
                            save_checkpoint(net, os.path.join(ckpt_dir, best_checkpoint_name(model_name, net.angRes, net.factor)), epoch + 1)
            log(msg)
            if warn:
                log(warn)
            if ckpt_dir:
                save_checkpoint(net, os.path.join(ckpt_dir, checkpoint_name(model_name, net.angRes, net.factor, epoch + 1)), epoch + 1)
                if ts.ema is not None:
                    save_weights(ts.ema_state_dict(), os.path.join(ckpt_dir, ema_checkpoint_name(model_name, net.angRes, net.factor, epoch + 1)),
                                 epoch + 1)
                if save_state:
                    save_training_state(os.path.join(ckpt_dir, training_state_name(model_name, net.angRes, net.factor)), ts, epoch + 1,
                                        {"history": list(history), "last_metrics": list(fit.last_metrics), "last_guard": list(fit.last_guard),
                                         "seed": seed, "global_batch": batch_size, "world": world, "best": dict(fit.best),
                                         "loss": loss_spec})
    return history
