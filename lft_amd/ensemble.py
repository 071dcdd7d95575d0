"""Geometric self-ensemble at inference (the "+" variant of SR toolboxes) and the dihedral transforms under it.

For a light field the dihedral group acts on the whole mosaic: a mirror of the mosaic mirrors the angular and the spatial axis
together, a transpose swaps (u, y) with (v, x) -- the three coin flips of the reference's ``augmentation``
(utils/utils_datasets.py:114-124).  A code ``t`` in 0..7 has three bits, applied in this order: bit 0 mirrors left-right
(``flip(-1)``), bit 1 up-down (``flip(-2)``), bit 2 transposes (``transpose(-1, -2)``).  A set of variants is an 8-bit ``mask``
(bit t set = code t takes part, E = popcount, ascending code order).  The ensemble super-resolves the E images of the input,
maps every result back with the inverse transform and averages: ``acc = first; acc += the others; acc * (1 / E)`` in fp32.

Everything here runs in liblft_hip.so (lft_dihedral_batch / _expand / _merge, include/lft_hip.h) on the input's HIP device; there
is no CPU fallback."""
from __future__ import annotations

import torch

from . import _lib

MASKS = {"dihedral": 0xFF, "flips": 0x0F, "none": 0x01}
TRANSPOSING = 0xF0                      # the codes with bit 2 set


def mask_of(mode) -> int:
    """A mode name of MASKS, or an 8-bit mask itself."""
    if isinstance(mode, str):
        if mode not in MASKS:
            raise ValueError(f"unknown ensemble mode {mode!r}: one of {sorted(MASKS)}")
        return MASKS[mode]
    mask = int(mode)
    if not 0 < mask <= 0xFF:
        raise ValueError(f"ensemble mask {mask:#x}: one bit per dihedral code 0..7, at least one set")
    return mask


def codes_of(mask: int):
    return [t for t in range(8) if mask >> t & 1]


def _images(x: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.LftError(f"{what}: lft_amd runs on a HIP device only (no CPU fallback); move the tensor to 'cuda'")
    if x.dim() != 4 or x.size(1) != 1:
        raise ValueError(f"{what}: expected [B,1,H,W], got {tuple(x.shape)}")
    return x.contiguous().float()


def _one_shape(mask: int, H: int, W: int, what: str) -> None:
    if H != W and mask & TRANSPOSING and mask & ~TRANSPOSING & 0xFF:
        raise ValueError(f"{what}: mask {mask:#x} mixes transposing and non-transposing codes, whose {H}x{W} images differ in shape "
                         'and cannot share one batch; use "flips" (0x0F) for non-square mosaics')


def dihedral_batch(x: torch.Tensor, codes) -> torch.Tensor:
    """out[b] = T_(codes[b] & 7)(x[b]) for x [B,1,H,W]; codes: B ints (a sequence, or an int32 tensor, which may already be on the
    device).  Returns [B,1,H,W]; for H != W every code must transpose ([B,1,W,H]) or none."""
    x = _images(x, "dihedral_batch")
    B, _, H, W = x.shape
    c = torch.as_tensor(codes, dtype=torch.int32)
    if c.numel() != B:
        raise ValueError(f"dihedral_batch: {c.numel()} codes for {B} images")
    tr = (c.cpu() & 4) != 0 if H != W else None
    if tr is not None and bool(tr.any()) and not bool(tr.all()):
        raise ValueError(f"dihedral_batch: transposing and non-transposing codes on {H}x{W} images differ in shape and cannot share "
                         'one batch (the "flips" codes 0..3 keep the shape)')
    c = c.to(x.device).contiguous()
    out = torch.empty((B, 1, W, H) if tr is not None and bool(tr.all()) else (B, 1, H, W), dtype=torch.float32, device=x.device)
    _lib.enqueue("lft_dihedral_batch", x.device, x.data_ptr(), out.data_ptr(), c.data_ptr(), B, H, W)
    return out


def expand(x: torch.Tensor, mask) -> torch.Tensor:
    """x [B,1,H,W] -> the E variants of every image, adjacent: out[b*E + k] = T_code_k(x[b]); [B*E,1,H,W] ([B*E,1,W,H] when every
    code of the mask transposes)."""
    mask = mask_of(mask)
    x = _images(x, "expand")
    B, _, H, W = x.shape
    _one_shape(mask, H, W, "expand")
    E = len(codes_of(mask))
    shape = (B * E, 1, W, H) if not mask & ~TRANSPOSING & 0xFF else (B * E, 1, H, W)
    out = torch.empty(shape, dtype=torch.float32, device=x.device)
    _lib.enqueue("lft_dihedral_expand", x.device, x.data_ptr(), out.data_ptr(), mask, B, H, W)
    return out


def merge(y: torch.Tensor, mask) -> torch.Tensor:
    """The inverse of `expand` with the average: y [B*E,1,·,·] (variants adjacent, as `expand` lays them out, each in the shape its
    code gives it) -> [B,1,H,W] = (1/E) sum_k T^-1_code_k(y[b*E + k])."""
    mask = mask_of(mask)
    y = _images(y, "merge")
    N, _, Hy, Wy = y.shape
    _one_shape(mask, Hy, Wy, "merge")
    E = len(codes_of(mask))
    if N % E:
        raise ValueError(f"merge: {N} images are not a multiple of the {E} variants of mask {mask:#x}")
    H, W = (Wy, Hy) if not mask & ~TRANSPOSING & 0xFF else (Hy, Wy)
    out = torch.empty((N // E, 1, H, W), dtype=torch.float32, device=y.device)
    _lib.enqueue("lft_dihedral_merge", y.device, y.data_ptr(), out.data_ptr(), mask, N // E, H, W)
    return out


def network_chunks(net, x: torch.Tensor, max_batch: int) -> torch.Tensor:
    """net(x) in contiguous chunks of at most max_batch network inputs."""
    max_batch = max(1, int(max_batch))
    if x.shape[0] <= max_batch:
        return net(x)
    return torch.cat([net(x[i:i + max_batch]) for i in range(0, x.shape[0], max_batch)], dim=0)


def self_ensemble(net, lr: torch.Tensor, mode="dihedral", max_batch: int = 64) -> torch.Tensor:
    """lr [B,1,A*h,A*w] -> the average over the variants of `mode` of T^-1(net(T(lr))), [B,1,A*h*s,A*w*s]: expand, the network in
    chunks of at most `max_batch` inputs (the variants of one patch are adjacent, so chunks are contiguous), merge.  Inference
    only: eval mode under no_grad (the module's mode is restored).  "dihedral" needs h == w: the transposed half would be another
    network shape -- use "flips" there."""
    mask = mask_of(mode)
    if not isinstance(lr, torch.Tensor) or not lr.is_cuda:
        raise _lib.LftError("self_ensemble: lft_amd runs on a HIP device only (no CPU fallback); move the input and the model to 'cuda'")
    was_training = net.training
    net.eval()
    try:
        with torch.no_grad():
            return merge(network_chunks(net, expand(lr, mask), max_batch), mask)
    finally:
        net.train(was_training)
