"""The colour path: a low-resolution RGB light field in, super-resolved RGB views out.

The network works on luma.  Per sub-aperture view, in fp64 with MATLAB's conventions (csrc/lft_colour.cuh):

  1. x = double(LF) / 255 for uint8, double(LF) for single / double (stored in [0, 1]) -- unlike lft_amd.prepare, which takes the
     values as stored;
  2. ycc = rgb2ycbcr(x) (reference utils/utils.py:160-168);
  3. ``luma``: single(ycc[..., 0]) as the mosaic [A*H, A*W] that ``scene.super_resolve_scene`` and ``evaluate`` take;
  4. the network super-resolves it to sr_y [A*s*H, A*s*W];
  5. Cb and Cr are up-scaled by the reference's imresize(., s) (utils/imresize.py, the up-scaling branch: Keys cubic a = -0.5, no
     antialiasing, symmetric border, rows first) -- ``up_contributions`` builds its tables;
  6. rgb = Minv * (255 * [sr_y, cb_up, cr_up] - [16, 128, 128]) with Minv = inv(M) in fp64, the exact inverse of step 2.  The
     reference's own ycbcr2rgb (utils/utils.py:171-183) subtracts the offsets after the matrix and is NOT what is computed here
     (DESIGN section 10);
  7. convertDouble2Byte (utils/imresize.py:141-144): clip to [0, 1], * 255, round half to even -> uint8.

``merge`` does 1, 2, 5, 6 and 7 in one kernel launch; with ``sr_y=None`` Y is up-scaled like the chroma, which gives the bicubic
baseline (``bicubic_lf``).  ``super_resolve_lf`` is ``luma`` -> ``scene.super_resolve_scene`` -> ``merge``.  Everything runs on
the light field's device and current stream; there is no CPU path.
"""
from __future__ import annotations

import ctypes
from functools import partial
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, prepare
from ._lib import LftError

YCBCR_MATRIX = np.array([[65.481, 128.553, 24.966],
                         [-37.797, -74.203, 112.0],
                         [112.0, -93.786, -18.214]], dtype=np.float64)     # rgb2ycbcr, reference utils/utils.py:163-165
_OUT_CLASS = {torch.uint8: _lib.LF_UINT8, torch.float32: _lib.LF_FLOAT32}
_device_table = partial(prepare._device_table, up=True)         # (in_len, s, device): the up-scaling tables, in prepare's cache


def inverse_matrix() -> np.ndarray:
    """Minv of step 6: np.linalg.inv of rgb2ycbcr's matrix, fp64 [3, 3]."""
    return np.linalg.inv(YCBCR_MATRIX)


def up_contributions(in_len: int, s: int) -> Tuple[np.ndarray, np.ndarray]:
    """The reference's ``contributions(L, L*s, s, cubic, 4.0)`` of one axis (utils/imresize.py:32-52, scale >= 1): (weights fp64
    [L*s, P], indices int32 [L*s, P]); prepare.imresize_table without antialiasing, 6 taps before the all-zero columns are dropped."""
    return prepare.imresize_table(in_len, s, up=True)


def _field(lf, A: int, device=None) -> torch.Tensor:
    """lf as the kernels take it: a [U, V, H, W, C] device tensor as it is, a loaded array through prepare.to_device."""
    if isinstance(lf, np.ndarray):
        return prepare.to_device(lf, A, prepare._dev(device))
    if not isinstance(lf, torch.Tensor):
        raise LftError(f"the light field must be a torch tensor or a numpy array, got {type(lf).__name__}")
    if lf.dim() != 5:
        raise LftError(f"the light field must be [U, V, H, W, C], got shape {tuple(lf.shape)}")
    if lf.device.type != "cuda":
        raise LftError(f"the light field must be on the GPU, got a tensor on {lf.device} (there is no CPU path)")
    if lf.dtype not in prepare._CLASS:
        raise LftError(f"light field of class {lf.dtype}: uint8, float32 and float64 are supported")
    return lf


def luma(lf, A: int, device=None) -> torch.Tensor:
    """lft_lf_luma: single(Y) of the centre A x A views, scaled to [0, 1], as the mosaic [A*H, A*W] fp32.  Enqueue only."""
    t = _field(lf, A, device)
    H, W = int(t.shape[2]), int(t.shape[3])
    if A < 1:
        raise LftError(f"angRes must be positive, got {A}")
    y = torch.empty(A * H, A * W, dtype=torch.float32, device=t.device)
    _lib.enqueue("lft_lf_luma", t.device, *prepare.lf_args(t), A, y.data_ptr() or None)
    return y


def merge(lf, sr_y: Optional[torch.Tensor], A: int, s: int, out_dtype=torch.uint8, device=None) -> torch.Tensor:
    """lft_colour_merge: RGB views [A, A, s*H, s*W, 3] from the light field's chroma, up-scaled s times, and the luma mosaic sr_y
    [A*s*H, A*s*W] fp32 (None: the light field's own luma, up-scaled like the chroma).  out_dtype torch.uint8 gives the quantised
    image, torch.float32 the unquantised, unclipped rgb.  Enqueue only."""
    t = _field(lf, A, device)
    H, W = int(t.shape[2]), int(t.shape[3])
    if out_dtype not in _OUT_CLASS:
        raise LftError(f"out_dtype must be torch.uint8 or torch.float32, got {out_dtype}")
    if A < 1:
        raise LftError(f"angRes must be positive, got {A}")
    if s not in (2, 4):
        raise LftError(f"scale factor must be 2 or 4, got {s}")
    if sr_y is not None:
        if not isinstance(sr_y, torch.Tensor) or sr_y.device != t.device:
            raise LftError("sr_y must be a tensor on the light field's device")
        if tuple(sr_y.shape) != (A * s * H, A * s * W):
            raise LftError(f"sr_y must be the mosaic [{A * s * H}, {A * s * W}], got shape {tuple(sr_y.shape)}")
        sr_y = sr_y.contiguous().float()
    wh, ih = _device_table(H, s, t.device)
    ww, iw = _device_table(W, s, t.device)
    out = torch.empty(A, A, s * H, s * W, 3, dtype=out_dtype, device=t.device)
    minv = (ctypes.c_double * 9)(*inverse_matrix().reshape(-1))
    _lib.enqueue("lft_colour_merge", t.device, *prepare.lf_args(t), A, s, sr_y.data_ptr() if sr_y is not None else None, wh.data_ptr(),
                 ih.data_ptr(), wh.shape[1], ww.data_ptr(), iw.data_ptr(), ww.shape[1], minv, out.data_ptr() or None, _OUT_CLASS[out_dtype])
    return out


def bicubic_lf(lf, A: int, s: int, out_dtype=torch.uint8, device=None) -> torch.Tensor:
    """The bicubic baseline: every channel up-scaled by imresize(., s), [A, A, s*H, s*W, 3]."""
    return merge(lf, None, A, s, out_dtype, device)


@torch.no_grad()
def super_resolve_lf(net, lf, patch: int = 32, stride: int = 16, max_batch: int = 64, ensemble=None,
                     out_dtype=torch.uint8, shear=None, blend=None, views: str = "centre", astride=None, angular="flat") -> torch.Tensor:
    """Super-resolved RGB views [A, A, s*H, s*W, 3] of a low-resolution RGB light field: ``luma`` -> the network over the whole
    scene (``scene.super_resolve_scene``: any precision of `net`, any ``ensemble=``, ``shear=`` or ``blend=``) -> ``merge``.  A loaded array goes to the
    device of the network's parameters.
    views: "centre" (the centre A x A views, as always) or "all": every view of a square U x U field, [U, U, s*H, s*W, 3], through
    ``field.super_resolve_field`` with its `astride` and `angular` (A x A windows over the views, a weighted mean where they overlap)."""
    from . import scene
    A, s = net.angRes, net.factor
    if views not in ("centre", "all"):
        raise LftError(f"views must be centre or all, got {views!r}")
    dev = None
    if isinstance(lf, np.ndarray):
        dev = next(net.parameters()).device
    if views == "all":
        from . import field
        shape = tuple(getattr(lf, "shape", ()))
        if len(shape) != 5:
            raise LftError(f"the light field must be [U, V, H, W, C], got shape {shape}")
        U, V = int(shape[0]), int(shape[1])
        if U != V:
            raise LftError(f"super_resolve_lf(views=all): a light field of shape {shape} has {U} x {V} views; the colour path takes a square field "
                           "(field.super_resolve_field takes U != V)")
        t = _field(lf, U, dev)
        sr_y = field.super_resolve_field(net, luma(t, U), U, V, patch, stride, max_batch, astride, angular, ensemble, shear, blend)
        return merge(t, sr_y, U, s, out_dtype)
    t = _field(lf, A, dev)
    sr_y = scene.super_resolve_scene(net, luma(t, A), patch, stride, max_batch, ensemble, shear, **({} if blend is None else {"blend": blend}))
    return merge(t, sr_y, A, s, out_dtype)
