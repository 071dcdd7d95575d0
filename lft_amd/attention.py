"""Attention maps of the LFT network: the softmax weights the reference gets from ``nn.MultiheadAttention`` when the
``need_weights=False`` of ``model/LFT.py:183-187`` (SpaTrans) and ``:230-233`` (AngTrans) is turned to ``True`` -- the quantity
behind the paper's "Spatial-Aware Angular Modeling" figure.

Here the attention lives inside HIP kernels and the weights never leave the chip; the fp32 training forward, however, keeps
``Q | K`` of every attention block in its tape, and ``lft_train_attn_maps`` (include/lft_hip.h) turns those into the weights
on the device.  Layouts (``H`` = 8 heads, present only with ``per_head=True``; ``V = A*A``):

  * angular  ``angL``: ``[B, h, w, (H,) V_query, V_key]`` -- the reference's ``(b h w)`` batch order;
  * spatial  ``spaL``: compact ``[B, V, (H,) h, w, 5, 5]`` -- element ``(dy, dx)`` is the weight of query ``(y, x)`` on key
    ``(y+dy-2, x+dx-2)``; exactly 0 where that key is outside the view or the reference's clamped window (whose column range
    is clamped with ``h``, LFT.py:155).  For ``h < w`` a query with ``x - 2 >= h`` has an empty window: 25 zeros here, NaN in
    torch's ``need_weights=True`` path.  :func:`dense_spatial` / :func:`compact_from_dense` convert to and from the
    reference's ``[..., h*w, h*w]`` form for small views.

There is no CPU fallback: the maps come from the HIP kernels or an :class:`~lft_amd._lib.LftError` is raised.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional

import torch

from . import _lib
from .train import MATH, tape_bytes, train_forward

LAYERS = 4
WINDOW = 5
TAPE_BUDGET = 4 << 30          # bytes of tape attention_maps allows itself when max_batch is not given


def map_floats(block: int, per_head: bool, B: int, A: int, h: int, w: int) -> int:
    """Number of floats of one block's maps (lft_attn_maps_floats)."""
    return _lib.query("lft_attn_maps_floats", block, _lib.MAPS_HEADS if per_head else _lib.MAPS_MEAN, B, A, h, w)


def map_shape(block: int, per_head: bool, B: int, A: int, h: int, w: int):
    V = A * A
    H = (8,) if per_head else ()
    return (B, h, w, *H, V, V) if block == _lib.BLOCK_ANG else (B, V, *H, h, w, WINDOW, WINDOW)


def maps_from_tape(tape: torch.Tensor, block: int, layer: int, per_head: bool, B: int, A: int, h: int, w: int, s: int,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """lft_train_attn_maps on the current stream: the maps of one block from a tape that holds a complete train_forward of this
    shape.  ``out`` (contiguous float32 of map_floats elements on the tape's device) is written if given -- nothing is
    allocated then, so the call can be captured in a HIP graph."""
    dev = tape.device
    shape = map_shape(block, per_head, B, A, h, w)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev or out.numel() != map_floats(block, per_head, B, A, h, w):
        raise _lib.LftError(f"out must be a contiguous float32 tensor of {shape} on {dev}")
    _lib.enqueue("lft_train_attn_maps", dev, tape.data_ptr(), block, layer, _lib.MAPS_HEADS if per_head else _lib.MAPS_MEAN, out.data_ptr(),
                 B, A, h, w, s)
    return out.view(shape)


def _parse_blocks(blocks: Optional[Iterable[str]]):
    names = [f"{k}{l}" for l in range(LAYERS) for k in ("ang", "spa")] if blocks is None else list(blocks)
    out = []
    for n in names:
        if len(n) != 4 or n[:3] not in ("ang", "spa") or n[3] not in "0123":
            raise ValueError(f"unknown attention block {n!r}: expected 'ang0'..'ang3' or 'spa0'..'spa3'")
        out.append((n, _lib.BLOCK_ANG if n[:3] == "ang" else _lib.BLOCK_SPA, int(n[3])))
    return out


@torch.no_grad()
def attention_maps(net, lr: torch.Tensor, blocks: Optional[Iterable[str]] = None, per_head: bool = False, math: str = "fp32",
                   max_batch: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """The attention maps of ``net`` (lft_amd.module.get_model) for the LR mosaics ``lr`` [B,1,A*h,A*w] on a HIP device:
    ``{"ang0": t, "spa0": t, ..., "spa3": t}`` (or the subset ``blocks``), device tensors in the layouts of this module's
    docstring; head-averaged as torch's default, or one map per head with ``per_head``.

    Runs ``lft_amd.train.train_forward`` at ``math`` ('fp32' is the exact one) without autograd and reads its tape.  The
    batch is processed in chunks of ``max_batch`` patches with one tape re-used by all of them, so the tape stays bounded
    while the returned maps grow with B.  ``max_batch=None`` takes the largest chunk whose tape fits TAPE_BUDGET (4 GiB;
    the tape is about 1 GB per 5x5 patch of 32x32), at least 1."""
    if lr.dim() != 4 or lr.size(1) != 1:
        raise ValueError(f"expected [B,1,A*h,A*w], got {tuple(lr.shape)}")
    if not lr.is_cuda:
        raise _lib.LftError("lft_amd computes attention maps on a HIP device only (no CPU fallback); move the input and the model to 'cuda'")
    if math not in MATH:
        raise ValueError(f"unknown math mode {math!r}")
    A, s = net.angRes, net.factor
    B, _, Hm, Wm = lr.shape
    if Hm % A or Wm % A:
        raise ValueError(f"mosaic {Hm}x{Wm} is not divisible by angRes {A}")
    h, w = Hm // A, Wm // A
    sel = _parse_blocks(blocks)
    if max_batch is None:
        max_batch = max(1, TAPE_BUDGET // tape_bytes(1, A, h, w, s))
    nb = max(1, min(int(max_batch), B))
    x = lr.contiguous().float()
    dev = x.device
    ps = [p.detach() for p in net._params_in_order()]
    out = {name: torch.empty(map_shape(block, per_head, B, A, h, w), dtype=torch.float32, device=dev) for name, block, _ in sel}
    tapes = {}
    for b0 in range(0, B, nb):
        n = min(nb, B - b0)
        if n not in tapes:
            tapes[n] = torch.empty(tape_bytes(n, A, h, w, s), dtype=torch.uint8, device=dev)
        _, tape = train_forward(ps, x[b0:b0 + n], A, s, tape=tapes[n], math=math)
        for name, block, layer in sel:
            maps_from_tape(tape, block, layer, per_head, n, A, h, w, s, out=out[name][b0:b0 + n])
    return out


def _window_index(h: int, w: int, device):
    """key index [h*w, 25] of the centred 5x5 taps (row-major (dy, dx)) and whether the tap lies inside the view."""
    yy = torch.arange(h, device=device).view(h, 1, 1, 1)
    xx = torch.arange(w, device=device).view(1, w, 1, 1)
    d = torch.arange(WINDOW, device=device) - WINDOW // 2
    ky = (yy + d.view(1, 1, WINDOW, 1)).expand(h, w, WINDOW, WINDOW)
    kx = (xx + d.view(1, 1, 1, WINDOW)).expand(h, w, WINDOW, WINDOW)
    inside = (ky >= 0) & (ky < h) & (kx >= 0) & (kx < w)
    key = ky.clamp(0, h - 1) * w + kx.clamp(0, w - 1)
    return key.reshape(h * w, WINDOW * WINDOW), inside.reshape(h * w, WINDOW * WINDOW)


def dense_spatial(compact: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """compact ``[..., h, w, 5, 5]`` -> the reference's dense ``[..., h*w, h*w]`` (query, key) form, zeros elsewhere.  Plain
    index arithmetic on any device; meant for small views (the dense form grows with (h*w)^2)."""
    lead = compact.shape[:-4]
    if tuple(compact.shape[-4:]) != (h, w, WINDOW, WINDOW):
        raise ValueError(f"expected [..., {h}, {w}, 5, 5], got {tuple(compact.shape)}")
    key, inside = _window_index(h, w, compact.device)
    c = compact.reshape(-1, h * w, WINDOW * WINDOW)
    c = torch.where(inside.unsqueeze(0), c, torch.zeros((), dtype=c.dtype, device=c.device))
    dense = torch.zeros((c.shape[0], h * w, h * w), dtype=compact.dtype, device=compact.device)
    dense.scatter_add_(2, key.unsqueeze(0).expand_as(c), c)     # taps outside the view were clamped onto a key and carry 0
    return dense.reshape(*lead, h * w, h * w)


def compact_from_dense(dense: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """dense ``[..., h*w, h*w]`` -> compact ``[..., h, w, 5, 5]``: the weights on the centred 5x5 taps, 0 for taps outside the
    view.  Values are copied as they are (NaN rows of torch's need_weights path stay NaN on the taps inside the view)."""
    lead = dense.shape[:-2]
    if tuple(dense.shape[-2:]) != (h * w, h * w):
        raise ValueError(f"expected [..., {h * w}, {h * w}], got {tuple(dense.shape)}")
    key, inside = _window_index(h, w, dense.device)
    d = dense.reshape(-1, h * w, h * w)
    c = torch.gather(d, 2, key.unsqueeze(0).expand(d.shape[0], -1, -1))
    c = torch.where(inside.unsqueeze(0), c, torch.zeros((), dtype=c.dtype, device=c.device))
    return c.reshape(*lead, h, w, WINDOW, WINDOW)


def angular_row_mosaic(maps: torch.Tensor, A: int, query_view: int) -> torch.Tensor:
    """Head-averaged angular maps ``[n, h, w, V, V]`` -> LR-style mosaics ``[n, 1, A*h, A*w]`` of query view ``query_view``'s
    row: tile (u, v) holds, at every pixel, the weight that view puts on view (u, v)."""
    n, h, w, V, _ = maps.shape
    row = maps[:, :, :, query_view, :].reshape(n, h, w, A, A)
    return row.permute(0, 3, 1, 4, 2).reshape(n, 1, A * h, A * w).contiguous()


@torch.no_grad()
def scene_angular_attention(net, lr_scene: torch.Tensor, layer: int, query_view: Optional[int] = None, patch: int = 32,
                            stride: int = 16, math: str = "fp32", max_batch: Optional[int] = None) -> torch.Tensor:
    """The paper's angular-attention figure for a whole scene: ``lr_scene`` [A*h0, A*w0] (LR mosaic on a HIP device) ->
    [A*h0, A*w0] whose tile (u, v) is the head-averaged weight that ``query_view`` (default: the centre view) puts on view
    (u, v) in angular block ``layer``, at every pixel.  The scene is cut and re-assembled like the SR output of the test loop
    (scene.divide / scene.integrate at scale 1: every pixel comes from the patch that holds it in its central region)."""
    from . import scene
    A = net.angRes
    if not 0 <= int(layer) < LAYERS:
        raise ValueError(f"layer {layer} out of range")
    V = A * A
    q = V // 2 if query_view is None else int(query_view)
    if not 0 <= q < V:
        raise ValueError(f"query_view {q} out of range (0..{V - 1})")
    h0, w0 = lr_scene.shape[0] // A, lr_scene.shape[1] // A
    patches = scene.divide(lr_scene, A, patch, stride)
    name = f"ang{int(layer)}"
    if max_batch is None:
        max_batch = max(1, TAPE_BUDGET // tape_bytes(1, A, patch, patch, net.factor))
    rows = []
    for i in range(0, patches.shape[0], max_batch):            # per chunk: only the query view's row of the maps is kept
        m = attention_maps(net, patches[i:i + max_batch], blocks=[name], per_head=False, math=math, max_batch=max_batch)[name]
        rows.append(angular_row_mosaic(m, A, q))
    return scene.integrate(torch.cat(rows, dim=0), A, h0, w0, 1, patch, stride)
