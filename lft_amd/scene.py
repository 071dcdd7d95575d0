"""Whole-scene inference around the hot path: the reference's test loop (test.py:83-101) cuts a scene into
overlapping 32x32-LR patches with LFdivide (utils/utils.py:91-123), runs the network ONE PATCH AT A TIME, and
re-assembles with LFintegrate (utils.py:141-157).  Here the cut and the re-assembly are GPU gathers
(lft_scene_divide / lft_scene_integrate) and all patches of the scene go through the network as batches.

Per-patch disparity compensation by integer shear
-------------------------------------------------
LFT's angular Transformer attends across the A×A views at the same pixel, which only works while a scene point stays within a
pixel or so across the views.  A shear by a whole number `k` of LR pixels per view step is lossless: view `(u, v)` of a patch is
cut at an offset of `k·(u−u0)`, `k·(v−u0)` pixels, the network sees a light field whose residual disparity is `d − k`, and the SR
patch is put back at `s·k·(u−u0)`, again a whole number of pixels.  No pixel is interpolated on either side.  ``divide`` and
``integrate`` take `shear=` (lft_scene_divide_shear, lft_scene_integrate_shear), ``estimate_shear`` chooses it (one plane sweep,
then lft_shear_vote), ``super_resolve_scene(..., shear=)`` joins them; csrc/lft_shear.cuh, declared in include/lft_hip_shear.h.

Let `bdr = (patch − stride)/2`, `u0 = A // 2`, `Δu = u − u0` and `Δv = v − u0` (whole numbers for even A too),
`R = max(u0, A−1−u0)`, and `kmax = LFT_SHEAR_MAX` if `R = 0`, else `min(LFT_SHEAR_MAX, bdr // R)` (``shear_limit``).  Every kernel
clamps `k_n` into `[−kmax, kmax]` itself: a device array can hold anything, and divide and integrate must stay inverse to each
other.  The sign is the disparity module's: a point seen at `y` in view `u` is seen at `y + d·(u'−u)` in view `u'`, so `k = d`
aligns the views.

**Sheared divide.** Patch `n = ku·nv + kv`, view `(u, v)`, pixel `(y, x)` of the patch.
- `ey = ku·stride + y`, and `ex` likewise.
- The value is 0 where `ey ≥ h0 + 2·bdr` or `ex ≥ w0 + 2·bdr`: today's test, on the unsheared coordinates.
- Elsewhere the value is `scene[u·h0 + fold(ey − bdr + k_n·Δu, h0), v·w0 + fold(ex − bdr + k_n·Δv, w0)]`.
- `fold(i, n)`: `m = i mod 2n` (non-negative), then `m` if `m < n`, else `2n−1−m`. This is `reflect_idx` continued to any integer;
  on `[−n, 2n−1]` the two agree.

**Sheared integrate.** SR view `(u, v)`, SR pixel `(Y, X)`.
- `ku = Y / (stride·s)`, `i = Y − ku·stride·s`, and `kv`, `j` likewise; `n = ku·nv + kv`, as today.
- The value is the SR patch `n`, view `(u, v)`, at row `bdr·s + i − s·k_n·Δu` and column `bdr·s + j − s·k_n·Δv`.
- With the clamp those lie inside the patch, and they never touch a zero-filled pixel.

**Vote.** `index` int32 and `confidence` fp32 `[B, H, W]`, D whole-number slopes.
- `count[b, j]` is the number of pixels with `margin ≤ y < H−margin`, `margin ≤ x < W−margin`, clamped index equal to `j`, and
  confidence finite and `≥ min_confidence`.
- `shear[b] = slopes[j*]`, where `j*` has the largest count. On a tie the smallest `|slope|` wins, then the smaller slope. If every
  count is 0 the result is 0.
- Counts are integers, so arrival order cannot matter.

Windowed blending of overlapping SR patches
-------------------------------------------
``integrate`` keeps the central `stride·s` square of every SR patch and drops the rest; the kept squares meet edge to edge, so an
error that differs from patch to patch shows as a seam.  With `blend=` every SR patch pixel that shows a scene pixel contributes to
it, weighted by a separable window over the patch (lft_scene_integrate_blend: one gather kernel, with or without `shear=`;
csrc/lft_blend.cuh, declared in include/lft_hip_blend.h).  `blend=None` is the crop and runs the kernels it always ran.

All sizes are in SR pixels.  `pz = patch·s`, `S = stride·s`, `bdr = (pz − S)/2` (an odd `patch − stride` is refused), `u0 = A // 2`,
`sk_n = s·clamp(shear[n], ±kmax)`, or 0 without shear.  Pixel `(a, b)` of view `(u, v)` of SR patch `n = ku·nv + kv` shows scene pixel
`Y = ku·S + a − bdr + sk_n·(u − u0)`, `X = kv·S + b − bdr + sk_n·(v − u0)`: the sheared integrate's map, read backwards.  The pixel
contributes iff `0 ≤ Y < h0·s` and `0 ≤ X < w0·s`; that drops the reflected margin and everything beyond the extended view, so no
zero-filled position ever contributes.  With the window table `w[0..pz)`, fp32 and strictly positive,
`out = Σ (w[a]·w[b])·sub[n,u,a,v,b] / Σ w[a]·w[b]`, summed over the contributing patches in ascending `ku`, then `kv`, every operation
one rounded fp32 operation and the quotient correctly rounded.  The tables (``window_table``) are built in fp64 and rounded once:
`"hann"`: `sin²(π(i+½)/pz)`, `"linear"`: `min(i+½, pz−i−½)·2/pz`, `"flat"`: 1.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import LftError


def scene_counts(h0: int, w0: int, patch: int = 32, stride: int = 16):
    nu, nv = ctypes.c_int(0), ctypes.c_int(0)
    _lib.call("lft_scene_counts", h0, w0, patch, stride, ctypes.byref(nu), ctypes.byref(nv))
    return nu.value, nv.value


def _reach(A: int) -> int:
    """R: the largest |u - u0| of the A views."""
    return max(A // 2, A - 1 - A // 2)


def shear_limit(A: int, patch: int = 32, stride: int = 16) -> int:
    """kmax: the largest |k| of a patch whose sheared cut stays inside the border the patch does not contribute.  A tiling with
    an odd patch - stride is refused, as the sheared kernels refuse it: its border is not the same on both sides."""
    if A < 1 or stride < 1 or stride > patch:
        raise LftError(f"shear_limit: angRes {A}, patch {patch}, stride {stride}")
    if (patch - stride) % 2:
        raise LftError(f"shear_limit: patch - stride = {patch - stride} is odd: the sheared tiling needs the same border on both sides")
    R = _reach(A)
    return _lib.SHEAR_MAX if R == 0 else min(_lib.SHEAR_MAX, (patch - stride) // 2 // R)


def check_shear_limit(k: int, A: int, patch: int, stride: int) -> None:
    """The refusal of one shear for all patches that the tiling cannot hold; the message says which tiling could."""
    kmax = shear_limit(A, patch, stride)
    if abs(k) <= kmax:
        return
    if abs(k) > _lib.SHEAR_MAX:
        raise LftError(f"shear {k}: kmax is {kmax} for angRes {A}, patch {patch}, stride {stride}, and no patch or stride allows more than {_lib.SHEAR_MAX}")
    need = 2 * abs(k) * _reach(A)                      # of patch - stride; even, so both offers keep the border the same on both sides
    other = f", or a stride of at most {patch - need} at this patch," if patch - need >= 1 else ""
    raise LftError(f"shear {k}: kmax is {kmax} for angRes {A}, patch {patch}, stride {stride}; a patch of at least {stride + need} at this stride{other} "
                   "would allow it")


def _shear_tensor(shear, n: int, like: torch.Tensor) -> torch.Tensor:
    """`shear` as the kernels take it: int32 [n], contiguous, on like's device; anything else is refused."""
    if not isinstance(shear, torch.Tensor) or shear.dtype != torch.int32 or tuple(shear.shape) != (n,):
        raise LftError(f"shear must be an int32 tensor of shape [{n}] (one value per patch), got "
                       f"{getattr(shear, 'dtype', type(shear).__name__)} {tuple(getattr(shear, 'shape', ()))}")
    if shear.device != like.device:
        raise LftError(f"shear is on {shear.device}, the scene on {like.device}")
    return shear.contiguous()


WINDOWS = ("hann", "linear", "flat")
_windows = {}                                           # (kind, pz, device) -> the window table on that device


def window_table(kind: str, pz: int) -> np.ndarray:
    """The window table of `kind` over a patch side of pz SR pixels: built in fp64, rounded once to fp32 [pz]; every entry is
    positive and the table is symmetric."""
    if kind not in WINDOWS:
        raise LftError(f"blend must be None, one of {', '.join(WINDOWS)}, or a float32 tensor, got {kind!r}")
    if isinstance(pz, bool) or int(pz) != pz or not 1 <= pz <= _lib.BLEND_MAX_PZ:
        raise LftError(f"a window of {pz!r} entries (1 .. {_lib.BLEND_MAX_PZ})")
    c = np.arange(int(pz), dtype=np.float64) + 0.5
    w = {"hann": lambda: np.sin(np.pi * c / pz) ** 2, "linear": lambda: np.minimum(c, pz - c) * 2.0 / pz, "flat": lambda: np.ones(int(pz))}[kind]()
    return w.astype(np.float32)


def blend_window(kind: str, pz: int, device=None) -> torch.Tensor:
    """``window_table(kind, pz)`` on `device` (default: the current HIP device), float32 [pz]; made once per device and kept."""
    table = window_table(kind, pz)                      # a wrong kind or size is refused before the device is asked for
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    key = (kind, int(pz), str(device))
    if key not in _windows:
        _windows[key] = torch.from_numpy(table).to(device)
    return _windows[key]


def clear_cache() -> None:
    """Drop the cached window tables."""
    _windows.clear()


def check_blend(blend, ang: int, patch: int, stride: int, scale: int) -> None:
    """What the blended integrate refuses without a device: a `blend` that is neither a window's name nor a float32 tensor
    [patch*scale], a tiling without the same border on both sides, a scale factor other than 2 or 4."""
    if isinstance(blend, str):
        window_table(blend, patch * scale)
    elif not isinstance(blend, torch.Tensor) or blend.dtype != torch.float32 or tuple(blend.shape) != (patch * scale,):
        raise LftError(f"blend must be None, one of {', '.join(WINDOWS)}, or a float32 tensor of shape [{patch * scale}] (positive weights over the SR "
                       f"patch side), got {getattr(blend, 'dtype', type(blend).__name__)} {tuple(getattr(blend, 'shape', ()))}")
    if scale not in (2, 4):
        raise LftError(f"blend: scale factor must be 2 or 4, got {scale}")
    shear_limit(ang, patch, stride)                     # the tiling: angRes, stride <= patch, an even patch - stride


def divide(scene: torch.Tensor, ang: int, patch: int = 32, stride: int = 16, shear=None) -> torch.Tensor:
    """scene: float32 [A*h0, A*w0] on a HIP device -> [numU*numV, 1, A*patch, A*patch].
    shear: None, or int32 [numU*numV] on the scene's device: view (u, v) of patch n is cut shear[n]*(u - u0), shear[n]*(v - u0)
    pixels further on (the module docstring has the definition; values beyond ``shear_limit`` are clamped to it)."""
    if scene.dim() != 2 or (shear is None and not scene.is_cuda):
        raise LftError("scene must be a 2-D float32 tensor on a HIP device")
    H, W = scene.shape
    h0, w0 = H // ang, W // ang
    nu, nv = scene_counts(h0, w0, patch, stride)
    if shear is not None:
        shear = _shear_tensor(shear, nu * nv, scene)         # a wrong shear is refused before the device is asked for
        if not scene.is_cuda:
            raise LftError("scene must be a 2-D float32 tensor on a HIP device")
    x = scene.contiguous().float()
    out = torch.empty((nu * nv, 1, ang * patch, ang * patch), dtype=torch.float32, device=scene.device)
    if shear is None:
        _lib.enqueue("lft_scene_divide", scene.device, x.data_ptr(), out.data_ptr(), ang, h0, w0, patch, stride)
    else:
        _lib.enqueue("lft_scene_divide_shear", scene.device, x.data_ptr(), shear.data_ptr(), out.data_ptr(), ang, h0, w0, patch, stride)
    return out


def integrate(sr_patches: torch.Tensor, ang: int, h0: int, w0: int, scale: int, patch: int = 32, stride: int = 16, shear=None, blend=None) -> torch.Tensor:
    """sr_patches: float32 [numU*numV, 1, A*patch*s, A*patch*s] -> SR scene mosaic [A*h0*s, A*w0*s].
    shear: None, or the int32 [numU*numV] the patches were cut with (``divide``): every SR patch is put back s*shear[n] pixels per
    view step against the cut.
    blend: None (the crop: the central stride*s square of every patch, today's kernels), "hann", "linear" or "flat"
    (``window_table``), or a float32 tensor [patch*s] of positive weights on the patches' device: the window-weighted mean of every
    SR patch pixel that shows a scene pixel (the module docstring has the definition), with or without `shear`."""
    if blend is not None:
        check_blend(blend, ang, patch, stride, scale)
    if shear is not None or blend is not None:
        nu, nv = scene_counts(h0, w0, patch, stride)
        if shear is not None:
            shear = _shear_tensor(shear, nu * nv, sr_patches)
        if blend is not None:
            side = ang * patch * scale
            if not isinstance(sr_patches, torch.Tensor) or tuple(sr_patches.shape) != (nu * nv, 1, side, side):
                raise LftError(f"sr_patches must be [{nu * nv}, 1, {side}, {side}] for this tiling, got {tuple(getattr(sr_patches, 'shape', ()))}")
            if isinstance(blend, torch.Tensor) and blend.device != sr_patches.device:
                raise LftError(f"blend is on {blend.device}, the patches on {sr_patches.device}")
        if not sr_patches.is_cuda:
            raise LftError("sr_patches must be a float32 tensor on a HIP device")
    x = sr_patches.contiguous().float()
    out = torch.empty((ang * h0 * scale, ang * w0 * scale), dtype=torch.float32, device=x.device)
    if blend is not None:
        w = blend_window(blend, patch * scale, x.device) if isinstance(blend, str) else blend.contiguous()
        _lib.enqueue("lft_scene_integrate_blend", x.device, x.data_ptr(), None if shear is None else shear.data_ptr(), w.data_ptr(), out.data_ptr(),
                     ang, h0, w0, patch, stride, scale)
    elif shear is None:
        _lib.enqueue("lft_scene_integrate", x.device, x.data_ptr(), out.data_ptr(), ang, h0, w0, patch, stride, scale)
    else:
        _lib.enqueue("lft_scene_integrate_shear", x.device, x.data_ptr(), shear.data_ptr(), out.data_ptr(), ang, h0, w0, patch, stride, scale)
    return out


def integrate_ensemble(sr_variants: torch.Tensor, mask: int, ang: int, h0: int, w0: int, scale: int, patch: int = 32,
                       stride: int = 16) -> torch.Tensor:
    """`integrate` and lft_amd.ensemble.merge in one pass: sr_variants float32 [numU*numV*E, 1, A*patch*s, A*patch*s] (the E
    variants of a patch adjacent, as lft_amd.ensemble.expand lays them out) -> SR scene mosaic [A*h0*s, A*w0*s]."""
    x = sr_variants.contiguous().float()
    out = torch.empty((ang * h0 * scale, ang * w0 * scale), dtype=torch.float32, device=x.device)
    _lib.enqueue("lft_scene_integrate_ens", x.device, x.data_ptr(), out.data_ptr(), mask, ang, h0, w0, patch, stride, scale)
    return out


def vote(index: torch.Tensor, confidence: torch.Tensor, slopes: torch.Tensor, margin: int, min_confidence: float = 0.5):
    """lft_shear_vote on the maps of a sweep: index int32 and confidence float32 [B, H, W], slopes int32 [D] (whole numbers), all on
    one GPU -> (shear int32 [B], counts int32 [B, D]).  The module docstring has the rule.  Enqueue only."""
    for name, t, dtype, dim in (("index", index, torch.int32, 3), ("confidence", confidence, torch.float32, 3), ("slopes", slopes, torch.int32, 1)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != dim:
            raise LftError(f"the {name} must be a {dtype} tensor of {dim} dimensions, got {getattr(t, 'dtype', type(t).__name__)} "
                           f"{tuple(getattr(t, 'shape', ()))}")
    if confidence.shape != index.shape:
        raise LftError(f"an index of {tuple(index.shape)} and a confidence of {tuple(confidence.shape)} do not vote together")
    if confidence.device != index.device or slopes.device != index.device:
        raise LftError(f"the index, the confidence and the slopes must be on one device, got {index.device}, {confidence.device} and {slopes.device}")
    if index.device.type != "cuda":
        raise LftError(f"the index must be on the GPU, got a tensor on {index.device} (there is no CPU path)")
    B, H, W = (int(n) for n in index.shape)
    D = int(slopes.shape[0])
    counts = torch.empty(B, D, dtype=torch.int32, device=index.device)
    shear = torch.empty(B, dtype=torch.int32, device=index.device)
    index, confidence, slopes = index.contiguous(), confidence.contiguous(), slopes.contiguous()
    if B:
        _lib.enqueue("lft_shear_vote", index.device, index.data_ptr(), confidence.data_ptr(), slopes.data_ptr(), B, H, W, D, int(margin),
                     float(min_confidence), counts.data_ptr(), shear.data_ptr())
    return shear, counts


def estimate_shear(patches: torch.Tensor, ang: int, max_shear=None, min_confidence: float = 0.5, radius: int = 2, margin=None,
                   stride: int = 16) -> torch.Tensor:
    """The shear of every patch of ``divide``'s (unsheared) batch [N, 1, A*patch, A*patch], int32 [N] on its device.  Two steps,
    enqueue only, nothing is read back to the host: one ``disparity.disparity`` of the batch over the whole-number slopes -K .. K
    (nearest samples, aggregation `radius`, seen from the view (u0, u0)), K = min(max_shear, ``shear_limit``), then lft_shear_vote
    over the pixels at least `margin` from the patch's edge -- by default bdr, the region the patch contributes.  `stride` is the
    tiling's: with the patch size it sets kmax and bdr."""
    if not isinstance(patches, torch.Tensor) or patches.dim() != 4 or patches.shape[1] != 1 or ang < 1 or patches.shape[2] != patches.shape[3] \
            or patches.shape[2] % ang:
        raise LftError(f"patches must be a batch [N, 1, A*patch, A*patch] of divide, got {tuple(getattr(patches, 'shape', ()))} with angRes {ang}")
    patch = int(patches.shape[2]) // ang
    kmax = shear_limit(ang, patch, stride)
    if max_shear is not None and (isinstance(max_shear, bool) or int(max_shear) != max_shear or max_shear < 0):
        raise LftError(f"max_shear must be None or a non-negative integer, got {max_shear!r}")
    K = kmax if max_shear is None else min(int(max_shear), kmax)
    margin = (patch - stride) // 2 if margin is None else margin
    if isinstance(margin, bool) or int(margin) != margin or margin < 0 or 2 * margin >= patch:
        raise LftError(f"margin must be an integer with 0 <= 2*margin < {patch}, got {margin!r}")
    from . import disparity
    u0 = ang // 2
    res = disparity.disparity(patches, [float(k) for k in range(-K, K + 1)], angRes=ang, interp="nearest", radius=radius, centre=(u0, u0))
    slopes = torch.arange(-K, K + 1, dtype=torch.int32, device=patches.device)
    return vote(res.index, res.confidence, slopes, int(margin), min_confidence)[0]


@torch.no_grad()
def super_resolve_scene(net, scene: torch.Tensor, patch: int = 32, stride: int = 16, max_batch: int = 64, ensemble=None, shear=None,
                        blend=None) -> torch.Tensor:
    """Equivalent of the body of the reference's test() for one scene (test.py:79-101), batched.
    ensemble: None, or a mode of lft_amd.ensemble.MASKS ("dihedral", "flips", "none") / an 8-bit mask -- geometric self-ensemble:
    every patch goes through the network in its E dihedral variants (chunks of max(1, max_batch // E) patches) and
    lft_scene_integrate_ens averages the back-transformed central regions straight into the scene; no merged patch is stored.
    shear: None (the plain cut: today's launches, today's bits), an int (one k for all patches; beyond ``shear_limit`` it is
    refused), an int32 tensor [numU*numV] on the scene's device (one k per patch, clamped to the limit), or "auto":
    ``estimate_shear`` on the unsheared patches.  The patches are cut with it and the SR patches put back against it (the module
    docstring has the definition).  shear together with ensemble is refused: the dihedral variants of a sheared patch are not
    sheared patches of the variant scene, and that pairing is not built.
    blend: None (the crop of ``integrate``: today's launches, today's bits), or a window of ``integrate``'s `blend=`: the SR patches
    are blended where they overlap, with or without `shear`.  With `ensemble` the variants of every patch are averaged by
    lft_amd.ensemble.merge and the merged patches blended: two launches in place of lft_scene_integrate_ens."""
    A, s = net.angRes, net.factor
    h0, w0 = scene.shape[0] // A, scene.shape[1] // A
    if blend is not None:
        check_blend(blend, A, patch, stride, s)
    if shear is not None:
        if ensemble is not None:
            raise LftError("shear together with ensemble is not supported: pass one of them")
        if isinstance(shear, bool) or not isinstance(shear, (int, str, torch.Tensor)) or (isinstance(shear, str) and shear != "auto"):
            raise LftError(f"shear must be None, an integer, an int32 tensor or auto, got {shear!r}")
        if isinstance(shear, int):
            check_shear_limit(shear, A, patch, stride)
            nu, nv = scene_counts(h0, w0, patch, stride)
            shear = torch.full((nu * nv,), shear, dtype=torch.int32, device=scene.device)
    patches = divide(scene, A, patch, stride, None if isinstance(shear, str) else shear)
    if ensemble is not None:
        from . import ensemble as ens
        mask = ens.mask_of(ensemble)
        per = max(1, max_batch // len(ens.codes_of(mask)))
        outs = [net(ens.expand(patches[i:i + per], mask)) for i in range(0, patches.shape[0], per)]
        if blend is not None:
            return integrate(ens.merge(torch.cat(outs, dim=0), mask), A, h0, w0, s, patch, stride, blend=blend)
        return integrate_ensemble(torch.cat(outs, dim=0), mask, A, h0, w0, s, patch, stride)
    if isinstance(shear, str):                      # auto: the sweep sees the unsheared patches, the network the re-cut ones
        shear = estimate_shear(patches, A, stride=stride)
        patches = divide(scene, A, patch, stride, shear)
    outs = [net(patches[i:i + max_batch]) for i in range(0, patches.shape[0], max_batch)]
    return integrate(torch.cat(outs, dim=0), A, h0, w0, s, patch, stride, shear, blend)


def parse_blend(text):
    """The --blend option of the tools: None or "none" (the crop), or a window's name."""
    if text is None or text == "none":
        return None
    if text not in WINDOWS:
        raise LftError(f"--blend takes none, {', '.join(WINDOWS)}, got {text!r}")
    return text


def parse_shear(text):
    """The --shear option of the tools: None, "auto" or a whole number."""
    if text is None or text == "auto":
        return text
    try:
        return int(text)
    except ValueError:
        raise LftError(f"--shear takes auto or a whole number, got {text!r}") from None
