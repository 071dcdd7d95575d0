"""Angular tiling: every view of a U×V light field through a network built for A×A views.

The network has a fixed angular resolution `A` (`net.angRes`); a 9×9 or 17×17 light field has more views than that.  Here A×A windows
slide over the U×V grid, every window of every spatial patch goes through the unchanged network in one batch, and one gather kernel
assembles all U×V super-resolved views, taking a weighted mean where windows overlap (lft_field_divide, lft_field_integrate;
csrc/lft_field.cuh, declared in include/lft_hip_field.h).  It composes with `shear=`, `blend=` and `ensemble=` of lft_amd.scene.

**Field mosaic.**
- A field mosaic is fp32 `[U·h0, V·w0]`.
- View `(p, q)` occupies rows `p·h0 …` and columns `q·w0 …`.
- This is the scene mosaic of lft_amd.scene with two angular sizes.

**Windows along one axis of `L` views, with `1 ≤ astride ≤ A ≤ L`.**
- `m(L) = 1` if `L = A`, else `ceil((L−A)/astride) + 1`.
- The origins are `o_i = min(i·astride, L−A)` (``origins``). They are strictly increasing.
- The last origin is clamped so the last view is covered.
- Consecutive origins are at most `A` apart, so every view is covered.
- `mu = m(U)` and `mv = m(V)` (``counts``). Window `w = wu·mv + wv` has origin `(o_wu, o_wv)`.
- `N = nu·nv` comes from lft_scene_counts. Batch element `b = w·N + n`.
- A view lies in at most `ceil(A/astride) + 1` windows per axis. The `+1` comes from the clamped last window: `A=2, astride=2, L=5`
  has origins 0, 2, 3, and view 3 is in two windows.

**Divide.** `[U·h0, V·w0] → [mu·mv·N, 1, A·patch, A·patch]`.
- Element `b` is exactly what lft_scene_divide gives for patch `n` of the A×A sub-mosaic of views `(o_wu+u, o_wv+v)`.
- With a `shear` (int32 `[mu·mv·N]`, one value per batch element, clamped to ±`kmax` of lft_hip_shear.h) it is exactly what
  lft_scene_divide_shear gives with `k = shear[b]`.
- No sub-mosaic is materialised.

**Integrate.** `[mu·mv·N, 1, A·pz, A·pz] → [U·h0·s, V·w0·s]`, with `pz = patch·s`.
- `g` is the angular table: fp32 `[A]`, strictly positive. `win` is the spatial table: either None, which means the crop, or fp32
  `[pz]` as in lft_amd.scene's blend.
- The terms of output view `(p, q)`, pixel `(Y, X)` are visited in ascending `wu`, then `wv`, then `ku`, then `kv`.
- A window `(wu, wv)` takes part when `0 ≤ u = p − o_wu < A` and `0 ≤ v = q − o_wv < A`. `ga = g[u]·g[v]`, one rounded product.
- With `win` None there is one term per window: the element lft_scene_integrate would read for that window's sub-scene, or
  lft_scene_integrate_shear when sheared. Its weight is `wt = ga`.
- With `win` set there is one term for every `(ku, kv)` that lft_scene_integrate_blend counts as contributing for that window's
  sub-scene: the same test and the same `sk_b = s·clamp(shear[b])`. Its weight is `wt = ga·(win[a]·win[b])`, each product rounded once.
- `num = num + wt·x`, `den = den + wt`, `out = num/den`. Every operation is one rounded fp32 operation, nothing is contracted and
  the quotient is correctly rounded, so a pixel's bits do not depend on the launch shape. Every pixel has at least one term.
- With `U = V = A` there is one window; with `g` flat that gives the bits of ``scene.integrate`` (crop, `shear=`, `blend=`). With
  `g` flat and the crop, the field equals the fp32 sum, in window order, of per-window ``scene.integrate`` results, divided by the
  fp32 count.

**Angular tables.** ``scene.window_table(kind, A)`` with `"flat"` (the default: a plain mean), `"linear"`, `"hann"`, or a float32
tensor `[A]`.

**Memory.** `mu·mv·N·(A·pz)²·4` bytes of SR patches are live at once. For 9×9 views of 512×512, A = 5, 2×, patch 32 / stride 16 that is
1.7 GB in the 4 windows of `astride` 4 and 3.8 GB in the 9 windows of `astride` 2.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib, scene
from ._lib import LftError


def _whole(x) -> bool:
    return not isinstance(x, bool) and isinstance(x, int)


def check_astride(astride, A: int) -> int:
    """`astride` as a whole number in 1 .. A; None means A (the fewest windows, abutting, the last one clamped)."""
    if not _whole(A) or A < 1:
        raise LftError(f"angRes must be a positive integer, got {A!r}")
    if astride is None:
        return A
    if not _whole(astride) or not 1 <= astride <= A:
        raise LftError(f"astride must be None or an integer in 1 .. angRes = {A}, got {astride!r}")
    return astride


def _views(U, V, A: int) -> None:
    if not _whole(U) or not _whole(V) or U < A or V < A or U > _lib.FIELD_MAX_VIEWS or V > _lib.FIELD_MAX_VIEWS:
        raise LftError(f"a field of {U!r} x {V!r} views: each axis must hold angRes = {A} .. {_lib.FIELD_MAX_VIEWS} views")


def origins(L: int, A: int, astride=None) -> list:
    """The origins o_i = min(i*astride, L - A) of the m(L) windows along an axis of L views."""
    astride = check_astride(astride, A)
    _views(L, L, A)
    m = 1 if L == A else -(-(L - A) // astride) + 1
    return [min(i * astride, L - A) for i in range(m)]


def counts(U: int, V: int, A: int, astride=None):
    """(mu, mv) of lft_field_counts: the windows along the two axes."""
    astride = check_astride(astride, A)
    _views(U, V, A)
    mu, mv = ctypes.c_int(0), ctypes.c_int(0)
    _lib.call("lft_field_counts", U, V, A, astride, ctypes.byref(mu), ctypes.byref(mv))
    return mu.value, mv.value


def check_angular(angular, A: int) -> None:
    """What the angular table refuses without a device: neither a window's name nor a float32 tensor [A]."""
    if isinstance(angular, str) and angular in scene.WINDOWS:
        return
    if not isinstance(angular, torch.Tensor) or angular.dtype != torch.float32 or tuple(angular.shape) != (A,):
        raise LftError(f"angular must be one of {', '.join(scene.WINDOWS)}, or a float32 tensor of shape [{A}] (positive weights over a window's views), got "
                       f"{angular if isinstance(angular, str) else getattr(angular, 'dtype', type(angular).__name__)!r} {tuple(getattr(angular, 'shape', ()))}")


def angular_table(angular, A: int, device=None) -> torch.Tensor:
    """The angular table on `device`, float32 [A]: ``scene.window_table(kind, A)`` through ``scene.blend_window`` (made once per device
    and kept), or the caller's tensor, contiguous."""
    check_angular(angular, A)
    if isinstance(angular, str):
        return scene.blend_window(angular, A, device)
    if device is not None and angular.device != torch.device(device):
        raise LftError(f"angular is on {angular.device}, the patches on {torch.device(device)}")
    return angular.contiguous()


def _geometry(field_shape, U, V, A, astride, patch, stride):
    """(astride, h0, w0, mu, mv, nu, nv) of a field mosaic of `field_shape`; every refusal that needs no device."""
    astride = check_astride(astride, A)
    _views(U, V, A)
    if len(field_shape) != 2 or field_shape[0] % U or field_shape[1] % V or 0 in field_shape:
        raise LftError(f"field must be a mosaic [U*h0, V*w0] of {U} x {V} views, got shape {tuple(field_shape)}")
    h0, w0 = field_shape[0] // U, field_shape[1] // V
    nu, nv = scene.scene_counts(h0, w0, patch, stride)
    mu, mv = counts(U, V, A, astride)
    return astride, h0, w0, mu, mv, nu, nv


def divide(field: torch.Tensor, U: int, V: int, A: int, patch: int = 32, stride: int = 16, astride=None, shear=None) -> torch.Tensor:
    """field: float32 [U*h0, V*w0] on a HIP device -> [mu*mv*numU*numV, 1, A*patch, A*patch], window-major (the module docstring has
    the definition).  shear: None, or int32 [mu*mv*numU*numV] on the field's device, one value per batch element."""
    if not isinstance(field, torch.Tensor) or field.dim() != 2:
        raise LftError(f"field must be a 2-D float32 tensor [U*h0, V*w0], got {tuple(getattr(field, 'shape', ()))}")
    astride, h0, w0, mu, mv, nu, nv = _geometry(tuple(field.shape), U, V, A, astride, patch, stride)
    B = mu * mv * nu * nv
    if shear is not None:
        scene.shear_limit(A, patch, stride)
        shear = scene._shear_tensor(shear, B, field)
    if not field.is_cuda:
        raise LftError("field must be a 2-D float32 tensor on a HIP device")
    x = field.contiguous().float()
    out = torch.empty((B, 1, A * patch, A * patch), dtype=torch.float32, device=x.device)
    _lib.enqueue("lft_field_divide", x.device, x.data_ptr(), None if shear is None else shear.data_ptr(), out.data_ptr(), U, V, A, astride, h0, w0, patch, stride)
    return out


def integrate(sr_patches: torch.Tensor, U: int, V: int, A: int, h0: int, w0: int, scale: int, patch: int = 32, stride: int = 16, astride=None,
              shear=None, blend=None, angular="flat") -> torch.Tensor:
    """sr_patches: float32 [mu*mv*numU*numV, 1, A*patch*s, A*patch*s] -> the SR field mosaic [U*h0*s, V*w0*s]: the weighted mean of
    the windows a view lies in (the module docstring has the definition).  shear: None, or the int32 the patches were cut with;
    blend: None (the crop) or a window of ``scene.integrate``; angular: "flat" (a plain mean), "linear", "hann" or a float32 tensor [A]."""
    if not _whole(h0) or not _whole(w0) or h0 < 1 or w0 < 1:
        raise LftError(f"views of {h0!r} x {w0!r}")
    astride, h0, w0, mu, mv, nu, nv = _geometry((U * h0, V * w0), U, V, A, astride, patch, stride)
    check_angular(angular, A)
    if scale not in (2, 4):
        raise LftError(f"field: scale factor must be 2 or 4, got {scale}")
    if blend is not None:
        scene.check_blend(blend, A, patch, stride, scale)
    B, side = mu * mv * nu * nv, A * patch * scale
    if not isinstance(sr_patches, torch.Tensor) or tuple(sr_patches.shape) != (B, 1, side, side):
        raise LftError(f"sr_patches must be [{B}, 1, {side}, {side}] for this tiling, got {tuple(getattr(sr_patches, 'shape', ()))}")
    if shear is not None:
        scene.shear_limit(A, patch, stride)
        shear = scene._shear_tensor(shear, B, sr_patches)
    for name, t in (("blend", blend), ("angular", angular)):
        if isinstance(t, torch.Tensor) and t.device != sr_patches.device:
            raise LftError(f"{name} is on {t.device}, the patches on {sr_patches.device}")
    if not sr_patches.is_cuda:
        raise LftError("sr_patches must be a float32 tensor on a HIP device")
    x = sr_patches.contiguous().float()
    g = angular_table(angular, A, x.device)
    w = None if blend is None else scene.blend_window(blend, patch * scale, x.device) if isinstance(blend, str) else blend.contiguous()
    out = torch.empty((U * h0 * scale, V * w0 * scale), dtype=torch.float32, device=x.device)
    _lib.enqueue("lft_field_integrate", x.device, x.data_ptr(), None if shear is None else shear.data_ptr(), None if w is None else w.data_ptr(), g.data_ptr(),
                 out.data_ptr(), U, V, A, astride, h0, w0, patch, stride, scale)
    return out


@torch.no_grad()
def super_resolve_field(net, field: torch.Tensor, U: int, V: int, patch: int = 32, stride: int = 16, max_batch: int = 64, astride=None, angular="flat",
                        ensemble=None, shear=None, blend=None) -> torch.Tensor:
    """All U x V super-resolved views of the LR field mosaic [U*h0, V*w0], as the SR field mosaic [U*h0*s, V*w0*s]: ``divide``, the
    network over the whole batch in chunks of `max_batch`, ``integrate``.
    astride: None means A = net.angRes: the fewest windows, abutting, the last one clamped.
    shear: None, an int (one k for all; beyond ``scene.shear_limit`` it is refused), an int32 tensor [mu*mv*numU*numV] on the field's
    device, or "auto": ``scene.estimate_shear`` on the whole unsheared batch.  shear together with ensemble is refused.
    ensemble: as in ``scene.super_resolve_scene``; the variants of every patch are averaged by lft_amd.ensemble.merge and the merged
    patches integrated.  blend, angular: as in ``integrate``."""
    A, s = net.angRes, net.factor
    if not isinstance(field, torch.Tensor) or field.dim() != 2:
        raise LftError(f"field must be a 2-D float32 tensor [U*h0, V*w0], got {tuple(getattr(field, 'shape', ()))}")
    astride, h0, w0, mu, mv, nu, nv = _geometry(tuple(field.shape), U, V, A, astride, patch, stride)
    check_angular(angular, A)
    if s not in (2, 4):
        raise LftError(f"field: scale factor must be 2 or 4, got {s}")
    if blend is not None:
        scene.check_blend(blend, A, patch, stride, s)
    for name, t in (("blend", blend), ("angular", angular)):
        if isinstance(t, torch.Tensor) and t.device != field.device:
            raise LftError(f"{name} is on {t.device}, the field on {field.device}")
    B = mu * mv * nu * nv
    if shear is not None:
        if ensemble is not None:
            raise LftError("shear together with ensemble is not supported: pass one of them")
        if isinstance(shear, bool) or not isinstance(shear, (int, str, torch.Tensor)) or (isinstance(shear, str) and shear != "auto"):
            raise LftError(f"shear must be None, an integer, an int32 tensor or auto, got {shear!r}")
        if isinstance(shear, int):
            scene.check_shear_limit(shear, A, patch, stride)
            shear = torch.full((B,), shear, dtype=torch.int32, device=field.device)
    patches = divide(field, U, V, A, patch, stride, astride, None if isinstance(shear, str) else shear)
    if ensemble is not None:
        from . import ensemble as ens
        mask = ens.mask_of(ensemble)
        per = max(1, max_batch // len(ens.codes_of(mask)))
        outs = [net(ens.expand(patches[i:i + per], mask)) for i in range(0, B, per)]
        return integrate(ens.merge(torch.cat(outs, dim=0), mask), U, V, A, h0, w0, s, patch, stride, astride, None, blend, angular)
    if isinstance(shear, str):                      # auto: the sweep sees the unsheared patches, the network the re-cut ones
        shear = scene.estimate_shear(patches, A, stride=stride)
        patches = divide(field, U, V, A, patch, stride, astride, shear)
    outs = [net(patches[i:i + max_batch]) for i in range(0, B, max_batch)]
    return integrate(torch.cat(outs, dim=0), U, V, A, h0, w0, s, patch, stride, astride, shear, blend, angular)


def parse_angular(text):
    """The --angular_window option of the tools: a window's name."""
    if text not in scene.WINDOWS:
        raise LftError(f"--angular_window takes {', '.join(scene.WINDOWS)}, got {text!r}")
    return text
