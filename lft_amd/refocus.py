"""Synthetic refocus and EPI slices: what a light field is looked at with.

  R_d[y, x, c] = sum_{u,v} a[u,v] * S(L[u,v,:,:,c], y + d*(u-uc), x + d*(v-uc)),   uc = (A-1)/2,

d the slope in pixels per view step, a the aperture (>= 0, sum 1).  A Lambertian plane L[u,v,y,x] = f(y - d0*(u-uc), x - d0*(v-uc))
comes back as f at d = +d0.  S is separable, rows first: ``nearest`` takes the tap floor(off + 0.5), ``linear`` the taps floor(off)
and floor(off) + 1 with weights 1-f and f, ``cubic`` the taps floor(off)-1 .. floor(off)+2 with Keys' kernel (a = -0.5,
``prepare._cubic``) at f+1, f, 1-f, 2-f; tap indices are clamped into the view (replicate), the weights are not renormalised.

``shift_table`` is the only place coefficients are computed: in fp64, rounded once to fp32.  ``refocus`` hands the table and the
light field, as it lies in memory, to one launch of k_refocus (csrc/lft_refocus.cuh); there is no CPU path.  ``epi`` is indexing.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, prepare
from ._lib import LftError

TAPS = {"nearest": 1, "linear": 2, "cubic": 4}
# lft_refocus_record of include/lft_hip.h: tap k of the row filter reads row clamp(y + oy + k), of the column filter column
# clamp(x + ox + k); weights beyond the tap count are 0; skip marks a view of aperture weight 0, which is never read
RECORD = np.dtype([("oy", np.int32), ("ox", np.int32), ("wy", np.float32, 4), ("wx", np.float32, 4), ("a", np.float32),
                   ("skip", np.int32)])
MAX_OFFSET = 1 << 30
_CLASS = {torch.uint8: _lib.LF_UINT8, torch.float32: _lib.LF_FLOAT32}
Aperture = Union[str, np.ndarray, Sequence[Sequence[float]]]


def aperture_weights(A: int, kind: str = "full", radius: Optional[float] = None, sigma: Optional[float] = None) -> np.ndarray:
    """fp64 [A, A], >= 0, sum 1.  ``full``: every view; ``disk``: the views with (u-uc)^2 + (v-uc)^2 <= radius^2 + 1e-9 (default
    radius uc); ``gaussian``: exp(-r^2 / (2 sigma^2)), sigma in view steps (default max(uc, 1) / 2)."""
    if A < 1:
        raise LftError(f"angRes must be positive, got {A}")
    uc = (A - 1) / 2
    r2 = (np.arange(A, dtype=np.float64)[:, None] - uc) ** 2 + (np.arange(A, dtype=np.float64)[None, :] - uc) ** 2
    if kind == "full":
        a = np.ones((A, A), dtype=np.float64)
    elif kind == "disk":
        r = uc if radius is None else float(radius)
        if r < 0:
            raise LftError(f"disk aperture: radius {r} is negative")
        a = (r2 <= r * r + 1e-9).astype(np.float64)
        if not a.any():                # an even A has no view at the centre: the default radius of A = 2 (0.5) reaches none
            raise LftError(f"disk aperture: radius {r} keeps none of the {A} x {A} views")
    elif kind == "gaussian":
        s = max(uc, 1.0) / 2 if sigma is None else float(sigma)
        if not s > 0:
            raise LftError(f"gaussian aperture: sigma must be positive, got {s}")
        a = np.exp(-r2 / (2 * s * s))
    else:
        raise LftError(f"aperture kind must be full, disk or gaussian, got {kind!r}")
    return a / a.sum()


def _aperture(A: int, aperture: Aperture) -> np.ndarray:
    if isinstance(aperture, str):
        return aperture_weights(A, aperture)
    a = np.array(aperture.detach().cpu().numpy() if isinstance(aperture, torch.Tensor) else aperture, dtype=np.float64)
    if a.shape != (A, A):
        raise LftError(f"the aperture must be [{A}, {A}], got shape {a.shape}")
    if not np.all(np.isfinite(a)) or np.any(a < 0) or not a.sum() > 0:
        raise LftError("the aperture's weights must be finite, >= 0 and not all zero")
    return a / a.sum()


def _axis(off: float, interp: str) -> Tuple[int, np.ndarray]:
    """(base offset, 4 fp64 weights) of one axis at the sample offset `off`."""
    w = np.zeros(4, dtype=np.float64)
    if interp == "nearest":
        base = int(np.floor(off + 0.5))
        w[0] = 1.0
    elif interp == "linear":
        base = int(np.floor(off))
        f = off - np.floor(off)
        w[:2] = 1.0 - f, f
    else:
        base = int(np.floor(off)) - 1
        f = off - np.floor(off)
        w[:] = prepare._cubic(np.array([f + 1.0, f, 1.0 - f, 2.0 - f]))
    return base, w


def _centre(A: int, centre) -> Tuple[float, float]:
    """(cu, cv) of a `centre` argument: None is (uc, uc); else two finite numbers in view-index units."""
    uc = (A - 1) / 2
    if centre is None:
        return uc, uc
    c = np.array(centre, dtype=np.float64).reshape(-1)
    if c.size != 2 or not np.all(np.isfinite(c)):
        raise LftError(f"centre must be two finite view coordinates (cu, cv), got {centre!r}")
    return float(c[0]), float(c[1])


def shift_table(A: int, slopes: Sequence[float], aperture: Aperture = "full", interp: str = "cubic", centre=None) -> np.ndarray:
    """The host table [D, A*A] of RECORD, slope-major, views in (u, v) order.  centre (default (uc, uc)): the angular position
    (cu, cv) the stack is seen from; the offsets are d*(u-cu), d*(v-cv)."""
    if interp not in TAPS:
        raise LftError(f"interp must be nearest, linear or cubic, got {interp!r}")
    if A < 1:
        raise LftError(f"angRes must be positive, got {A}")
    sl = np.array(slopes, dtype=np.float64).reshape(-1)
    if sl.size < 1 or not np.all(np.isfinite(sl)):
        raise LftError(f"slopes must be a non-empty sequence of finite numbers, got {slopes!r}")
    a = _aperture(A, aperture)
    cu, cv = _centre(A, centre)
    if np.abs(sl).max() * max(abs(i - c) for c in (cu, cv) for i in (0, A - 1)) > MAX_OFFSET:
        raise LftError(f"slope {np.abs(sl).max()} shifts the outer views by more than 2^30 pixels")
    tab = np.zeros((sl.size, A * A), dtype=RECORD)
    for k, d in enumerate(sl):
        rows, cols = [_axis(d * (i - cu), interp) for i in range(A)], [_axis(d * (i - cv), interp) for i in range(A)]
        for u in range(A):
            for v in range(A):
                r = tab[k, u * A + v]
                r["oy"], r["ox"] = rows[u][0], cols[v][0]
                r["wy"], r["wx"] = rows[u][1], cols[v][1]                # rounded once, here
                r["a"] = a[u, v]
                r["skip"] = int(r["a"] == 0)
    return tab


def parse_slopes(text: str):
    """The slopes of a command line: LO:HI:N (N slopes from LO to HI) or a comma list."""
    if ":" in text:
        lo, hi, n = text.split(":")
        return [float(x) for x in np.linspace(float(lo), float(hi), int(n))]
    return [float(x) for x in text.split(",")]


_tables: Dict[tuple, torch.Tensor] = {}


def _device_table(A: int, slopes, aperture: Aperture, interp: str, device, centre=None) -> torch.Tensor:
    sl = tuple(float(s) for s in np.array(slopes, dtype=np.float64).reshape(-1))
    ap = aperture if isinstance(aperture, str) else _aperture(A, aperture).tobytes()
    key = (A, sl, ap, interp, str(device), None if centre is None else _centre(A, centre))
    if key not in _tables:
        tab = shift_table(A, sl, aperture, interp, centre)
        _tables[key] = torch.from_numpy(tab.view(np.int32).reshape(tab.shape[0], A * A, RECORD.itemsize // 4).copy()).to(device)
    return _tables[key]


def _layout(lf: torch.Tensor, angRes: Optional[int]):
    """(B, A, H, W, C, element strides of (b, u, v, y, x, c), shape of the result after [B, D, H, W, C]) of an input."""
    sh, st = tuple(int(d) for d in lf.shape), tuple(int(s) for s in lf.stride())
    if lf.dim() == 5 or (lf.dim() == 4 and (angRes is None or (sh[0] == sh[1] == angRes and sh[1] != 1))):
        A = sh[0]
        if sh[1] != A or (angRes is not None and angRes != A):
            raise LftError(f"views must be [A, A, H, W(, C)]{'' if angRes is None else f' with A = {angRes}'}, got shape {sh}")
        C = sh[4] if lf.dim() == 5 else 1
        return 1, A, sh[2], sh[3], C, (0, st[0], st[1], st[2], st[3], st[4] if lf.dim() == 5 else 0), "views5" if lf.dim() == 5 else "views4"
    if lf.dim() not in (2, 4):
        raise LftError(f"the light field must be views [A, A, H, W(, C)], a mosaic [A*H, A*W] or a batch [B, 1, A*H, A*W], got shape {sh}")
    if angRes is None or angRes < 1:
        raise LftError("a mosaic needs angRes")
    A = int(angRes)
    if lf.dim() == 4 and sh[1] != 1:
        raise LftError(f"a batch of mosaics must be [B, 1, A*H, A*W], got shape {sh}")
    mh, mw, sy, sx = sh[-2], sh[-1], st[-2], st[-1]
    if mh % A or mw % A:
        raise LftError(f"a mosaic of {mh} x {mw} does not hold {A} x {A} views")
    H, W = mh // A, mw // A
    return (sh[0] if lf.dim() == 4 else 1), A, H, W, 1, (st[0] if lf.dim() == 4 else 0, H * sy, W * sx, sy, sx, 0), \
        "batch" if lf.dim() == 4 else "mosaic"


def _field(lf, angRes: Optional[int], out_name: str, out_dtype, before_device=None):
    """What refocus and disparity ask of their input: (B, A, H, W, C, the six strides as a C array, kind of _layout).  out_dtype
    (None: the input's), named out_name, is the class of the image they return.  A tensor off the GPU is refused first, or, with
    before_device (disparity's further refusals), after the classes and those."""
    if not isinstance(lf, torch.Tensor):
        raise LftError(f"the light field must be a torch tensor, got {type(lf).__name__}")
    off_gpu = LftError(f"the light field must be on the GPU, got a tensor on {lf.device} (there is no CPU path)")
    if before_device is None and lf.device.type != "cuda":
        raise off_gpu
    if lf.dtype not in _CLASS:
        raise LftError(f"light field of class {lf.dtype}: uint8 and float32 are supported")
    if out_dtype is not None and out_dtype not in _CLASS:
        raise LftError(f"{out_name} must be torch.uint8 or torch.float32, got {out_dtype}")
    if before_device is not None:
        before_device()
        if lf.device.type != "cuda":
            raise off_gpu
    B, A, H, W, C, strides, kind = _layout(lf, angRes)
    if C < 1 or C > 4:
        raise LftError(f"{C} channels: 1 to 4 are supported")
    return B, A, H, W, C, _lib.strides_array(strides), kind


def _as_given(kind: str, t, image: bool = False):
    """A result [B, ...] (image: [B, ..., C]) in the layout of the caller's input, by the kind of _layout: the batch axis stays for
    a kind that starts with "batch", the channel axis for one that ends in "5" (views5; ``disparity.regularize`` also has batch5).
    None stays None."""
    if t is None:
        return None
    if image and not kind.endswith("5"):
        t = t[..., 0]
    return t if kind.startswith("batch") else t[0]


def _device_scratch(cache: Dict[tuple, torch.Tensor], query: str, args: tuple, device) -> torch.Tensor:
    """The scratch of an entry point, as many bytes as its size query `query` answers for `args`: one buffer in `cache` per query,
    arguments and device, so calls of one shape on different streams must not overlap."""
    key = (query, *args, str(device))
    if key not in cache:
        cache[key] = torch.empty(max(_lib.query(query, *args) // 4, 1), dtype=torch.int32, device=device)
    return cache[key]


def refocus(lf: torch.Tensor, slopes: Sequence[float], angRes: Optional[int] = None, aperture: Aperture = "full",
            interp: str = "cubic", out_dtype=None, centre=None) -> torch.Tensor:
    """The focal stack of a light field on the GPU, one slice per slope, on lf's device and current stream (enqueue only).

      views  [A, A, H, W, C] (C <= 4) or [A, A, H, W]   ->  [D, H, W, C] or [D, H, W]
      mosaic [A*H, A*W] with angRes                       ->  [D, H, W]
      batch  [B, 1, A*H, A*W] with angRes                 ->  [B, D, H, W]       (the network's input and output)

    Any strides are read in place.  uint8 input enters as x / 255, float32 as stored.  out_dtype (default: the input's) is
    torch.float32, the unclipped sum, or torch.uint8: clip to [0, 1], * 255, round half to even.  aperture: "full", "disk",
    "gaussian" or an [A, A] array (``aperture_weights`` for a radius or sigma); views of weight 0 are not read.  centre: the
    angular position (cu, cv) the stack is seen from (``shift_table``), default the centre of the views."""
    B, A, H, W, C, strides, kind = _field(lf, angRes, "out_dtype", out_dtype)
    out_dtype = lf.dtype if out_dtype is None else out_dtype
    table = _device_table(A, slopes, aperture, interp, lf.device, centre)
    D = int(table.shape[0])
    out = torch.empty(B, D, H, W, C, dtype=out_dtype, device=lf.device)
    _lib.enqueue("lft_refocus", lf.device, lf.data_ptr() or None, _CLASS[lf.dtype], B, A, H, W, C, strides, table.data_ptr(), D, TAPS[interp],
                 out.data_ptr() or None, _CLASS[out_dtype])
    return _as_given(kind, out, image=True)


def refocus_adjoint(stack_grad: torch.Tensor, slopes: Sequence[float], angRes: int, aperture: Aperture = "full", interp: str = "cubic",
                    centre=None, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """The adjoint of ``refocus`` on a batch of mosaics (lft_refocus_adjoint, include/lft_hip_focal.h): a contiguous float32 stack
    gradient [B, D, H, W] on the GPU -> the mosaic [B, 1, A*H, A*W] whose view (u, v) collects, through the clamped taps, what every
    stack pixel took from it: <refocus(x), g> = <x, refocus_adjoint(g)>.  out / accumulate: a mosaic to write, or to add to.  Only
    enqueues, on stack_grad's device and current stream; no autograd hook on ``refocus`` itself."""
    if not isinstance(stack_grad, torch.Tensor) or stack_grad.dtype != torch.float32 or stack_grad.dim() != 4 or not stack_grad.is_contiguous():
        raise LftError("the stack gradient must be a contiguous float32 tensor [B, D, H, W]")
    if interp not in TAPS:
        raise LftError(f"interp must be nearest, linear or cubic, got {interp!r}")
    A = int(angRes)
    if A < 1:
        raise LftError(f"angRes must be positive, got {angRes}")
    B, D, H, W = (int(d) for d in stack_grad.shape)
    nslopes = np.array(slopes, dtype=np.float64).reshape(-1).size
    if nslopes != D:
        raise LftError(f"{nslopes} slopes for a stack of {D} slices")
    if accumulate and out is None:
        raise LftError("accumulate adds to `out`: pass the mosaic that holds the other terms")
    if out is not None and (out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (B, 1, A * H, A * W) or out.device != stack_grad.device):
        raise LftError(f"out must be a contiguous float32 tensor [{B}, 1, {A * H}, {A * W}] on the device of the stack gradient")
    if stack_grad.device.type != "cuda":
        raise LftError(f"the stack gradient must be on the GPU, got a tensor on {stack_grad.device} (there is no CPU path)")
    table = _device_table(A, slopes, aperture, interp, stack_grad.device, centre)
    out = torch.empty(B, 1, A * H, A * W, dtype=torch.float32, device=stack_grad.device) if out is None else out
    _lib.enqueue("lft_refocus_adjoint", stack_grad.device, stack_grad.data_ptr() or None, B, A, H, W, table.data_ptr(), D, TAPS[interp],
                 out.data_ptr() or None, int(bool(accumulate)))
    return out


def _views(lf, angRes: Optional[int]):
    """lf as views [A, A, H, W(, C)] by indexing only (a torch tensor or a numpy array, on any device)."""
    if lf.ndim in (4, 5):
        if lf.shape[0] != lf.shape[1] or (angRes is not None and angRes != lf.shape[0]):
            raise LftError(f"views must be [A, A, H, W(, C)], got shape {tuple(lf.shape)}")
        return lf
    if lf.ndim != 2 or angRes is None or angRes < 1 or lf.shape[0] % angRes or lf.shape[1] % angRes:
        raise LftError(f"epi takes views [A, A, H, W(, C)] or a mosaic [A*H, A*W] with angRes, got shape {tuple(lf.shape)}")
    A = int(angRes)
    m = lf.reshape(A, lf.shape[0] // A, A, lf.shape[1] // A)
    return m.permute(0, 2, 1, 3) if isinstance(m, torch.Tensor) else m.transpose(0, 2, 1, 3)


def epi(lf, angRes: Optional[int] = None, row: Optional[int] = None, col: Optional[int] = None, u: Optional[int] = None,
        v: Optional[int] = None):
    """An epipolar-plane image by indexing (no kernel; tensors on any device and numpy arrays).  The horizontal EPI [A, W(, C)]
    fixes the view row u and the image row `row` and runs over v and x; the vertical EPI [A, H(, C)] fixes v and `col` and runs
    over u and y, and is what `col` or `v` ask for.  Defaults: the centre view row / column A // 2 and the middle image row /
    column."""
    L = _views(lf, angRes)
    A, H, W = (int(d) for d in (L.shape[0], L.shape[2], L.shape[3]))
    vertical = col is not None or v is not None
    if vertical and (row is not None or u is not None):
        raise LftError("epi: give row / u for the horizontal EPI or col / v for the vertical one, not both")
    if vertical:
        v, col = A // 2 if v is None else v, W // 2 if col is None else col
        if not (0 <= v < A and 0 <= col < W):
            raise LftError(f"epi: v = {v}, col = {col} outside {A} views of width {W}")
        return L[:, v, :, col]
    u, row = A // 2 if u is None else u, H // 2 if row is None else row
    if not (0 <= u < A and 0 <= row < H):
        raise LftError(f"epi: u = {u}, row = {row} outside {A} views of height {H}")
    return L[u, :, row]
