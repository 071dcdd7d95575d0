"""Data preparation of the reference on the GPU: what Generate_Data_for_Training.m and Generate_Data_for_Test.m make of the raw
light fields ``<src_data_path>/<dataset>/{training,test}/<scene>.mat``, without MATLAB.

Per sub-aperture view, in fp64 as MATLAB's ``double``: Y = rgb2ycbcr(rgb)(:,:,1) of the stored values (uint8 enters as 0..255),
``single(Y)`` for Hr_SAI_y and ``single(imresize(Y, 1/s))`` for Lr_SAI_y -- MATLAB's antialiased bicubic: cubic kernel a = -0.5
stretched to 4*s taps, weights normalised per output, symmetric border, rows first.  One HIP kernel (lft_lf_prepare,
csrc/lft_prepare.cuh) does it for every crop of every centre view; this module builds its contribution tables, loads ``.mat`` files
(v7.3 through lft_amd.h5lite, v5 / v7 through scipy), and offers

  * ``test_pair`` / ``training_pairs``: one scene as the test script / the training script cuts it (MATLAB matrix orientation);
  * ``RawLFPatchSource``: a patch source of lft_amd.trainer.fit that makes every training sample on the device, in the order and
    orientation in which lft_amd.datasets.H5PatchSource reads the tree the training script writes;
  * ``raw_test_scenes``: the (lr, hr) scenes of one test dataset, as lft_amd.evaluate.test takes them.

tools/prepare_data.py writes the scripts' .h5 trees with it (lft_amd.h5write).
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Dict, Iterator, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib, h5lite
from ._lib import LftError

PATCH_LR, STRIDE_LR = 32, 16                     # Generate_Data_for_Training.m:7-8: patchsize = 32*s, stride = patchsize/2
TEST_MULTIPLE = 4                                # Generate_Data_for_Test.m:33-38: H, W cut to multiples of 4 whatever the factor
_CLASS = {torch.uint8: _lib.LF_UINT8, torch.float32: _lib.LF_FLOAT32, torch.float64: _lib.LF_FLOAT64}


# ---------------------------------------------------------------------------------------------- imresize tables
def _cubic(x: np.ndarray) -> np.ndarray:
    """Keys' cubic, a = -0.5 (MATLAB imresize's 'bicubic')."""
    absx = np.absolute(x)
    absx2 = absx * absx
    absx3 = absx2 * absx
    return (np.multiply(1.5 * absx3 - 2.5 * absx2 + 1, absx <= 1)
            + np.multiply(-0.5 * absx3 + 2.5 * absx2 - 4 * absx + 2, (1 < absx) & (absx <= 2)))


def out_length(in_len: int, s: int) -> int:
    return int(math.ceil(in_len * (1.0 / s)))


def imresize_table(in_len: int, s: int, up: bool) -> Tuple[np.ndarray, np.ndarray]:
    """imresize's contribution table of one axis (MATLAB's, and the reference's utils/imresize.py:32-52), down by s or up by s:
    (weights fp64 [out, P], indices int32 [out, P]), 0-based input indices.  Down (scale = 1/s, out = ceil(in_len / s)) the kernel
    is the antialiased scale * cubic(scale * x) of width 4 / scale; up (scale = s, out = in_len * s) the plain cubic of width 4.
    P = ceil(width) + 2 taps per output, weights normalised per output, indices mirrored into [0, in_len) symmetrically (period
    2 * in_len), tap columns that are zero for every output dropped."""
    if in_len < 1 or s < 1:
        raise ValueError(f"{'up_contributions' if up else 'contributions'}: length {in_len}, scale factor {s}")
    scale = float(s) if up else 1.0 / s
    width = 4.0 if up else 4.0 / scale
    x = np.arange(1, (in_len * s if up else out_length(in_len, s)) + 1, dtype=np.float64)
    u = x / scale + 0.5 * (1 - 1 / scale)                        # the output sample's centre in 1-based input coordinates
    left = np.floor(u - width / 2)
    P = int(math.ceil(width)) + 2
    ind = (left[:, None] + np.arange(P) - 1).astype(np.int32)   # 0-based
    w = _cubic(u[:, None] - ind - 1) if up else scale * _cubic(scale * (u[:, None] - ind - 1))
    w = np.divide(w, np.sum(w, axis=1)[:, None])
    mirror = np.concatenate((np.arange(in_len), np.arange(in_len - 1, -1, -1))).astype(np.int32)
    ind = mirror[np.mod(ind, mirror.size)]
    keep = np.nonzero(np.any(w, axis=0))[0]
    return np.ascontiguousarray(w[:, keep]), np.ascontiguousarray(ind[:, keep])


def contributions(in_len: int, s: int) -> Tuple[np.ndarray, np.ndarray]:
    """The table of MATLAB's imresize(., 1/s): 4*s + 2 taps per output before the all-zero columns are dropped."""
    return imresize_table(in_len, s, up=False)


_tables: Dict[Tuple[int, int, bool, str], Tuple[torch.Tensor, torch.Tensor]] = {}


def _device_table(in_len: int, s: int, device, up: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    key = (in_len, s, bool(up), str(device))                     # one cache for both directions
    if key not in _tables:
        w, i = imresize_table(in_len, s, up)
        _tables[key] = (torch.from_numpy(w).to(device), torch.from_numpy(i).to(device))
    return _tables[key]


def lf_args(lf: torch.Tensor) -> tuple:
    """The leading arguments (lf, lf_class, U, V, H, W, C, strides) of the entry points that read a light field [U, V, H, W, C] in
    place.  An empty tensor goes as a null pointer and an unknown class as -1: the library does the refusing."""
    return (lf.data_ptr() if lf.numel() else None, _CLASS.get(lf.dtype, -1), *(int(d) for d in lf.shape), _lib.strides_array(lf))


# ---------------------------------------------------------------------------------------------- the kernel
def lf_prepare(lf: torch.Tensor, A: int, s: int, crops: Sequence[Tuple[int, int]], crop_h: int,
               crop_w: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """lft_lf_prepare on lf's device and current stream: lf [U, V, H, W, C] (uint8 / float32 / float64, any strides) ->
    (hr [N, A*crop_h, A*crop_w], lr [N, A*ceil(crop_h/s), A*ceil(crop_w/s)]) fp32, MATLAB matrix orientation, for the centre
    A x A views and the N crop origins (y0, x0).  Enqueue only."""
    if lf.dim() != 5:
        raise LftError(f"lft_lf_prepare: the light field must be [U, V, H, W, C], got shape {tuple(lf.shape)}")
    if lf.device.type != "cuda":
        raise LftError(f"lft_lf_prepare: the light field must be on the GPU, got a tensor on {lf.device}")
    dev = lf.device
    cr = np.ascontiguousarray(np.asarray(crops, dtype=np.int32).reshape(-1, 2))
    n = cr.shape[0]
    if n == 0:
        raise LftError("lft_lf_prepare: no crops")
    if s in (2, 4) and 1 <= crop_h and 1 <= crop_w:
        wh, ih = _device_table(crop_h, s, dev)
        ww, iw = _device_table(crop_w, s, dev)
        oh, ow = wh.shape[0], ww.shape[0]
    else:                                                       # the library refuses these; give it well-formed pointers
        wh = ww = torch.zeros(1, 1, dtype=torch.float64, device=dev)
        ih = iw = torch.zeros(1, 1, dtype=torch.int32, device=dev)
        oh = ow = 1
    hr = torch.empty(n, A * crop_h, A * crop_w, dtype=torch.float32, device=dev) if A >= 1 else torch.empty(0, device=dev)
    lr = torch.empty(n, A * oh, A * ow, dtype=torch.float32, device=dev) if A >= 1 else torch.empty(0, device=dev)
    cptr = cr.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    _lib.enqueue("lft_lf_prepare", dev, *lf_args(lf), A, s, cptr, n, crop_h, crop_w, wh.data_ptr(), ih.data_ptr(), wh.shape[1],
                 ww.data_ptr(), iw.data_ptr(), ww.shape[1], hr.data_ptr() or None, lr.data_ptr() or None)
    return hr, lr


# ---------------------------------------------------------------------------------------------- raw light fields
def load_lf(path: str) -> np.ndarray:
    """The ``LF`` array of a light-field .mat file as [U, V, H, W, C] in its stored class (no scaling).  v7.3 files are HDF5
    behind a 512-byte user block, holding LF column-major as [C, W, H, V, U]: the result is a transposed VIEW of that array.
    v5 / v7 files are read with scipy.io.loadmat."""
    with open(path, "rb") as f:
        head = f.read(520)
    if h5lite.SIGNATURE in (head[:8], head[512:520]):
        with h5lite.File(path) as hf:
            ds = hf.get("LF")
            if ds is None:
                raise LftError(f"{path}: no LF dataset (has {hf.keys()})")
            lf = np.array(ds)
        if lf.ndim != 5:
            raise LftError(f"{path}: LF has shape {lf.shape}, expected [C, W, H, V, U]")
        return lf.transpose(4, 3, 2, 1, 0)
    try:
        import scipy.io
    except ImportError as e:
        raise LftError(f"{path} is a MATLAB v5/v7 file: reading it needs scipy (scipy.io.loadmat), which is not installed; "
                       "save it with -v7.3 or install scipy") from e
    m = scipy.io.loadmat(path)
    if "LF" not in m:
        raise LftError(f"{path}: no variable LF (has {[k for k in m if not k.startswith('__')]})")
    lf = m["LF"]
    if lf.ndim != 5:
        raise LftError(f"{path}: LF has shape {lf.shape}, expected [U, V, H, W, C]")
    return lf


def centre_views(lf: np.ndarray, A: int) -> Tuple[int, int]:
    """0-based first centre view (Generate_Data_for_*.m: LF(0.5*(U-A+2) : 0.5*(U+A), ...))."""
    U, V = lf.shape[:2]
    if A < 1 or A > U or A > V or (U - A) % 2 or (V - A) % 2:
        raise LftError(f"angRes {A} of a {U} x {V} light field: the scripts' centre-view index 0.5*(U-A+2) needs A <= U, V and "
                       "U-A, V-A even")
    return (U - A) // 2, (V - A) // 2


def to_device(lf: np.ndarray, A: int, device) -> torch.Tensor:
    """The centre A x A views (channels 0..2) of a loaded light field on `device`, in the stored class and the stored memory order
    (a v7.3 file's reversed layout stays reversed: no transpose on the host)."""
    u0, v0 = centre_views(lf, A)
    if lf.dtype not in (np.uint8, np.float32, np.float64):
        raise LftError(f"light field of class {lf.dtype}: uint8, single and double are supported")
    sub = np.array(lf[u0:u0 + A, v0:v0 + A, :, :, :3], order="K")       # a dense copy in the array's own axis order
    return torch.from_numpy(sub).to(device)


def patch_grid(H: int, W: int, s: int) -> List[Tuple[int, int]]:
    """Generate_Data_for_Training.m:40-41: h = 1:stride:H-patchsize+1 (outer), w likewise (inner); 0-based origins."""
    ps, st = PATCH_LR * s, STRIDE_LR * s
    return [(h, w) for h in range(0, H - ps + 1, st) for w in range(0, W - ps + 1, st)]


def _dev(device):
    return torch.device(device if device is not None else "cuda")


def test_pair(lf, A: int, s: int, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Generate_Data_for_Test.m for one scene: (Lr_SAI_y [A*H/s, A*W/s], Hr_SAI_y [A*H, A*W]) fp32 on the device, MATLAB matrix
    orientation, H and W cut down to multiples of 4.  lf: a loaded [U, V, H, W, C] array or the tensor of ``to_device``."""
    t = lf if isinstance(lf, torch.Tensor) else to_device(lf, A, _dev(device))
    H, W = int(t.shape[2]) // TEST_MULTIPLE * TEST_MULTIPLE, int(t.shape[3]) // TEST_MULTIPLE * TEST_MULTIPLE
    if H < 1 or W < 1:
        raise LftError(f"views of {t.shape[2]} x {t.shape[3]} are smaller than {TEST_MULTIPLE} x {TEST_MULTIPLE}")
    hr, lr = lf_prepare(t, A, s, [(0, 0)], H, W)
    return lr[0], hr[0]


def training_pairs(lf, A: int, s: int, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Generate_Data_for_Training.m for one scene: every grid patch, (Lr_SAI_y [n, A*32, A*32], Hr_SAI_y [n, A*32*s, A*32*s]) fp32
    on the device in the script's order, MATLAB matrix orientation (the files store them transposed)."""
    t = lf if isinstance(lf, torch.Tensor) else to_device(lf, A, _dev(device))
    crops = patch_grid(int(t.shape[2]), int(t.shape[3]), s)
    ps = PATCH_LR * s
    if not crops:
        dev = t.device
        return (torch.empty(0, A * PATCH_LR, A * PATCH_LR, device=dev), torch.empty(0, A * ps, A * ps, device=dev))
    hr, lr = lf_prepare(t, A, s, crops, ps, ps)
    return lr, hr


# ---------------------------------------------------------------------------------------------- directory walk
def list_datasets(src_data_path: str) -> List[str]:
    """The scripts' ``dir(src_data_path)`` minus '.' and '..': the non-hidden entries, sorted by name."""
    return sorted(d for d in os.listdir(src_data_path) if not d.startswith(".") and os.path.isdir(os.path.join(src_data_path, d)))


def list_scenes(src_data_path: str, dataset: str, split: str) -> List[Tuple[str, str]]:
    """(scene name, path) of the sorted ``*.mat`` files of <dataset>/<split>/; the name drops the last 4 characters."""
    d = os.path.join(src_data_path, dataset, split)
    if not os.path.isdir(d):
        return []
    return [(f[:-4], os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".mat") and not f.startswith(".")]


def training_plan(src_data_path: str, A: int, s: int, data_name: str = "ALL") -> List[Tuple[str, str, str, int, int]]:
    """The files Generate_Data_for_Training.m writes, in order: (dataset, file name %06d.h5 numbered from 1 per dataset, scene,
    y0, x0) -- datasets by name, scenes by name, then the patch grid (h outer, w inner).  Reads every scene's shape."""
    plan = []
    for ds in (list_datasets(src_data_path) if data_name == "ALL" else [data_name]):
        n = 0
        for name, path in list_scenes(src_data_path, ds, "training"):
            lf = load_lf(path)
            centre_views(lf, A)
            for y0, x0 in patch_grid(lf.shape[2], lf.shape[3], s):
                n += 1
                plan.append((ds, "%06d.h5" % n, name, y0, x0))
    return plan


class RawLFPatchSource:
    """Patch source of lft_amd.trainer.fit made straight from raw light fields: ``get(indices) -> (lr [n,1,A*32,A*32],
    hr [n,1,A*32*s,A*32*s])`` fp32 on `device`.  Sample i is the i-th file of the tree Generate_Data_for_Training.m (and
    tools/prepare_data.py) writes, in the order of lft_amd.datasets.H5PatchSource over that tree -- datasets by name, samples
    000001.h5 .. per dataset -- and transposed as that reader returns it.  Every scene's centre views stay on the device in their
    stored class; ``get`` makes the samples with one lft_lf_prepare call per scene it touches."""

    def __init__(self, src_data_path: str, angRes: int, scale: int, data_name: str = "ALL", device=None):
        self.A, self.s, self.device = angRes, scale, _dev(device)
        names = list_datasets(src_data_path) if data_name == "ALL" else [data_name]
        self.scenes: List[torch.Tensor] = []
        self.scene_names: List[Tuple[str, str]] = []
        owner, origin = [], []
        for ds in names:
            for name, path in list_scenes(src_data_path, ds, "training"):
                t = to_device(load_lf(path), angRes, self.device)
                grid = patch_grid(int(t.shape[2]), int(t.shape[3]), scale)
                if not grid:
                    continue
                owner += [len(self.scenes)] * len(grid)
                origin += grid
                self.scenes.append(t)
                self.scene_names.append((ds, name))
        self._owner = np.asarray(owner, dtype=np.int64)
        self._origin = np.asarray(origin, dtype=np.int32).reshape(-1, 2)

    def __len__(self):
        return int(self._owner.size)

    def locate(self, i: int) -> Tuple[str, str, int, int]:
        """(dataset, scene, y0, x0) of sample i (0-based origins of its HR patch in the views)."""
        d, n = self.scene_names[int(self._owner[i])]
        return d, n, int(self._origin[i, 0]), int(self._origin[i, 1])

    def get(self, indices: Sequence[int]):
        ix = np.asarray(indices, dtype=np.int64).reshape(-1)
        if ix.size and (ix.min() < 0 or ix.max() >= len(self)):
            raise IndexError(f"sample index outside 0 .. {len(self) - 1}")
        A, s = self.A, self.s
        p, ps = PATCH_LR, PATCH_LR * s
        lr = torch.empty(ix.size, 1, A * p, A * p, dtype=torch.float32, device=self.device)
        hr = torch.empty(ix.size, 1, A * ps, A * ps, dtype=torch.float32, device=self.device)
        own = self._owner[ix]
        for sc in np.unique(own):
            pos = np.nonzero(own == sc)[0]
            h, l = lf_prepare(self.scenes[int(sc)], A, s, self._origin[ix[pos]], ps, ps)
            where = torch.from_numpy(pos).to(self.device)
            hr[where, 0] = h.transpose(-1, -2)                  # the training loader sees the stored (transposed) matrix
            lr[where, 0] = l.transpose(-1, -2)
        return lr, hr


def raw_test_scenes(src_data_path: str, angRes: int, scale: int, dataset: str, device=None) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
    """(lr [A*H/s, A*W/s], hr [A*H, A*W]) of every test scene of `dataset` (sorted *.mat of <dataset>/test/), made on the device:
    what lft_amd.datasets.TestSetDataLoader returns for the tree Generate_Data_for_Test.m writes, ready for evaluate.test."""
    dev = _dev(device)
    for _, path in list_scenes(src_data_path, dataset, "test"):
        yield test_pair(load_lf(path), angRes, scale, dev)
