"""Numpy restatement of lft_lf_prepare (tests only): the per-view path of the reference's data scripts, fp64, sums tap by tap in
table order, one rounding to fp32.  The yardstick for cases too large to store as fixtures."""
import os

import numpy as np

from lft_amd import prepare


def rgb_to_y(rgb: np.ndarray) -> np.ndarray:
    x = rgb.astype(np.float64)
    return (((65.481 * x[..., 0] + 128.553 * x[..., 1]) + 24.966 * x[..., 2]) + 16.0) / 255.0


def resize_view(y: np.ndarray, s: int) -> np.ndarray:
    """MATLAB imresize(y, 1/s), fp64: rows first, then columns."""
    wh, ih = prepare.contributions(y.shape[0], s)
    ww, iw = prepare.contributions(y.shape[1], s)
    t = wh[:, 0:1] * y[ih[:, 0], :]
    for k in range(1, wh.shape[1]):
        t = t + wh[:, k:k + 1] * y[ih[:, k], :]
    o = ww[:, 0][None, :] * t[:, iw[:, 0]]
    for k in range(1, ww.shape[1]):
        o = o + ww[:, k][None, :] * t[:, iw[:, k]]
    return o


def prepare_np(lf: np.ndarray, A: int, s: int, crops, ch: int, cw: int):
    """(hr [N, A*ch, A*cw], lr [N, A*oh, A*ow]) fp32, MATLAB orientation, for the centre A x A views of lf [U, V, H, W, C]."""
    u0, v0 = (lf.shape[0] - A) // 2, (lf.shape[1] - A) // 2
    oh, ow = prepare.out_length(ch, s), prepare.out_length(cw, s)
    crops = np.asarray(crops).reshape(-1, 2)
    hr = np.empty((len(crops), A * ch, A * cw), np.float32)
    lr = np.empty((len(crops), A * oh, A * ow), np.float32)
    for n, (y0, x0) in enumerate(crops):
        for u in range(A):
            for v in range(A):
                y = rgb_to_y(lf[u0 + u, v0 + v, y0:y0 + ch, x0:x0 + cw, :3])
                hr[n, u * ch:(u + 1) * ch, v * cw:(v + 1) * cw] = y.astype(np.float32)
                lr[n, u * oh:(u + 1) * oh, v * ow:(v + 1) * ow] = resize_view(y, s).astype(np.float32)
    return hr, lr


def ulp_diff(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Distance in fp32 units in the last place (ordered-integer difference)."""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# (dataset, split, scene, U, V, H, W, class, .mat form): odd sizes, 5x5 / 7x7 / 9x9 light fields, every class, both forms
TREE = [("EPFL", "training", "Bikes", 7, 7, 75, 101, np.uint8, "v5"),
        ("EPFL", "training", "Flowers", 5, 5, 97, 70, np.float32, "v73"),
        ("EPFL", "test", "Ankylosaurus", 5, 5, 46, 38, np.float64, "v5"),
        ("EPFL", "test", "Bench", 9, 9, 50, 61, np.float32, "v73"),
        ("HCI_new", "training", "bedroom", 5, 5, 66, 97, np.float64, "v5"),
        ("HCI_new", "training", "boxes", 9, 9, 70, 67, np.float32, "v73"),
        ("HCI_new", "training", "dino", 5, 5, 99, 99, np.uint8, "v5"),
        ("HCI_new", "test", "herbs", 5, 5, 51, 45, np.uint8, "v5")]


def write_v73(path: str, lf: np.ndarray) -> None:
    """A v7.3-like .mat: HDF5 behind a 512-byte user block, LF stored as [C, W, H, V, U] (MATLAB's column-major order)."""
    from lft_amd import h5write
    h5write.write_datasets(path, [("LF", np.ascontiguousarray(lf.transpose(4, 3, 2, 1, 0)))], userblock=512)


def make_datasets_tree(root: str, seed: int = 0):
    """The raw-data tree of TREE under root (<dataset>/<split>/<scene>.mat).  Returns {(dataset, split, scene): lf}."""
    import scipy.io
    rng = np.random.default_rng(seed)
    out = {}
    for ds, split, name, U, V, H, W, cls, form in TREE:
        os.makedirs(os.path.join(root, ds, split), exist_ok=True)
        lf = rng.random((U, V, H, W, 3))
        lf = np.round(lf * 255).astype(np.uint8) if cls == np.uint8 else lf.astype(cls)
        path = os.path.join(root, ds, split, name + ".mat")
        if form == "v5":
            scipy.io.savemat(path, {"LF": lf})
        else:
            write_v73(path, lf)
        out[(ds, split, name)] = lf
    return out
