"""Numpy restatement of the colour path (tests only) and the loader of its fixtures (tools/gen_golden_colour.py).

Steps 1-7 of lft_amd/colour.py per sub-aperture view in fp64: scale, rgb2ycbcr in the reference's operation order, the
reference's up-scaling imresize with sums tap by tap in table order (rows first), the exact inverse transform with the products
summed left to right, and convertDouble2Byte.  It restates what lft_colour_merge computes, in the same order."""
import glob
import os

import numpy as np

from lft_amd import colour

from prepare_util import ulp_diff  # noqa: F401  (fp32 distance in units in the last place)

# name: (U, V, A, H, W, s, class, stored v7.3-reversed)
CASES = {
    "a3_s2_u8": (5, 5, 3, 13, 10, 2, np.uint8, False),
    "a3_s4_f64": (3, 5, 3, 14, 11, 4, np.float64, False),
    "a5_s2_f32": (7, 5, 5, 12, 15, 2, np.float32, False),
    "a5_s4_u8": (7, 9, 5, 20, 13, 4, np.uint8, False),          # 3 x 2 HR tiles with partial edges
    "a1_s2_u8": (1, 1, 1, 9, 7, 2, np.uint8, False),
    "a9_s4_f64": (9, 11, 9, 6, 5, 4, np.float64, False),
    "tiny": (5, 5, 5, 3, 2, 4, np.uint8, False),                # views smaller than the tap support
    "one": (3, 3, 3, 1, 4, 2, np.float64, False),
    "v73_s2_u8": (5, 5, 3, 9, 7, 2, np.uint8, True),            # used through the reversed [C, W, H, V, U] layout
    "sat_s4_u8": (3, 3, 3, 10, 12, 4, np.uint8, False),         # blocks of pure 0 next to pure 255: overshoot on both sides
}
TABLE_LENGTHS = (1, 2, 3, 5, 7, 8, 13, 17, 32, 33)


def load_case(golden_dir: str, name: str) -> dict:
    """The arrays of one case; an array too large for one committed file is stored in pieces `key@i` along axis 0."""
    files = sorted(glob.glob(os.path.join(golden_dir, f"colour_{name}.npz")) + glob.glob(os.path.join(golden_dir, f"colour_{name}.p*.npz")))
    assert files, name
    raw = {}
    for f in files:
        with np.load(f) as z:
            raw.update({k: z[k] for k in z.files})
    out = {k: v for k, v in raw.items() if "@" not in k}
    for key in sorted({k.split("@")[0] for k in raw if "@" in k}):
        n = sum(1 for k in raw if k.split("@")[0] == key and "@" in k)
        out[key] = np.concatenate([raw[f"{key}@{i}"] for i in range(n)], axis=0)
    return out


def scale_in(lf: np.ndarray) -> np.ndarray:
    x = lf.astype(np.float64)
    return x / 255.0 if lf.dtype == np.uint8 else x


def rgb2ycbcr(x: np.ndarray) -> np.ndarray:
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    return np.stack([(((65.481 * r + 128.553 * g) + 24.966 * b) + 16.0) / 255.0,
                     (((-37.797 * r - 74.203 * g) + 112.0 * b) + 128.0) / 255.0,
                     (((112.0 * r - 93.786 * g) - 18.214 * b) + 128.0) / 255.0], axis=-1)


def upscale(z: np.ndarray, s: int) -> np.ndarray:
    """imresize(z, s) of one [H, W] plane, fp64: rows first, then columns, sums tap by tap."""
    wh, ih = colour.up_contributions(z.shape[0], s)
    ww, iw = colour.up_contributions(z.shape[1], s)
    t = wh[:, 0:1] * z[ih[:, 0], :]
    for k in range(1, wh.shape[1]):
        t = t + wh[:, k:k + 1] * z[ih[:, k], :]
    o = ww[:, 0][None, :] * t[:, iw[:, 0]]
    for k in range(1, ww.shape[1]):
        o = o + ww[:, k][None, :] * t[:, iw[:, k]]
    return o


def ycc2rgb(y: np.ndarray, cb: np.ndarray, cr: np.ndarray) -> np.ndarray:
    """Minv * (255 * [y, cb, cr] - offset), the three products of a row summed left to right."""
    m = colour.inverse_matrix()
    e = [255.0 * y - 16.0, 255.0 * cb - 128.0, 255.0 * cr - 128.0]
    return np.stack([(m[j, 0] * e[0] + m[j, 1] * e[1]) + m[j, 2] * e[2] for j in range(3)], axis=-1)


def quantise(rgb: np.ndarray) -> np.ndarray:
    return np.rint(255.0 * np.clip(rgb, 0.0, 1.0)).astype(np.uint8)


def tie_distance(rgb: np.ndarray) -> np.ndarray:
    """How far 255 * clip(rgb) is from the nearest rounding tie (k + 0.5)."""
    q = 255.0 * np.clip(rgb, 0.0, 1.0)
    return np.abs(q - np.floor(q) - 0.5)


def colour_np(lf: np.ndarray, A: int, s: int, sr_y=None) -> dict:
    """Every stage for the centre A x A views of lf [U, V, H, W, C]: ycc [A, A, H, W, 3] fp64, lr_y [A*H, A*W] fp32, cb_up / cr_up
    [A, A, s*H, s*W] fp64, rgb [A, A, s*H, s*W, 3] fp64, out uint8.  sr_y: the fp32 mosaic [A*s*H, A*s*W], or None (baseline)."""
    U, V, H, W = lf.shape[:4]
    u0, v0 = (U - A) // 2, (V - A) // 2
    ycc = rgb2ycbcr(scale_in(np.asarray(lf[u0:u0 + A, v0:v0 + A, :, :, :3])))
    lr_y = ycc[..., 0].transpose(0, 2, 1, 3).reshape(A * H, A * W).astype(np.float32)
    up = np.empty((3, A, A, s * H, s * W))
    for u in range(A):
        for v in range(A):
            for c in range(0 if sr_y is None else 1, 3):
                up[c, u, v] = upscale(ycc[u, v, :, :, c], s)
    if sr_y is not None:
        up[0] = np.asarray(sr_y, dtype=np.float32).astype(np.float64).reshape(A, s * H, A, s * W).transpose(0, 2, 1, 3)
    rgb = ycc2rgb(up[0], up[1], up[2])
    return dict(ycc=ycc, lr_y=lr_y, y_up=up[0], cb_up=up[1], cr_up=up[2], rgb=rgb, out=quantise(rgb))

