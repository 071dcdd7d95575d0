#!/usr/bin/env python3
"""Generate tests/golden/colour_*.npz (build container only; numpy is all it needs).

The yardstick of lft_amd.colour / lft_lf_luma / lft_colour_merge is the reference's own code wherever that code is right:
``rgb2ycbcr`` of utils/utils.py (compiled out of the file by the ast subset of tools/gen_golden_prepare.py, because the module
imports skimage and the argparse singleton) and ``imresize`` / ``contributions`` / ``convertDouble2Byte`` of utils/imresize.py
(plain numpy, imported as it is).  The inverse transform is NOT the reference's ``ycbcr2rgb`` (utils/utils.py:171-183): that
function subtracts the offsets after the matrix instead of before it and does not invert ``rgb2ycbcr`` (this script measures
the miss and prints it).  The yardstick of that step is the exact inverse, rgb = inv(M) * (255 * ycc - offset), whose round trip
through the reference's ``rgb2ycbcr`` is asserted here to 1e-12.

  colour_tables.npz   up-scaling contribution tables (weights fp64, 0-based indices) for L in TABLE_LENGTHS, s = 2 and 4
  colour_<case>.npz   per case: lf (stored class), meta [A, s, v73], ycc, lr_y, a random fp32 sr_y in [-0.05, 1.05] (so that the
                      clip is exercised), cb_up, cr_up, the unquantised rgb, the uint8 out, and the baseline's out_base (Y up-scaled
                      like the chroma).  Floats are stored as fp32.  An array too large for one committed file is cut along
                      axis 0 into `key@i` pieces over colour_<case>.p<i>.npz.
Every case is reseeded until no recorded pixel has 255 * clip(rgb) within 1e-6 of a rounding tie, so that tests can ask for equal
bytes.  The files record inputs and outputs only.
"""
import ast
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
REF = "/root/reference"
PART_BYTES = 900_000                 # uncompressed bytes per file, below the 1 MiB limit of a committed file

M = np.array([[65.481, 128.553, 24.966], [-37.797, -74.203, 112.0], [112.0, -93.786, -18.214]])
OFFSET = np.array([16.0, 128.0, 128.0])
TABLE_LENGTHS = (1, 2, 3, 5, 7, 8, 13, 17, 32, 33)
CASES = [   # name, U, V, A, H, W, s, class, kind
    ("a3_s2_u8", 5, 5, 3, 13, 10, 2, np.uint8, ""),
    ("a3_s4_f64", 3, 5, 3, 14, 11, 4, np.float64, ""),
    ("a5_s2_f32", 7, 5, 5, 12, 15, 2, np.float32, ""),
    ("a5_s4_u8", 7, 9, 5, 20, 13, 4, np.uint8, ""),
    ("a1_s2_u8", 1, 1, 1, 9, 7, 2, np.uint8, ""),
    ("a9_s4_f64", 9, 11, 9, 6, 5, 4, np.float64, ""),
    ("tiny", 5, 5, 5, 3, 2, 4, np.uint8, ""),
    ("one", 3, 3, 3, 1, 4, 2, np.float64, ""),
    ("v73_s2_u8", 5, 5, 3, 9, 7, 2, np.uint8, "v73"),
    ("sat_s4_u8", 3, 3, 3, 10, 12, 4, np.uint8, "sat"),
]


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_imresize", os.path.join(REF, "utils", "imresize.py"))
    imr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(imr)
    tree = ast.parse(open(os.path.join(REF, "utils", "utils.py")).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("rgb2ycbcr", "ycbcr2rgb")]
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "reference_utils_subset", "exec"), ns)
    return imr, ns["rgb2ycbcr"], ns["ycbcr2rgb"]


def smooth_lf(rng, U, V, H, W, dtype, kind):
    """A light field with some structure (a shifted smooth texture plus noise), uint8 in [0, 255] or floats in [0, 1]."""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    f = rng.uniform(0.05, 0.6, size=(3, 2))
    lf = np.empty((U, V, H, W, 3))
    for u in range(U):
        for v in range(V):
            for c in range(3):
                lf[u, v, :, :, c] = 0.5 + 0.3 * np.sin(f[c, 0] * (yy + 0.7 * u) + f[c, 1] * (xx + 0.7 * v) + c)
    lf = np.clip(lf + 0.08 * rng.standard_normal(lf.shape), 0, 1)
    if kind == "sat":                # 3 x 3 blocks of pure 0 and pure 255 next to each other, per channel, in the upper left
        blocks = ((yy // 3 + xx // 3) % 2)[:H - 2, :W - 3]
        for c in range(3):
            lf[:, :, :H - 2, :W - 3, c] = blocks if c != 1 else 1.0 - blocks
    return np.round(lf * 255).astype(np.uint8) if dtype == np.uint8 else lf.astype(dtype)


def ycc2rgb(y, cb, cr):
    minv = np.linalg.inv(M)
    e = [255.0 * y - 16.0, 255.0 * cb - 128.0, 255.0 * cr - 128.0]
    return np.stack([(minv[j, 0] * e[0] + minv[j, 1] * e[1]) + minv[j, 2] * e[2] for j in range(3)], axis=-1)


def tie_distance(rgb):
    q = 255.0 * np.clip(rgb, 0.0, 1.0)
    return np.abs(q - np.floor(q) - 0.5)


def make_case(imr, rgb2ycbcr, rng, U, V, A, H, W, s, cls, kind):
    lf = smooth_lf(rng, U, V, H, W, cls, kind)
    u0, v0 = (U - A) // 2, (V - A) // 2
    x = lf[u0:u0 + A, v0:v0 + A].astype(np.float64)
    if cls == np.uint8:
        x = x / 255.0
    ycc = np.stack([np.stack([rgb2ycbcr(x[u, v]) for v in range(A)]) for u in range(A)])            # [A, A, H, W, 3]
    back = ycc2rgb(ycc[..., 0], ycc[..., 1], ycc[..., 2])
    assert np.abs(back - x).max() <= 1e-12, np.abs(back - x).max()                                      # step 6 inverts step 2
    up = np.stack([np.stack([np.stack([imr.imresize(ycc[u, v, :, :, c], scalar_scale=s) for v in range(A)]) for u in range(A)])
                   for c in range(3)])                                                                 # [3, A, A, sH, sW]
    assert up.shape == (3, A, A, s * H, s * W)
    sr_y = rng.uniform(-0.05, 1.05, size=(A * s * H, A * s * W)).astype(np.float32)
    sr_views = sr_y.astype(np.float64).reshape(A, s * H, A, s * W).transpose(0, 2, 1, 3)
    rgb = ycc2rgb(sr_views, up[1], up[2])
    rgb_base = ycc2rgb(up[0], up[1], up[2])
    if min(tie_distance(rgb).min(), tie_distance(rgb_base).min()) <= 1e-6:
        return None
    return dict(lf=lf, meta=np.array([A, s, int(kind == "v73")], dtype=np.int64), ycc=ycc.astype(np.float32),
                lr_y=ycc[..., 0].transpose(0, 2, 1, 3).reshape(A * H, A * W).astype(np.float32), sr_y=sr_y,
                cb_up=up[1].astype(np.float32), cr_up=up[2].astype(np.float32), rgb=rgb.astype(np.float32),
                out=imr.convertDouble2Byte(rgb), out_base=imr.convertDouble2Byte(rgb_base))


def write_parts(name, arrays):
    """One file if it fits, else pieces of at most PART_BYTES: whole arrays first-fit, a larger array cut along axis 0."""
    items = []
    for k, a in arrays.items():
        if a.nbytes <= PART_BYTES:
            items.append((k, a))
        else:
            n = -(-a.nbytes // PART_BYTES)
            items += [(f"{k}@{i}", p) for i, p in enumerate(np.array_split(a, n, axis=0))]
    parts = []
    for k, a in items:
        for p in parts:
            if sum(x.nbytes for x in p.values()) + a.nbytes <= PART_BYTES:
                p[k] = a
                break
        else:
            parts.append({k: a})
    total = 0
    for i, p in enumerate(parts):
        path = os.path.join(OUT, f"colour_{name}.npz" if i == 0 else f"colour_{name}.p{i}.npz")
        np.savez_compressed(path, **p)
        assert os.path.getsize(path) < (1 << 20), path
        total += os.path.getsize(path)
    return len(parts), total


def main():
    imr, rgb2ycbcr, ycbcr2rgb_ref = load_reference()

    # the reference's inverse does not invert its forward transform: measured on random uint8 input scaled to [0, 1]
    x = np.random.default_rng(1).integers(0, 256, size=(64, 64, 3)).astype(np.float64) / 255.0
    print(f"reference ycbcr2rgb(rgb2ycbcr(x)) misses x by up to {np.abs(ycbcr2rgb_ref(rgb2ycbcr(x)) - x).max():.4f} on [0, 1] data")

    tables = {}
    for L in TABLE_LENGTHS:
        for s in (2, 4):
            w, ind = imr.contributions(L, L * s, float(s), imr.cubic, 4.0)
            tables[f"w_{L}_{s}"] = np.ascontiguousarray(w.reshape(L * s, -1))
            tables[f"i_{L}_{s}"] = np.ascontiguousarray(ind.reshape(L * s, -1).astype(np.int32))
            assert tables[f"w_{L}_{s}"].shape[1] == 4 and 0 <= ind.min() and ind.max() <= L - 1
    np.savez_compressed(os.path.join(OUT, "colour_tables.npz"), **tables)
    print("colour_tables.npz", os.path.getsize(os.path.join(OUT, "colour_tables.npz")), "bytes")

    for n, (name, U, V, A, H, W, s, cls, kind) in enumerate(CASES):
        for attempt in range(64):
            case = make_case(imr, rgb2ycbcr, np.random.default_rng([30, n, attempt]), U, V, A, H, W, s, cls, kind)
            if case is not None:
                break
        else:
            raise SystemExit(f"{name}: no tie-free seed")
        clipped = (case["rgb"] < 0).mean(), (case["rgb"] > 1).mean()
        files, size = write_parts(name, case)
        print(f"colour_{name}: seed attempt {attempt}, {files} file(s), {size} bytes, clipped below / above {clipped[0]:.3f} / {clipped[1]:.3f}")


if __name__ == "__main__":
    main()
