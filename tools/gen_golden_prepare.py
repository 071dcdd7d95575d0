#!/opt/conda/bin/python3.9
"""Generate tests/golden/prepare_*.npz and tests/golden/prepare_lf_v73.mat (build container only).

The yardstick of lft_amd.prepare / lft_lf_prepare is the reference's own Python port of the MATLAB steps its data scripts take per
view (Generate_Data_for_Training.m:47-58, Generate_Data_for_Test.m:57-66): ``rgb2ycbcr`` of utils/utils.py and ``imresize`` /
``contributions`` of utils/imresize.py.  utils/utils.py imports skimage and the argparse singleton, so only the ``rgb2ycbcr``
definition is compiled out of it (the ast subset of tools/gen_golden.py:load_reference_tiling); utils/imresize.py is plain numpy and
is imported as it is.  As in the scripts, the RGB values enter as ``double(LF)``: no scaling, uint8 as 0..255.  The files record
inputs and outputs only.

  prepare_tables.npz  contribution tables (weights fp64, 0-based indices) for several (L, s), L down to below the kernel support
  prepare_views.npz   whole views of small light fields (A = 3, 5, 9; s = 2, 4; uint8 and double; non-square and tiny):
                      hr = single(Y), lr = single(imresize(Y, 1/s)) as mosaics in the MATLAB matrix orientation
  prepare_grid.npz    the training script's patch grid of one small scene: every patch, its Y and its downscale
  prepare_lf_v73.mat  a light field written the way MATLAB's -v7.3 save leaves it: HDF5 behind a 512-byte user block, LF stored
                      as [3, W, H, V, U] uint8 in deflated chunks; prepare_views.npz holds the array ('v73_lf', [U, V, H, W, 3])

It runs under /opt/conda/bin/python3.9 (the interpreter with h5py):  /opt/conda/bin/python3.9 tools/gen_golden_prepare.py
"""
import ast
import importlib.util
import os

import h5py
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
REF = "/root/reference"


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_imresize", os.path.join(REF, "utils", "imresize.py"))
    imr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(imr)
    tree = ast.parse(open(os.path.join(REF, "utils", "utils.py")).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "rgb2ycbcr"]
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "reference_utils_subset", "exec"), ns)
    return imr, ns["rgb2ycbcr"]


def view_y_lr(imr, rgb2ycbcr, rgb, s):
    y = rgb2ycbcr(rgb.astype(np.float64))[:, :, 0]                         # double(...) then rgb2ycbcr, channel 1
    return y.astype(np.float32), imr.imresize(y, scalar_scale=1.0 / s).astype(np.float32)


def mosaics(imr, rgb2ycbcr, lf, A, s, y0, x0, ch, cw):
    U, V = lf.shape[:2]
    u0, v0 = (U - A) // 2, (V - A) // 2
    oh, ow = int(np.ceil(ch / s)), int(np.ceil(cw / s))
    hr = np.zeros((A * ch, A * cw), np.float32)
    lr = np.zeros((A * oh, A * ow), np.float32)
    for u in range(A):
        for v in range(A):
            h, l = view_y_lr(imr, rgb2ycbcr, lf[u0 + u, v0 + v, y0:y0 + ch, x0:x0 + cw, :3], s)
            hr[u * ch:(u + 1) * ch, v * cw:(v + 1) * cw] = h
            lr[u * oh:(u + 1) * oh, v * ow:(v + 1) * ow] = l
    return hr, lr


def smooth_lf(rng, U, V, H, W, dtype):
    """A light field with some structure (a shifted smooth texture plus noise), in [0, 255] for uint8 and [0, 1] for double."""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    f = rng.uniform(0.05, 0.6, size=(3, 2))
    lf = np.empty((U, V, H, W, 3))
    for u in range(U):
        for v in range(V):
            for c in range(3):
                lf[u, v, :, :, c] = 0.5 + 0.3 * np.sin(f[c, 0] * (yy + 0.7 * u) + f[c, 1] * (xx + 0.7 * v) + c)
    lf = np.clip(lf + 0.08 * rng.standard_normal(lf.shape), 0, 1)
    return np.round(lf * 255).astype(np.uint8) if dtype == np.uint8 else lf.astype(dtype)


def main():
    imr, rgb2ycbcr = load_reference()
    rng = np.random.default_rng(20)

    tables = {}
    for L in (1, 2, 3, 5, 7, 8, 13, 17, 32, 64, 65, 128, 203):
        for s in (2, 4):
            out = int(np.ceil(L / s))
            w, ind = imr.contributions(L, out, 1.0 / s, imr.cubic, 4.0)
            tables[f"w_{L}_{s}"] = np.ascontiguousarray(w.reshape(out, -1))
            tables[f"i_{L}_{s}"] = np.ascontiguousarray(ind.reshape(out, -1).astype(np.int32))
    np.savez_compressed(os.path.join(OUT, "prepare_tables.npz"), **tables)

    views = {}
    cases = [   # name: U, V, A, H, W, s, class
        ("a3_s2_u8", 5, 5, 3, 13, 10, 2, np.uint8),
        ("a3_s4_f64", 3, 5, 3, 14, 11, 4, np.float64),
        ("a5_s2_f64", 7, 5, 5, 12, 15, 2, np.float64),
        ("a5_s4_u8", 7, 9, 5, 24, 17, 4, np.uint8),
        ("a9_s2_u8", 9, 9, 9, 7, 6, 2, np.uint8),
        ("a9_s4_f64", 9, 11, 9, 6, 5, 4, np.float64),
        ("a5_s4_tiny_u8", 5, 5, 5, 3, 2, 4, np.uint8),
        ("a3_s2_one_f64", 3, 3, 3, 1, 4, 2, np.float64),
    ]
    for name, U, V, A, H, W, s, cls in cases:
        lf = smooth_lf(rng, U, V, H, W, cls)
        hr, lr = mosaics(imr, rgb2ycbcr, lf, A, s, 0, 0, H, W)
        views[f"{name}_lf"], views[f"{name}_meta"] = lf, np.array([A, s], dtype=np.int64)
        views[f"{name}_hr"], views[f"{name}_lr"] = hr, lr

    # a v7.3-like .mat: MATLAB writes LF [U, V, H, W, 3] column-major, i.e. an HDF5 dataset [3, W, H, V, U]
    lf73 = smooth_lf(rng, 5, 5, 9, 7, np.uint8)
    path73 = os.path.join(OUT, "prepare_lf_v73.mat")
    with h5py.File(path73, "w", userblock_size=512, libver="earliest") as hf:
        d = hf.create_dataset("LF", data=lf73.transpose(4, 3, 2, 1, 0), chunks=(3, 7, 9, 1, 1), compression="gzip", compression_opts=3)
        d.attrs["MATLAB_class"] = np.bytes_("uint8")
    head = b"MATLAB 7.3 MAT-file, Platform: GLNXA64, Created on: Thu Jan  1 00:00:00 1970 HDF5 schema 1.00 ."
    with open(path73, "r+b") as f:
        f.write(head.ljust(116) + b"\0" * 8 + b"\x00\x02IM" + b"\0" * (512 - 128))
    views["v73_lf"] = lf73
    np.savez_compressed(os.path.join(OUT, "prepare_views.npz"), **views)

    # the training script's grid over one scene: A = 2 of 2 x 2 views of 96 x 100, s = 2 -> patches of 64, stride 32
    A, s = 2, 2
    lf = smooth_lf(rng, 2, 2, 96, 100, np.uint8)
    ps, st = 32 * s, 16 * s
    origins, hrs, lrs = [], [], []
    for h in range(1, 96 - ps + 2, st):                                     # h = 1 : stride : H - patchsize + 1
        for w in range(1, 100 - ps + 2, st):
            hr, lr = mosaics(imr, rgb2ycbcr, lf, A, s, h - 1, w - 1, ps, ps)
            origins.append((h - 1, w - 1))
            hrs.append(hr)
            lrs.append(lr)
    np.savez_compressed(os.path.join(OUT, "prepare_grid.npz"), lf=lf, meta=np.array([A, s], dtype=np.int64),
                        origins=np.array(origins, dtype=np.int32), hr=np.stack(hrs), lr=np.stack(lrs))
    for f in ("prepare_tables.npz", "prepare_views.npz", "prepare_grid.npz", "prepare_lf_v73.mat"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
