#!/usr/bin/env python3
"""Drop-in replacement for the reference's Generate_Data_for_Training.m / Generate_Data_for_Test.m, on the GPU.

    python tools/prepare_data.py --mode train --angRes 5 --scale_factor 2 --src_data_path ./datasets/ --out ./data_for_train/
    python tools/prepare_data.py --mode test  --angRes 5 --scale_factor 2 --src_data_path ./datasets/ --out ./data_for_test/

reads ``<src_data_path>/<dataset>/{training,test}/<scene>.mat`` (v7.3 or v5 / v7, LF [U, V, H, W, 3]) and writes the scripts' trees:

    train: <out>/SR_{A}x{A}_{s}x/<dataset>/000001.h5 ...   one file per 32*s patch (stride 16*s) of every centre view grid, numbered
                                                            from 1 per dataset in scene order
    test:  <out>/SR_{A}x{A}_{s}x/<dataset>/<scene>.h5      one file per scene, views cut to multiples of 4

with ``Lr_SAI_y`` / ``Hr_SAI_y`` single-precision datasets in MATLAB's h5write form (lft_amd.h5write).  One lft_lf_prepare call per
scene (all its patches at once); the files are written from one thread.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from lft_amd import h5write, prepare  # noqa: E402


def tree_dir(out: str, A: int, s: int, dataset: str) -> str:
    return os.path.join(out, f"SR_{A}x{A}_{s}x", dataset)


def run(mode: str, A: int, s: int, src: str, out: str, device="cuda", log=print) -> dict:
    """Write the tree; returns {dataset: number of files written}."""
    split = "training" if mode == "train" else "test"
    written = {}
    for ds in prepare.list_datasets(src):
        n = 0
        for name, path in prepare.list_scenes(src, ds, split):
            t = prepare.to_device(prepare.load_lf(path), A, device)
            if mode == "train":
                lr, hr = prepare.training_pairs(t, A, s)
            else:
                lr, hr = prepare.test_pair(t, A, s)
                lr, hr = lr[None], hr[None]
            lr, hr = lr.cpu().numpy(), hr.cpu().numpy()
            if lr.shape[0]:
                os.makedirs(tree_dir(out, A, s, ds), exist_ok=True)       # as the scripts: a directory once there is a file for it
            for i in range(lr.shape[0]):
                n += 1
                fname = "%06d.h5" % n if mode == "train" else name + ".h5"           # Training.m:72, Test.m:71
                h5write.write_sai_pair(os.path.join(tree_dir(out, A, s, ds), fname), lr[i], hr[i], hr_first=mode == "test")
            log(f"Generating {'training' if mode == 'train' else 'test'} data of Scene_{name} in Dataset {ds}: "
                f"{lr.shape[0]} {'training' if mode == 'train' else 'test'} samples have been generated")
            del t
        written[ds] = n
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("train", "test"), required=True)
    ap.add_argument("--angRes", type=int, default=5)
    ap.add_argument("--scale_factor", type=int, default=4, choices=(2, 4))
    ap.add_argument("--src_data_path", default="./datasets/")
    ap.add_argument("--out", default=None, help="default ./data_for_train/ or ./data_for_test/")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    out = a.out or ("./data_for_train/" if a.mode == "train" else "./data_for_test/")
    t0 = time.perf_counter()
    written = run(a.mode, a.angRes, a.scale_factor, a.src_data_path, out, torch.device(a.device))
    print(f"wrote {sum(written.values())} files under {os.path.join(out, f'SR_{a.angRes}x{a.angRes}_{a.scale_factor}x')} "
          f"in {time.perf_counter() - t0:.1f} s: {written}")


if __name__ == "__main__":
    main()
