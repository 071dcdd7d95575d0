#!/usr/bin/env python3
"""Export the attention maps of a trained LFT (the paper's "Spatial-Aware Angular Modeling" figure, and the windowed spatial
attention) for one scene: lft_amd.attention on the GPU, written as ``maps.npz``.

    python tools/attention_maps.py --angRes 5 --scale_factor 4 --path_pre_pth ./pth/LFT_5x5_4x_epoch_50_model.pth \\
        --scene ./data_for_test/SR_5x5_4x/HCI_new/bedroom.h5 --out maps.npz
    python tools/attention_maps.py --angRes 5 --scale_factor 2 --path_pre_pth model.pth --data scene.npz     (array "lr": [A*h0, A*w0])
    python tools/attention_maps.py --bench                                                                  (one JSON line)

maps.npz holds, per angular layer L, ``scene_angL`` [A*h0, A*w0] -- tile (u, v) is the head-averaged weight the query view puts
on view (u, v) at every pixel (lft_amd.attention.scene_angular_attention) -- and, for the patch ``--patch_index`` of the scene's
LFdivide (default: the middle one), the maps of all eight blocks: ``angL`` [h, w, (8,) V, V] and ``spaL`` compact
[V, (8,) h, w, 5, 5] (``--per_head`` adds the head dimension).  No image is rendered: .npz is the product.

--bench: HIP-event median milliseconds per lft_train_attn_maps call for the angular and the spatial block in both head modes at
5x5 views of 32x32, batch 8, with the bytes each call writes and the achieved fraction of the HBM rate (8 TB/s peak)."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # bytes / s, MI355X specification (the project's rooflines use the same figure)


def bench(reps: int):
    from lft_amd import _lib, attention as AT, train as T
    from lft_amd.params import deterministic_state, param_table, synthetic_lr
    A, s, B, h, w = 5, 2, 8, 32, 32
    dev = torch.device("cuda", 0)
    sd = deterministic_state(64, s, seed=1)
    ps = [torch.from_numpy(sd[n]).to(dev).contiguous() for n, _, _ in param_table(64, s)]
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0)).to(dev)
    fwd = []
    tape = None
    for _ in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _, tape = T.train_forward(ps, lr, A, s, tape=tape)
        e1.record()
        torch.cuda.synchronize()
        fwd.append(e0.elapsed_time(e1))
    res = {"metric": "lft_train_attn_maps ms per call", "config": f"{A}x{A} views of {h}x{w}, B={B}, fp32 tape", "reps": reps,
           "train_forward_ms": round(min(fwd[1:]), 3), "hbm_peak_TBps": HBM_PEAK / 1e12, "calls": {}}
    for block, bname in ((_lib.BLOCK_ANG, "ang"), (_lib.BLOCK_SPA, "spa")):
        for per_head in (False, True):
            out = torch.empty(AT.map_shape(block, per_head, B, A, h, w), dtype=torch.float32, device=dev)
            for _ in range(3):
                AT.maps_from_tape(tape, block, 1, per_head, B, A, h, w, s, out=out)
            ms = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                AT.maps_from_tape(tape, block, 1, per_head, B, A, h, w, s, out=out)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = float(np.median(ms))
            nbytes = out.numel() * 4
            res["calls"][f"{bname}_{'heads' if per_head else 'mean'}"] = {
                "ms": round(med, 4), "bytes_written": nbytes, "TBps": round(nbytes / (med * 1e-3) / 1e12, 3),
                "fraction_of_hbm_peak": round(nbytes / (med * 1e-3) / HBM_PEAK, 3)}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--angRes", type=int, default=5)
    ap.add_argument("--scale_factor", type=int, default=4)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--path_pre_pth", default=None, help="checkpoint in the reference's format")
    ap.add_argument("--scene", default=None, help="one scene .h5 of the test tree (datasets Lr_SAI_y / Hr_SAI_y)")
    ap.add_argument("--data", default=None, help=".npz with the LR mosaic as array 'lr' [A*h0, A*w0]")
    ap.add_argument("--out", default="maps.npz")
    ap.add_argument("--query_view", type=int, default=None, help="view whose attention row is shown (default: the centre view)")
    ap.add_argument("--patch_index", type=int, default=None)
    ap.add_argument("--per_head", action="store_true")
    ap.add_argument("--patch_size_for_test", type=int, default=32)
    ap.add_argument("--stride_for_test", type=int, default=16)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if args.bench:
        return bench(args.reps)
    if not args.path_pre_pth or (args.scene is None) == (args.data is None):
        ap.error("needs --path_pre_pth and exactly one of --scene / --data (or --bench)")
    from lft_amd import attention as AT, datasets, scene, trainer
    from model import LFT
    dev = torch.device("cuda", 0)
    net = LFT.get_model(SimpleNamespace(channels=args.channels, angRes=args.angRes, scale_factor=args.scale_factor)).to(dev).eval()
    trainer.load_checkpoint(net, args.path_pre_pth)
    if args.scene:
        lr, _ = datasets.read_pair(args.scene)
        lr = datasets.to_tensor(np.transpose(lr, (1, 0)).copy()).squeeze(0)          # as TestSetDataLoader hands it to the test loop
    else:
        lr = torch.from_numpy(np.asarray(np.load(args.data)["lr"], dtype=np.float32))
    A, patch, stride = args.angRes, args.patch_size_for_test, args.stride_for_test
    if lr.dim() != 2 or lr.shape[0] % A or lr.shape[1] % A:
        raise SystemExit(f"the LR mosaic must be [A*h0, A*w0] with A = {A}, got {tuple(lr.shape)}")
    lr = lr.float().to(dev).contiguous()
    rec = {"meta": np.array([A, args.scale_factor, lr.shape[0] // A, lr.shape[1] // A, patch, stride], dtype=np.int64)}
    for l in range(AT.LAYERS):
        rec[f"scene_ang{l}"] = AT.scene_angular_attention(net, lr, l, args.query_view, patch, stride).cpu().numpy()
    patches = scene.divide(lr, A, patch, stride)
    k = patches.shape[0] // 2 if args.patch_index is None else args.patch_index
    for name, t in AT.attention_maps(net, patches[k:k + 1], per_head=args.per_head).items():
        rec[name] = t[0].cpu().numpy()
    rec["patch_index"] = np.array(k)
    np.savez_compressed(args.out, **rec)
    print(f"{args.out}: {patches.shape[0]} patches; scene mosaics {rec['scene_ang0'].shape}, block maps of patch {k}: "
          + ", ".join(f"{n} {rec[n].shape}" for n in ("ang0", "spa0")))


if __name__ == "__main__":
    main()
