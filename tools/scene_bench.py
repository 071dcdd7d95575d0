"""Whole-scene inference throughput (reference test.py:83-101 as one batched call): LFdivide on the GPU, every
numU x numV patch through the network as one batch, LFintegrate.  python tools/scene_bench.py [--ang 5 --scale 4 --size 128]
"metrics_ms": the event-timed milliseconds of one lft_view_metrics call (PSNR and SSIM of every view) on the scene's SR output, the
median of 50."""
import argparse, json, os, sys, time
from types import SimpleNamespace
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from lft_amd import metrics, scene                                 # noqa: E402
from lft_amd.params import deterministic_state                     # noqa: E402
from model import LFT                                              # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ang", type=int, default=5); ap.add_argument("--scale", type=int, default=4)
ap.add_argument("--size", type=int, default=128, help="LR view height = width"); ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--precision", default="bf16")
ap.add_argument("--ensemble", default="none", choices=["none", "flips", "dihedral"], help="geometric self-ensemble (lft_amd.ensemble)")
a = ap.parse_args()
net = LFT.get_model(SimpleNamespace(channels=64, angRes=a.ang, scale_factor=a.scale), precision=a.precision)
net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, a.scale, seed=1).items()})
net = net.cuda().eval()
ens = None if a.ensemble == "none" else a.ensemble
sc = torch.from_numpy(np.random.default_rng(0).random((a.ang * a.size, a.ang * a.size), dtype=np.float32)).cuda()
with torch.no_grad():
    for _ in range(3):
        out = scene.super_resolve_scene(net, sc, patch=32, stride=16, ensemble=ens)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(a.reps):
        out = scene.super_resolve_scene(net, sc, patch=32, stride=16, ensemble=ens)
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / a.reps
label, ms = (out * 0.98 + 0.01).contiguous(), []
for i in range(55):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); metrics.view_metrics(label, out, a.ang); e1.record(); e1.synchronize()
    ms.append(e0.elapsed_time(e1))
nu, nv = scene.scene_counts(a.size, a.size, 32, 16)
print(json.dumps({"metric": "LF scenes/sec", "value": 1 / dt, "ms_per_scene": 1e3 * dt, "patches_per_scene": nu * nv,
                  "patches_per_s": nu * nv / dt, "config": f"{a.ang}x{a.ang} views of {a.size}x{a.size} LR, {a.scale}x, patch 32 stride 16, {a.precision}",
                  "ensemble": a.ensemble, "out_shape": list(out.shape), "metrics_ms": float(np.median(ms[5:]))}))
