"""Cost of the data preparation (GPU box).  Prints one JSON line:

  * lft_lf_prepare on a 9x9 light field of 512x512 RGB views (uint8 and double), A = 5, s = 2 and 4: median microseconds per test
    scene (test_pair) and per full patch grid of the scene (training_pairs), HIP events around back-to-back launches; the byte
    contract (centre-view RGB read once, Hr and Lr written) and its fraction of the 8 TB/s HBM peak;
  * the numpy restatement's CPU time for the same work (tests/prepare_util.py, uint8 input);
  * the training-step time of trainer.fit fed by RawLFPatchSource against a cached H5PatchSource over the tree of the same raw
    data, alternating runs.

  python tools/prepare_bench.py [--reps 20] [--fit-runs 5] [--no-cpu]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lft_amd import datasets, prepare, trainer  # noqa: E402

HBM_PEAK = 8.0e12


def event_us(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1000.0)
    return statistics.median(out), min(out), max(out)


def kernel_figures(reps, cpu):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    base = rng.random((9, 9, 512, 512, 3))
    rows = []
    for cls in (np.uint8, np.float64):
        lf = np.round(base * 255).astype(np.uint8) if cls == np.uint8 else base
        t = prepare.to_device(lf, 5, dev)
        rgb = 25 * 512 * 512 * 3 * lf.itemsize
        for s in (2, 4):
            lr, hr = prepare.test_pair(t, 5, s)
            us, lo, hi = event_us(lambda: prepare.test_pair(t, 5, s), reps)
            nbytes = rgb + 4 * (hr.numel() + lr.numel())
            r = {"class": np.dtype(cls).name, "s": s, "test_us": round(us, 1), "test_spread_us": [round(lo, 1), round(hi, 1)],
                 "test_bytes": nbytes, "test_hbm_frac": round(nbytes / (us * 1e-6) / HBM_PEAK, 3)}
            lrg, hrg = prepare.training_pairs(t, 5, s)
            us, lo, hi = event_us(lambda: prepare.training_pairs(t, 5, s), reps)
            nbytes = rgb + 4 * (hrg.numel() + lrg.numel())
            r.update({"grid_patches": int(lrg.shape[0]), "grid_us": round(us, 1), "grid_spread_us": [round(lo, 1), round(hi, 1)],
                      "grid_bytes": nbytes, "grid_hbm_frac": round(nbytes / (us * 1e-6) / HBM_PEAK, 3)})
            if cpu and cls == np.uint8:
                from prepare_util import prepare_np
                t0 = time.perf_counter()
                prepare_np(lf, 5, s, [(0, 0)], 512, 512)
                t1 = time.perf_counter()
                prepare_np(lf, 5, s, prepare.patch_grid(512, 512, s), 32 * s, 32 * s)
                t2 = time.perf_counter()
                r.update({"numpy_test_ms": round((t1 - t0) * 1e3, 1), "numpy_grid_ms": round((t2 - t1) * 1e3, 1)})
            rows.append(r)
        del t
    return rows


def fit_figures(runs, batch):
    import prepare_data
    from lft_amd.params import deterministic_state
    from model import LFT
    dev = torch.device("cuda", 0)
    A, s = 5, 2
    with tempfile.TemporaryDirectory() as d:
        import scipy.io
        src = os.path.join(d, "datasets") + "/"
        rng = np.random.default_rng(2)
        os.makedirs(src + "D/training")
        for k in range(2):
            scipy.io.savemat(src + f"D/training/s{k}.mat", {"LF": np.round(rng.random((5, 5, 192, 224, 3)) * 255).astype(np.uint8)})
        prepare_data.run("train", A, s, src, os.path.join(d, "train") + "/", dev, log=lambda *a: None)
        sources = {"raw": prepare.RawLFPatchSource(src, A, s, device=dev),
                   "h5": datasets.H5PatchSource(os.path.join(d, "train") + "/", A, s, cache=True)}
        sources["h5"].get(range(len(sources["h5"])))                           # fill the cache
        n = len(sources["raw"])
        times = {"raw": [], "h5": []}
        net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s))
        net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, s, seed=1).items()})
        net = net.to(dev)
        nb = (n + batch - 1) // batch
        for i in range(2 * (runs + 1)):
            name = ("raw", "h5")[i % 2]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainer.fit(net, sources[name], epochs=1, batch_size=batch, seed=i, log=lambda *a: None)
            torch.cuda.synchronize()
            if i >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3 / nb)
    return {"samples": n, "batch": batch, "steps_per_run": nb, "raw_step_ms": round(statistics.median(times["raw"]), 3),
            "h5_step_ms": round(statistics.median(times["h5"]), 3),
            "raw_spread_ms": [round(min(times["raw"]), 3), round(max(times["raw"]), 3)],
            "h5_spread_ms": [round(min(times["h5"]), 3), round(max(times["h5"]), 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fit-runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    out = {"kernel": kernel_figures(a.reps, not a.no_cpu)}
    if a.fit_runs:
        out["fit"] = fit_figures(a.fit_runs, a.batch)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
