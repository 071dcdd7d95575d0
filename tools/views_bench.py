"""Cost of densifying a light field (GPU box).  Prints one JSON line.

Workload: 5 x 5 views of 512 x 512 x 3 uint8 (the 4x output of a 128 x 128 scene) densified 2x: the 56 new views of the 9 x 9 grid,
quad blend, linear, from a disparity map at the centre (one sweep of 33 slopes from -2 to 2, made outside the timed region).
  * ``render_ms``: one `views.render` call for the 56 targets (k_view_splat + k_view_render): views, target maps and holes, with
    the host's share of the call (weights, table lookup, three output allocations).
  * ``replay_ms``: the same call captured once into a graph and replayed: the two kernels alone.
  * ``sweep_ms``: the plane-sweep baseline for the same 56 targets -- per target one `disparity.disparity(..., centre=target,
    all_in_focus=True)` over the 33 slopes, whose all-in-focus image is the view there.
The two are timed in the same process, alternating, in `--rounds` rounds (HIP events around `--reps` / `--sweep_reps` calls after
a warm-up).  ``contract_bytes``: per target the views of non-zero weight and Dr read once, the view and Dt written (holes too);
``hbm_frac`` is that over the best replay time as a share of the 8 TB/s HBM peak.

--visibility: the cost of the per-view visibility test on the same workload instead, without the sweep baseline.  Alternating in
the same process, per round: ``render_ms`` and ``replay_ms`` of the unchanged plain call, ``visible_ms`` and ``visible_replay_ms`` of
`views.render(..., visibility=dict(tau=TAU))` with the 25 per-view maps warped in the call (k_view_splat + k_view_fill, then
k_view_splat + k_view_render_vis), ``given_replay_ms`` of the same with the maps handed in (the render alone), and ``warp_ms`` /
``warp_replay_ms`` of `views.warp_disparity` to the 25 positions alone.  TAU is the sweep's slope step.  ``visible_contract_bytes``:
the plain contract, plus four bytes of Dv per pixel and view of non-zero weight, plus the count written; ``warp_contract_bytes``: Dr
read once per position, 25 maps and 25 hole maps written.

  python tools/views_bench.py [--rounds 3] [--reps 50] [--sweep_reps 3] [--warmup 2] [--out profiles/views_bench.txt]
  python tools/views_bench.py --visibility [--out profiles/views_visible_bench.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lft_amd import disparity, views  # noqa: E402
from refocus_bench import timed  # noqa: E402  (tools/refocus_bench.py)

A, H, W, C, D, RADIUS, FACTOR = 5, 512, 512, 3, 33, 2, 2
HBM_PEAK = 8.0e12          # bytes / s, MI355X specification (the project's rooflines use the same figure)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sweep_reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the line to this file")
    ap.add_argument("--visibility", action="store_true", help="the cost of the per-view visibility test beside the plain render")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    slopes = [float(x) for x in np.linspace(-2.0, 2.0, D)]
    d_range = (slopes[0], slopes[-1])
    lf = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (A, A, H, W, C)).astype(np.uint8)).to(dev)
    dr = disparity.disparity(lf, slopes, interp="linear", radius=RADIUS).disparity
    g = views.grid_targets(A, FACTOR)
    targets = [tuple(g[i, j]) for i in range(g.shape[0]) for j in range(g.shape[1]) if i % FACTOR or j % FACTOR]
    T = len(targets)

    def render():
        return views.render(lf, dr, targets, d_range)

    def sweep():
        return [disparity.disparity(lf, slopes, interp="linear", radius=RADIUS, centre=t, all_in_focus=True).all_in_focus for t in targets]

    if args.visibility:
        return visibility(args, lf, dr, targets, d_range, render, slopes[1] - slopes[0])
    for _ in range(args.warmup):
        render(), sweep()
    holes = float(render().holes.double().mean())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        render()
    torch.cuda.synchronize()
    rounds = []
    for _ in range(args.rounds):
        rounds.append({"render_ms": round(timed(render, args.reps), 4), "replay_ms": round(timed(graph.replay, args.reps), 4),
                       "sweep_ms": round(timed(sweep, args.sweep_reps), 4)})
    used = int((views.blend_weights(A, targets) > 0).sum())                # views of non-zero weight, over the targets
    nbytes = used * H * W * C + T * H * W * 4 + T * H * W * C + T * H * W * 4 + T * H * W
    best, best_sweep = min(r["render_ms"] for r in rounds), min(r["sweep_ms"] for r in rounds)
    replay = min(r["replay_ms"] for r in rounds)
    line = json.dumps({"bench": "views", "device": torch.cuda.get_device_name(0), "A": A, "view": [H, W, C], "in": "uint8", "factor": FACTOR,
                       "targets": T, "interp": "linear", "blend": "quad", "views_read": used, "hole_share": round(holes, 5), "reps": args.reps,
                       "sweep_reps": args.sweep_reps, "sweep_slopes": D, "rounds": rounds, "render_ms_best": best, "replay_ms_best": replay,
                       "sweep_ms_best": best_sweep, "contract_bytes": nbytes, "replay_GBps": round(nbytes / (replay * 1e-3) / 1e9, 1),
                       "hbm_frac": round(nbytes / (replay * 1e-3) / HBM_PEAK, 4), "sweep_over_render": round(best_sweep / best, 1),
                       "render_faster_in_every_round": all(r["render_ms"] < r["sweep_ms"] for r in rounds)})
    emit(line, args.out)


def emit(line, out):
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def captured(fn):
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        keep = fn()
    torch.cuda.synchronize()
    graph.keep = keep                       # the outputs live as long as the graph
    return graph


def visibility(args, lf, dr, targets, d_range, render, tau):
    T = len(targets)
    positions = [(u, v) for u in range(A) for v in range(A)]
    centre = ((A - 1) / 2, (A - 1) / 2)
    maps = views.warp_disparity(dr, positions, d_range, centre)[0].reshape(A, A, H, W)

    def visible():
        return views.render(lf, dr, targets, d_range, visibility=dict(tau=tau))

    def given():
        return views.render(lf, dr, targets, d_range, visibility=dict(tau=tau, view_disparity=maps))

    def warp():
        return views.warp_disparity(dr, positions, d_range, centre)

    for _ in range(args.warmup):
        render(), visible(), given(), warp()
    seen = visible().visible
    weights = views.blend_weights(A, targets) > 0
    used = int(weights.sum())
    occluded = 1.0 - float(seen.double().sum()) / (used * H * W)          # of the (pixel, view) pairs of non-zero weight: outside ones included
    graphs = {name: captured(fn) for name, fn in (("replay_ms", render), ("visible_replay_ms", visible), ("given_replay_ms", given), ("warp_replay_ms", warp))}
    rounds = []
    for _ in range(args.rounds):
        r = {"render_ms": round(timed(render, args.reps), 4), "visible_ms": round(timed(visible, args.reps), 4), "warp_ms": round(timed(warp, args.reps), 4)}
        r.update({name: round(timed(g.replay, args.reps), 4) for name, g in graphs.items()})
        rounds.append(r)
    best = {k: min(r[k] for r in rounds) for k in rounds[0]}
    plain_bytes = used * H * W * C + T * H * W * 4 + T * H * W * C + T * H * W * 4 + T * H * W
    vis_bytes = plain_bytes + used * H * W * 4 + T * H * W
    warp_bytes = A * A * (H * W * 4 + H * W * 4 + H * W)
    share = lambda n, ms: round(n / (ms * 1e-3) / HBM_PEAK, 4)
    emit(json.dumps({"bench": "views_visible", "device": torch.cuda.get_device_name(0), "A": A, "view": [H, W, C], "in": "uint8", "factor": FACTOR,
                     "targets": T, "interp": "linear", "blend": "quad", "views_read": used, "tau": tau, "not_visible_share": round(occluded, 5),
                     "reps": args.reps, "rounds": rounds, **{k + "_best": v for k, v in best.items()},
                     "contract_bytes": plain_bytes, "visible_contract_bytes": vis_bytes, "warp_contract_bytes": warp_bytes,
                     "hbm_frac": share(plain_bytes, best["replay_ms"]), "visible_hbm_frac": share(vis_bytes, best["given_replay_ms"]),
                     "warp_hbm_frac": share(warp_bytes, best["warp_replay_ms"]),
                     "visible_over_plain": round(best["visible_replay_ms"] / best["replay_ms"], 3),
                     "given_over_plain": round(best["given_replay_ms"] / best["replay_ms"], 3)}), args.out)


if __name__ == "__main__":
    main()
