#!/usr/bin/env python3
"""Bit-level regression of the inference output against another build: the forward of BASELINE configs[1], a ragged 2x shape that
takes the kernels' general paths, and one small shape per angular kernel variant (k_ang for up to 25 views, every k_ang_multi
form from 36 to 121 views) under each library given, each in its own process; prints whether the outputs are bit-identical.
  tools/out_bits.py ab_so/liblft_base0.so lft_amd/liblft_hip.so
--lightfield: the light-field analysis instead -- refocus, disparity, regularize, render with and without the visibility test and
warp_disparity over shapes small enough that every tile is ragged, one hash per output of every case.
  tools/out_bits.py --lightfield ab_so/liblft_base0.so lft_amd/liblft_hip.so"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    sys.path.insert(0, ROOT)
    from types import SimpleNamespace
    import torch
    from model import LFT
    from lft_amd.params import deterministic_state, synthetic_lr
    for A, s, B, h, w in ((5, 4, 2, 32, 32), (3, 2, 1, 13, 22), (2, 4, 1, 6, 12),
                          (6, 2, 1, 8, 8), (8, 2, 1, 8, 8), (9, 2, 1, 8, 8), (10, 2, 1, 8, 8), (11, 2, 1, 8, 8)):
        for prec in ("bf16", "fp16", "fp32"):
            net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s), precision=prec, streams=1).cuda().eval()
            net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, s, seed=1).items()})
            with torch.no_grad():
                out = net(torch.from_numpy(synthetic_lr(B, A, h, w, seed=0)).cuda())
            print(f"A{A} s{s} B{B} {h}x{w} {prec}", hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16], flush=True)


def child_lightfield():
    """Views of 40 x 37 (9 x 9 views of 12 x 10 for the visibility mask's second test), 3 x 3 views; C = 1 as a batch of two
    mosaics, C = 3 as views; uint8 and float32 in and out; every tap count an entry point takes."""
    sys.path.insert(0, ROOT)
    import itertools
    import numpy as np
    import torch
    from lft_amd import disparity as Dm, refocus as Rf, views as V
    U8, F32 = torch.uint8, torch.float32

    def show(case, result):
        named = zip(getattr(result, "_fields", ("maps", "holes")), result) if isinstance(result, tuple) else [("out", result)]
        for name, t in named:
            if t is not None:
                print(f"{case} {name}", hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16], flush=True)

    def field(rng, A, H, W, C, dtype):
        """(light field, angRes argument, leading shape of its maps): C = 1 a batch [2, 1, A*H, A*W], else views [A, A, H, W, C]."""
        shape = (2, 1, A * H, A * W) if C == 1 else (A, A, H, W, C)
        x = rng.integers(0, 256, shape).astype(np.uint8) if dtype == U8 else rng.random(shape, dtype=np.float32)
        return torch.from_numpy(x).cuda(), (A if C == 1 else None), ((2,) if C == 1 else ())

    def depth(rng, lead, H, W, amp):
        """A map with a step edge (holes, occlusions), noise and a few non-finite pixels."""
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        d = np.where((y > H // 3) & (x > W // 4) & (x < 3 * W // 4), amp, -0.6 * amp) + 0.2 * amp * rng.standard_normal(lead + (H, W))
        d = d.astype(np.float32)
        d[..., 1, 2], d[..., H - 2, W - 3], d[..., H // 2, W // 2] = np.nan, np.inf, -np.inf
        return torch.from_numpy(d).cuda()

    slopes = [-1.5, -0.7, 0.0, 0.6, 1.4]
    targets = [(0.25, 1.5), (1.0, 0.4), (1.75, 1.9)]
    rng = np.random.default_rng(7)
    A, H, W = 3, 40, 37
    for C, din, dout in itertools.product((1, 3), (U8, F32), (U8, F32)):
        lf, ang, lead = field(rng, A, H, W, C, din)
        tag = f"A{A} {H}x{W} C{C} {str(din)[6:]}->{str(dout)[6:]}"
        for interp in ("nearest", "linear", "cubic"):
            show(f"{tag} refocus {interp}", Rf.refocus(lf, slopes, ang, interp=interp, out_dtype=dout))
            for radius in (0, 2):
                swept = Dm.disparity(lf, slopes, ang, interp=interp, radius=radius, all_in_focus=True, cost_volume=True, aif_dtype=dout)
                show(f"{tag} disparity {interp} r{radius}", swept)
        stack = Rf.refocus(lf, slopes, ang, interp="linear", out_dtype=F32)
        guide = depth(rng, lead, H, W, 1.0).nan_to_num(0.0, 0.0, 0.0)
        p1, p2 = 0.002, 0.03
        for paths, guided, stacked in itertools.product((4, 8), (False, True), (False, True)):
            show(f"{tag} regularize paths{paths} guide{int(guided)} stack{int(stacked)}",
                 Dm.regularize(swept.cost, slopes, p1, p2, paths, guide if guided else None, 0.05 if guided else 0.0,
                               stack if stacked else None, dout if stacked else None, aggregated=True))
        dr = depth(rng, lead, H, W, 1.5)
        for interp, near, fill in itertools.product(("linear", "cubic"), ("larger", "smaller"), (0, 32)):
            kw = dict(angRes=ang, interp=interp, near=near, fill=fill, out_dtype=dout)
            show(f"{tag} render {interp} {near} fill{fill}", V.render(lf, dr, targets, (-2.0, 2.0), **kw))
            show(f"{tag} render_visible {interp} {near} fill{fill}", V.render(lf, dr, targets, (-2.0, 2.0), visibility=dict(tau=0.1), **kw))
    for near, fill in itertools.product(("larger", "smaller"), (0, 32)):
        show(f"A{A} {H}x{W} warp_disparity {near} fill{fill}", V.warp_disparity(dr, [(u, v) for u in range(A) for v in range(A)] + targets, (-2.0, 2.0), (1, 1), near, fill))
    lf, ang, lead = field(rng, 9, 12, 10, 3, F32)
    show("A9 12x10 C3 float32 render_visible cubic", V.render(lf, depth(rng, lead, 12, 10, 0.9), [(3.5, 4.25)], (-1.0, 1.0), blend="gaussian", sigma=3.0,
                                             interp="cubic", visibility=dict(tau=0.05)))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] in ("--child", "--child-lightfield"):
        child() if sys.argv[1] == "--child" else child_lightfield()
        raise SystemExit(0)
    mode = "--child-lightfield" if "--lightfield" in sys.argv[1:] else "--child"
    outs = []
    for lib in (a for a in sys.argv[1:] if a != "--lightfield"):
        env = dict(os.environ, LFT_LIB_PATH=os.path.abspath(lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=env, capture_output=True, text=True, cwd=ROOT)
        if r.returncode:
            raise SystemExit(f"{lib} failed:\n{r.stderr[-2000:]}")
        outs.append([l for l in r.stdout.splitlines() if l.startswith("A")])
        print(lib)
        print("\n".join("   " + l for l in outs[-1]))
    same = all(o == outs[0] for o in outs[1:])
    print("bit-identical" if same else "DIFFERENT")
    raise SystemExit(0 if same else 1)
