#!/usr/bin/env python3
"""Bit-level regression of the inference output against another build: the forward of BASELINE configs[1], a ragged 2x shape that
takes the kernels' general paths, and one small shape per angular kernel variant (k_ang for up to 25 views, every k_ang_multi
form from 36 to 121 views, and the two-position forms once more with an odd position count) under each library given, each in its
own process, with the outputs of lft_init_features_fwd and of lft_ang_block_fwd (layer 0) beside it; prints whether all are bit-identical.
  tools/out_bits.py ab_so/liblft_base0.so lft_amd/liblft_hip.so
--lightfield: the light-field analysis instead -- refocus, disparity with and without the occlusion-aware cost, regularize, render with and without the visibility test and
warp_disparity over shapes small enough that every tile is ragged, one hash per output of every case.
  tools/out_bits.py --lightfield ab_so/liblft_base0.so lft_amd/liblft_hip.so
--pipeline: the data and objective kernels instead -- lf_prepare, luma, merge, view_metrics, the three losses, Adam, the guarded step
and the EMA, again over shapes small enough that every tile is ragged, the fall-back paths of both resamplers included.
  tools/out_bits.py --pipeline ab_so/liblft_base0.so lft_amd/liblft_hip.so"""
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
    from lft_amd import _lib, module
    from lft_amd.params import deterministic_state, param_table, synthetic_lr
    ACT = {"bf16": (_lib.PREC_BF16, torch.bfloat16), "fp16": (_lib.PREC_F16, torch.float16), "fp32": (_lib.PREC_F32, torch.float32)}

    def digest(t):
        return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]

    # 3x5 at B = 1: 15 positions, so a k_ang_multi workgroup that holds two positions (16-bit, A = 6, 8, 9) ends on an inactive group
    for A, s, B, h, w in ((5, 4, 2, 32, 32), (3, 2, 1, 13, 22), (2, 4, 1, 6, 12),
                          (6, 2, 1, 8, 8), (8, 2, 1, 8, 8), (9, 2, 1, 8, 8), (10, 2, 1, 8, 8), (11, 2, 1, 8, 8),
                          (6, 2, 1, 3, 5), (8, 2, 1, 3, 5), (9, 2, 1, 3, 5)):
        for prec in ("bf16", "fp16", "fp32"):
            sd = deterministic_state(64, s, seed=1)
            lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0)).cuda()
            net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s), precision=prec, streams=1).cuda().eval()
            net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            with torch.no_grad():
                out = net(lr)
            # the first two stages on their own, called as tests/test_gpu_parity.py calls them: a changed bit there cannot hide
            # behind the rounding of the stages after it
            p, dtype = ACT[prec]
            packed = module.pack_weights([torch.from_numpy(sd[n]).cuda() for n, _, _ in param_table(64, s)], A, h, w, s, p, _lib.stream_ptr("cuda"))
            work = torch.empty(_lib.workspace_bytes(B, A, h, w, s, p), dtype=torch.uint8, device="cuda")
            feat = torch.empty(B, A * A, h, w, 64, dtype=dtype, device="cuda")
            ang = torch.empty_like(feat)
            _lib.enqueue("lft_init_features_fwd", "cuda", packed.data_ptr(), lr.data_ptr(), feat.data_ptr(), work.data_ptr(), B, A, h, w, s, p)
            _lib.enqueue("lft_ang_block_fwd", "cuda", packed.data_ptr(), 0, feat.data_ptr(), ang.data_ptr(), B, A, h, w, s, p)
            print(f"A{A} s{s} B{B} {h}x{w} {prec}", digest(out), "init_features", digest(feat), "ang_block0", digest(ang), flush=True)


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
            if isinstance(t, torch.Tensor):
                print(f"{case} {name}", hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16], flush=True)
            elif t is not None:
                print(f"{case} {name}", t, flush=True)                  # subsets_kept

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
    masks = np.zeros((3, A, A), bool)                                   # one view (dropped: fewer than min_views), a row, every view
    masks[0, 0, 0], masks[1, 1, :], masks[2] = True, True, True
    occlusions = (("halves", "halves"), ("quadrants", dict(subsets="quadrants", margin=1.5)), ("array", dict(subsets=masks, margin=1.25)))
    for C, din, dout in itertools.product((1, 3), (U8, F32), (U8, F32)):
        lf, ang, lead = field(rng, A, H, W, C, din)
        tag = f"A{A} {H}x{W} C{C} {str(din)[6:]}->{str(dout)[6:]}"
        for interp in ("nearest", "linear", "cubic"):
            show(f"{tag} refocus {interp}", Rf.refocus(lf, slopes, ang, interp=interp, out_dtype=dout))
            for radius in (0, 2):
                swept = Dm.disparity(lf, slopes, ang, interp=interp, radius=radius, all_in_focus=True, cost_volume=True, aif_dtype=dout)
                show(f"{tag} disparity {interp} r{radius}", swept)
            for name, occ in occlusions:
                show(f"{tag} disparity {interp} occlusion {name}",
                     Dm.disparity(lf, slopes, ang, interp=interp, all_in_focus=True, cost_volume=True, aif_dtype=dout, occlusion=occ))
            show(f"{tag} disparity {interp} occlusion halves maps only", Dm.disparity(lf, slopes, ang, interp=interp, occlusion="halves"))
            show(f"{tag} occlusion_volume {interp}", Dm.occlusion_volume(lf, slopes, ang, interp=interp, occlusion=occlusions[-1][1]))
            show(f"{tag} disparity {interp} occlusion quadrants regularize",
                 Dm.disparity(lf, slopes, ang, interp=interp, all_in_focus=True, cost_volume=True, aif_dtype=dout, occlusion="quadrants",
                              regularize=dict(p1=0.002, p2=0.03)))
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


def child_pipeline():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctypes
    import itertools
    import numpy as np
    import torch
    from lft_amd import _lib, colour, loss as L, metrics, prepare, train as T
    from ssim_loss_util import SHAPES
    DEV = torch.device("cuda:0")
    rng = np.random.default_rng(11)

    def show(case, **tensors):
        for name, t in tensors.items():
            print(f"P {case} {name}", hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16], flush=True)

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)

    def far_table(w, i, L_, far):
        """One more tap of weight 0 at the end farther from each output's own taps: every tile leaves the staged region."""
        if not far:
            return dev(w), dev(i)
        end = np.where(L_ - 1 - i.min(axis=1) >= i.max(axis=1), L_ - 1, 0).astype(np.int32)
        return dev(np.concatenate([w, np.zeros((w.shape[0], 1))], axis=1)), dev(np.concatenate([i, end[:, None]], axis=1))

    def field(dtype, shape):
        x = rng.integers(0, 256, shape)
        return dev(x.astype(np.uint8) if dtype == "uint8" else (x / 255.0).astype(dtype))

    # ---- lf_prepare: every input class, two ragged crops; then the fall-back through the C ABI
    for dtype, s in itertools.product(("uint8", "float32", "float64"), (2, 4)):
        hr, lr = prepare.lf_prepare(field(dtype, (3, 3, 45, 41, 3)), 3, s, [(0, 0), (5, 4)], 40, 37)
        show(f"lf_prepare {dtype} s{s}", hr=hr, lr=lr)
    lf = field("uint8", (4, 4, 96, 80, 3))
    crop = np.zeros((1, 2), dtype=np.int32)
    for s, (far_h, far_w) in itertools.product((2, 4), ((True, True), (True, False), (False, True))):
        (wh, ih), (ww, iw) = far_table(*prepare.contributions(96, s), 96, far_h), far_table(*prepare.contributions(80, s), 80, far_w)
        hr, lr = torch.zeros(1, 2 * 96, 2 * 80, device=DEV), torch.zeros(1, 2 * wh.shape[0], 2 * ww.shape[0], device=DEV)
        _lib.enqueue("lft_lf_prepare", DEV, *prepare.lf_args(lf), 2, s, crop.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 1, 96, 80,
                     wh.data_ptr(), ih.data_ptr(), wh.shape[1], ww.data_ptr(), iw.data_ptr(), ww.shape[1], hr.data_ptr(), lr.data_ptr())
        show(f"lf_prepare fallback s{s} rows{int(far_h)} cols{int(far_w)}", hr=hr, lr=lr)

    # ---- luma and merge: contiguous and strided input, both outputs, with and without sr_y; the fall-back
    A, H, W = 3, 21, 19
    minv = (ctypes.c_double * 9)(*colour.inverse_matrix().reshape(-1))
    for dtype, strided in itertools.product(("uint8", "float32", "float64"), (False, True)):
        lf = field(dtype, (3, 3, W, H, 3)).permute(0, 1, 3, 2, 4) if strided else field(dtype, (3, 3, H, W, 3))
        show(f"luma {dtype} strided{int(strided)}", y=colour.luma(lf, A))
        for s, od, with_sr in itertools.product((2, 4), (torch.uint8, torch.float32), (False, True)):
            sr = dev(rng.uniform(-0.05, 1.05, (A * s * H, A * s * W)).astype(np.float32)) if with_sr else None
            show(f"merge {dtype} strided{int(strided)} s{s} {str(od)[6:]} sr{int(with_sr)}", out=colour.merge(lf, sr, A, s, od))
    lf = field("uint8", (2, 2, 40, 45, 3))
    for s, od, with_sr, (far_h, far_w) in itertools.product((2, 4), (torch.uint8, torch.float32), (False, True), ((True, True), (True, False), (False, True))):
        sr = dev(rng.uniform(-0.05, 1.05, (2 * s * 40, 2 * s * 45)).astype(np.float32)) if with_sr else None
        (wh, ih), (ww, iw) = far_table(*colour.up_contributions(40, s), 40, far_h), far_table(*colour.up_contributions(45, s), 45, far_w)
        out = torch.zeros(2, 2, s * 40, s * 45, 3, dtype=od, device=DEV)
        _lib.enqueue("lft_colour_merge", DEV, *prepare.lf_args(lf), 2, s, sr.data_ptr() if with_sr else None, wh.data_ptr(), ih.data_ptr(), wh.shape[1],
                     ww.data_ptr(), iw.data_ptr(), ww.shape[1], minv, out.data_ptr(), colour._OUT_CLASS[od])
        show(f"merge fallback s{s} {str(od)[6:]} sr{int(with_sr)} rows{int(far_h)} cols{int(far_w)}", out=out)

    def mosaics(B, A, h, w, lo=0.0):
        hr = rng.uniform(lo, 1.0, (B, 1, A * h, A * w)).astype(np.float32)
        return dev(np.clip(hr + 0.05 * rng.standard_normal(hr.shape), lo, 1.0).astype(np.float32)), dev(hr)

    # ---- view_metrics
    for (B, A, h, w), rng_ in itertools.product(((2, 3, 40, 33), (1, 5, 11, 17), (1, 2, 64, 64)), (1.0, 2.0)):
        sr, hr = mosaics(B, A, h, w, -1.0 if rng_ == 2.0 else 0.0)
        psnr, ssim = metrics.view_metrics(hr, sr, A, rng_)
        show(f"view_metrics B{B} A{A} {h}x{w} range{rng_}", psnr=psnr, ssim=ssim)

    # ---- l1_loss and lf_loss: A*W % 4 != 0 | W < 4 on the 16-byte path | W % 4 == 0
    for B, A, h, w in ((2, 2, 3, 3), (2, 4, 5, 3), (2, 2, 12, 8)):
        sr, hr = mosaics(B, A, h, w)
        n = sr.numel()
        for grad in (False, True):
            dsr, loss, scratch = torch.zeros_like(sr), torch.zeros(1, device=DEV), torch.zeros(1024, device=DEV)
            _lib.enqueue("lft_l1_loss", DEV, sr.data_ptr(), hr.data_ptr(), n, dsr.data_ptr() if grad else None, 1.0 / n, loss.data_ptr(), scratch.data_ptr())
            show(f"l1_loss B{B} A{A} {h}x{w} grad{int(grad)}", loss=loss, dsr=dsr)
            for pen in ("l1", "mse", "charbonnier"):
                dsr = torch.zeros_like(sr)
                loss3 = L.lf_loss(sr, hr, A, pen, 1e-3, 0.7, 0.4, dsr if grad else None, 0.37)
                show(f"lf_loss B{B} A{A} {h}x{w} {pen} grad{int(grad)}", loss3=loss3, dsr=dsr)

    # ---- ssim_loss
    for (B, A, h, w), grad, acc in itertools.product(SHAPES, (False, True), (False, True)):
        sr, hr = mosaics(B, A, h, w)
        dsr, total = torch.full_like(sr, 0.125), torch.full((1,), 0.25, device=DEV)
        total, S = L.ssim_loss(sr, hr, A, 1.0, 0.3, dsr if grad else None, 0.37, acc, total)
        show(f"ssim_loss B{B} A{A} {h}x{w} grad{int(grad)} acc{int(acc)}", total=total, S=S, dsr=dsr)

    # ---- Adam, the guarded step (aligned and offset by one float), the EMA
    n = 3 * 2048 + 1234 + 5 + 3
    segments = [(0, 2051, True), (2051, 1234, False), (3285, 5, True), (3290, n - 3290, True)]
    state = [rng.standard_normal(n + 1).astype(np.float32) * sc for sc in (1.0, 0.01, 0.1, 0.001)]
    state[3] = np.abs(state[3])

    def buffers(off):
        return [dev(x)[off:off + n] for x in state]

    p, g, m, v = buffers(0)
    for step in (1, 2):
        _lib.enqueue("lft_adam_step", DEV, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 2e-4, 0.9, 0.999, 1e-8, step, 0.5, 1e-4)
    show("adam_step", p=p, m=m, v=v)
    for off in (0, 1):
        p, g, m, v = buffers(off)
        ema = p.clone()                                                 # a fresh allocation: shares p's alignment at off 0 only
        guard = T.guard_new(segments, n, DEV)
        for what, max_norm in (("plain", None), ("clipped", 0.5), ("nan", 0.5), ("after", None)):
            if what == "nan":
                g[7], g[2100], g[n - 2] = float("nan"), float("inf"), float("-inf")       # 2100 lies in the frozen segment
            if what == "after":
                g.nan_to_num_(0.0, 0.0, 0.0)
            T.adam_step_guarded(p, g, m, v, guard, 2e-4, gscale=0.5, weight_decay=1e-4, max_norm=max_norm)
            T.ema_update(ema, p, 0.999, True, 0, guard)
            rep = T.guard_read(guard)
            show(f"adam_step_guarded off{off} {what}", p=p, m=m, v=v, ema=ema, report=torch.frombuffer(bytearray(bytes(rep)), dtype=torch.uint8))
        for warm, step in ((True, 3), (False, 50)):
            T.ema_update(ema, p, 0.999, warm, step)
            show(f"ema_update off{off} plain warm{int(warm)}", ema=ema)


MODES = {"--lightfield": ("--child-lightfield", child_lightfield), "--pipeline": ("--child-pipeline", child_pipeline)}

if __name__ == "__main__":
    children = {"--child": child, **{c: f for c, f in MODES.values()}}
    if len(sys.argv) > 1 and sys.argv[1] in children:
        children[sys.argv[1]]()
        raise SystemExit(0)
    mode = next((MODES[a][0] for a in sys.argv[1:] if a in MODES), "--child")
    outs = []
    for lib in (a for a in sys.argv[1:] if a not in MODES):
        env = dict(os.environ, LFT_LIB_PATH=os.path.abspath(lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=env, capture_output=True, text=True, cwd=ROOT)
        if r.returncode:
            raise SystemExit(f"{lib} failed:\n{r.stderr[-2000:]}")
        outs.append([l for l in r.stdout.splitlines() if l.startswith(("A", "P "))])
        print(lib)
        print("\n".join("   " + l for l in outs[-1]))
    same = all(o == outs[0] for o in outs[1:])
    print("bit-identical" if same else "DIFFERENT")
    raise SystemExit(0 if same else 1)
