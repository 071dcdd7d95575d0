"""Shared by tests/test_guard_host.py, tests/test_gpu_guard.py and tests/test_gpu_guard_train.py: the reference model of the guarded
Adam step (lft_adam_step_guarded), the cases it is checked on, and the tolerances.

Reference model: `ref_guarded_step` is torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam(foreach=False) over the TRAINABLE
tensors only, on the CPU in a chosen dtype; a non-finite total norm means no step at all (what error_if_nonfinite=False leaves to
the caller).  Hyper-parameters are the fp32 values that cross the C ABI (tests/test_gpu_loss_adam.py explains why that matters
for beta2); max_norm crosses it as a float too, so kernel and reference both get F32(max_norm).

Tolerances are measured, not invented: GUARD_LEVEL is what fp32 torch departs from fp64 torch on the very cases below
(test_guard_tolerances_are_4x_fp32_torch re-measures it without a GPU); the kernel is gated at 4 times that.  The data keeps
|g * gscale * coef + wd * p| >= 5e-3 (|g| >= 0.04, gscale 0.5, coef >= 0.5; wd |p| <= 5e-3), so that no element's first-step
direction hangs on rounding and fp32 torch itself stays inside the outlier rule of the `p` check."""
import numpy as np
import torch

F32 = lambda x: float(np.float32(x))                              # the value a `float` argument of the C ABI carries
LR, B1, B2, EPS, GSCALE = F32(2e-4), F32(0.9), F32(0.999), F32(1e-8), 0.5
GUARD_N = 100003                                                  # odd: the last block is partial
MODES = ("off", "twice", "half")                                 # max_norm: none; 2 x the norm (coef exactly 1); half the norm (coef ~0.5)
GUARD_CASES = [(step, wd, mode) for step in (1, 2, 1000) for wd in (0.0, F32(1e-2)) for mode in MODES]
CASE_IDS = [f"{s}-{w:.2g}-{m}" for s, w, m in GUARD_CASES]

# fp32 torch (clip_grad_norm_ + Adam) against fp64 torch over GUARD_CASES: max |p32 - p64| / lr (mostly the rounding of p itself),
# max |m32 - m64| / max|m|, the same for v (both largest at step 1 with the clip on: the fp32 coefficient is off by 1.3e-7 relative)
GUARD_LEVEL = {"p": 7.54e-5, "m": 1.93e-7, "v": 4.18e-7}
GUARD_TOL = {k: 4 * v for k, v in GUARD_LEVEL.items()}
OUTLIER_SHARE, OUTLIER_STEPS = 1e-3, 2.1                          # under 1e-3 of the elements beyond the p tolerance, each within 2.1 x the largest step


def table_from_counts(counts, frozen=()):
    """(first, count, trainable) triples tiling [0, sum(counts))."""
    segs, off = [], 0
    for i, c in enumerate(counts):
        segs.append((off, int(c), 0 if i in frozen else 1))
        off += int(c)
    return segs


# segments that begin at float offsets 1, 3 and 7 (and every other residue mod 4 further on), lengths 1, 2, 63, 64, 65 and 4097
ODD_COUNTS = [1, 2, 4, 63, 64, 65, 4097, 3, 4097, 65, 2, 1, 64, 63, 5]
CLIP_COUNTS = [1, 4097, 63, 30001, GUARD_N - 1 - 4097 - 63 - 30001]      # the table of the clipped-step cases: odd starts, several blocks


def real_table(s, frozen=()):
    """The 78-segment table of the network's flat buffer (state-dict order), as TrainStep builds it."""
    from lft_amd.params import param_table
    return table_from_counts([int(np.prod(sh)) for _, sh, _ in param_table(64, s)], frozen)


def guard_data(step, wd, mode, counts=CLIP_COUNTS):
    """p, g, m, v (fp32 numpy) before Adam step number `step`, the segment table and max_norm (None = clipping off)."""
    n = sum(counts)
    rng = np.random.default_rng(7000 * step + int(wd * 1e4) + 13 * MODES.index(mode))
    p = np.clip(0.1 * rng.standard_normal(n), -0.5, 0.5).astype(np.float32)
    g = (rng.uniform(0.04, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    if step == 1:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:                                                         # a plausible history: moments of earlier gradients
        m = (0.3 * rng.standard_normal(n)).astype(np.float32)
        v = (rng.uniform(0.01, 1.0, n) ** 2 * 0.25).astype(np.float32)
    norm = GSCALE * float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    max_norm = {"off": None, "twice": F32(2.0 * norm), "half": F32(0.5 * norm)}[mode]
    return p, g, m, v, table_from_counts(counts), max_norm


def ref_guarded_step(p, g, m, v, segments, step, wd, max_norm, dtype, gscale=GSCALE, lr=LR):
    """clip_grad_norm_ + torch.optim.Adam(foreach=False) over the trainable segments, step number `step`, in `dtype` on the CPU.
    p, g, m, v: flat fp32 numpy.  Returns ((p, m, v) as float64 numpy, frozen segments unchanged), info = dict(norm, coef, skipped)."""
    params, opt_state = [], []
    for first, count, trainable in segments:
        if not trainable:
            continue
        sl = slice(first, first + count)
        t = torch.from_numpy(p[sl].copy()).to(dtype).requires_grad_(True)
        t.grad = torch.from_numpy(g[sl].copy()).to(dtype) * gscale
        params.append(t)
        opt_state.append((sl, torch.from_numpy(m[sl].copy()).to(dtype), torch.from_numpy(v[sl].copy()).to(dtype)))
    out = [a.astype(np.float64) for a in (p, m, v)]
    total = torch.nn.utils.clip_grad_norm_(params, float("inf") if max_norm is None else max_norm, foreach=False)
    norm = float(total)
    if not np.isfinite(norm):
        return out, {"norm": norm, "coef": 0.0, "skipped": True}
    coef = 1.0 if max_norm is None else min(1.0, max_norm / (norm + 1e-6))
    opt = torch.optim.Adam(params, lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
    for t, (_, mm, vv) in zip(params, opt_state):
        opt.state[t] = {"step": torch.tensor(float(step - 1)), "exp_avg": mm, "exp_avg_sq": vv}
    opt.step()
    for t, (sl, _, _) in zip(params, opt_state):
        st = opt.state[t]
        assert int(st["step"]) == step
        out[0][sl] = t.detach().double().numpy()
        out[1][sl] = st["exp_avg"].double().numpy()
        out[2][sl] = st["exp_avg_sq"].double().numpy()
    return out, {"norm": norm, "coef": coef, "skipped": False}


def step_errors(got, ref, lr=LR):
    """got, ref = (p, m, v) float64: the three figures the tolerances are written in."""
    return {"p": float(np.abs(got[0] - ref[0]).max() / lr),
            "m": float(np.abs(got[1] - ref[1]).max() / np.abs(ref[1]).max()),
            "v": float(np.abs(got[2] - ref[2]).max() / np.abs(ref[2]).max())}


def outliers(got_p, ref_p, p0, tol_p, lr=LR):
    """(share of elements whose p error exceeds tol_p * lr, whether each of those is within OUTLIER_STEPS x the largest step)."""
    err = np.abs(got_p - ref_p)
    out = err / lr > tol_p
    stepmax = float(np.abs(ref_p - p0).max())
    return float(out.mean()), bool(np.all(err[out] <= OUTLIER_STEPS * stepmax))


def check_step(got, ref, p0, what, lr=LR):
    """The gate of a guarded step against its fp64 reference: m and v at GUARD_TOL, p at GUARD_TOL with the outlier rule."""
    e = step_errors(got, ref, lr)
    share, bounded = outliers(got[0], ref[0], p0, GUARD_TOL["p"], lr)
    print(f"{what}: vs fp64 reference {e}; outlier share {share:.2e}; tolerances {GUARD_TOL}")
    assert e["m"] <= GUARD_TOL["m"] and e["v"] <= GUARD_TOL["v"], (what, e)
    assert share < OUTLIER_SHARE and bounded, (what, share, bounded, e)
    return e
