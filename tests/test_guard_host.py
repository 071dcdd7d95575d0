"""CPU: the guarded Adam step's C ABI (declarations, exports, argument errors before any device work), the reference model the GPU
tests use, and the measurement behind their tolerances (tests/guard_util.py)."""
import ctypes
import os
import re

import numpy as np
import torch

from lft_amd import _lib

import guard_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lft_guard_bytes", "lft_guard_init", "lft_adam_step_guarded", "lft_guard_read")
ERR_ARG, ERR_SHAPE = -1, -2


def test_header_declares_and_library_exports_the_guard_entry_points():
    hdr = open(os.path.join(ROOT, "include", "lft_hip.h")).read()
    declared = set(re.findall(r"^int\s+(lft_\w+)\s*\(", hdr, flags=re.M))
    assert set(NAMES) <= declared and set(NAMES) <= set(_lib.EXPORTS) and set(NAMES) == set(_lib.GUARD_EXPORTS)
    assert "typedef struct { long long first, count; int trainable; } lft_segment;" in hdr
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
    assert _lib.lib().lft_version() == 5                                       # additive: the ABI version does not change
    # the ctypes mirrors have the C layout: 24-byte segments, a report of 48 bytes + 128 floats without padding
    assert ctypes.sizeof(_lib.GuardSegment) == 24 and ctypes.sizeof(_lib.GuardReport) == 48 + 4 * 128
    assert _lib.GuardReport.seg_norm.offset == 48 and _lib.GuardReport.nonfinite_last.offset == 16


def segs_of(table):
    return (_lib.GuardSegment * len(table))(*[_lib.GuardSegment(*t) for t in table])


def test_argument_errors_come_before_any_device_work():
    """Every call below must be refused on the host: nothing is dereferenced on a device, nothing is launched (this runs without a GPU)."""
    L = _lib.lib()
    nb = ctypes.c_size_t(0)
    assert L.lft_guard_bytes(78, ctypes.byref(nb)) == 0 and 1024 <= nb.value < 1 << 20 and nb.value % 16 == 0
    small = nb.value
    assert L.lft_guard_bytes(128, ctypes.byref(nb)) == 0 and nb.value > small
    assert L.lft_guard_bytes(0, ctypes.byref(nb)) == ERR_ARG and L.lft_guard_bytes(129, ctypes.byref(nb)) == ERR_ARG
    assert L.lft_guard_bytes(78, None) == ERR_ARG
    good = U.table_from_counts([3, 5, 2])
    G = 4096                                                                   # a 16-byte aligned address that is never dereferenced
    assert L.lft_guard_init(None, segs_of(good), 3, 10, 0, None) == ERR_ARG
    assert L.lft_guard_init(G, None, 3, 10, 0, None) == ERR_ARG
    assert L.lft_guard_init(G + 4, segs_of(good), 3, 10, 0, None) == ERR_ARG and b"aligned" in L.lft_last_error()
    assert L.lft_guard_init(G, segs_of(good), 0, 10, 0, None) == ERR_ARG
    assert L.lft_guard_init(G, segs_of(good * 43), 129, 10, 0, None) == ERR_ARG
    assert L.lft_guard_init(G, segs_of(good), 3, 10, -1, None) == ERR_ARG
    bad_tables = {"gap": [(0, 3, 1), (4, 4, 1), (8, 2, 1)], "overlap": [(0, 3, 1), (2, 6, 1), (8, 2, 1)],
                  "descending": [(5, 5, 1), (0, 5, 1)], "first not 0": [(1, 9, 1)], "empty segment": [(0, 3, 1), (3, 0, 1), (3, 7, 1)],
                  "short": [(0, 3, 1), (3, 5, 1)], "long": [(0, 3, 1), (3, 8, 1)], "negative": [(0, -3, 1), (-3, 13, 1)]}
    for what, table in bad_tables.items():
        assert L.lft_guard_init(G, segs_of(table), len(table), 10, 0, None) == ERR_SHAPE, what
    assert L.lft_guard_init(G, segs_of(good), 3, 0, 0, None) == ERR_SHAPE
    P = 8192
    args = (10, U.LR, U.B1, U.B2, U.EPS, 1.0, 0.0)
    for i in range(4):                                                         # a null p, g, m or v
        ptrs = [P] * 4
        ptrs[i] = None
        assert L.lft_adam_step_guarded(*ptrs, *args, 1.0, G, None) == ERR_ARG
    assert L.lft_adam_step_guarded(P, P, P, P, *args, 1.0, None, None) == ERR_ARG
    assert L.lft_adam_step_guarded(P, P, P, P, *args, float("nan"), G, None) == ERR_ARG and b"NaN" in L.lft_last_error()
    assert L.lft_adam_step_guarded(P, P, P, P, 10, U.LR, U.B1, U.B2, U.EPS, 1.0, -0.1, 1.0, G, None) == ERR_ARG      # weight decay >= 0
    # a block lft_guard_init never wrote (the n check against an initialised block needs a device: tests/test_gpu_guard.py)
    assert L.lft_adam_step_guarded(P, P, P, P, *args, 1.0, G, None) == ERR_ARG and b"not initialised" in L.lft_last_error()
    rep = _lib.GuardReport()
    assert L.lft_guard_read(None, None, ctypes.byref(rep)) == ERR_ARG and L.lft_guard_read(G, None, None) == ERR_ARG
    assert L.lft_guard_read(G, None, ctypes.byref(rep)) == ERR_ARG             # not initialised either


def test_reference_model_clips_freezes_and_skips():
    """ref_guarded_step is what it says: against formulas written out in numpy (fp64) on a tiny table with a frozen segment."""
    rng = np.random.default_rng(5)
    table = U.table_from_counts([3, 4, 5], frozen=(1,))
    p, g = rng.standard_normal(12).astype(np.float32), rng.standard_normal(12).astype(np.float32)
    m, v = rng.standard_normal(12).astype(np.float32), (rng.random(12) + 0.1).astype(np.float32)
    tr = np.r_[0:3, 7:12]
    norm = U.GSCALE * np.sqrt((g[tr].astype(np.float64) ** 2).sum())
    mx, wd, t = U.F32(0.25 * norm), U.F32(1e-2), 7
    (rp, rm, rv), info = U.ref_guarded_step(p, g, m, v, table, t, wd, mx, torch.float64)
    assert not info["skipped"] and abs(info["norm"] - norm) <= 1e-12 * norm
    coef = mx / (norm + 1e-6)
    assert abs(info["coef"] - coef) <= 1e-15 and coef < 1
    p64, m64, v64 = (a.astype(np.float64) for a in (p, m, v))
    gi = g.astype(np.float64) * U.GSCALE * coef + wd * p64
    em, ev = U.B1 * m64 + (1 - U.B1) * gi, U.B2 * v64 + (1 - U.B2) * gi * gi
    ep = p64 - U.LR / (1 - U.B1 ** t) * em / (np.sqrt(ev) / np.sqrt(1 - U.B2 ** t) + U.EPS)
    for got, exp, old in ((rp, ep, p), (rm, em, m), (rv, ev, v)):
        assert np.allclose(got[tr], exp[tr], rtol=1e-11, atol=0)
        assert np.array_equal(got[3:7], old[3:7].astype(np.float64))           # the frozen segment
    g2 = g.copy()
    g2[4] = np.nan                                                             # in the frozen segment: ignored
    assert not U.ref_guarded_step(p, g2, m, v, table, t, wd, mx, torch.float64)[1]["skipped"]
    for bad in (np.nan, np.inf, -np.inf):                                      # in a trainable one: no step
        g2 = g.copy()
        g2[8] = bad
        (sp, sm, sv), info = U.ref_guarded_step(p, g2, m, v, table, t, wd, mx, torch.float64)
        assert info["skipped"] and np.array_equal(sp, p.astype(np.float64)) and np.array_equal(sm, m.astype(np.float64)) and np.array_equal(sv, v.astype(np.float64))


def test_guard_tolerances_are_4x_fp32_torch():
    """No GPU: GUARD_LEVEL is what fp32 torch (clip_grad_norm_ + Adam) shows against fp64 torch on the very cases of the GPU test, and
    fp32 torch itself stays inside the outlier rule on them (the data keeps the clipped gradient away from zero)."""
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for step, wd, mode in U.GUARD_CASES:
        p, g, m, v, table, mx = U.guard_data(step, wd, mode)
        coef = 0.5 if mode == "half" else 1.0
        assert np.abs(g.astype(np.float64) * U.GSCALE * coef + wd * p).min() >= 5e-3
        r64, i64 = U.ref_guarded_step(p, g, m, v, table, step, wd, mx, torch.float64)
        r32, i32 = U.ref_guarded_step(p, g, m, v, table, step, wd, mx, torch.float32)
        assert i64["coef"] == 1.0 if mode != "half" else abs(i64["coef"] - 0.5) < 1e-6
        e = U.step_errors(r32, r64)
        share, bounded = U.outliers(r32[0], r64[0], p.astype(np.float64), U.GUARD_TOL["p"])
        print(f"step {step} wd {wd} {mode}: fp32 torch vs fp64 torch {e}, outlier share {share:.2e}")
        assert share < U.OUTLIER_SHARE and bounded
        worst = {k: max(worst[k], e[k]) for k in worst}
    for k in worst:
        assert U.GUARD_LEVEL[k] / 2 <= worst[k] <= U.GUARD_LEVEL[k] * 1.001, (k, worst[k], U.GUARD_LEVEL[k])
