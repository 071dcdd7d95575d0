"""lft_adam_step_guarded / lft_guard_init / lft_guard_read called through the C ABI on the GPU (tests/guard_util.py has the reference
model, the cases and the measured tolerances).

The kernels give one block at most 2 048 consecutive floats of one segment (kGuardChunk of lft_amd/csrc/lft_optim.cuh; more only
beyond 2 048 * 2 048 floats), split into a scalar head up to the first 16-byte boundary, 16-byte accesses and a scalar tail.  The
shapes below sit on every side of those: single segments around the wave (64), the block (256) and the chunk (2 047 | 2 048 |
2 049), one buffer beyond 2 048 chunks (the chunk grows), a table whose segments start at float offsets 1, 3 and 7, buffers whose
base addresses differ in alignment (the scalar path of the update), and the network's own 78-segment tables.
Every buffer has 64 floats of 7.0 behind it that must stay; the gradient buffer must keep its bits."""
import ctypes

import numpy as np
import pytest
import torch

from lft_amd import _lib
from lft_amd import train as T

import gpu_util as G
import guard_util as U

PAD = 64
EPS23 = 2.0 ** -23


class Bufs:
    """p, g, m, v on the device, each `offset[i]` floats into an allocation of its own and followed by PAD floats of 7.0."""

    def __init__(self, p, g, m, v, offsets=(0, 0, 0, 0)):
        self.n = len(p)
        self.raw, self.t = [], []
        for a, off in zip((p, g, m, v), offsets):
            raw = torch.full((off + self.n + PAD,), 7.0, device=G.DEV)
            raw[off:off + self.n] = torch.from_numpy(a).to(G.DEV)
            self.raw.append(raw)
            self.t.append(raw[off:off + self.n])
        self.offsets = offsets

    def step(self, guard, wd, max_norm, gscale=U.GSCALE, lr=U.LR):
        T.adam_step_guarded(self.t[0], self.t[1], self.t[2], self.t[3], guard, lr, U.B1, U.B2, U.EPS, gscale, wd, max_norm)

    def set_g(self, g):
        self.t[1].copy_(torch.from_numpy(g).to(G.DEV))

    def host(self):
        """(p, g, m, v) as fp32 numpy, after checking the 7.0 around each of them."""
        out = []
        for raw, off in zip(self.raw, self.offsets):
            a = raw.cpu().numpy()
            assert np.all(a[:off] == 7.0) and np.all(a[off + self.n:] == 7.0), "wrote outside [0, n)"
            out.append(a[off:off + self.n].copy())
        return out

    def pmv64(self):
        p, _, m, v = self.host()
        return [a.astype(np.float64) for a in (p, m, v)]


def same_bits(a, b):
    return np.array_equal(a.view(np.int32), b.view(np.int32))


def ref_norms(g, table, gscale=U.GSCALE):
    """fp64 numpy: (norm over the trainable segments, norm of every segment, non-finite count over the trainable segments, first bad
    trainable segment or -1); non-finite elements are left out of the sums."""
    g64 = g.astype(np.float64)
    fin = np.isfinite(g64)
    sq = np.where(fin, g64, 0.0) ** 2
    seg, tot, bad, bad_seg = [], 0.0, 0, -1
    for i, (first, count, trainable) in enumerate(table):
        ss = float(sq[first:first + count].sum())
        seg.append(gscale * np.sqrt(ss))
        if trainable:
            tot += ss
            nb = int((~fin[first:first + count]).sum())
            if nb and bad_seg < 0:
                bad_seg = i
            bad += nb
    return gscale * np.sqrt(tot), np.array(seg), bad, bad_seg


def check_norms(rep, g, table, what):
    norm, seg, bad, bad_seg = ref_norms(g, table)
    got_seg = np.array(rep.seg_norm[:len(table)], dtype=np.float64)
    rel = abs(rep.grad_norm - norm) / norm if norm else abs(rep.grad_norm)
    rel_seg = np.abs(got_seg - seg) / np.where(seg > 0, seg, 1.0)
    print(f"{what}: grad_norm {rep.grad_norm:.9g} (fp64 {norm:.9g}, rel {rel:.2e}); worst seg_norm rel {rel_seg.max():.2e} of {len(table)}")
    assert rel <= EPS23 and rel_seg.max() <= EPS23, (what, rel, rel_seg.max())
    assert all(x == 0.0 for x in rep.seg_norm[len(table):])
    assert rep.nonfinite_last == bad and rep.bad_segment == bad_seg


STAT_SHAPES = {f"single-{n}": [n] for n in (1, 63, 255, 256, 257, 2047, 2048, 2049, 100003, 2048 * 2048 + 4099)}
STAT_SHAPES["odd-table"] = U.ODD_COUNTS
STAT_SHAPES["real-2x"] = [c for _, c, _ in U.real_table(2)]
STAT_SHAPES["real-4x"] = [c for _, c, _ in U.real_table(4)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(STAT_SHAPES))
def test_gradient_statistics_match_fp64(shape):
    counts = STAT_SHAPES[shape]
    n = sum(counts)
    assert n == {"real-2x": 1_114_240, "real-4x": 1_163_392}.get(shape, n)
    table = U.table_from_counts(counts)
    rng = np.random.default_rng(n)
    g = rng.standard_normal(n).astype(np.float32)
    for i, (first, count, _) in enumerate(table):                             # segments of very different sizes, as real layers have
        g[first:first + count] *= np.float32(10.0 ** ((i % 7) - 3))
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    b = Bufs(p, g, np.zeros(n, np.float32), np.zeros(n, np.float32))
    guard = T.guard_new(table, n, G.DEV)
    b.step(guard, 0.0, None)
    rep = T.guard_read(guard)
    check_norms(rep, g, table, shape)
    hp, hg, hm, hv = b.host()
    assert same_bits(hg, g), "the gradient buffer changed"
    assert rep.skipped_last == 0 and rep.steps_applied == 1 and rep.steps_skipped == 0 and rep.steps_clipped == 0 and rep.clip_coef == 1.0
    # first step from zero moments moves every weight by lr (to within eps / |g|): no element was left out, none stepped twice
    moved = np.abs(hp.astype(np.float64) - p) / U.LR
    big = np.abs(g) * U.GSCALE > 1e-4
    assert np.all(np.abs(moved[big] - 1.0) < 1e-3 + 4e-8 / U.LR), (moved[big].min(), moved[big].max())
    assert np.all(hv >= 0) and np.all((hm != 0) == (g != 0))


@pytest.mark.gpu
@pytest.mark.parametrize("step,wd,mode", U.GUARD_CASES, ids=U.CASE_IDS)
def test_clipped_step_matches_fp64_reference(step, wd, mode):
    p, g, m, v, table, mx = U.guard_data(step, wd, mode)
    n = len(p)
    ref, info = U.ref_guarded_step(p, g, m, v, table, step, wd, mx, torch.float64)
    b = Bufs(p, g, m, v)
    guard = T.guard_new(table, n, G.DEV, steps_applied0=step - 1)
    b.step(guard, wd, mx)
    rep = T.guard_read(guard)
    check_norms(rep, g, table, f"step {step} wd {wd} {mode}")
    assert same_bits(b.host()[1], g), "the gradient buffer changed"
    rel = abs(rep.clip_coef - info["coef"]) / info["coef"]
    print(f"clip_coef {rep.clip_coef:.9g} (fp64 {info['coef']:.12g}, rel {rel:.2e})")
    assert rel <= EPS23
    if mode != "half":
        assert rep.clip_coef == 1.0
    assert rep.steps_clipped == (1 if mode == "half" else 0) and rep.steps_applied == step and rep.skipped_last == 0 and rep.steps_skipped == 0
    U.check_step(b.pmv64(), ref, p.astype(np.float64), f"step {step} wd {wd} {mode}")
    if mode != "half":                                                        # reported, not gated: coef == 1 against the unguarded kernel
        u = Bufs(p, g, m, v)
        _lib.call("lft_adam_step", u.t[0].data_ptr(), u.t[1].data_ptr(), u.t[2].data_ptr(), u.t[3].data_ptr(), n, U.LR, U.B1, U.B2, U.EPS, step,
                  U.GSCALE, wd, G.stream())
        diff = [int((x.view(np.int32) != y.view(np.int32)).sum()) for x, y in zip(b.host(), u.host())]
        print(f"elements that differ from lft_adam_step on the same inputs (p, g, m, v): {diff} of {n}")


@pytest.mark.gpu
def test_buffers_of_different_alignment_take_the_scalar_path():
    """p, g, m, v that start 1, 2, 3 and 1 floats into their allocations share no 16-byte phase: the statistics' head / tail logic
    works from g's own address, the update falls back to scalar accesses; same gates as the aligned case."""
    step, wd, mode = 2, U.F32(1e-2), "half"
    p, g, m, v, table, mx = U.guard_data(step, wd, mode)
    ref, info = U.ref_guarded_step(p, g, m, v, table, step, wd, mx, torch.float64)
    b = Bufs(p, g, m, v, offsets=(1, 2, 3, 1))
    guard = T.guard_new(table, len(p), G.DEV, steps_applied0=step - 1)
    b.step(guard, wd, mx)
    rep = T.guard_read(guard)
    check_norms(rep, g, table, "misaligned")
    assert same_bits(b.host()[1], g)
    U.check_step(b.pmv64(), ref, p.astype(np.float64), "misaligned")
    same = Bufs(p, g, m, v, offsets=(3, 3, 3, 3))                             # a common phase other than 0: 16-byte accesses again
    guard2 = T.guard_new(table, len(p), G.DEV, steps_applied0=step - 1)
    same.step(guard2, wd, mx)
    check_norms(T.guard_read(guard2), g, table, "common phase 3")
    U.check_step(same.pmv64(), ref, p.astype(np.float64), "common phase 3")


@pytest.mark.gpu
def test_frozen_segments_are_left_alone_and_ignored():
    step, wd = 2, U.F32(1e-2)
    p, g, m, v, _, _ = U.guard_data(step, wd, "half", counts=U.ODD_COUNTS)
    frozen = tuple(range(0, len(U.ODD_COUNTS), 3))
    table = U.table_from_counts(U.ODD_COUNTS, frozen)
    n = len(p)
    norm_tr, seg, _, _ = ref_norms(g, table)
    norm_all = ref_norms(g, U.table_from_counts(U.ODD_COUNTS))[0]
    assert norm_tr < 0.999 * norm_all                                         # the frozen ones would show in the norm
    mx = U.F32(0.5 * norm_tr)
    ref, info = U.ref_guarded_step(p, g, m, v, table, step, wd, mx, torch.float64)
    b = Bufs(p, g, m, v)
    guard = T.guard_new(table, n, G.DEV, steps_applied0=step - 1)
    b.step(guard, wd, mx)
    rep = T.guard_read(guard)
    check_norms(rep, g, table, "frozen")                                      # grad_norm without, seg_norm with the frozen segments
    assert all(rep.seg_norm[i] > 0 for i in frozen)
    assert abs(rep.clip_coef - info["coef"]) <= EPS23 * info["coef"] and rep.steps_clipped == 1
    hp, hg, hm, hv = b.host()
    for i in frozen:
        sl = slice(table[i][0], table[i][0] + table[i][1])
        assert same_bits(hp[sl], p[sl]) and same_bits(hm[sl], m[sl]) and same_bits(hv[sl], v[sl]), f"frozen segment {i} changed"
    live = np.concatenate([np.arange(first, first + count) for first, count, trainable in table if trainable])
    assert (hp[live] != p[live]).mean() > 0.99                                # the others did step (a p may move by less than its ulp)
    U.check_step(b.pmv64(), ref, p.astype(np.float64), "frozen")
    # a NaN (and an inf) in frozen segments: no skip, the same bits as without them
    g2 = g.copy()
    g2[table[3][0]] = np.nan
    g2[table[6][0] + 2048] = np.inf
    b2 = Bufs(p, g2, m, v)
    guard2 = T.guard_new(table, n, G.DEV, steps_applied0=step - 1)
    b2.step(guard2, wd, mx)
    rep2 = T.guard_read(guard2)
    assert rep2.skipped_last == 0 and rep2.steps_skipped == 0 and rep2.steps_applied == step and rep2.nonfinite_last == 0 and rep2.bad_segment == -1
    check_norms(rep2, g2, table, "frozen with NaN")
    for x, y in zip(b2.host(), (hp, g2, hm, hv)):
        assert same_bits(x, y)


SKIP_T = 5                                                                    # the step number the clean call must carry
BLOCK_EDGE = 199 + 2048                                                       # ODD table: segment 6 starts at 199, its second block here


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
def test_nonfinite_gradient_skips_the_step(bad):
    wd = U.F32(1e-2)
    p, g, m, v, table, mx = U.guard_data(SKIP_T, wd, "half", counts=U.ODD_COUNTS)
    n = len(p)
    ref, _ = U.ref_guarded_step(p, g, m, v, table, SKIP_T, wd, mx, torch.float64)          # step number t, NOT t + 1
    spots = {"element 0": (0, 0), "last element": (n - 1, len(table) - 1), "end of a block": (BLOCK_EDGE - 1, 6),
             "start of a block": (BLOCK_EDGE, 6), "first of the segment at offset 7": (7, 3)}
    assert table[3][0] == 7 and table[6][0] == 199 and table[6][1] > 2048
    for what, (at, seg) in spots.items():
        b = Bufs(p, g, m, v)
        guard = T.guard_new(table, n, G.DEV, steps_applied0=SKIP_T - 1)
        g2 = g.copy()
        g2[at] = bad
        b.set_g(g2)
        b.step(guard, wd, mx)
        rep = T.guard_read(guard)
        hp, hg, hm, hv = b.host()
        assert same_bits(hp, p) and same_bits(hm, m) and same_bits(hv, v), f"{what}: a skipped step changed p, m or v"
        assert same_bits(hg, g2)
        assert rep.skipped_last == 1 and rep.steps_skipped == 1 and rep.steps_applied == SKIP_T - 1 and rep.steps_clipped == 0, what
        assert rep.bad_segment == seg and rep.nonfinite_last == 1, (what, rep.bad_segment, rep.nonfinite_last)
        check_norms(rep, g2, table, what)                                     # the finite elements' norm is still reported
        b.set_g(g)                                                            # the next, clean, batch
        b.step(guard, wd, mx)
        rep = T.guard_read(guard)
        assert rep.skipped_last == 0 and rep.steps_skipped == 1 and rep.steps_applied == SKIP_T and rep.steps_clipped == 1, what
        assert rep.bad_segment == -1 and rep.nonfinite_last == 0
        U.check_step(b.pmv64(), ref, p.astype(np.float64), f"clean call after a skip ({what})")
    # several at once: all counted, the first segment named
    b = Bufs(p, g, m, v)
    guard = T.guard_new(table, n, G.DEV, steps_applied0=SKIP_T - 1)
    g2 = g.copy()
    g2[[table[4][0] + 1, table[8][0], n - 1]] = bad
    b.set_g(g2)
    b.step(guard, wd, mx)
    rep = T.guard_read(guard)
    assert rep.skipped_last == 1 and rep.nonfinite_last == 3 and rep.bad_segment == 4


def sequence_data():
    """Four gradient buffers of one run on the ODD table: clean, clipped harder, poisoned, clean."""
    wd = U.F32(1e-2)
    p, g, m, v, table, mx = U.guard_data(2, wd, "half", counts=U.ODD_COUNTS)
    rng = np.random.default_rng(99)
    gs = [g, (3.0 * g).astype(np.float32), g.copy(), rng.permutation(g)]
    gs[2][4000] = np.nan
    return p, gs, m, v, table, mx, wd


def run_sequence(replay=None):
    p, gs, m, v, table, mx, wd = sequence_data()
    b = Bufs(p, gs[0], m, v)
    guard = T.guard_new(table, len(p), G.DEV, steps_applied0=1)
    graph = None
    if replay:                                                                # the call captured once (a linear graph), nothing runs yet
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode=T.CAPTURE_MODE):
            b.step(guard, wd, mx)
    reports = []
    for g in gs:
        b.set_g(g)
        if graph is None:
            b.step(guard, wd, mx)
        else:
            graph.replay()
        reports.append(bytes(T.guard_read(guard)))
    return b.host(), reports


@pytest.mark.gpu
def test_two_runs_and_a_captured_call_give_the_same_bits():
    first, rep1 = run_sequence()
    second, rep2 = run_sequence()
    for x, y in zip(first, second):
        assert same_bits(x, y), "two runs of the same sequence differ"
    assert rep1 == rep2
    last = _lib.GuardReport.from_buffer_copy(rep1[-1])
    assert last.steps_applied == 4 and last.steps_skipped == 1 and last.steps_clipped == 3
    replayed, rep3 = run_sequence(replay=True)
    for x, y in zip(first, replayed):
        assert same_bits(x, y), "a replayed capture differs from the eager calls"
    assert rep1 == rep3


@pytest.mark.gpu
def test_another_n_than_the_blocks_is_refused():
    table = U.table_from_counts([60, 40])
    guard = T.guard_new(table, 100, G.DEV)
    x = torch.zeros(100, device=G.DEV)
    L = _lib.lib()
    rc = L.lft_adam_step_guarded(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 99, U.LR, U.B1, U.B2, U.EPS, 1.0, 0.0, 0.0,
                                 guard.data_ptr(), G.stream())
    assert rc == -2 and b"initialised for 100" in L.lft_last_error()
    assert T.guard_read(guard).steps_applied == 0                             # nothing was launched
