"""lft_ema_update called through the C ABI on the GPU: ema += a * (p - ema), a = (float)(1 - d_t), guarded and unguarded.

Reference: the same recurrence in fp64 numpy with the SAME a (the float the kernel forms from d_t in double).  Tolerance, derived:
the kernel rounds three times per element and step (p - ema, a * that, the sum; two with an FMA), each on a magnitude <= 2 M with M
the largest |p| or |ema| seen, so at most 4 * 2^-24 * M per step; the recurrence contracts earlier errors by d_t <= 1, so after K
steps |ema - ref| <= K * 4 * 2^-24 * M.  (A numpy fp32 restatement stays below 0.06 of that for decay 0.5, 0.9, 0.999.)

The guarded form reads its step number from the guard block.  The tests advance that counter with lft_adam_step_guarded on a ZERO
gradient: with zero moments such a step is exactly p -= 0, so p is whatever the test wrote and only steps_applied moves.
Every buffer sits `offset` floats into its allocation between floats of 7.0 that must stay."""
import ctypes

import numpy as np
import pytest
import torch

from lft_amd import _lib
from lft_amd import train as T

import gpu_util as G
import guard_util as U

pytestmark = pytest.mark.gpu

PAD = 64
K = 24
STEP_ERR = 4 * 2.0 ** -24                                                     # per step, times M


def d_t(decay, warmup, t):
    d = float(np.float32(decay))
    return min(d, (1.0 + t) / (10.0 + t)) if warmup else d


def alpha(decay, warmup, t):
    return float(np.float32(1.0 - d_t(decay, warmup, t)))


class Buf:
    """n floats on the device, `offset` floats into an allocation of 7.0 with PAD more of them behind."""

    def __init__(self, a, offset=0):
        self.n, self.offset = len(a), offset
        self.raw = torch.full((offset + self.n + PAD,), 7.0, device=G.DEV)
        self.t = self.raw[offset:offset + self.n]
        self.set(a)

    def set(self, a):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(G.DEV))

    def host(self):
        a = self.raw.cpu().numpy()
        assert np.all(a[:self.offset] == 7.0) and np.all(a[self.offset + self.n:] == 7.0), "wrote outside [0, n)"
        return a[self.offset:self.offset + self.n].copy()


class Run:
    """ema and p (and, guarded, zero g / m / v with a guard block) for one sequence of updates."""

    def __init__(self, ema0, p0, table=None, steps0=0, offsets=(0, 0)):
        n = len(ema0)
        self.ema, self.p = Buf(ema0, offsets[0]), Buf(p0, offsets[1])
        self.guard = None
        if table is not None:
            self.zero = [Buf(np.zeros(n, np.float32), offsets[1]) for _ in range(3)]
            self.guard = T.guard_new(table, n, G.DEV, steps_applied0=steps0)

    def count(self, g=None):
        """One guarded Adam step on g (default: zeros, which moves nothing but the counter)."""
        if g is not None:
            self.zero[0].set(g)
        T.adam_step_guarded(self.p.t, self.zero[0].t, self.zero[1].t, self.zero[2].t, self.guard, U.LR, U.B1, U.B2, U.EPS, 1.0, 0.0, None)

    def update(self, decay, warmup, step):
        if self.guard is not None:
            self.count()
        T.ema_update(self.ema.t, self.p.t, decay, warmup, step, self.guard)


def same_bits(a, b):
    return np.array_equal(a.view(np.int32), b.view(np.int32))


def data(n, seed):
    rng = np.random.default_rng(seed)
    ema0 = rng.standard_normal(n).astype(np.float32)
    ps = [(rng.standard_normal(n) * (1.0 + 0.1 * k)).astype(np.float32) for k in range(K)]
    return ema0, ps


def run_sequence(ema0, ps, table, guarded, decay, warmup, steps0, offsets=(0, 0), frozen=()):
    """K updates with changing p; returns (ema on the host, fp64 reference, M)."""
    run = Run(ema0, ps[0], table if guarded else None, steps0, offsets)
    ref = ema0.astype(np.float64)
    live = np.ones(len(ema0), bool)
    for i in frozen:
        live[table[i][0]:table[i][0] + table[i][1]] = False
    M = float(np.abs(ema0).max())
    for k, p in enumerate(ps):
        t = steps0 + k + 1
        run.p.set(p)
        run.update(decay, warmup, 987654 if guarded else t)                    # guarded: the argument must be ignored
        a = alpha(decay, warmup, t)
        ref[live] += a * (p.astype(np.float64)[live] - ref[live])
        M = max(M, float(np.abs(p).max()), float(np.abs(ref).max()))
    got = run.ema.host()
    assert same_bits(run.p.host(), ps[-1]), "p was written"
    if guarded:
        rep = T.guard_read(run.guard)
        assert rep.steps_applied == steps0 + len(ps) and rep.steps_skipped == 0
    return got, ref, M


def check(got, ref, M, steps, what):
    err = float(np.abs(got.astype(np.float64) - ref).max())
    tol = steps * STEP_ERR * M
    print(f"{what}: max |ema - fp64| {err:.3e}, bound {tol:.3e} (K {steps}, M {M:.3g}): {err / tol:.3f} of it")
    assert np.all(np.isfinite(got)) and err <= tol, (what, err, tol)


SHAPES = {f"single-{n}": [n] for n in (1, 3, 4, 5, 2047, 2048, 2049, 4099)}
SHAPES["odd-table"] = U.ODD_COUNTS                                            # boundaries on every residue mod 4
OFFSETS = {"aligned": (0, 0), "ema-one-float-off": (1, 0), "common-phase-3": (3, 3)}


@pytest.mark.parametrize("offsets", list(OFFSETS))
@pytest.mark.parametrize("guarded", [True, False], ids=["guarded", "plain"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_k_updates_match_the_fp64_recurrence(shape, guarded, offsets):
    counts = SHAPES[shape]
    if shape == "odd-table":
        starts = {f % 4 for f, _, _ in U.table_from_counts(counts)}
        assert starts == {0, 1, 2, 3}
    n = sum(counts)
    ema0, ps = data(n, n)
    # decay 0.9 with the warm-up from step 71: (1 + t) / (10 + t) reaches 0.9 at t = 80, inside the K steps
    got, ref, M = run_sequence(ema0, ps, U.table_from_counts(counts), guarded, 0.9, True, 70, OFFSETS[offsets])
    check(got, ref, M, K, f"{shape} {'guarded' if guarded else 'plain'} {offsets}")
    assert not same_bits(got, ema0)


SCHEDULES = [(0.5, True, 0), (0.9, True, 0), (0.999, True, 0), (0.999, False, 0), (0.0, False, 0), (0.999, True, 8980)]


@pytest.mark.parametrize("guarded", [True, False], ids=["guarded", "plain"])
@pytest.mark.parametrize("decay,warmup,steps0", SCHEDULES, ids=[f"{d}-{'warm' if w else 'flat'}-from{s}" for d, w, s in SCHEDULES])
def test_decays_and_warmup_on_the_odd_table(decay, warmup, steps0, guarded):
    n = sum(U.ODD_COUNTS)
    ema0, ps = data(n, 1000 + steps0)
    got, ref, M = run_sequence(ema0, ps, U.table_from_counts(U.ODD_COUNTS), guarded, decay, warmup, steps0)
    check(got, ref, M, K, f"decay {decay} warmup {warmup} from step {steps0 + 1}")
    if decay == 0.0:                                                          # a = 1: the average IS the weights (p - ema rounds, so to the bound)
        assert np.abs(got - ps[-1]).max() <= STEP_ERR * M


def reach(decay):
    """First t with (1 + t) / (10 + t) >= decay as the kernel sees it."""
    d = float(np.float32(decay))
    t = 1
    while (1.0 + t) / (10.0 + t) < d:
        t += 1
    return t


@pytest.mark.parametrize("guarded", [True, False], ids=["guarded", "plain"])
def test_warmup_schedule_is_exact_at_its_corners(guarded):
    """ema = 0, p = 1: one update leaves exactly a = (float)(1 - d_t) (0 + a * 1 rounds nowhere).  t = 1, 2 and both sides of the step
    at which (1 + t) / (10 + t) reaches the decay; the guarded call is handed a wrong `step` and must use the block's."""
    n = 5
    for decay in (0.5, 0.9, 0.999):
        r = reach(decay)
        assert d_t(decay, True, r) == float(np.float32(decay)) > d_t(decay, True, r - 1) if r > 1 else True
        for t in sorted({1, 2, max(1, r - 1), r, r + 1}):
            run = Run(np.zeros(n, np.float32), np.ones(n, np.float32), [(0, n, 1)] if guarded else None, steps0=t - 1)
            run.update(decay, True, 1 if guarded else t)                      # guarded: step 1 would give a = 1 - 2/11
            got = run.ema.host()
            want = np.full(n, alpha(decay, True, t), np.float32)
            assert same_bits(got, want), (decay, t, got, want)
            flat = Run(np.zeros(n, np.float32), np.ones(n, np.float32), [(0, n, 1)] if guarded else None, steps0=t - 1)
            flat.update(decay, False, t)
            assert same_bits(flat.ema.host(), np.full(n, np.float32(1.0 - float(np.float32(decay))), np.float32))
    assert alpha(0.999, True, 1) == float(np.float32(1.0 - 2.0 / 11.0)) and alpha(0.999, True, 2) == float(np.float32(0.75))


def test_a_skipped_step_leaves_the_average_alone():
    counts = U.ODD_COUNTS
    table = U.table_from_counts(counts)
    n = sum(counts)
    ema0, ps = data(n, 5)
    run = Run(ema0, ps[0], table, steps0=3)
    run.update(0.9, True, 0)                                                  # a clean step: t = 4
    after1 = run.ema.host()
    assert not same_bits(after1, ema0)
    bad = np.zeros(n, np.float32)
    bad[table[6][0] + 2050] = np.nan                                          # second block of a trainable segment
    run.p.set(ps[1])
    run.count(bad)
    T.ema_update(run.ema.t, run.p.t, 0.9, True, 0, run.guard)
    rep = T.guard_read(run.guard)
    assert rep.skipped_last == 1 and rep.steps_applied == 4 and rep.steps_skipped == 1
    assert same_bits(run.ema.host(), after1), "a skipped step moved the average"
    run.count(np.zeros(n, np.float32))                                        # the next clean step is t = 5, not 6
    T.ema_update(run.ema.t, run.p.t, 0.9, True, 0, run.guard)
    ref = ema0.astype(np.float64)
    ref += alpha(0.9, True, 4) * (ps[0].astype(np.float64) - ref)
    ref += alpha(0.9, True, 5) * (ps[1].astype(np.float64) - ref)
    assert alpha(0.9, True, 5) != alpha(0.9, True, 6)
    check(run.ema.host(), ref, float(max(np.abs(ps[0]).max(), np.abs(ps[1]).max(), np.abs(ema0).max())), 2, "clean step after a skip")


def test_a_frozen_segment_in_the_middle_is_never_written():
    counts = U.ODD_COUNTS
    frozen = (3, 6, 7)                                                        # lengths 63, 4097 (several blocks) and 3, odd starts
    table = U.table_from_counts(counts, frozen)
    n = sum(counts)
    ema0, ps = data(n, 11)
    got, ref, M = run_sequence(ema0, ps, table, True, 0.9, True, 0, frozen=frozen)
    for i in frozen:
        sl = slice(table[i][0], table[i][0] + table[i][1])
        assert same_bits(got[sl], ema0[sl]), f"frozen segment {i} was written"
    live = np.concatenate([np.arange(f, f + c) for f, c, tr in table if tr])
    assert np.all(got[live] != ema0[live])
    check(got, ref, M, K, "frozen segments")


def test_a_captured_call_replayed_three_times_equals_three_eager_calls():
    counts = U.ODD_COUNTS
    table = U.table_from_counts(counts)
    n = sum(counts)
    ema0, ps = data(n, 21)
    results = {}
    for guarded in (True, False):
        eager = Run(ema0, ps[0], table if guarded else None)
        for k in range(3):
            eager.p.set(ps[k])
            eager.update(0.9, True, 1)                                        # plain: t = 1 each time, as a capture freezes it
        results[guarded] = eager.ema.host()
        cap = Run(ema0, ps[0], table if guarded else None)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode=T.CAPTURE_MODE):
            cap.update(0.9, True, 1)
        assert same_bits(cap.ema.host(), ema0), "capturing ran the kernel"
        for k in range(3):
            cap.p.set(ps[k])
            graph.replay()
        assert same_bits(cap.ema.host(), results[guarded]), f"replayed capture differs from eager calls (guarded={guarded})"
        if guarded:                                                           # the counter advanced on the device: t = 1, 2, 3
            assert T.guard_read(cap.guard).steps_applied == 3
    assert not same_bits(results[True], results[False])                      # t = 1, 2, 3 against t = 1, 1, 1


def test_refusals_launch_nothing():
    n = 100
    L = _lib.lib()
    ema0 = np.full(n, 2.0, np.float32)
    ema, p = Buf(ema0), Buf(np.ones(n, np.float32))
    guard = T.guard_new([(0, 60, 1), (60, 40, 1)], n, G.DEV)
    other_n = T.guard_new([(0, 99, 1)], 99, G.DEV)
    never = torch.zeros(T.guard_bytes(2), dtype=torch.uint8, device=G.DEV)    # a block lft_guard_init never saw
    e, q, g, st = ema.t.data_ptr(), p.t.data_ptr(), guard.data_ptr(), G.stream()
    nan = float("nan")
    cases = {
        "null ema": (None, q, n, 0.9, 1, 1, None),
        "null p": (e, None, n, 0.9, 1, 1, None),
        "ema == p": (e, e, n, 0.9, 1, 1, None),
        "overlapping ranges": (e, e + 4 * 10, n - 10, 0.9, 1, 1, None),
        "overlapping the other way": (e + 4 * 10, e, n - 10, 0.9, 1, 1, None),
        "n = 0": (e, q, 0, 0.9, 1, 1, None),
        "n < 0": (e, q, -5, 0.9, 1, 1, None),
        "decay = 1": (e, q, n, 1.0, 1, 1, None),
        "decay < 0": (e, q, n, -0.1, 1, 1, None),
        "decay NaN": (e, q, n, nan, 1, 1, None),
        "decay NaN, guarded": (e, q, n, nan, 1, 1, g),
        "step 0 without a guard": (e, q, n, 0.9, 1, 0, None),
        "negative step without a guard": (e, q, n, 0.9, 0, -3, None),
        "a block that was never initialised": (e, q, n, 0.9, 1, 1, never.data_ptr()),
        "a block initialised for another n": (e, q, n, 0.9, 1, 1, other_n.data_ptr()),
        "another n than the block's": (e, q, n - 1, 0.9, 1, 1, g),
    }
    for what, (a0, a1, nn, decay, warm, step, gd) in cases.items():
        rc = L.lft_ema_update(a0, a1, nn, decay, warm, step, gd, st)
        assert rc == -1, (what, rc)                                           # LFT_ERR_ARG
        assert L.lft_last_error(), what
    torch.cuda.synchronize()
    assert same_bits(ema.host(), ema0) and same_bits(p.host(), np.ones(n, np.float32)), "a refused call launched something"
    # adjacent, not overlapping, is fine; so is step 0 WITH a guard (it is ignored)
    both = Buf(np.concatenate([np.zeros(50, np.float32), np.ones(50, np.float32)]))
    assert L.lft_ema_update(both.t.data_ptr(), both.t.data_ptr() + 4 * 50, 50, 0.5, 0, 1, None, st) == 0
    assert np.all(both.host()[:50] == 0.5)
    assert L.lft_ema_update(e, q, n, 0.5, 0, 0, g, st) == 0
    assert np.all(ema.host() == 1.5)
