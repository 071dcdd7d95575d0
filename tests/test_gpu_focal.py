"""GPU tests of the focal-stack term (lft_focal_loss: k_focal_residual, k_focal_fold, k_focal_adjoint; lft_refocus_adjoint) against
lft_refocus on the materialised difference (bits) and against the fp64 restatement of tests/focal_util.py (tolerances derived there
and in tests/refocus_util.py).  Every case runs the kernels once (``run``); the tests share that run and its restatement.

The cases cover A in {1, 2, 3, 5}; views of 1x1, 1x9, 5x7, 33x35 and 16x70 (the 32 x 8 tile: one pixel, one row, less than a tile,
one pixel more than a tile in both axes, two tile rows with a third column tile); D in {1, 3, 7} out of refocus_util.SLOPES, 0 and
40 among them (at 40 every tap of an off-centre view clamps); the three interpolations and penalties; B in {1, 3}."""
import functools

import numpy as np
import pytest
import torch

from lft_amd import _lib, loss as L, refocus as R
from lft_amd import train as T

import focal_util as FU
import gpu_util as G
import refocus_util as RU

pytestmark = pytest.mark.gpu
DEV = G.DEV
W_FOCAL, GSCALE, EPS = 0.75, 1.25, 2.0 ** -10            # exact in fp32: the restatement sees the numbers the kernels see

#        B  A  H   W   slopes                 interp     penalty
CASES = [(1, 1, 1, 1, [0.0], "nearest", "l1"),
         (3, 2, 1, 9, [-1.0, 0.0, 40.0], "linear", "mse"),
         (1, 3, 5, 7, RU.SLOPES, "cubic", "charbonnier"),
         (3, 5, 5, 7, [-2.5, 0.0, 40.0], "linear", "l1"),
         (1, 2, 33, 35, RU.SLOPES, "cubic", "l1"),
         (1, 3, 16, 70, [0.75, 0.0, 40.0], "linear", "charbonnier"),
         (1, 5, 33, 35, [2.0], "nearest", "mse"),
         (3, 1, 16, 70, [-0.3, 0.0, 40.0], "cubic", "l1"),
         (1, 2, 5, 7, [-0.3, 2.0, 40.0], "nearest", "charbonnier")]
IDS = ["B%d-A%d-%dx%d-D%d-%s-%s" % (c[0], c[1], c[2], c[3], len(c[4]), c[5], c[6]) for c in CASES]
assert {c[1] for c in CASES} == {1, 2, 3, 5} and {len(c[4]) for c in CASES} == {1, 3, 7} and {c[0] for c in CASES} == {1, 3}
assert {(c[2], c[3]) for c in CASES} == {(1, 1), (1, 9), (5, 7), (33, 35), (16, 70)} and {(c[5], c[6]) for c in CASES} >= {
    (i, p) for i, p in zip(("nearest", "linear", "cubic"), FU.PENALTIES)}


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def inputs(case):
    B, A, H, W = case[:4]
    rng = np.random.default_rng(1000 * B + 100 * A + H + W)
    return (rng.standard_normal((B, 1, A * H, A * W)).astype(np.float32) for _ in range(2))


@functools.lru_cache(maxsize=None)
def run(i):
    """One run of lft_focal_loss on case i (guarded outputs), lft_refocus on the materialised difference, and the restatement."""
    case = CASES[i]
    B, A, H, W, slopes, interp, penalty = case
    D, taps = len(slopes), R.TAPS[interp]
    sr_np, hr_np = inputs(case)
    sr, hr = torch.from_numpy(sr_np).to(DEV), torch.from_numpy(hr_np).to(DEV)
    dbuf, dsr = G.guarded((B, 1, A * H, A * W), torch.float32)
    rbuf, residual = G.guarded((B, D, H, W), torch.float32)
    total, F = L.focal_loss(sr, hr, A, slopes, interp, "full", penalty, EPS, W_FOCAL, dsr=dsr, residual=residual, gscale=GSCALE)
    plain = R.refocus(sr - hr, slopes, angRes=A, interp=interp, out_dtype=torch.float32)      # fl32(sr - hr), materialised
    torch.cuda.synchronize()
    assert G.guard_intact(dbuf) and G.guard_intact(rbuf)
    table = R.shift_table(A, slopes, "full", interp)
    r64 = FU.refocus_batch_np(FU.difference(sr_np, hr_np), A, table, taps)
    return dict(case=case, sr=sr, hr=hr, dsr=dsr, residual=residual, total=total, F=F, plain=plain, table=table, taps=taps, r64=r64,
                tol_r=RU.tol(A, table, taps, float(np.abs(FU.difference(sr_np, hr_np)).max())))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_residual_is_refocus_of_the_difference_bit_for_bit(i):
    c = run(i)
    assert c["plain"].shape == c["residual"].shape and not torch.isnan(c["residual"]).any()
    assert torch.equal(bits(c["residual"]), bits(c["plain"]))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_residual_and_value_against_the_restatement(i):
    c = run(i)
    penalty = c["case"][6]
    r = c["residual"].cpu().numpy().astype(np.float64)
    err = float(np.abs(r - c["r64"]).max())
    print(f"{IDS[i]}: |r - r64| {err:.3e} (tolerance {c['tol_r']:.3e})")
    assert err <= c["tol_r"]
    # the value: the fp64 mean of rho over the GPU's own residual, rounded once
    F64 = float(FU.rho(r, penalty, EPS).mean())
    F, total = float(c["F"]), float(c["total"])
    print(f"{IDS[i]}: F {F:.9g} against {F64:.12g}, total {total:.9g}")
    assert abs(F - F64) <= 2.0 * FU.U24 * abs(F64) and abs(total - W_FOCAL * F64) <= 2.0 * FU.U24 * abs(W_FOCAL * F64)
    # the restatement's own sign agrees wherever its residual is decided
    decided = np.abs(c["r64"]) > c["tol_r"]
    assert np.all(np.sign(r[decided]) == np.sign(c["r64"][decided])) and 1.0 - decided.mean() <= 0.01, 1.0 - decided.mean()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_gradient_is_the_adjoint_of_the_stack_gradient(i):
    """dsr against the restatement's adjoint of the G computed in fp64 from the GPU's own residual (so an L1 sign is the GPU's),
    within tol_adj plus one store rounding."""
    c = run(i)
    B, A, H, W, slopes, interp, penalty = c["case"]
    r = c["residual"].cpu().numpy().astype(np.float64)
    G64 = FU.stack_grad_np(r, penalty, EPS, W_FOCAL, GSCALE)
    ref, n, M = FU.adjoint_np(G64, A, c["table"], c["taps"], bound=True)
    got = c["dsr"].cpu().numpy().astype(np.float64)
    assert not np.isnan(got).any()
    tol = FU.tol_adj(n, M) + FU.U24 * np.abs(ref)
    err = np.abs(got - ref)
    worst = float((err / np.where(tol > 0, tol, 1.0)).max())
    print(f"{IDS[i]}: |dsr - ref| {err.max():.3e}, largest |ref| {np.abs(ref).max():.3e}, largest n {int(n.max())}, worst error / tolerance {worst:.3f}")
    assert np.all(err <= tol)
    assert np.all(got[M == 0] == 0.0)                               # a pixel no tap reads gets exactly 0


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_refocus_adjoint_and_the_dot_product_identity(i):
    B, A, H, W, slopes, interp, _ = CASES[i]
    taps = R.TAPS[interp]
    rng = np.random.default_rng(77 + i)
    for aperture in ("full", RU.user_aperture(A, 5)):
        table = R.shift_table(A, slopes, aperture, interp)
        g = rng.standard_normal((B, len(slopes), H, W)).astype(np.float32)
        x = rng.standard_normal((B, 1, A * H, A * W)).astype(np.float32)
        obuf, out = G.guarded((B, 1, A * H, A * W), torch.float32)
        R.refocus_adjoint(torch.from_numpy(g).to(DEV), slopes, A, aperture, interp, out=out)
        Rx = R.refocus(torch.from_numpy(x).to(DEV), slopes, angRes=A, aperture=aperture, interp=interp, out_dtype=torch.float32).cpu().numpy().astype(np.float64)
        got = out.cpu().numpy().astype(np.float64)
        assert G.guard_intact(obuf) and not np.isnan(got).any()
        ref, n, M = FU.adjoint_np(g, A, table, taps, bound=True)
        tol = FU.tol_adj(n, M) + FU.U24 * np.abs(ref)
        assert np.all(np.abs(got - ref) <= tol), float((np.abs(got - ref) / np.where(tol > 0, tol, 1.0)).max())
        # <R x, g> = <x, R^T g> in fp64 of the two fp32 outputs: each side is off by at most its own tolerance times the other factor
        lhs, rhs = float((Rx * g).sum()), float((got * x).sum())
        bound = RU.tol(A, table, taps, float(np.abs(x).max())) * float(np.abs(g).sum()) + float((tol * np.abs(x)).sum())
        print(f"{IDS[i]}: <Rx, g> {lhs:.9g}, <x, RTg> {rhs:.9g}, differ by {abs(lhs - rhs):.3e} (bound {bound:.3e})")
        assert abs(lhs - rhs) <= bound
        # accumulate adds to what the mosaic holds with one rounding
        prior = torch.from_numpy(x).to(DEV).clone()
        R.refocus_adjoint(torch.from_numpy(g).to(DEV), slopes, A, aperture, interp, out=prior, accumulate=True)
        assert torch.equal(bits(prior), bits(torch.from_numpy(x).to(DEV) + out))


@pytest.mark.parametrize("i", [2, 3, 4, 5], ids=[IDS[i] for i in (2, 3, 4, 5)])
def test_accumulate_null_gradient_repeat_and_capture(i):
    c = run(i)
    B, A, H, W, slopes, interp, penalty = c["case"]
    sr, hr = c["sr"], c["hr"]
    call = lambda **kw: L.focal_loss(sr, hr, A, slopes, interp, "full", penalty, EPS, W_FOCAL, gscale=GSCALE, **kw)
    # accumulate = 1: dsr = fl32(prior + the accumulate = 0 result), total likewise from the fp64 sum
    prior = torch.from_numpy(np.random.default_rng(3).standard_normal(tuple(sr.shape)).astype(np.float32)).to(DEV)
    acc, total = prior.clone(), torch.full((1,), 0.25, dtype=torch.float32, device=DEV)
    _, F = call(dsr=acc, accumulate=True, total=total)
    assert torch.equal(bits(acc), bits(prior + c["dsr"])) and torch.equal(bits(F), bits(c["F"]))
    r = c["residual"].cpu().numpy().astype(np.float64)
    want = 0.25 + W_FOCAL * float(FU.rho(r, penalty, EPS).mean())
    assert abs(float(total) - want) <= 2.0 * FU.U24 * abs(want)
    # dsr = NULL leaves the values unchanged; a second call gives the same bits
    total0, F0 = call()
    assert torch.equal(bits(total0), bits(c["total"])) and torch.equal(bits(F0), bits(c["F"]))
    dsr2, res2 = torch.full_like(sr, 9.0), torch.full_like(c["residual"], 9.0)
    total2, F2 = call(dsr=dsr2, residual=res2)
    for a, b in ((dsr2, c["dsr"]), (res2, c["residual"]), (total2, c["total"]), (F2, c["F"])):
        assert torch.equal(bits(a), bits(b))
    # capture and replay
    scratch = torch.empty(L.focal_scratch_bytes(B, len(slopes), A, H, W), dtype=torch.uint8, device=DEV)
    dsr3, tot3, F3 = torch.empty_like(sr), torch.empty(1, device=DEV), torch.empty(1, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side, capture_error_mode=T.CAPTURE_MODE):
            call(dsr=dsr3, total=tot3, focal_out=F3, scratch=scratch)
        for t in (dsr3, tot3, F3):
            t.fill_(9)
        graph.replay()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    for a, b in ((dsr3, c["dsr"]), (tot3, c["total"]), (F3, c["F"])):
        assert torch.equal(bits(a), bits(b))


def test_equal_inputs_give_zero_and_an_empty_batch_is_refused():
    A, H, W, slopes = 3, 16, 70, [-1.0, 0.0, 40.0]
    sr = torch.from_numpy(np.random.default_rng(0).standard_normal((2, 1, A * H, A * W)).astype(np.float32)).to(DEV)
    for penalty, F_want in (("l1", 0.0), ("mse", 0.0), ("charbonnier", EPS)):
        dsr = torch.full_like(sr, 9.0)
        total, F = L.focal_loss(sr, sr.clone(), A, slopes, "cubic", "full", penalty, EPS, W_FOCAL, dsr=dsr)
        assert abs(float(F) - F_want) <= FU.U24 * F_want and abs(float(total) - W_FOCAL * F_want) <= 2 * FU.U24 * F_want
        assert float(dsr.abs().max()) == 0.0
    assert L.focal_error(sr, sr.clone(), A, slopes) == 0.0
    hr = sr + 0.5                                                   # a constant difference comes back as itself: the weights sum to 1
    assert abs(L.focal_error(sr, hr, A, slopes, "linear") - 0.5) <= 1e-6 and abs(L.focal_error(sr[0, 0], hr[0, 0], A, slopes) - 0.5) <= 1e-6
    # B = 0: the mean over no pixels is not defined; refused before anything is launched, as lft_lf_loss and lft_ssim_loss do
    empty = sr[:0]
    dsr, total = torch.full_like(sr, 9.0)[:0], torch.full((1,), 9.0, device=DEV)
    with pytest.raises(_lib.LftError, match="lft_focal_loss: sizes must be positive"):
        L.focal_loss(empty, empty.clone(), A, slopes, dsr=dsr, total=total, scratch=torch.empty(8, dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.LftError, match="lft_focal_loss_scratch_bytes: sizes must be positive"):
        L.focal_loss(empty, empty.clone(), A, slopes)
    with pytest.raises(_lib.LftError, match="lft_refocus_adjoint: sizes must be positive"):
        R.refocus_adjoint(torch.empty(0, 3, H, W, device=DEV), slopes, A)
    torch.cuda.synchronize()
    assert float(total) == 9.0
