"""lft_ssim_loss called directly through the C ABI against the fp64 restatement of tests/ssim_loss_util.py: S against lft_view_metrics
and against the restatement, the gradient at a DERIVED bound, sr == hr, accumulation behind lft_lf_loss, dsr == NULL, bit
reproducibility, graph capture, and every refusal.  Every buffer the call is handed sits inside padding of 7.0 that must survive.

The gradient bound: the kernel is fp64 between its fp32 loads and its one fp32 store, so an element is off by the store's rounding,
2^-24 of itself, plus fp64 noise; the gate is four times that unit, 2^-22 of the largest reference element (an exact evaluation
measures 3.6e-8).  An fp32 moment pass misses it by two to three orders of magnitude (1e-5 ... 6.5e-5), which is the point."""
import numpy as np
import pytest
import torch

from lft_amd import _lib, loss, metrics

import gpu_util as G
import lf_loss_util as LU
import ssim_loss_util as U
from test_gpu_lf_loss import padded, padding_intact

ERR_ARG, ERR_SHAPE = -1, -2       # LFT_ERR_ARG, LFT_ERR_SHAPE
GRAD_BOUND = 2.0 ** -22           # of the largest reference element
W_SSIM = 0.2


def scratch_floats(B, A, H, W):
    n = loss.ssim_scratch_bytes(B, A, H, W)
    assert n % 8 == 0
    return n // 4


class Call:
    """One lft_ssim_loss call on padded device buffers.  shift: floats by which sr, hr and dsr sit off the 16-byte grid."""

    def __init__(self, sr, hr, shape, with_dsr=True, shift=0):
        self.shape, self.n, self.shift = shape, int(sr.size), shift
        sr, hr = np.array(sr), np.array(hr)                       # the shared cases are read-only
        self.sr_buf, self.sr = padded(sr, shift=shift)
        self.hr_buf, self.hr = padded(hr, shift=shift)
        self.dsr_buf, self.dsr = padded(n=self.n, shift=shift)
        self.t_buf, self.total = padded(n=1)
        self.o_buf, self.ssim = padded(n=1)
        self.ns = scratch_floats(*shape)
        self.s_buf, self.scratch = padded(n=self.ns)
        self.with_dsr = with_dsr

    def run(self, ssim_range=2.0, w=W_SSIM, gscale=1.0, accumulate=0, check=True):
        rc = _lib.lib().lft_ssim_loss(self.sr.data_ptr(), self.hr.data_ptr(), *self.shape, ssim_range, w,
                                      self.dsr.data_ptr() if self.with_dsr else None, gscale, accumulate, self.total.data_ptr(),
                                      self.ssim.data_ptr(), self.scratch.data_ptr(), G.stream())
        if check:
            _lib.check(rc, "lft_ssim_loss")
        return rc

    def intact(self):
        return (padding_intact(self.sr_buf, self.n, self.shift) and padding_intact(self.hr_buf, self.n, self.shift)
                and padding_intact(self.dsr_buf, self.n, self.shift) and padding_intact(self.t_buf, 1) and padding_intact(self.o_buf, 1)
                and padding_intact(self.s_buf, self.ns))

    def grad(self):
        B, A, H, W = self.shape
        return self.dsr.cpu().numpy().astype(np.float64).reshape(B, 1, A * H, A * W)


@pytest.mark.gpu
@pytest.mark.parametrize("ssim_range", [1.0, 2.0], ids=["range1", "range2"])
@pytest.mark.parametrize("shape", U.SHAPES, ids=U.SHAPE_IDS)
def test_s_equals_view_metrics_and_the_restatement(shape, ssim_range):
    B, A, H, W = shape
    sr, hr, S, _ = U.case(shape, ssim_range)
    c = Call(sr, hr, shape, with_dsr=False)
    c.run(ssim_range)
    _, per_view = metrics.view_metrics(c.hr.view(B, 1, A * H, A * W), c.sr.view(B, 1, A * H, A * W), A, ssim_range)
    torch.cuda.synchronize()
    got, total = float(c.ssim[0]), float(c.total[0])
    vm = float(per_view.double().mean())
    print(f"{shape} range {ssim_range}: S {got:.9f}, mean of lft_view_metrics {vm:.9f} (diff {abs(got - vm):.2e}), "
          f"restatement {S:.9f} (rel {abs(got - S) / S:.2e})")
    assert c.intact()
    assert abs(got - vm) <= 1e-6
    assert abs(got - S) <= 1e-6 * S
    assert abs(total - W_SSIM * (1.0 - S)) <= 1e-6 * W_SSIM


@pytest.mark.gpu
@pytest.mark.parametrize("gscale", [1.0, 1.0 / 3.0], ids=["g1", "g_third"])
@pytest.mark.parametrize("shape", U.SHAPES, ids=U.SHAPE_IDS)
def test_gradient_within_the_derived_bound(shape, gscale):
    sr, hr, S, g = U.case(shape)
    for shift in (0, 1):                                          # 16-byte aligned pointers and pointers off that grid
        c = Call(sr, hr, shape, shift=shift)
        c.run(2.0, W_SSIM, gscale)
        torch.cuda.synchronize()
        assert c.intact(), "wrote outside a buffer"
        assert np.array_equal(c.sr.cpu().numpy(), sr.reshape(-1)) and np.array_equal(c.hr.cpu().numpy(), hr.reshape(-1))
        want = -float(np.float32(gscale)) * float(np.float32(W_SSIM)) * g       # the call takes both factors as fp32
        worst, top = float(np.abs(c.grad() - want).max()), float(np.abs(want).max())
        print(f"{shape} gscale {gscale:.3f} shift {shift}: worst |dsr - ref| {worst:.3e} = {worst / top:.3e} of the largest element, "
              f"bound {GRAD_BOUND:.3e}")
        assert worst <= GRAD_BOUND * top, (worst / top)
        assert abs(float(c.ssim[0]) - S) <= 1e-6 * S


@pytest.mark.gpu
@pytest.mark.parametrize("shape", U.SHAPES, ids=U.SHAPE_IDS)
def test_sr_equal_to_hr_gives_one_and_no_gradient(shape):
    sr, hr = U.clean_inputs(*shape)
    c = Call(sr, hr, shape)
    c.run()
    torch.cuda.synchronize()
    top = W_SSIM * float(np.abs(U.case(shape)[3]).max())
    print(f"{shape}: S {float(c.ssim[0]):.9f}, max |dsr| {float(c.dsr.abs().max()):.3e} against the noisy case's {top:.3e}")
    assert c.intact()
    assert abs(float(c.ssim[0]) - 1.0) <= 1e-6 and abs(float(c.total[0])) <= 1e-6
    assert float(c.dsr.abs().max()) <= 1e-6 * top


@pytest.mark.gpu
@pytest.mark.parametrize("shape", U.SHAPES, ids=U.SHAPE_IDS)
def test_accumulate_adds_to_what_lf_loss_left(shape):
    B, A, H, W = shape
    sr, hr, S, g = U.case(shape)
    c = Call(sr, hr, shape)
    lf_scratch = torch.empty(loss.scratch_bytes(B, A, H, W), dtype=torch.uint8, device=G.DEV)
    loss3 = torch.empty(3, dtype=torch.float32, device=G.DEV)
    _lib.call("lft_lf_loss", c.sr.data_ptr(), c.hr.data_ptr(), B, A, H, W, LU.PEN_ENUM["charbonnier"], 1e-3, 1.0, 0.5, c.dsr.data_ptr(), 1.0,
              loss3.data_ptr(), lf_scratch.data_ptr(), G.stream())
    c.total.copy_(loss3[:1])
    pre_g, pre_t = c.grad(), float(loss3[0])
    c.run(accumulate=1)
    torch.cuda.synchronize()
    assert c.intact()
    term_g = -float(np.float32(W_SSIM)) * g
    term_t = float(np.float32(W_SSIM)) * (1.0 - S)
    err = np.abs(c.grad() - (pre_g + term_g))
    room = 2.0 ** -22 * (np.abs(pre_g) + np.abs(term_g))
    print(f"{shape}: worst error / room {float((err / np.maximum(room, 1e-300)).max()):.3f}; total {float(c.total[0]):.9f} = {pre_t:.9f} + {term_t:.9f}")
    assert np.all(err <= room)
    assert abs(float(c.total[0]) - (pre_t + term_t)) <= 2.0 ** -22 * (abs(pre_t) + abs(term_t))
    assert abs(float(c.ssim[0]) - S) <= 1e-6 * S


@pytest.mark.gpu
@pytest.mark.parametrize("shape", U.SHAPES, ids=U.SHAPE_IDS)
def test_dsr_null_writes_only_total_and_s(shape):
    sr, hr, S, _ = U.case(shape)
    c = Call(sr, hr, shape, with_dsr=False)
    c.run()
    torch.cuda.synchronize()
    assert c.intact()
    assert bool((c.dsr == 7.0).all()), "dsr == NULL, yet the buffer behind it was written"
    assert np.array_equal(c.sr.cpu().numpy(), sr.reshape(-1)) and np.array_equal(c.hr.cpu().numpy(), hr.reshape(-1))
    d = Call(sr, hr, shape)
    d.run()
    torch.cuda.synchronize()
    assert float(c.ssim[0]) == float(d.ssim[0]) and float(c.total[0]) == float(d.total[0])      # the same sums in the same order
    assert abs(float(c.ssim[0]) - S) <= 1e-6 * S


@pytest.mark.gpu
def test_two_calls_give_identical_bits():
    shape = U.SHAPES[3]
    sr, hr, _, _ = U.case(shape)
    res = []
    for _ in range(2):
        c = Call(sr, hr, shape)
        c.run(gscale=1.0 / 3.0)
        torch.cuda.synchronize()
        res.append(tuple(t.cpu().numpy().view(np.int32) for t in (c.total, c.ssim, c.dsr)))
    assert all(np.array_equal(a, b) for a, b in zip(*res))


@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", [0, 1], ids=["overwrite", "accumulate"])
def test_captured_call_replayed_on_new_inputs_equals_eager(accumulate):
    shape = U.SHAPES[1]
    sr, hr, _, _ = U.case(shape)
    sr2, hr2, S2, _ = U.case(shape, 2.0, 9)
    c = Call(sr, hr, shape)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c.run(accumulate=accumulate)                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c.run(accumulate=accumulate)
    c.sr.copy_(torch.from_numpy(np.array(sr2).reshape(-1)))
    c.hr.copy_(torch.from_numpy(np.array(hr2).reshape(-1)))
    for t in (c.dsr, c.total, c.ssim):
        t.fill_(0.25)
    graph.replay()
    torch.cuda.synchronize()
    e = Call(sr2, hr2, shape)
    for t in (e.dsr, e.total, e.ssim):
        t.fill_(0.25)
    e.run(accumulate=accumulate)
    torch.cuda.synchronize()
    assert c.intact() and e.intact()
    for a, b in ((c.total, e.total), (c.ssim, e.ssim), (c.dsr, e.dsr)):
        assert np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))
    assert abs(float(c.ssim[0]) - S2) <= 1e-6 * S2
    assert abs(float(c.total[0]) - (0.25 * accumulate + W_SSIM * (1.0 - S2))) <= 1e-6


NAN, INF = float("nan"), float("inf")
GOOD = dict(ssim_range=2.0, w=0.2, gscale=1.0, accumulate=0)
REFUSALS = [("null_sr", dict(sr=None), ERR_ARG), ("null_hr", dict(hr=None), ERR_ARG), ("null_total", dict(total=None), ERR_ARG),
            ("null_ssim_out", dict(ssim=None), ERR_ARG), ("null_scratch", dict(scratch=None), ERR_ARG),
            ("sr_misaligned", dict(sr="sr+2b"), ERR_ARG), ("dsr_misaligned", dict(dsr="dsr+1b"), ERR_ARG),
            ("total_misaligned", dict(total="total+2b"), ERR_ARG), ("scratch_misaligned", dict(scratch="scratch+4b"), ERR_ARG),
            ("range_0", dict(ssim_range=0.0), ERR_ARG), ("range_neg", dict(ssim_range=-2.0), ERR_ARG), ("range_nan", dict(ssim_range=NAN), ERR_ARG),
            ("range_inf", dict(ssim_range=INF), ERR_ARG), ("w_0", dict(w=0.0), ERR_ARG), ("w_neg", dict(w=-0.2), ERR_ARG), ("w_nan", dict(w=NAN), ERR_ARG),
            ("w_inf", dict(w=INF), ERR_ARG), ("gscale_nan", dict(gscale=NAN), ERR_ARG), ("accumulate_2", dict(accumulate=2), ERR_ARG),
            ("accumulate_neg", dict(accumulate=-1), ERR_ARG),
            ("dsr_is_sr", dict(dsr="sr"), ERR_ARG), ("dsr_is_hr", dict(dsr="hr"), ERR_ARG), ("dsr_inside_sr", dict(dsr="sr+4"), ERR_ARG),
            ("dsr_before_hr", dict(dsr="hr-4"), ERR_ARG),
            ("B_0", dict(B=0), ERR_SHAPE), ("A_0", dict(A=0), ERR_SHAPE), ("H_0", dict(H=0), ERR_SHAPE), ("W_neg", dict(W=-3), ERR_SHAPE),
            ("H_10", dict(H=10), ERR_SHAPE), ("W_10", dict(W=10), ERR_SHAPE)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,change,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_everything_untouched(name, change, code):
    shape = U.SHAPES[1]
    sr, hr, _, _ = U.case(shape)
    c = Call(sr, hr, shape)
    a = dict(GOOD, sr=c.sr.data_ptr(), hr=c.hr.data_ptr(), dsr=c.dsr.data_ptr(), total=c.total.data_ptr(), ssim=c.ssim.data_ptr(),
             scratch=c.scratch.data_ptr(), B=shape[0], A=shape[1], H=shape[2], W=shape[3])
    named = {"sr": a["sr"], "hr": a["hr"], "sr+4": a["sr"] + 16, "hr-4": a["hr"] - 16, "sr+2b": a["sr"] + 2, "dsr+1b": a["dsr"] + 1,
             "total+2b": a["total"] + 2, "scratch+4b": a["scratch"] + 4}
    a.update({k: named[v] if isinstance(v, str) else v for k, v in change.items()})
    rc = _lib.lib().lft_ssim_loss(a["sr"], a["hr"], a["B"], a["A"], a["H"], a["W"], a["ssim_range"], a["w"], a["dsr"], a["gscale"],
                                  a["accumulate"], a["total"], a["ssim"], a["scratch"], G.stream())
    torch.cuda.synchronize()
    assert rc == code, (name, rc, _lib.lib().lft_last_error())
    assert c.intact()
    assert all(bool((t == 7.0).all()) for t in (c.dsr, c.total, c.ssim, c.scratch))
    assert np.array_equal(c.sr.cpu().numpy(), sr.reshape(-1)) and np.array_equal(c.hr.cpu().numpy(), hr.reshape(-1))


@pytest.mark.gpu
def test_the_good_arguments_of_the_refusal_test_are_accepted():
    shape = U.SHAPES[1]
    sr, hr, _, _ = U.case(shape)
    c = Call(sr, hr, shape)
    assert c.run(GOOD["ssim_range"], GOOD["w"], GOOD["gscale"], GOOD["accumulate"], check=False) == 0
    assert c.run(1.0, 3.0, -1.0, 1, check=False) == 0             # a negative or infinite gscale is the caller's business
    torch.cuda.synchronize()
    assert c.intact()
