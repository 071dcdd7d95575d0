"""lft_lf_loss called directly through the C ABI against the fp64 restatement of tests/lf_loss_util.py: every shape class, the three
penalties, pixel-only / EPI-only / mixed weights, dsr given and NULL, a gradient scale that is not 1; the border semantics of the
four differences in one launch; bit reproducibility, graph capture, and every refusal.  Every buffer the call is handed sits inside
padding of 7.0 that must survive.

Inputs are multiples of 2^-8 (lf_loss_util.lattice_inputs): d and all its differences are exact in fp32, so the L1 gradient is gated
by a DERIVED bound (lf_loss_util.l1_grad_bound) and the smooth penalties at 4 times the level an equally valid fp32 implementation --
the restatement run in fp32 by torch on the CPU -- shows against fp64 on these very cases.  tests/test_lf_loss_host.py
(test_gpu_tolerances_are_4x_fp32_torch) measures that level without a GPU: over every shape, weight pair and eps below, for MSE and
Charbonnier, the worst gradient error is 1.99e-7 of the largest gradient element (the worst relative loss error 1.5e-7, held here to
the project's LOSS_RTOL)."""
import functools

import numpy as np
import pytest
import torch

from lft_amd import _lib, loss

import gpu_util as G
import lf_loss_util as U

GRAD_LEVEL = 2.0e-7               # fp32 torch against fp64 torch, see above
GRAD_TOL = 4 * GRAD_LEVEL
PAD = 64                          # floats of 7.0 on either side of every buffer: 256 bytes, so the 16-byte path stays in reach
ERR_ARG, ERR_SHAPE = -1, -2       # LFT_ERR_ARG, LFT_ERR_SHAPE
CASES = [("l1", 1e-3), ("mse", 1e-3), ("charbonnier", U.EPS_VALUES[0]), ("charbonnier", U.EPS_VALUES[1])]
CASE_IDS = ["l1", "mse", "charb1e-3", "charb0.1"]
SHAPE_IDS = ["x".join(map(str, s)) for s in U.SHAPES]


def padded(values=None, n=None, shift=0):
    """(buffer, view): the view holds `values` (or n floats of 7.0) with PAD + shift floats of 7.0 in front and PAD behind."""
    n = int(values.size) if values is not None else n
    buf = torch.full((PAD + shift + n + PAD,), 7.0, dtype=torch.float32, device=G.DEV)
    view = buf[PAD + shift:PAD + shift + n]
    if values is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(values).reshape(-1)))
    return buf, view


def padding_intact(buf, view_len, shift=0):
    b = buf.cpu().numpy()
    return bool(np.all(b[:PAD + shift] == 7.0) and np.all(b[PAD + shift + view_len:] == 7.0))


def scratch_floats(B, A, H, W):
    n = loss.scratch_bytes(B, A, H, W)
    assert n % 8 == 0
    return n // 4


class Call:
    """One lft_lf_loss call on padded device buffers."""

    def __init__(self, sr, hr, shape, with_dsr=True, shift=0):
        self.shape, self.n, self.shift = shape, int(sr.size), shift
        self.sr_buf, self.sr = padded(sr, shift=shift)
        self.hr_buf, self.hr = padded(hr, shift=shift)
        self.dsr_buf, self.dsr = padded(n=self.n, shift=shift)
        self.l_buf, self.loss3 = padded(n=3)
        self.ns = scratch_floats(*shape)
        self.s_buf, self.scratch = padded(n=self.ns)
        self.with_dsr = with_dsr

    def run(self, penalty, eps, w_pix, w_epi, gscale, check=True):
        rc = _lib.lib().lft_lf_loss(self.sr.data_ptr(), self.hr.data_ptr(), *self.shape, U.PEN_ENUM[penalty], eps, w_pix, w_epi,
                                    self.dsr.data_ptr() if self.with_dsr else None, gscale, self.loss3.data_ptr(),
                                    self.scratch.data_ptr(), G.stream())
        if check:
            _lib.check(rc, "lft_lf_loss")
        return rc

    def intact(self):
        return (padding_intact(self.sr_buf, self.n, self.shift) and padding_intact(self.hr_buf, self.n, self.shift)
                and padding_intact(self.dsr_buf, self.n, self.shift) and padding_intact(self.l_buf, 3) and padding_intact(self.s_buf, self.ns))


@functools.lru_cache(maxsize=None)
def inputs(shape):
    return U.lattice_inputs(*shape)


@functools.lru_cache(maxsize=None)
def reference(shape, penalty, eps, w_pix, w_epi):
    """Computed once per case and shared between the dsr and the dsr-NULL test; never written to."""
    sr, hr = inputs(shape)
    ref3, g = U.reference(sr, hr, shape[1], penalty, eps, w_pix, w_epi)
    g.setflags(write=False)
    return ref3, g


def all_nine_tie(sr, hr, shape):
    """Mask [B,1,A*H,A*W]: d is 0 at the pixel and at every neighbour the definition pairs it with."""
    B, A, H, W = shape
    t = (sr == hr).reshape(B, A, H, A, W)
    out = t.copy()
    for ax in (1, 2, 3, 4):
        nxt = np.ones_like(t)
        prv = np.ones_like(t)
        sl_a, sl_b = [slice(None)] * 5, [slice(None)] * 5
        sl_a[ax], sl_b[ax] = slice(0, -1), slice(1, None)
        nxt[tuple(sl_a)] = t[tuple(sl_b)]
        prv[tuple(sl_b)] = t[tuple(sl_a)]
        out &= nxt & prv
    return out.reshape(B, 1, A * H, A * W)


def check_case(shape, penalty, eps, w_pix, w_epi, with_dsr, shift=0):
    sr, hr = inputs(shape)
    ref3, ref_g = reference(shape, penalty, eps, w_pix, w_epi)
    gscale = 3.0 if penalty == "l1" else 0.5                      # 0.5: exact, the smooth penalties' level was measured without a scale
    c = Call(sr, hr, shape, with_dsr, shift)
    c.run(penalty, eps, w_pix, w_epi, gscale)
    torch.cuda.synchronize()
    assert c.intact(), "wrote outside a buffer"
    assert np.array_equal(c.sr.cpu().numpy(), sr.reshape(-1)) and np.array_equal(c.hr.cpu().numpy(), hr.reshape(-1))
    got3 = [float(x) for x in c.loss3.cpu()]
    le = U.loss_error(got3, ref3)
    print(f"{shape} {penalty} eps {eps} w {w_pix, w_epi}: (total, P, E) {got3} ref {ref3} rel {le:.2e}")
    assert le <= U.LOSS_RTOL, (got3, ref3)
    out = c.dsr.cpu().numpy().astype(np.float64).reshape(ref_g.shape)
    if not with_dsr:
        assert np.all(out == 7.0), "dsr == NULL, yet the buffer behind it was written"
        return
    want = gscale * ref_g
    if penalty == "l1":
        bound = U.l1_grad_bound(*shape, w_pix, w_epi, gscale)
        worst = float(np.abs(out - want).max())
        print(f"    L1 gradient: worst |dsr - ref| {worst:.3e}, derived bound {bound:.3e}")
        assert worst <= bound, (worst, bound)
        ties = all_nine_tie(sr, hr, shape)
        assert np.all(out[ties] == 0.0), "an element whose nine contributions all tie must be exactly 0"
        if shape[2] >= 3 and shape[3] >= 3:
            assert ties.sum() >= shape[1] ** 2                    # the planted corner of every view
    else:
        ge = U.grad_error(out, want)
        print(f"    gradient error {ge:.3e} of the largest element, gate {GRAD_TOL:.1e}")
        assert ge <= GRAD_TOL, ge


@pytest.mark.gpu
@pytest.mark.parametrize("with_dsr", [True, False], ids=["dsr", "dsr_null"])
@pytest.mark.parametrize("w", U.WEIGHTS, ids=["pix", "epi", "mixed"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("shape", U.SHAPES, ids=SHAPE_IDS)
def test_lf_loss(shape, case, w, with_dsr):
    check_case(shape, case[0], case[1], w[0], w[1], with_dsr)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,shift", [((8, 5, 64, 64), 1), ((11, 5, 96, 80), 0), ((3, 2, 34, 66), 0), ((3, 2, 34, 66), 2)],
                         ids=["scalar_past_cap", "vec_past_cap", "vec_ragged_views", "scalar_even_pitch"])
def test_lf_loss_both_access_paths_and_the_launch_cap(shape, shift):
    """The stencil pass has a 16-byte path (pitch a multiple of 4, 16-byte aligned pointers) and a scalar one, and strides over the
    mosaic beyond 2 048 blocks of 256 threads: pointers shifted off the 16-byte grid put the BASELINE shape (3 200 scalar blocks) past
    that cap, 2 112 000 pixels put the 16-byte path past it (2 063 blocks); 3x2x34x66 has a pitch of 132 with views of 66 columns,
    so a 16-byte chunk straddles two views."""
    for penalty, eps in (("l1", 1e-3), ("charbonnier", 0.1)):
        check_case(shape, penalty, eps, 1.0, 0.5, True, shift)


@pytest.mark.gpu
def test_random_inputs_reported():
    """Non-lattice inputs, Charbonnier at eps 0.1 (reported; gated at the lattice gate plus the effect of the argument's own rounding).
    d = sr - hr is rounded to fp32 once (2^-25 for |d| < 1) and a difference of two d once more (2^-24 for |D| < 2): |delta D| <= 2^-23,
    and rho'' <= 1 / eps, so a term's rho' moves by at most 2^-23 / eps whatever the kernel does after the subtraction -- a property of
    the argument (the fp64 reference subtracts exactly), weighted by the sum of the nine coefficients."""
    shape, eps, w_pix, w_epi = (2, 3, 5, 7), 0.1, 1.0, 0.5
    B, A, H, W = shape
    rng = np.random.default_rng(5)
    sr = rng.random((B, 1, A * H, A * W), dtype=np.float32)
    hr = rng.random((B, 1, A * H, A * W), dtype=np.float32)
    ref3, ref_g = U.reference(sr, hr, A, "charbonnier", eps, w_pix, w_epi)
    c = Call(sr, hr, shape)
    c.run("charbonnier", eps, w_pix, w_epi, 1.0)
    torch.cuda.synchronize()
    out = c.dsr.cpu().numpy().astype(np.float64).reshape(ref_g.shape)
    n, nt = U.counts(*shape)
    coef = w_pix / n + (w_epi / 4) * sum(2.0 / k for k in nt)
    allowance = 2.0 ** -23 / eps * coef / float(np.abs(ref_g).max())
    ge, le = U.grad_error(out, ref_g), U.loss_error([float(x) for x in c.loss3.cpu()], ref3)
    print(f"random inputs, eps {eps}: gradient error {ge:.3e} of the largest element (lattice gate {GRAD_TOL:.1e}, argument rounding up to "
          f"{allowance:.3e}), loss error {le:.2e}")
    assert c.intact() and le <= U.LOSS_RTOL
    assert ge <= GRAD_TOL + allowance


@pytest.mark.gpu
def test_border_semantics_in_one_launch():
    """Image b of 180 is hr + 0.5 e_b, one impulse per mosaic pixel; L1, EPI term only.  The support of dsr[b] must be exactly pixel b,
    its in-view x +- 1 and y +- 1 neighbours and the same pixel of views a2 +- 1 and a1 +- 1: a spatial difference that crossed a view
    border, or an angular one paired with the wrong pixel, shows here."""
    A, H, W = 3, 4, 5
    R, C = A * H, A * W
    B = R * C
    assert B == 180
    hr = np.random.default_rng(3).integers(0, 256, (B, 1, R, C)).astype(np.float32) / 256.0
    sr = hr.copy()
    sr.reshape(B, R * C)[np.arange(B), np.arange(B)] += 0.5
    c = Call(sr, hr, (B, A, H, W))
    c.run("l1", 1e-3, 0.0, 1.0, 1.0)
    torch.cuda.synchronize()
    assert c.intact()
    out = c.dsr.cpu().numpy().reshape(B, R, C)
    for b in range(B):
        r, col = divmod(b, C)
        a1, y, a2, x = r // H, r % H, col // W, col % W
        want = {(r, col)}
        if x > 0: want.add((r, col - 1))
        if x < W - 1: want.add((r, col + 1))
        if y > 0: want.add((r - 1, col))
        if y < H - 1: want.add((r + 1, col))
        if a2 > 0: want.add((r, col - W))
        if a2 < A - 1: want.add((r, col + W))
        if a1 > 0: want.add((r - H, col))
        if a1 < A - 1: want.add((r + H, col))
        got = {(int(i), int(j)) for i, j in zip(*np.nonzero(out[b]))}
        assert got == want, (b, sorted(got ^ want))
        assert out[b, r, col] > 0 and all(out[b, i, j] < 0 for i, j in want - {(r, col)}), b


@pytest.mark.gpu
def test_two_calls_give_identical_bits():
    shape = (3, 2, 33, 65)
    sr, hr = inputs(shape)
    res = []
    for _ in range(2):
        c = Call(sr, hr, shape)
        c.run("charbonnier", 1e-3, 1.0, 0.5, 1.0)
        torch.cuda.synchronize()
        res.append((c.loss3.cpu().numpy().view(np.int32), c.dsr.cpu().numpy().view(np.int32)))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


@pytest.mark.gpu
def test_captured_call_replayed_on_new_inputs_equals_eager():
    shape = (2, 3, 5, 7)
    sr, hr = inputs(shape)
    sr2, hr2 = U.lattice_inputs(*shape, seed=9)
    c = Call(sr, hr, shape)
    args = ("charbonnier", 0.1, 1.0, 0.5, 2.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c.run(*args)                                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c.run(*args)
    c.sr.copy_(torch.from_numpy(sr2.reshape(-1)))
    c.hr.copy_(torch.from_numpy(hr2.reshape(-1)))
    c.dsr.fill_(7.0)
    c.loss3.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    e = Call(sr2, hr2, shape)
    e.run(*args)
    torch.cuda.synchronize()
    assert c.intact()
    assert np.array_equal(c.loss3.cpu().numpy().view(np.int32), e.loss3.cpu().numpy().view(np.int32))
    assert np.array_equal(c.dsr.cpu().numpy().view(np.int32), e.dsr.cpu().numpy().view(np.int32))
    assert U.loss_error([float(x) for x in c.loss3.cpu()], U.reference(sr2, hr2, 3, "charbonnier", 0.1, 1.0, 0.5)[0]) <= U.LOSS_RTOL


NAN = float("nan")
GOOD = dict(penalty=2, eps=1e-3, w_pix=1.0, w_epi=0.5, gscale=1.0)
REFUSALS = [("null_sr", dict(sr=None), ERR_ARG), ("null_hr", dict(hr=None), ERR_ARG), ("null_loss3", dict(loss3=None), ERR_ARG),
            ("null_scratch", dict(scratch=None), ERR_ARG), ("penalty_3", dict(penalty=3), ERR_ARG), ("penalty_neg", dict(penalty=-1), ERR_ARG),
            ("charb_eps_0", dict(eps=0.0), ERR_ARG), ("charb_eps_neg", dict(eps=-1e-3), ERR_ARG), ("charb_eps_nan", dict(eps=NAN), ERR_ARG),
            ("w_pix_neg", dict(w_pix=-1.0), ERR_ARG), ("w_epi_neg", dict(w_epi=-0.5), ERR_ARG), ("w_pix_nan", dict(w_pix=NAN), ERR_ARG),
            ("w_epi_nan", dict(w_epi=NAN), ERR_ARG), ("both_zero", dict(w_pix=0.0, w_epi=0.0), ERR_ARG), ("gscale_nan", dict(gscale=NAN), ERR_ARG),
            ("dsr_is_sr", dict(dsr="sr"), ERR_ARG), ("dsr_is_hr", dict(dsr="hr"), ERR_ARG), ("dsr_inside_sr", dict(dsr="sr+4"), ERR_ARG),
            ("dsr_before_hr", dict(dsr="hr-4"), ERR_ARG),
            ("B_0", dict(B=0), ERR_SHAPE), ("A_0", dict(A=0), ERR_SHAPE), ("H_0", dict(H=0), ERR_SHAPE), ("W_neg", dict(W=-3), ERR_SHAPE),
            ("views_144", dict(A=12), ERR_SHAPE)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,change,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_everything_untouched(name, change, code):
    shape = (2, 3, 5, 7)
    sr, hr = inputs(shape)
    c = Call(sr, hr, shape)
    a = dict(GOOD, sr=c.sr.data_ptr(), hr=c.hr.data_ptr(), dsr=c.dsr.data_ptr(), loss3=c.loss3.data_ptr(), scratch=c.scratch.data_ptr(),
             B=shape[0], A=shape[1], H=shape[2], W=shape[3])
    a.update(change)
    if isinstance(a["dsr"], str):
        a["dsr"] = {"sr": c.sr.data_ptr(), "hr": c.hr.data_ptr(), "sr+4": c.sr.data_ptr() + 16, "hr-4": c.hr.data_ptr() - 16}[a["dsr"]]
    rc = _lib.lib().lft_lf_loss(a["sr"], a["hr"], a["B"], a["A"], a["H"], a["W"], a["penalty"], a["eps"], a["w_pix"], a["w_epi"],
                                a["dsr"], a["gscale"], a["loss3"], a["scratch"], G.stream())
    torch.cuda.synchronize()
    assert rc == code, (name, rc, _lib.lib().lft_last_error())
    assert c.intact()
    assert bool((c.dsr == 7.0).all()) and bool((c.loss3 == 7.0).all()) and bool((c.scratch == 7.0).all())
    assert np.array_equal(c.sr.cpu().numpy(), sr.reshape(-1)) and np.array_equal(c.hr.cpu().numpy(), hr.reshape(-1))


@pytest.mark.gpu
def test_the_good_arguments_of_the_refusal_test_are_accepted():
    shape = (2, 3, 5, 7)
    sr, hr = inputs(shape)
    c = Call(sr, hr, shape)
    assert c.run("charbonnier", GOOD["eps"], GOOD["w_pix"], GOOD["w_epi"], GOOD["gscale"], check=False) == 0
    # MSE and L1 ignore eps
    assert c.run("mse", 0.0, 1.0, 0.0, 1.0, check=False) == 0 and c.run("l1", NAN, 0.0, 1.0, 1.0, check=False) == 0
    torch.cuda.synchronize()
    assert c.intact()
