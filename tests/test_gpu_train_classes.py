"""GPU parity of the training step in EVERY size class of its dispatch: the kernels run_lin / wgrad choose by token count
N = B A^2 h w and view width (k_lin<1|2|4, MM, tiled | untiled>, the ring-fed k_linr<2|4, MM, 0|4|8>, k_wgrad's fast3 path, weight
gradient chunking with empty chunks and short last shares, k_ln_bwd at its block cap), against float64 autograd over the oracle.
tests/test_gpu_train.py compares gradients with a reference up to 12 800 tokens, where every GEMM but two runs k_lin<1>.

Each case (tests/train_classes.py: GPU_CASES, with the classes it must reach -- asserted here and, without a GPU, in
tests/test_train_classes.py) builds one forward tape per math mode and runs lft_train_block_backward for the up-sampler, SpaTrans of
layer 1, AngTrans of layer 0 and the feature extractor.  As in test_block_backward_matches_oracle_autograd the block's input is our
tape's activation, the incoming gradient random, the ReLU / LeakyReLU branches ours; the reference (tests/train_ref.py) is autograd in
FLOAT64, SpaTrans over chunks of view images.  The block's own forward output on the tape is compared with the reference's as well.
One whole-network case above the ring threshold (11 x 11 views, 72 600 tokens) checks all 78 gradients: the gradient arena, the
partial-sum buffer at its high-water mark and the chained reduction segments at ring sizes.

Gates, per tensor, relative to max|ref|: the project's TOL = 1e-3 (hard), and a tight level that makes the test sensitive:
KINK_ALIGNED_LEVEL (fp32 / bf16x6 5e-5, bf16x3 3e-4) wherever it holds; where a case exceeds it the level is 4 x the reference's
OWN fp32 noise (torch-fp32 autograd of the same block against the fp64 one, same inputs and branches: tests/diag_train_class_levels.py
prints it), x 6 (= 3e-4 / 5e-5) for bf16x3 -- never a figure taken from our kernels.

MEASURED (tests/diag_train_class_levels.py on an MI355X; worst tensor of the four blocks, relative to max|ref|):
  case               tokens   reference's fp32 noise   ours fp32   bf16x3    bf16x6    tight level (fp32 / bf16x3 / bf16x6)
  A2_s2_B1_32x32      4 096   3.9e-6                   2.9e-6      2.0e-5    3.4e-6    5e-5 / 3e-4 / 5e-5
  A5_s2_B16_10x10    40 000   3.4e-6                   2.1e-6      1.9e-5    7.3e-6    5e-5 / 3e-4 / 5e-5
  A8_s4_B16_8x8      65 536   5.7e-6                   4.1e-6      1.6e-5    1.3e-5    5e-5 / 3e-4 / 5e-5
  A11_s2_B6_10x10    72 600   1.1e-5                   8.7e-6      1.2e-5    1.1e-5    5e-5 / 3e-4 / 5e-5
  A5_s2_B3_32x32     76 800   1.3e-5                   4.5e-6      1.6e-5    1.3e-5    5e-5 / 3e-4 / 5e-5
  A6_s4_B2_31x31     69 192   8.0e-6                   1.3e-6      1.6e-5    1.8e-5    5e-5 / 3e-4 / 5e-5
  whole network, A11_s2_B6_10x10 (78 gradients)        2.1e-6      3.2e-5    2.6e-6    (hard gate only)
Block forward outputs: <= 1.0e-6 (fp32, bf16x6), <= 1.1e-5 (bf16x3).  No case exceeds KINK_ALIGNED_LEVEL, so LEVEL below is empty: the
weight gradients sum six times the tokens of the fixtures, and the reference's own fp32 noise grows to 1.3e-5 with them, ours stays
below it in fp32.  No comparison failed: the size classes held no defect.  Mutation check (scratch builds, not committed): the dx of
k_linr<.., KS3>'s transposed taps not flipped -> A5_s2_B3_32x32 spa (d_in 1.2) and init fail; k_wgrad dropping a wave's short
last share -> all four blocks of A11_s2_B6_10x10 fail (2e-2); fast3's left neighbour read across the row seam -> spa and init of
both 32-wide cases fail, the other blocks pass.
CPU cost of the fp64 reference: 0.1 .. 4.5 s per block (the 4x up-sampler is the slowest), 9 s for the whole network.
Wall time of the tests: 0.2 .. 4.8 s per block test, 9.3 .. 9.7 s per whole-network test.
"""
import time

import pytest
import torch

from lft_amd import _lib, train as T
from lft_amd.params import param_table
from oracle import lft_oracle as O

import gpu_util as G
import train_classes as C
import train_ref as R
from test_gpu_train import KINK_ALIGNED_LEVEL, TOL, compare_all, make_inputs, our_branches

pytestmark = pytest.mark.gpu

BLOCK_OF = {"upsample": (_lib.BLOCK_UPSAMPLE, 0), "spa": (_lib.BLOCK_SPA, 1), "ang": (_lib.BLOCK_ANG, 0), "init": (_lib.BLOCK_INIT, 0)}
OUT_TAPE = {"spa": "spa1.y", "ang": "ang0.y", "init": "feat"}
IN_TAPE = {"upsample": "body", "spa": "ang1.y", "ang": "feat"}
# Tight level per (shape, math) where it is not KINK_ALIGNED_LEVEL: 4 x the measured fp32 noise of the reference (see the header).
LEVEL = {}
WHOLE = (11, 2, 6, 10, 10)

_live = {}           # the one forward tape alive: {"key": (shape, math), "case": {...}}; the largest is about 3 GiB


def level(shape, math):
    return LEVEL.get((shape, math), KINK_ALIGNED_LEVEL[math])


def get_case(shape, math):
    """The forward tape of (shape, math); the previous one is freed first."""
    if _live.get("key") != (shape, math):
        _live.clear()
        torch.cuda.empty_cache()
        A, s, B, h, w = shape
        sd_np, lr, hr = make_inputs(A, s, B, h, w)
        names = [n for n, _, _ in param_table(64, s)]
        ps = [torch.from_numpy(sd_np[n]).to(G.DEV).contiguous() for n in names]
        lr_d = lr.to(G.DEV)
        out, tape = T.train_forward(ps, lr_d, A, s, math=math)
        torch.cuda.synchronize()
        _live.update(key=(shape, math), case=dict(math=math, sd=O.state_from_numpy(sd_np), A=A, s=s, B=B, h=h, w=w, names=names, ps=ps,
                                                  lr=lr_d, hr=hr, out=out, tape=tape))
    return _live["case"]


@pytest.fixture(scope="module", autouse=True)
def _free_last_tape():
    yield
    _live.clear()
    torch.cuda.empty_cache()


def block_inputs(case, kind):
    """(block input [B,64,V,h,w] or None, incoming gradient in the layout of the block's output, branch masks) from OUR tape."""
    A, s, B, h, w = case["A"], case["s"], case["B"], case["h"], case["w"]
    V, ss = A * A, s * s
    block, layer = BLOCK_OF[kind]
    tv = lambda name, ch=64: T.tape_view(case["tape"], name, B, A, h, w, s, (B, V, h, w, ch))       # noqa: E731
    pos = lambda name, ch: (tv(name, ch) > 0).cpu()                                                   # noqa: E731
    if kind == "init":
        masks = {f"conv{i}": pos(nm, 64).permute(0, 4, 1, 2, 3) for i, nm in zip((0, 2, 4), ("c1", "c2", "c3"))}
    elif kind == "ang":
        masks = {f"ang{layer}": pos(f"ang{layer}.hdn", 128).permute(1, 0, 2, 3, 4).reshape(V, B * h * w, 128)}
    elif kind == "spa":
        masks = {f"spa{layer}": pos(f"spa{layer}.hdn", 256).permute(2, 3, 0, 1, 4).reshape(h * w, B * V, 256)}
    else:
        masks = {"up": O.views_to_mosaic(pos("act", 64 * ss).permute(0, 4, 1, 2, 3), A)}
    x = None if kind == "init" else tv(IN_TAPE[kind]).cpu().permute(0, 4, 1, 2, 3).contiguous()
    shape = (B, 1, A * h * s, A * w * s) if kind == "upsample" else (B, 64, V, h, w)
    gen = torch.Generator().manual_seed(11 + 7 * block + layer)
    n = 1
    for d in shape:
        n *= d
    d_out = torch.randn(shape, generator=gen) / n ** 0.5
    return x, d_out, masks


def reference(case, kind, x, d_out, masks):
    """The fp64 reference of the block on OUR input and branches (they differ between the math modes, so each mode has its own)."""
    return R.block_reference(kind, case["sd"], BLOCK_OF[kind][1], x, case["lr"].cpu(), d_out, case["A"], case["s"], masks)


def ours(case, kind, d_out):
    """lft_train_block_backward of the block and the block's forward output from the tape, as a train_ref result (CPU tensors);
    asserts that no gradient outside the block was written, that none inside is NaN, and the number of tensors."""
    A, s, B, h, w = case["A"], case["s"], case["B"], case["h"], case["w"]
    V = A * A
    block, layer = BLOCK_OF[kind]
    d_out_dev = (d_out if kind == "upsample" else d_out.permute(0, 2, 3, 4, 1)).contiguous().to(G.DEV)
    flat = torch.full((T.grad_floats(s),), float("nan"), device=G.DEV)
    d_in = T.block_backward(case["ps"], case["lr"], case["tape"], block, layer, d_out_dev, A, s, flat, math=case["math"])
    torch.cuda.synchronize()
    prefix = R.PREFIX[kind].format(layer)
    grads, off = {}, 0
    for name, p in zip(case["names"], case["ps"]):
        k = p.numel()
        got = flat[off:off + k]
        off += k
        if name.startswith(prefix):
            assert not bool(torch.isnan(got).any()), name
            grads[name] = got.cpu().view(p.shape)
        else:
            assert bool(torch.isnan(got).all()), f"{name}: a gradient outside the block was written"
    assert off == flat.numel() and len(grads) == R.COUNT[kind] == {"upsample": 2, "spa": 10, "ang": 8, "init": 4}[kind]
    if kind == "upsample":
        y = case["out"].cpu().double() - O.bicubic_skip(case["lr"].cpu().double(), A, s)
    else:
        y = T.tape_view(case["tape"], OUT_TAPE[kind], B, A, h, w, s, (B, V, h, w, 64)).cpu().permute(0, 4, 1, 2, 3)
    if d_in is not None:
        assert not bool(torch.isnan(d_in).any()), "d_in"
        d_in = d_in.cpu().permute(0, 4, 1, 2, 3)
    return {"y": y, "d_in": d_in, "grads": grads}


_ID = lambda v: ("A%d_s%d_B%d_%dx%d" % v) if isinstance(v, tuple) else str(v)      # noqa: E731
BLOCK_PARAMS = [(shape, math, kind) for shape, blocks in C.GPU_CASES for math in C.MATHS for kind in blocks]


@pytest.mark.parametrize("shape,math,kind", BLOCK_PARAMS, ids=_ID)
def test_block_backward_in_every_size_class(shape, math, kind):
    C.check_case(shape)                                   # the case still reaches the classes it was chosen for
    t0 = time.time()
    case = get_case(shape, math)
    x, d_out, masks = block_inputs(case, kind)
    t1 = time.time()
    got = ours(case, kind, d_out)
    t2 = time.time()
    ref = reference(case, kind, x, d_out, masks)
    t3 = time.time()
    fwd = float((got["y"] - ref["y"]).abs().max() / ref["y"].abs().max())
    errs = R.rel_errors(got, ref)
    worst = max(errs, key=errs.get)
    print(f"{_ID(shape)} {math} {kind}: forward {fwd:.2e}; worst gradient {errs[worst]:.2e} ({worst}); level {level(shape, math):.1e}; "
          f"tape + inputs {t1 - t0:.1f} s, GPU {t2 - t1:.1f} s, fp64 reference {t3 - t2:.1f} s")
    assert fwd <= TOL, f"{kind} forward output: {fwd:.3e}"
    for name, e in errs.items():
        assert e <= TOL, f"{name}: {e:.3e} of max|ref| (hard gate {TOL})"
    for name, e in errs.items():
        assert e <= level(shape, math), f"{name}: {e:.3e} of max|ref| (tight gate {level(shape, math):.1e})"


@pytest.mark.parametrize("math", C.MATHS)
def test_all_78_gradients_above_the_ring_threshold(math):
    """test_all_78_gradients_exact_given_our_branches at 72 600 tokens (11 x 11 views; every GEMM but VW_UPM rides the ring): the full
    backward pass -- arena, partial-sum buffer, chained reduction segments -- against fp64 autograd over the whole oracle, told to
    take OUR branches and to start from OUR d loss / d out."""
    assert C.check_case(WHOLE)["N"] > C.RING_N
    case = get_case(WHOLE, math)
    A, s = case["A"], case["s"]
    out, hr = case["out"], case["hr"].to(G.DEV)
    dout = torch.empty_like(out)
    scratch = torch.empty(1025, device=G.DEV)
    _lib.call("lft_l1_loss", out.data_ptr(), hr.data_ptr(), out.numel(), dout.data_ptr(), 1.0 / out.numel(), scratch[1024:].data_ptr(),
              scratch.data_ptr(), G.stream())
    case["flat"] = T.train_backward(case["ps"], case["lr"], case["tape"], dout, A, s, math=math)
    torch.cuda.synchronize()
    masks, dout_c = our_branches(case), dout.cpu()
    t0 = time.time()
    O.branch_masks = masks
    try:
        ref = O.param_grads({k: v.double() for k, v in case["sd"].items()}, case["lr"].cpu().double(), A, s, dout_c.double())
    finally:
        O.branch_masks = None
    print(f"whole network {_ID(WHOLE)} {math}: fp64 reference {time.time() - t0:.1f} s")
    try:
        compare_all(case, ref, "backward given our branches, 72 600 tokens")
    finally:
        del case["flat"]
