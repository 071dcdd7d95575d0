"""The product policy of the training GEMMs (Prod<MM>, lft_amd/csrc/lft_train.cuh) in isolation: one wave packs W with the real
pack kernels, splits X, multiplies, and repeats the product with the operand shifted one token left / right (lft_prod_selftest).

No tolerance: the inputs are integers for which every part of the split operands, every product and every partial sum is exact
in fp32 whatever the accumulation order, so every mode must return the exact integer matrix (int64 product on the host).
  16-bit cases (all modes): one operand has 16 significant bits (exactly hi + lo, lo != 0 for most entries), the other |v| <= 8:
      products < 2^19, sums of 16 < 2^23.  bf16x3 drops lo * lo, which is 0 here (the small operand has no lo part).
  24-bit cases (fp32, bf16x6): one operand is odd with 24 significant bits (a + b + c, c != 0), the other is in {-1, 0, 1} with at
      most one non-zero per row: each output is one exact product.  bf16x3 cannot represent these operands, by design.
The bounds are asserted on the host before the GPU call, so an edit of the data cannot silently leave the exact regime."""
import numpy as np
import pytest
import torch

from lft_amd import _lib

import gpu_util as G

pytestmark = pytest.mark.gpu

MODES = {"fp32": _lib.MATH_F32, "bf16x3": _lib.MATH_BF16X3, "bf16x6": _lib.MATH_BF16X6}


def sig_bits(a):
    """Largest number of significant bits of the integers in `a` (bit length without the trailing zeros)."""
    v = np.abs(a.astype(np.int64)).ravel()
    v = v[v != 0]
    v = v // (v & -v)
    return int(np.floor(np.log2(v)).max()) + 1 if v.size else 0


def bf16_inexact(a):
    """Entries whose nearest bf16 differs from them, i.e. whose lo part is non-zero."""
    t = torch.from_numpy(a.astype(np.float32))
    return int((t.to(torch.bfloat16).float() != t).sum())


def wide(rng, bits, shape, odd=False):
    mag = rng.integers(1 << (bits - 1), 1 << bits, size=shape)
    return (mag | 1 if odd else mag) * rng.choice([-1, 1], size=shape)


def one_hot_rows(rng, rows):
    m = np.zeros((rows, 16), dtype=np.int64)
    for r in range(rows):
        if r % 5 != 4:                  # every fifth row stays zero
            m[r, (7 * r + 3) % 16] = rng.choice([-1, 1])
    return m


def make_case(case):
    """(W [32][16], X [32][16]) as int64."""
    rng = np.random.default_rng(11)
    if case in ("w16", "x16"):
        big, small = wide(rng, 16, (32, 16)), rng.integers(-8, 9, size=(32, 16))
        assert sig_bits(big) == 16 and np.abs(big).max() < 1 << 16 and bf16_inexact(big) > big.size // 2
        assert np.abs(small).max() <= 8 and bf16_inexact(small) == 0
    else:
        big, small = wide(rng, 24, (32, 16), odd=True), one_hot_rows(rng, 32)
        assert sig_bits(big) == 24 and np.abs(big).max() < 1 << 24 and (big & 1).all()
        assert np.abs(small).max() == 1 and (np.count_nonzero(small, axis=1) <= 1).all() and len(set(np.nonzero(small)[1])) == 16
    W, X = (big, small) if case[0] == "w" else (small, big)
    # every partial sum, in any order, is bounded by the sum of the magnitudes
    assert (np.abs(X) @ np.abs(W).T).max() < (1 << 23 if case in ("w16", "x16") else 1 << 24)
    return W, X


CASES = [(m, c) for m in MODES for c in ("w16", "x16")] + [(m, c) for m in ("fp32", "bf16x6") for c in ("w24", "x24")]


@pytest.mark.parametrize("mode,case", CASES, ids=lambda v: v)
def test_prod_exact(mode, case):
    W, X = make_case(case)
    w, x = (torch.from_numpy(a.astype(np.float32)).to(G.DEV) for a in (W, X))
    assert torch.equal(w.cpu().long(), torch.from_numpy(W)) and torch.equal(x.cpu().long(), torch.from_numpy(X))   # exact as fp32
    Y, Yl, Yr = (torch.full((32, 32), float("nan"), device=G.DEV) for _ in range(3))
    _lib.call("lft_prod_selftest", w.data_ptr(), x.data_ptr(), Y.data_ptr(), Yl.data_ptr(), Yr.data_ptr(), MODES[mode], G.stream())
    torch.cuda.synchronize()
    zero = np.zeros((1, 16), dtype=np.int64)
    for name, got, Xs in (("Y", Y, X), ("Yl", Yl, np.concatenate([zero, X[:-1]])), ("Yr", Yr, np.concatenate([X[1:], zero]))):
        ref = torch.from_numpy(Xs @ W.T)                                  # int64, [token][o]
        bad = (got.cpu().double() != ref.double()).nonzero()
        assert bad.numel() == 0, f"{name} [{mode}, {case}]: {len(bad)} of 1024 entries differ, first at {bad[0].tolist()}: " \
                                 f"{got.cpu()[tuple(bad[0])].item()!r} != {ref[tuple(bad[0])].item()}"
