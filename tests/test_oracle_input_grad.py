"""The CPU oracle's autograd gradient with respect to the INPUT reproduces the real reference's (tests/golden/input_grad_*.npz,
tools/gen_golden_input_grad.py).  This pins the yardstick of tests/test_gpu_input_grad.py: it checks the oracle, not the HIP
kernels, and passes without a GPU."""
import glob
import os

import numpy as np
import pytest
import torch

from lft_amd.params import deterministic_state, synthetic_lr
from oracle import lft_oracle as O
from fixture_util import stats, sub_indices

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "input_grad_*.npz")))
TOL = 1e-3


def fixture_inputs(g):
    A, s, B, h, w, wseed, iseed, dseed = (int(v) for v in g["meta"])
    sd_np = deterministic_state(64, s, seed=wseed, flavor=str(g["flavor"]))
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=iseed))
    rng = np.random.Generator(np.random.PCG64([dseed, B, A, h, w, s]))
    dout = torch.from_numpy(rng.standard_normal((B, 1, A * h * s, A * w * s), dtype=np.float32))
    return (A, s, B, h, w), sd_np, lr, dout


def oracle_input_grad(sd, lr, dout, A, s):
    x = lr.detach().clone().requires_grad_()
    with torch.enable_grad():
        out = O._forward(sd, x, A, s, None)            # O.forward would drop autograd: no weight requires grad
        (g,) = torch.autograd.grad(out, x, dout)
    return g


def compare_to_fixture(g, got: np.ndarray):
    """max |got - ref| / max |ref| over the fixture's stored elements (whole tensor when stored), and the statistics check."""
    a = got.astype(np.float32).ravel()
    if "d_lr_full" in g.files:
        ref = g["d_lr_full"].ravel()
        err = float(np.abs(a - ref).max() / np.abs(ref).max())
    else:
        ref = g["d_lr_sub"]
        err = float(np.abs(a[sub_indices(a.size)] - ref).max() / np.abs(ref).max())
    st, rst = stats(a), g["d_lr_stats"]
    assert st[0] == rst[0]
    return err, abs(st[2] - rst[2]) / rst[2]


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_oracle_input_grad_matches_reference(path):
    g = np.load(path)
    (A, s, B, h, w), sd_np, lr, dout = fixture_inputs(g)
    got = oracle_input_grad(O.state_from_numpy(sd_np), lr, dout, A, s)
    assert tuple(got.shape) == (B, 1, A * h, A * w)
    err, l1_rel = compare_to_fixture(g, got.numpy())
    print(f"{os.path.basename(path)}: rel max err {err:.2e}, sum|.| rel {l1_rel:.2e}, min |pre-activation| {float(g['min_abs_pre']):.1e}")
    assert err <= TOL
    assert l1_rel <= TOL


def test_fixtures_present():
    assert len(FILES) >= 5
