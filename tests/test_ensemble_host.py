"""CPU-side tests of the self-ensemble feature: the C ABI is declared, exported and bound, the masks are the documented ones, the
transforms' definition is self-consistent, argument errors come before any device work, and nothing falls back to the CPU."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from lft_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lft_dihedral_batch", "lft_dihedral_expand", "lft_dihedral_merge", "lft_scene_integrate_ens")


def T(x, t):
    if t & 1:
        x = x.flip(-1)
    if t & 2:
        x = x.flip(-2)
    if t & 4:
        x = x.transpose(-1, -2)
    return x


def Tinv(y, t):
    if t & 4:
        y = y.transpose(-1, -2)
    if t & 2:
        y = y.flip(-2)
    if t & 1:
        y = y.flip(-1)
    return y


def test_abi_declares_and_exports_the_transforms():
    hdr = open(os.path.join(ROOT, "include", "lft_hip.h")).read()
    declared = set(re.findall(r"^int\s+(lft_\w+)\s*\(", hdr, flags=re.M))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.EXPORTS)
    assert re.search(r"^#define LFT_ABI_VERSION 5$", hdr, flags=re.M) and _lib.ABI_VERSION == 5      # additive: no version bump
    _lib.build()
    L = _lib.lib()
    assert L.lft_version() == 5
    for name in NEW:
        assert hasattr(L, name), name


def test_masks():
    from lft_amd import ensemble
    assert ensemble.MASKS == {"dihedral": 0xFF, "flips": 0x0F, "none": 0x01}
    assert ensemble.codes_of(0xA5) == [0, 2, 5, 7] and ensemble.mask_of("flips") == 0x0F and ensemble.mask_of(0xA5) == 0xA5
    for bad in ("rot90", 0, 0x100):
        with pytest.raises(ValueError):
            ensemble.mask_of(bad)


def test_transform_definition_round_trips():
    """The torch restatement of the contract the GPU tests compare with: T_t^-1(T_t(x)) == x for every code; 5 and 6 are each other's
    inverse, not their own."""
    sq, rect = torch.arange(36.0).reshape(6, 6), torch.arange(35.0).reshape(5, 7)
    for t in range(8):
        assert torch.equal(Tinv(T(sq, t), t), sq)
        assert T(sq, t).shape == (6, 6)
        if not t & 4:
            assert torch.equal(Tinv(T(rect, t), t), rect)
    assert all(not torch.equal(T(T(sq, t), t), sq) for t in (5, 6))
    assert torch.equal(T(T(sq, 5), 6), sq) and torch.equal(T(T(sq, 6), 5), sq)
    assert all(torch.equal(T(T(sq, t), t), sq) for t in (0, 1, 2, 3, 4, 7))
    assert T(rect, 4).shape == (7, 5)


def test_argument_errors_come_before_any_launch():
    """Never-dereferenced pointers (1, 2): every call is rejected by its argument checks (no GPU needed)."""
    L = _lib.lib()
    ARG, SHAPE = -1, -2
    for fn in (L.lft_dihedral_expand, L.lft_dihedral_merge):
        assert fn(None, 2, 0xFF, 1, 4, 4, None) == ARG and fn(1, None, 0xFF, 1, 4, 4, None) == ARG
        assert fn(1, 1, 0xFF, 1, 4, 4, None) == ARG                       # in == out
        assert fn(1, 2, 0, 1, 4, 4, None) == ARG and fn(1, 2, 0x100, 1, 4, 4, None) == ARG
        assert b"mask" in L.lft_last_error()
        assert fn(1, 2, 0xFF, 0, 4, 4, None) == SHAPE and fn(1, 2, 0xFF, 1, 0, 4, None) == SHAPE and fn(1, 2, 0xFF, 1, 4, -1, None) == SHAPE
    assert L.lft_dihedral_batch(1, 2, None, 1, 4, 4, None) == ARG
    assert L.lft_dihedral_batch(None, 2, 3, 1, 4, 4, None) == ARG and L.lft_dihedral_batch(1, 1, 3, 1, 4, 4, None) == ARG
    assert L.lft_dihedral_batch(1, 2, 3, 0, 4, 4, None) == SHAPE
    ens = L.lft_scene_integrate_ens
    assert ens(None, 2, 0xFF, 2, 20, 20, 8, 4, 2, None) == ARG and ens(1, 1, 0xFF, 2, 20, 20, 8, 4, 2, None) == ARG
    assert ens(1, 2, 0, 2, 20, 20, 8, 4, 2, None) == ARG and ens(1, 2, 0x1FF, 2, 20, 20, 8, 4, 2, None) == ARG
    assert ens(1, 2, 0xFF, 0, 20, 20, 8, 4, 2, None) == SHAPE and ens(1, 2, 0xFF, 2, 20, 20, 8, 4, 0, None) == SHAPE
    assert ens(1, 2, 0xFF, 2, 0, 20, 8, 4, 2, None) == SHAPE and ens(1, 2, 0xFF, 2, 20, 20, 4, 8, 2, None) == SHAPE


def test_no_cpu_fallback():
    from lft_amd import ensemble, trainer
    from model import LFT
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=2, scale_factor=2))
    x = torch.zeros(1, 1, 12, 12)
    with pytest.raises(_lib.LftError):
        net.self_ensemble(x)
    with pytest.raises(_lib.LftError):
        ensemble.self_ensemble(net, x, mode="flips")
    for fn in (lambda: ensemble.expand(x, 0xFF), lambda: ensemble.merge(x, 0x01), lambda: ensemble.dihedral_batch(x, [3])):
        with pytest.raises(_lib.LftError):
            fn()
    import numpy as np
    with pytest.raises(_lib.LftError):
        trainer.augment_gpu(x, x, np.random.default_rng(0))
