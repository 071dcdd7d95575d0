"""CPU-side tests of the attention-map export (lft_amd/attention.py, lft_attn_maps_floats / lft_train_attn_maps): sizes and
argument validation of the C ABI (no device is touched), the compact <-> dense conversion, and the integrity of the reference
fixtures tests/golden/attention_*.npz (tools/gen_golden_attention.py)."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from lft_amd import _lib, attention as AT
from oracle import lft_oracle as O

import attention_util as U

ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -3          # LFT_ERR_* of include/lft_hip.h


def test_header_declares_the_maps_abi_and_the_version_stays():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lft_hip.h")).read()
    assert "#define LFT_MAPS_MEAN 0" in hdr and "#define LFT_MAPS_HEADS 1" in hdr
    assert (_lib.MAPS_MEAN, _lib.MAPS_HEADS) == (0, 1)
    assert {"lft_attn_maps_floats", "lft_train_attn_maps"} <= set(_lib.EXPORTS)
    assert "#define LFT_ABI_VERSION 5" in hdr and _lib.ABI_VERSION == 5           # additive: no existing signature changed


@pytest.mark.parametrize("B,A,h,w", [(2, 5, 32, 32), (1, 9, 8, 8), (3, 3, 7, 12), (1, 2, 12, 6)])
def test_map_sizes_are_the_products_of_the_layouts(B, A, h, w):
    V = A * A
    assert AT.map_floats(_lib.BLOCK_ANG, False, B, A, h, w) == B * h * w * V * V
    assert AT.map_floats(_lib.BLOCK_ANG, True, B, A, h, w) == B * h * w * 8 * V * V
    assert AT.map_floats(_lib.BLOCK_SPA, False, B, A, h, w) == B * V * h * w * 25
    assert AT.map_floats(_lib.BLOCK_SPA, True, B, A, h, w) == B * V * 8 * h * w * 25
    for block in (_lib.BLOCK_ANG, _lib.BLOCK_SPA):
        for per_head in (False, True):
            n = 1
            for d in AT.map_shape(block, per_head, B, A, h, w):
                n *= d
            assert n == AT.map_floats(block, per_head, B, A, h, w)


def test_arguments_are_validated_before_any_device_work():
    """Every refusal below comes back before a stream, the tape or the output is touched: the pointers are not device memory
    (this test runs without a GPU)."""
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    fl = lambda block, mode, B=1, A=5, h=8, w=8, out=ctypes.byref(n): L.lft_attn_maps_floats(block, mode, B, A, h, w, out)   # noqa: E731
    assert fl(_lib.BLOCK_UPSAMPLE, 0) == ERR_ARG and b"block" in L.lft_last_error()
    assert fl(_lib.BLOCK_INIT, 0) == ERR_ARG and fl(7, 0) == ERR_ARG
    assert fl(_lib.BLOCK_ANG, 2) == ERR_ARG and b"heads_mode" in L.lft_last_error()
    assert fl(_lib.BLOCK_SPA, -1) == ERR_ARG
    assert fl(_lib.BLOCK_ANG, 0, out=None) == ERR_ARG
    assert fl(_lib.BLOCK_ANG, 0, A=12) == ERR_UNSUPPORTED
    assert fl(_lib.BLOCK_ANG, 0, h=0) == ERR_SHAPE

    fake = ctypes.c_void_p(4096)           # never dereferenced

    def maps(tape=fake, block=_lib.BLOCK_ANG, layer=0, mode=_lib.MAPS_MEAN, out=fake, B=1, A=5, h=8, w=8, s=2):
        return L.lft_train_attn_maps(tape, block, layer, mode, out, B, A, h, w, s, None)

    assert maps(block=_lib.BLOCK_UPSAMPLE) == ERR_ARG and b"block" in L.lft_last_error()
    assert maps(block=_lib.BLOCK_INIT) == ERR_ARG
    assert maps(mode=2) == ERR_ARG and b"heads_mode" in L.lft_last_error()
    assert maps(mode=-1) == ERR_ARG
    assert maps(layer=4) == ERR_ARG and b"layer" in L.lft_last_error()
    assert maps(layer=-1) == ERR_ARG
    assert maps(tape=None) == ERR_ARG and maps(out=None) == ERR_ARG
    assert maps(s=3) == ERR_SHAPE and b"scale factor" in L.lft_last_error()
    assert maps(A=12) == ERR_UNSUPPORTED
    assert maps(block=_lib.BLOCK_SPA, s=3) == ERR_SHAPE and maps(block=_lib.BLOCK_SPA, A=12) == ERR_UNSUPPORTED


def test_attention_maps_refuses_cpu_tensors():
    from model import LFT
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=5, scale_factor=2))
    with pytest.raises(_lib.LftError):
        AT.attention_maps(net, torch.zeros(1, 1, 40, 40))
    with pytest.raises(_lib.LftError):
        net.attention_maps(torch.zeros(1, 1, 40, 40), per_head=True)
    with pytest.raises(_lib.LftError):
        AT.scene_angular_attention(net, torch.zeros(5 * 48, 5 * 40), 0)


@pytest.mark.parametrize("h,w", [(6, 6), (6, 12), (12, 6), (3, 4), (1, 7)])
def test_compact_and_dense_forms_convert_exactly(h, w):
    g = torch.Generator().manual_seed(h * 100 + w)
    inside = (O.window_mask(h, w) == 0)
    dense = torch.rand((2, 3, h * w, h * w), generator=g) * inside             # weight only where the reference allows it
    c = AT.compact_from_dense(dense, h, w)
    assert tuple(c.shape) == (2, 3, h, w, 5, 5)
    assert torch.equal(AT.dense_spatial(c, h, w), dense)
    # taps outside the view are 0 in the compact form, and a dense weight outside the 5x5 taps is dropped, not moved
    _, in_view = AT._window_index(h, w, "cpu")
    assert torch.all(c.reshape(2, 3, h * w, 25)[..., ~in_view] == 0)
    with pytest.raises(ValueError):
        AT.dense_spatial(c, h + 1, w)


@pytest.mark.parametrize("name", U.FIXTURES)
def test_reference_puts_no_weight_outside_the_compact_window(name):
    z, _, _, (A, s, B, h, w) = U.load_fixture(name)
    mask_open = (O.window_mask(h, w) == 0)
    empty = U.empty_window_queries(h, w).reshape(-1)
    assert bool(empty.any()) == (h < w)
    for l in range(4):
        x = torch.from_numpy(z[f"spa{l}_mean_dense"])                            # as the reference returned it
        assert tuple(x.shape) == (B, A * A, h * w, h * w)
        nan_rows = torch.isnan(x).all(dim=-1)
        assert torch.equal(nan_rows, empty.view(1, 1, -1).expand_as(nan_rows))    # torch's NaN rows are the empty windows, nothing else
        assert not torch.isnan(x[:, :, ~empty]).any()
        x0 = torch.nan_to_num(x)
        c = AT.compact_from_dense(x, h, w)
        assert torch.equal(torch.nan_to_num(c), torch.nan_to_num(torch.from_numpy(z[f"spa{l}_mean"])))
        assert torch.equal(AT.dense_spatial(torch.nan_to_num(c), h, w), x0)        # exactly: the compact form loses nothing
        assert torch.equal((x0 != 0)[:, :, ~empty], mask_open[~empty].expand(B, A * A, -1, -1))
        rows = x0[:, :, ~empty].sum(-1)
        assert float((rows - 1).abs().max()) <= 1e-5


@pytest.mark.parametrize("name", U.FIXTURES)
def test_fixtures_match_the_functional_attention_on_oracle_taps(name):
    """Fixture integrity: the maps of the REAL reference equal torch's functional multi-head attention on the oracle's taps
    within the fp32 stage tolerance (measured: <= 2.4e-7 absolute on maps whose maximum is 0.07 .. 0.5)."""
    z, sd, lr, (A, s, B, h, w) = U.load_fixture(name)
    for per_head, key in ((False, "mean"), (True, "heads")):
        got = U.functional_maps(sd, lr, A, s, per_head)
        for l in range(4):
            for kind in ("ang", "spa"):
                if f"{kind}{l}_{key}" not in z.files:
                    continue
                ref = torch.from_numpy(z[f"{kind}{l}_{key}"])
                g = got[f"{kind}{l}"]
                assert g.shape == ref.shape
                assert torch.equal(torch.isnan(g), torch.isnan(ref))
                ref, g = torch.nan_to_num(ref), torch.nan_to_num(g)
                rel = float((g - ref).abs().max() / ref.abs().max())
                print(f"{name} {kind}{l} {key}: max {float(ref.max()):.3f} abs err {float((g - ref).abs().max()):.2e} rel_max {rel:.2e}")
                assert rel <= U.FP32_STAGE_TOL, (kind, l, key, rel)
    assert all(f"{kind}{l}_heads" in z.files for kind in ("ang", "spa") for l in (0, 3))


@pytest.mark.parametrize("A", range(1, 12))
def test_am_div_is_exact_for_every_view_count(A):
    """k_ang_maps (lft_attn_maps.cuh) splits a flat element e of a [V][V] map into (e / V, e % V) with a float product,
    (int)(((float)e + 0.5f) * (1.0f / (float)V)): the same expression in fp32 numpy equals e // V for every e < V*V."""
    import numpy as np
    V = A * A
    e = np.arange(V * V, dtype=np.int64)
    inv = np.float32(1.0) / np.float32(V)
    i = ((e.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int64)
    assert i.dtype == np.int64 and ((e.astype(np.float32) + np.float32(0.5)) * inv).dtype == np.float32
    assert np.array_equal(i, e // V)
