"""CPU tests of the colour path's host side: the up-scaling tables, the numpy restatement against the reference's fixtures
(tools/gen_golden_colour.py), the inverse transform, the PNG writer, and the argument errors of lft_amd.colour."""
import os
import struct
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import colour, png
from lft_amd._lib import LftError

from colour_util import CASES, TABLE_LENGTHS, colour_np, load_case, quantise, rgb2ycbcr, tie_distance, ulp_diff, ycc2rgb


def test_up_contributions_equal_the_reference_tables(golden_dir):
    t = np.load(os.path.join(golden_dir, "colour_tables.npz"))
    for L in TABLE_LENGTHS:
        for s in (2, 4):
            w, i = colour.up_contributions(L, s)
            assert w.dtype == np.float64 and i.dtype == np.int32
            assert w.shape == i.shape == (L * s, 4) == t[f"w_{L}_{s}"].shape, (L, s)
            assert np.array_equal(w, t[f"w_{L}_{s}"]) and np.array_equal(i, t[f"i_{L}_{s}"]), (L, s)
            assert i.min() >= 0 and i.max() <= L - 1
    with pytest.raises(ValueError):
        colour.up_contributions(0, 2)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_fixture(golden_dir, name):
    U, V, A, H, W, s, cls, v73 = CASES[name]
    g = load_case(golden_dir, name)
    assert g["lf"].shape == (U, V, H, W, 3) and g["lf"].dtype == cls and tuple(g["meta"]) == (A, s, int(v73))
    assert g["sr_y"].dtype == np.float32 and g["sr_y"].shape == (A * s * H, A * s * W)
    assert g["sr_y"].min() < 0 and g["sr_y"].max() > 1        # the clip is exercised
    r = colour_np(g["lf"], A, s, g["sr_y"])
    for k in ("ycc", "lr_y", "cb_up", "cr_up", "rgb"):
        assert g[k].dtype == np.float32 and g[k].shape == r[k].shape, k
        assert ulp_diff(r[k].astype(np.float32), g[k]).max() <= 1, (name, k)
    assert tie_distance(r["rgb"]).min() > 1e-6                                       # the generator's guarantee
    assert g["out"].dtype == np.uint8 and np.array_equal(r["out"], g["out"])
    assert (g["out"] == 0).any() and (g["out"] == 255).any()
    b = colour_np(g["lf"], A, s, None)
    assert tie_distance(b["rgb"]).min() > 1e-6
    assert np.array_equal(b["out"], g["out_base"])
    assert np.array_equal(b["cb_up"], r["cb_up"]) and np.array_equal(b["cr_up"], r["cr_up"])


def test_saturated_case_overshoots_on_both_sides(golden_dir):
    g = load_case(golden_dir, "sat_s4_u8")
    assert (g["lf"] == 0).mean() > 0.2 and (g["lf"] == 255).mean() > 0.2
    b = colour_np(g["lf"], 3, 4, None)["rgb"]
    assert b.min() < -0.02 and b.max() > 1.02                                        # the cubic's overshoot, clipped in out_base


def test_inverse_matrix_round_trip():
    m = colour.inverse_matrix()
    assert m.dtype == np.float64 and np.abs(m @ colour.YCBCR_MATRIX - np.eye(3)).max() < 1e-15
    rng = np.random.default_rng(0)
    for x in (rng.random((50, 40, 3)), rng.integers(0, 256, (50, 40, 3)).astype(np.float64) / 255.0,
              np.array([[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]])):
        ycc = rgb2ycbcr(x)
        assert np.abs(ycc2rgb(ycc[..., 0], ycc[..., 1], ycc[..., 2]) - x).max() <= 1e-12
        assert np.array_equal(quantise(ycc2rgb(ycc[..., 0], ycc[..., 1], ycc[..., 2])), np.rint(255 * x).astype(np.uint8))
    # the form that subtracts the offsets after the matrix (the reference's ycbcr2rgb) is not an inverse
    ycc = rgb2ycbcr(rng.random((8, 8, 3)))
    wrong = np.einsum("jk,...k->...j", m * 255.0, ycc) - np.array([16.0, 128.0, 128.0]) / 255.0
    assert np.abs(wrong - ycc2rgb(ycc[..., 0], ycc[..., 1], ycc[..., 2])).max() > 0.5


def _chunks(buf):
    assert buf[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(buf):
        n, kind = struct.unpack(">I4s", buf[pos:pos + 8])
        data = buf[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", buf[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + data) & 0xFFFFFFFF, kind
        out.append((kind, data))
        pos += 12 + n
    assert pos == len(buf)
    return out


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (7, 2), (16, 33), (40, 64)])
def test_png_write_read_identity(tmp_path, h, w):
    img = np.random.default_rng(h * 100 + w).integers(0, 256, (h, w, 3)).astype(np.uint8)
    path = str(tmp_path / "a.png")
    png.write_png(path, img)
    back = png.read_png(path)
    assert back.dtype == np.uint8 and np.array_equal(back, img)
    ch = _chunks(open(path, "rb").read())
    assert [k for k, _ in ch] == [b"IHDR", b"IDAT", b"IEND"]
    assert ch[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0) and ch[2][1] == b""
    raw = zlib.decompress(ch[1][1])
    assert len(raw) == h * (1 + 3 * w)
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any() and np.array_equal(rows[:, 1:].reshape(h, w, 3), img)
    png.write_png(path, torch.from_numpy(img))                                      # a CPU tensor is written as it is
    assert np.array_equal(png.read_png(path), img)


def test_png_refuses_what_it_does_not_handle(tmp_path):
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            png.write_png(str(tmp_path / "b.png"), bad)
    path = str(tmp_path / "c.png")
    png.write_png(path, np.zeros((2, 2, 3), np.uint8))
    buf = bytearray(open(path, "rb").read())
    buf[-20] ^= 1                                                                    # inside IDAT: its CRC no longer holds
    open(path, "wb").write(bytes(buf))
    with pytest.raises(ValueError, match="CRC"):
        png.read_png(path)
    open(path, "wb").write(b"not a png at all")
    with pytest.raises(ValueError):
        png.read_png(path)


def test_python_layer_argument_errors():
    lf = torch.zeros(5, 5, 4, 4, 3, dtype=torch.uint8)
    net = SimpleNamespace(angRes=3, factor=2)
    for call in (lambda: colour.luma(lf, 3), lambda: colour.merge(lf, None, 3, 2), lambda: colour.bicubic_lf(lf, 3, 2),
                 lambda: colour.super_resolve_lf(net, lf)):
        with pytest.raises(LftError, match="GPU"):                                   # a CPU tensor: there is no CPU path
            call()
    with pytest.raises(LftError, match=r"\[U, V, H, W, C\]"):
        colour.luma(lf[0], 3)
    with pytest.raises(LftError, match="torch tensor or a numpy array"):
        colour.merge([[1, 2, 3]], None, 1, 2)
    with pytest.raises(LftError, match="angRes"):                                    # a loaded array goes through prepare.centre_views
        colour.luma(np.zeros((5, 5, 4, 4, 3), np.uint8), 4, device="cpu")
    with pytest.raises(LftError, match="class"):
        colour.luma(np.zeros((5, 5, 4, 4, 3), np.int16), 3, device="cpu")
