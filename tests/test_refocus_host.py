"""CPU: the refocus entry point of the C ABI (declaration, export, argument errors before any device work), the coefficient table
and apertures of lft_amd.refocus, the EPI slices, and the numpy restatement the GPU tests use (tests/refocus_util.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from lft_amd import _lib, prepare, refocus as R
from lft_amd._lib import LftError

import refocus_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = -1, -2
ULP = 2.0 ** -23


def test_header_declares_and_library_exports_the_refocus_entry_point():
    hdr = open(os.path.join(ROOT, "include", "lft_hip.h")).read()
    declared = set(re.findall(r"^int\s+(lft_\w+)\s*\(", hdr, flags=re.M))
    assert _lib.REFOCUS_EXPORTS == ("lft_refocus",)
    assert set(_lib.REFOCUS_EXPORTS) <= declared and set(_lib.REFOCUS_EXPORTS) <= set(_lib.EXPORTS)
    assert "typedef struct { int oy, ox; float wy[4], wx[4]; float a; int skip; } lft_refocus_record;" in hdr
    assert "lft_refocus.cuh" in _lib.SOURCES
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in _lib.REFOCUS_EXPORTS:
        assert hasattr(L, name), name
    assert _lib.lib().lft_version() == 5                                       # additive: the ABI version does not change
    assert R.RECORD.itemsize == 48 and R.RECORD.fields["a"][1] == 40 and R.RECORD.fields["skip"][1] == 44      # the C layout


def test_argument_errors_come_before_any_device_work():
    """Every call below is refused on the host: nothing is dereferenced on a device, nothing is launched (this runs without a GPU)."""
    L = _lib.lib()
    P = 4096                                                                   # an address that is never dereferenced
    st = (ctypes.c_longlong * 6)(0, 500, 100, 10, 1, 0)
    good = dict(lf=P, cls=_lib.LF_UINT8, B=1, A=5, H=10, W=10, C=1, st=st, table=P, D=3, taps=4, out=P, ocls=_lib.LF_FLOAT32)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return L.lft_refocus(a["lf"], a["cls"], a["B"], a["A"], a["H"], a["W"], a["C"], a["st"], a["table"], a["D"], a["taps"],
                             a["out"], a["ocls"], None)

    neg = (ctypes.c_longlong * 6)(0, 500, 100, -10, 1, 0)
    bad = [dict(A=0), dict(A=-3), dict(C=0), dict(C=5), dict(C=-1), dict(taps=0), dict(taps=3), dict(taps=5), dict(taps=8),
           dict(taps=-1), dict(cls=_lib.LF_FLOAT64), dict(cls=7), dict(cls=-1), dict(ocls=_lib.LF_FLOAT64), dict(ocls=9), dict(D=0),
           dict(D=-2), dict(lf=None), dict(st=None), dict(table=None), dict(out=None), dict(st=neg)]
    for kw in bad:
        L.lft_refocus(None, 99, 1, 1, 1, 1, 1, None, None, 1, 1, None, 0, None)          # leaves another message behind
        assert call(**kw) == ERR_ARG, kw
        msg = L.lft_last_error().decode()
        assert msg.startswith("lft_refocus:") and "99" not in msg, (kw, msg)
    assert call(taps=3) == ERR_ARG and b"taps" in L.lft_last_error()
    assert call(C=5) == ERR_ARG and b"channels" in L.lft_last_error()
    for kw in (dict(B=-1), dict(H=-1), dict(W=-4)):
        assert call(**kw) == ERR_SHAPE, kw
    assert call(B=1 << 20, H=1 << 20, W=1 << 20) == ERR_SHAPE and b"2^31" in L.lft_last_error()
    wide = (ctypes.c_longlong * 6)(0, 0, 0, 1 << 28, 1, 0)                     # rows 2^28 elements apart: 10 of them span 2^31
    assert call(st=wide) == ERR_SHAPE and b"spans" in L.lft_last_error()
    # an empty stack is no error and no work, null pointers included
    for kw in (dict(B=0), dict(H=0), dict(W=0)):
        assert call(lf=None, out=None, **kw) == 0, kw


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_table_weights_sum_to_one_per_axis(interp):
    taps = R.TAPS[interp]
    for A in (2, 3, 5, 9):
        t = R.shift_table(A, U.SLOPES + [0.1, 1 / 3, -7.77], "full", interp)
        assert t.shape == (10, A * A) and t.dtype == R.RECORD
        for ax in ("wy", "wx"):
            s = t[ax].astype(np.float64)
            assert np.all(s[..., taps:] == 0)
            assert np.abs(s[..., :taps].sum(-1) - 1).max() <= ULP, (A, ax)
        assert 1.0 <= U.abs_sum(t, taps) <= (1.25 if interp == "cubic" else 1.0) + ULP


def test_table_offsets_and_special_weights():
    # cubic at f = 0 is exactly [0, 1, 0, 0], base floor(off) - 1; linear [1, 0]; nearest one tap at floor(off + 0.5)
    t = R.shift_table(5, [0.0, 1.0, -2.0], "full", "cubic")
    assert np.array_equal(t["wy"], np.broadcast_to(np.float32([0, 1, 0, 0]), t["wy"].shape)) and np.array_equal(t["wx"], t["wy"])
    assert [int(t[1, u * 5]["oy"]) for u in range(5)] == [-3, -2, -1, 0, 1]
    assert [int(t[2, v]["ox"]) for v in range(5)] == [3, 1, -1, -3, -5]
    t = R.shift_table(5, [0.0], "full", "linear")
    assert np.array_equal(t["wy"][..., :2], np.broadcast_to(np.float32([1, 0]), t["wy"][..., :2].shape)) and np.all(t["oy"] == 0)
    # A = 2 at slope 1: offsets -0.5 and +0.5, half-pixel taps
    t = R.shift_table(2, [1.0], "full", "linear")[0]
    assert [int(r["oy"]) for r in t] == [-1, -1, 0, 0] and [int(r["ox"]) for r in t] == [-1, 0, -1, 0]
    assert np.array_equal(t["wy"][:, :2], np.full((4, 2), 0.5, np.float32)) and np.array_equal(t["wx"][:, :2], np.full((4, 2), 0.5, np.float32))
    assert np.array_equal(t["a"], np.full(4, 0.25, np.float32))
    t = R.shift_table(2, [1.0], "full", "nearest")[0]                          # floor(-0.5 + 0.5) = 0, floor(0.5 + 0.5) = 1
    assert [int(r["oy"]) for r in t] == [0, 0, 1, 1] and np.all(t["wy"][:, 0] == 1) and np.all(t["wy"][:, 1:] == 0)
    t = R.shift_table(2, [1.0], "full", "cubic")[0]
    want = prepare._cubic(np.array([1.5, 0.5, 0.5, 1.5])).astype(np.float32)
    assert np.array_equal(t["wy"], np.broadcast_to(want, (4, 4))) and [int(r["oy"]) for r in t] == [-2, -2, -1, -1]
    # a fractional offset: -0.3 * (0 - 2) = 0.6 -> base 0, f = 0.6
    r = R.shift_table(5, [-0.3], "full", "linear")[0, 0]
    assert int(r["oy"]) == 0 and np.array_equal(r["wy"][:2], np.float32([1 - (0.6 - 0.0), 0.6]))
    for bad in (lambda: R.shift_table(5, [], "full"), lambda: R.shift_table(5, [np.nan]), lambda: R.shift_table(0, [1.0]),
                lambda: R.shift_table(5, [1.0], "full", "lanczos"), lambda: R.shift_table(5, [1.0], "ring"),
                lambda: R.shift_table(5, [1.0], np.ones((4, 4))), lambda: R.shift_table(5, [1.0], -np.ones((5, 5))),
                lambda: R.shift_table(5, [1.0], np.zeros((5, 5))), lambda: R.shift_table(5, [1e12])):
        with pytest.raises(LftError):
            bad()


def test_apertures():
    for A in (1, 2, 3, 5, 8):
        for kind, kw in (("full", {}), ("disk", {}), ("disk", dict(radius=1.0)), ("gaussian", {}), ("gaussian", dict(sigma=0.7))):
            if A == 2 and kind == "disk" and not kw:                           # uc = 0.5 reaches no view (all at 0.5 * sqrt 2): refused
                with pytest.raises(LftError, match="keeps none"):
                    R.aperture_weights(A, kind, **kw)
                continue
            a = R.aperture_weights(A, kind, **kw)
            assert a.shape == (A, A) and a.dtype == np.float64 and np.all(a >= 0) and abs(a.sum() - 1) <= 4 * 2.0 ** -52
            assert np.array_equal(a, a.T) and np.array_equal(a, a[::-1, ::-1])
    d = R.aperture_weights(5, "disk")                                          # r = uc = 2: 13 of the 25 views
    assert int((d > 0).sum()) == 13 and np.all(d[d > 0] == 1 / 13) and d[0, 0] == 0 and d[0, 2] > 0
    assert int((R.aperture_weights(5, "disk", radius=1.0) > 0).sum()) == 5
    g = R.aperture_weights(5, "gaussian", sigma=1.0)
    assert abs(g[2, 2] / g[2, 3] - np.exp(0.5)) < 1e-12 and abs(g[2, 2] / g[1, 1] - np.exp(1.0)) < 1e-12
    # zero-weight views are flagged, the others carry the normalised weight
    t = R.shift_table(5, [0.5, -1.0], "disk", "cubic")
    assert np.array_equal(t["skip"], np.broadcast_to((d.reshape(-1) == 0).astype(np.int32), (2, 25)))
    assert np.array_equal(t["a"], np.broadcast_to(d.reshape(-1).astype(np.float32), (2, 25)))
    user = U.user_aperture(5, 3)
    assert (user == 0).any()
    t = R.shift_table(5, [0.5], user, "linear")
    assert np.array_equal(t["skip"][0] != 0, user.reshape(-1) == 0)
    assert np.array_equal(t["a"][0], (user / user.sum()).reshape(-1).astype(np.float32))
    with pytest.raises(LftError):
        R.aperture_weights(5, "square")


def test_epi_agrees_with_indexing():
    rng = np.random.default_rng(2)
    A, H, W = 3, 6, 7
    v5 = rng.random((A, A, H, W, 3)).astype(np.float32)
    v4 = v5[..., 0]
    mosaic = np.ascontiguousarray(v4.transpose(0, 2, 1, 3)).reshape(A * H, A * W)
    for mk in (lambda x: x, torch.from_numpy):
        e = R.epi(mk(v5))
        assert tuple(e.shape) == (A, W, 3) and np.array_equal(np.asarray(e), v5[A // 2, :, H // 2])
        e = R.epi(mk(v4), row=1, u=2)
        assert tuple(e.shape) == (A, W) and np.array_equal(np.asarray(e), v4[2, :, 1])
        e = R.epi(mk(v5), col=4)
        assert tuple(e.shape) == (A, H, 3) and np.array_equal(np.asarray(e), v5[:, A // 2, :, 4])
        e = R.epi(mk(v4), v=0)
        assert tuple(e.shape) == (A, H) and np.array_equal(np.asarray(e), v4[:, 0, :, W // 2])
        e = R.epi(mk(mosaic), angRes=A, row=5)
        assert tuple(e.shape) == (A, W) and np.array_equal(np.asarray(e), v4[A // 2, :, 5])
        e = R.epi(mk(mosaic), angRes=A, col=0, v=2)
        assert tuple(e.shape) == (A, H) and np.array_equal(np.asarray(e), v4[:, 2, :, 0])
        for bad in (lambda: R.epi(mk(mosaic)), lambda: R.epi(mk(mosaic), angRes=4), lambda: R.epi(mk(v4), row=1, col=1),
                    lambda: R.epi(mk(v4), row=H), lambda: R.epi(mk(v4), v=A), lambda: R.epi(mk(v4), angRes=2)):
            with pytest.raises(LftError):
                bad()


def test_refocus_has_no_cpu_path():
    with pytest.raises(LftError, match="no CPU path"):
        R.refocus(torch.zeros(3, 3, 4, 4), [0.0])
    with pytest.raises(LftError):
        R.refocus(np.zeros((3, 3, 4, 4), np.float32), [0.0])


def test_numpy_restatement_brings_a_plane_back_at_plus_d0():
    """The sign of the definition, on the oracle alone: the plane of slope d0 comes back as f at +d0 (cubic: to the interpolation
    error of a smooth f, nearest at an integer d0: to fp32 rounding of the views) and not at -d0."""
    A, n = 5, 32
    for d0, interp, gate in ((2.0, "nearest", 2.0 ** -24), (1.5, "cubic", 2e-3)):
        L, f = U.plane(A, n, n, d0)
        t = R.shift_table(A, [d0, -d0], "full", interp)
        r = U.refocus_np(L[..., None], t, R.TAPS[interp])[..., 0]
        m = int(np.ceil(abs(d0) * (A - 1) / 2)) + 2
        inner = (slice(m, n - m), slice(m, n - m))
        assert np.abs(r[0][inner] - f[inner]).max() <= gate
        assert np.abs(r[1][inner] - f[inner]).max() > 0.1
    # quantisation helpers
    assert np.array_equal(U.quantise(np.array([-0.2, 0.5 / 255, 1.5 / 255, 2.5 / 255, 1.7])), np.uint8([0, 0, 2, 2, 255]))
    assert np.allclose(U.tie_distance(np.array([0.5 / 255, 1.0 / 255, 1.25 / 255])), [0, 0.5, 0.25], atol=1e-12)
