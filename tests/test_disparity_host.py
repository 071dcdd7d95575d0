"""CPU: the disparity entry points of the C ABI (declaration, export, argument errors before any device work), the Python
validation of lft_amd.disparity, and the numpy restatement the GPU tests use (tests/disparity_util.py) on the two scenes whose
properties those tests lean on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from lft_amd import _lib, refocus as R
from lft_amd._lib import LftError

import disparity_util as DU
import refocus_util as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = -1, -2
# the contract's sentences that must stand in the header comments and the module docstring (symbols differ between ASCII and
# the docstring's Unicode, the words do not)
CONTRACT = ["Slopes", "are strictly increasing; they need not be uniform.",
            "is exactly refocus's: rows first, clamped taps,", "weights not renormalised.",
            "This is the aperture-weighted variance of the views at slope", "summed", "over channels.",
            "the lowest k on an exact tie.",
            "All of it is fp32, each step a single rounded operation, with the compiler's contraction off as in",
            "so there is no cancellation.", "Otherwise, and at either end of the sweep,",
            "The slopes are rounded once to fp32 on the host.", "summed in k order.", "all give 0.",
            "is accumulated in refocus's order: views in (u,v) order, taps in table order, explicit FMAs.", "bit for bit",
            "A pixel's results must not depend on the tile, on the image around the support of its taps and window, or on the launch",
            "That requires a fixed aggregation order, dy then dx."]


def test_header_declares_and_library_exports_the_disparity_entry_points():
    from lft_amd import disparity as Dm
    hdr = open(os.path.join(ROOT, "include", "lft_hip.h")).read()
    declared = set(re.findall(r"^int\s+(lft_\w+)\s*\(", hdr, flags=re.M))
    assert _lib.DISPARITY_EXPORTS == ("lft_disparity_scratch_bytes", "lft_disparity")
    assert set(_lib.DISPARITY_EXPORTS) <= declared and set(_lib.DISPARITY_EXPORTS) <= set(_lib.EXPORTS)
    assert "#define LFT_DISPARITY_AIF 1" in hdr and _lib.DISPARITY_AIF == 1
    assert "lft_disparity.cuh" in _lib.SOURCES
    kernels = open(os.path.join(_lib.CSRC, "lft_disparity.cuh")).read()
    for text in (hdr, kernels, Dm.__doc__):
        flat = " ".join(re.sub(r"^\s*(//|\*)\s?", "", line).replace("`", "").replace("**", "").strip() for line in text.splitlines())
        for sentence in CONTRACT:
            assert sentence in flat, sentence
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in _lib.DISPARITY_EXPORTS:
        assert hasattr(L, name), name
    assert _lib.lib().lft_version() == 5                                       # additive: the ABI version does not change
    assert _lib.REFOCUS_EXPORTS == ("lft_refocus",)


def test_scratch_bytes():
    L = _lib.lib()
    n = ctypes.c_size_t(7)
    assert L.lft_disparity_scratch_bytes(2, 9, 33, 65, 3, 0, ctypes.byref(n)) == 0 and n.value == 2 * 9 * 33 * 65 * 4
    assert L.lft_disparity_scratch_bytes(2, 9, 33, 65, 3, _lib.DISPARITY_AIF, ctypes.byref(n)) == 0 and n.value == 2 * 9 * 33 * 65 * 4 * 4
    assert L.lft_disparity_scratch_bytes(0, 9, 33, 65, 3, 0, ctypes.byref(n)) == 0 and n.value == 0
    for args in ((1, 0, 4, 4, 1, 0), (1, 3, 4, 4, 5, 0), (1, 3, 4, 4, 0, 0), (1, 3, 4, 4, 1, 2)):
        assert L.lft_disparity_scratch_bytes(*args, ctypes.byref(n)) == ERR_ARG, args
        assert L.lft_last_error().decode().startswith("lft_disparity:")
    assert L.lft_disparity_scratch_bytes(1, 3, 4, 4, 1, 0, None) == ERR_ARG
    assert L.lft_disparity_scratch_bytes(-1, 3, 4, 4, 1, 0, ctypes.byref(n)) == ERR_SHAPE
    assert L.lft_disparity_scratch_bytes(1 << 20, 64, 1 << 20, 1 << 20, 1, 0, ctypes.byref(n)) == ERR_SHAPE


def test_argument_errors_come_before_any_device_work():
    """Every call below is refused on the host: nothing is dereferenced on a device, nothing is launched (this runs without a GPU)."""
    L = _lib.lib()
    P = 4096                                                                   # an address that is never dereferenced
    st = (ctypes.c_longlong * 6)(0, 500, 100, 10, 1, 0)
    good = dict(lf=P, cls=_lib.LF_UINT8, B=1, A=5, H=10, W=10, C=1, st=st, table=P, slopes=P, D=3, taps=4, radius=2, scratch=P,
                disp=P, conf=P, index=P, cost=None, aif=None, acls=_lib.LF_FLOAT32)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return L.lft_disparity(a["lf"], a["cls"], a["B"], a["A"], a["H"], a["W"], a["C"], a["st"], a["table"], a["slopes"], a["D"],
                               a["taps"], a["radius"], a["scratch"], a["disp"], a["conf"], a["index"], a["cost"], a["aif"], a["acls"], None)

    neg = (ctypes.c_longlong * 6)(0, 500, 100, -10, 1, 0)
    bad = [dict(A=0), dict(A=-3), dict(C=0), dict(C=5), dict(taps=0), dict(taps=3), dict(taps=8), dict(cls=_lib.LF_FLOAT64),
           dict(cls=7), dict(acls=_lib.LF_FLOAT64), dict(acls=9), dict(D=0), dict(D=-2), dict(radius=-1), dict(radius=9),
           dict(lf=None), dict(st=None), dict(table=None), dict(slopes=None), dict(scratch=None), dict(disp=None), dict(conf=None),
           dict(index=None), dict(st=neg), dict(scratch=P + 2)]
    for kw in bad:
        L.lft_refocus(None, 99, 1, 1, 1, 1, 1, None, None, 1, 1, None, 0, None)          # leaves another message behind
        assert call(**kw) == ERR_ARG, kw
        msg = L.lft_last_error().decode()
        assert msg.startswith("lft_disparity:") and "99" not in msg, (kw, msg)
    assert call(radius=9) == ERR_ARG and b"radius" in L.lft_last_error()
    for kw in (dict(B=-1), dict(H=-1), dict(W=-4)):
        assert call(**kw) == ERR_SHAPE, kw
        assert L.lft_last_error().decode().startswith("lft_disparity:")
    assert call(B=1 << 20, H=1 << 20, W=1 << 20) == ERR_SHAPE and b"2^31" in L.lft_last_error()
    wide = (ctypes.c_longlong * 6)(0, 0, 0, 1 << 28, 1, 0)
    assert call(st=wide) == ERR_SHAPE and b"spans" in L.lft_last_error()
    assert call(B=64, D=4096, H=2048, W=2048) == ERR_SHAPE and b"2^40" in L.lft_last_error()
    # empty maps are no error and no work, null pointers included
    for kw in (dict(B=0), dict(H=0), dict(W=0)):
        assert call(lf=None, scratch=None, disp=None, conf=None, index=None, **kw) == 0, kw


def test_python_validation():
    """Arguments are judged before the device is: every refusal below comes for a CPU tensor, and names what is wrong."""
    from lft_amd import disparity as Dm
    lf = torch.zeros(3, 3, 4, 4)
    with pytest.raises(LftError, match="no CPU path"):
        Dm.disparity(lf, [0.0, 1.0])
    with pytest.raises(LftError, match="torch tensor"):
        Dm.disparity(np.zeros((3, 3, 4, 4), np.float32), [0.0])
    for bad in ([1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 1.0], [], [0.0, np.nan], [0.0, np.inf], [1.0, 1.0 + 1e-12]):
        with pytest.raises(LftError, match="slopes"):
            Dm.disparity(lf, bad)
    assert Dm.check_slopes(np.linspace(-2, 2, 5)) == (-2.0, -1.0, 0.0, 1.0, 2.0) and Dm.check_slopes([0.25]) == (0.25,)
    for radius in (9, -1, 1.5, True):
        with pytest.raises(LftError, match="radius"):
            Dm.disparity(lf, [0.0, 1.0], radius=radius)
    with pytest.raises(LftError, match="float64"):
        Dm.disparity(lf.double(), [0.0, 1.0])
    with pytest.raises(LftError, match="aif_dtype"):
        Dm.disparity(lf, [0.0, 1.0], aif_dtype=torch.float16)
    with pytest.raises(LftError, match="interp"):
        Dm.disparity(lf, [0.0, 1.0], interp="lanczos")
    with pytest.raises(LftError, match="no CPU path"):
        Dm.disparity_error(lf, lf, [0.0, 1.0])


def test_pick_rules_on_small_volumes():
    """Steps 4-6 of the definition on hand-made costs: the tie rule, the ends of the sweep, the clamp, flat costs, non-uniform slopes."""
    sl = [-1.0, 0.0, 0.5, 2.0]
    E = np.float32([[3, 1, 1, 0, 2, 5], [1, 1, 2, 0, 2, 1], [2, 3, 1, 0, 2, 3], [1, 0.5, 3, 0, 2, 0]]).reshape(4, 6)
    k, d, c = DU.pick_np(E, sl)
    assert k.tolist() == [1, 3, 0, 0, 0, 3]                 # column 0: E_1 = E_3 = 1, the lower k; column 3: all zero; column 4: all equal
    # column 0: den = (3 - 1) + (2 - 1) = 3, delta = 0.5 * (3 - 2) / 3 = 1/6 >= 0: towards d_2, step 0.5
    assert d[0] == np.float32(0.0) + (np.float32(0.5) * np.float32(1.0) / np.float32(3.0)) * np.float32(0.5)
    assert d[1] == 2.0 and d[2] == -1.0 and d[3] == -1.0 and d[4] == -1.0 and d[5] == 2.0          # the ends: delta = 0
    assert c[3] == 0.0 and c[4] == 0.0 and c[1] == np.float32(1) - np.float32(0.5) / (np.float32(5.5) / np.float32(4))
    # a negative delta uses the step below, and the clamp holds it at half a step
    k, d, _ = DU.pick_np(np.float32([[1.0], [0.0], [4.0], [9.0]]), sl)
    assert k[0] == 1 and d[0] == np.float32(0.5 * (1.0 - 4.0) / 5.0) * np.float32(1.0)
    k, d, _ = DU.pick_np(np.float32([[5.0], [1.0], [1.0], [9.0]]), sl)                               # tie between 1 and 2: k = 1, delta = +0.5, half a step
    assert k[0] == 1 and d[0] == np.float32(0.25)
    k, d, c = DU.pick_np(np.float32([[0.25]]), [0.7])                                                # D = 1
    assert k[0] == 0 and d[0] == np.float32(0.7) and c[0] == 0.0


@pytest.mark.parametrize("d0", [1.5, -0.6, 0.1])
@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_oracle_brings_a_plane_back_at_its_slope(d0, interp):
    A, n, r = 5, 32, 2
    slopes = np.linspace(-2.0, 2.0, 17)
    L, _ = RU.plane(A, n, n, d0)
    table = R.shift_table(A, slopes, "full", interp)
    E, _ = DU.cost_np(L[..., None], table, R.TAPS[interp], r)
    _, disp, _ = DU.pick_np(E, slopes, np.float64)
    m = r + int(np.ceil(2.0 * (A - 1) / 2)) + 2
    err = float(np.abs(disp[m:n - m, m:n - m] - d0).max())
    print(f"plane d0={d0} {interp}: interior error {err:.3e}")
    assert err <= 0.02


SWEEPS = [("nearest", 0, 5), ("linear", 1, 9), ("cubic", 2, 17)]


@pytest.mark.parametrize("interp,r,D", SWEEPS)
def test_oracle_separates_the_two_layers(interp, r, D):
    """The conditions the GPU tests lean on, on the reference alone: both interiors at their layer's index, by a margin between the
    best and the second-best cost far above the GPU's error bound, with confidence above 0.9999."""
    A, H, W = 5, 72, 64
    slopes = np.linspace(-2.0, 2.0, D)
    L, centre = DU.two_layer(A, H, W)
    table = R.shift_table(A, slopes, "full", interp)
    taps = R.TAPS[interp]
    E, m = DU.cost_np(L, table, taps, r)
    k, disp, conf = DU.pick_np(E, slopes, np.float64)
    fg, bg = DU.two_layer_interiors(A, H, W, r)
    assert fg.sum() >= 300 and bg.sum() >= 300
    k_fg, k_bg = int(np.argmin(np.abs(slopes - 1.0))), int(np.argmin(np.abs(slopes + 1.0)))
    assert slopes[k_fg] == 1.0 and slopes[k_bg] == -1.0
    assert np.all(k[fg] == k_fg) and np.all(k[bg] == k_bg)
    both = fg | bg
    second = np.sort(E, axis=0)[1]
    margin = float((second - E.min(0))[both].min())
    tol = DU.tol_E(A, 1, r, table, taps, 1.0)
    print(f"{interp} r={r} D={D}: margin {margin:.4f}, tol_E {tol:.3e}, min confidence {float(conf[both].min()):.6f}, "
          f"max |disparity - layer| {float(np.abs(disp - np.where(fg, 1.0, -1.0))[both].max()):.3e}")
    assert margin > 100 * tol
    assert float(conf[both].min()) > 0.9999
    aif = np.take_along_axis(m[..., 0], k[None].astype(np.int64), axis=0)[0]
    assert float(np.abs(aif - centre)[both].max()) <= 1e-7
    k0 = int(np.argmin(np.abs(slopes)))
    assert float(np.abs(m[k0, ..., 0] - centre)[both].max()) > 0.2          # the slope-0 stack is far from the centre view there
