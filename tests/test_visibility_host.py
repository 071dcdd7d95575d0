"""CPU: the per-view visibility test of view synthesis up to the device -- the numpy restatement (tests/visibility_util.py) on the
two-layer scene and on the inputs the GPU parity test uses, the new header and its binding, every refusal of the three entry points
on the host, and the Python refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from lft_amd import _lib, views as V
from lft_amd._lib import LftError

import disparity_util as DU
import views_util as VU
import visibility_util as XU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = -1, -2
P, Q = 1 << 20, 2 << 20                                                       # addresses that are never dereferenced
TWO_LAYER_TARGETS = ((0, 1), (4, 4), (1, 3), (2, 2), (0, 0), (2, 0))


def two_layer_scene():
    """(views [5, 5, 72, 64, 1], the true centre map)."""
    L, _ = DU.two_layer(5, 72, 64)
    y0, y1, x0, x1 = DU.FG_BOX
    yy, xx = np.meshgrid(np.arange(72), np.arange(64), indexing="ij")
    return L, np.where((yy >= y0) & (yy < y1) & (xx >= x0) & (xx < x1), 1.0, -1.0).astype(np.float32)


def border(m, H=72, W=64):
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (yy >= m) & (yy < H - m) & (xx >= m) & (xx < W - m)


def parity_inputs(A, seed, near, H=37, W=45, d_range=(-1.5, 2.0)):
    """What tests/test_gpu_visibility.py::test_parity renders: test_gpu_views' random map, Dv warped from it, its three targets with
    the gaussian blend."""
    from test_gpu_views import disparity_map, targets_of
    tg = targets_of(A)
    Dr = disparity_map(H, W, seed=seed)
    Dv = XU.warp_np(Dr, A, d_range, near=near)
    rec = V.record_table(A, tg, V.blend_weights(A, tg, "gaussian"))
    deltas = V.target_deltas(A, tg)
    Dt = [VU.fill_np(VU.splat_np(Dr, deltas[t], d_range, near), Dr, d_range, near) for t in range(len(tg))]
    return tg, Dr, Dv, rec, Dt


def test_restatement_recovers_the_held_out_view_of_the_two_layers():
    """With the test, the held-out view comes back to fp64 rounding on every pixel >= 9 from the border, ring included; without it
    the restatement of the plain definition is off at hundreds of ring pixels.  The default Dv, warped from the centre map, is the
    analytic per-view map."""
    L, Dr = two_layer_scene()
    A = 5
    Dv = XU.warp_np(Dr, A, (-1, 1))
    for u in range(A):
        for v in range(A):
            want, b5, _, _ = VU.occlusion_masks((u, v))
            assert np.array_equal(Dv[u, v][b5], want[b5]), (u, v)
    b9 = border(9)
    for t in TWO_LAYER_TARGETS:
        _, _, held, _ = VU.occlusion_masks(t)
        delta = V.target_deltas(A, [t])[0]
        Dt, _ = VU.fill_np(VU.splat_np(Dr, delta, (-1, 1)), Dr, (-1, 1))
        ex = np.zeros((A, A), bool)
        ex[t] = True
        rec = V.record_table(A, [t], V.blend_weights(A, [t], "gaussian", exclude=ex))[0]
        truth = L[t[0], t[1], ..., 0].astype(np.float64)
        for taps in (2, 4):
            got, count, _ = XU.render_np(L, Dt, rec, taps, Dv, 0.5)
            err = np.abs(got[..., 0] - truth)
            plain = np.abs(VU.render_np(L, Dt, rec, taps)[..., 0] - truth)
            off = int((plain[b9 & ~held] > 1e-3).sum())
            print(f"target {t} taps {taps}: max error {float(err[b9].max()):.2e}, fewest visible views {int(count[b9].min())}, plain wrong at {off} ring pixels")
            assert float(err[b9].max()) <= 1e-12, (t, taps)
            assert int(count[b9].min()) >= 1 and (count[held] == 24).all(), (t, taps)
            assert off >= 200, (t, taps, off)


@pytest.mark.parametrize("near", ["larger", "smaller"])
@pytest.mark.parametrize("A", [2, 3, 5])
def test_parity_inputs_do_their_job(A, near):
    """The GPU parity inputs reach the test: a fifth to seven tenths of the inside (pixel, view) pairs are occluded for every target,
    and each of the three classes decides some pixel."""
    tg, Dr, Dv, rec, Dt = parity_inputs(A, seed=100, near=near)
    classes = set()
    for t in range(len(tg)):
        _, inside, visible, count = XU.classes_np(Dt[t][0], rec[t], Dv, 0.25, near)
        share = 1.0 - visible.sum() / inside.sum()
        print(f"A={A} near={near} target {tg[t]}: occluded share of inside pairs {share:.3f}")
        assert 0.2 <= share <= 0.7, (tg[t], share)
        classes |= set(np.unique(np.where(visible.any(0), 0, np.where(inside.any(0), 1, 2))).tolist())
        assert np.array_equal(count, visible.sum(0).astype(np.uint8))
    assert classes == {0, 1, 2}


def test_non_finite_maps_and_a_large_tau_occlude_nothing():
    tg, Dr, Dv, rec, Dt = parity_inputs(3, seed=101, near="larger")
    lf = np.random.default_rng(0).random((3, 3, 37, 45, 2)).astype(np.float32)
    for t in range(len(tg)):
        plain = VU.render_np(lf, Dt[t][0], rec[t], 2)
        _, inside, _, _ = XU.classes_np(Dt[t][0], rec[t], Dv, 0.25)
        for maps, tau in ((Dv, 3.6), (np.full_like(Dv, np.nan), 0.0), (np.full_like(Dv, -np.inf), 0.0), (np.full_like(Dv, np.inf), 0.0)):
            got, count, _ = XU.render_np(lf, Dt[t][0], rec[t], 2, maps, tau)
            assert np.array_equal(got, plain) and np.array_equal(count, inside.sum(0))


def test_header_declares_and_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "lft_hip_visibility.h")).read()
    declared = re.findall(r"^int\s+(lft_\w+)\s*\(", hdr, flags=re.M)
    names = ("lft_view_visible_scratch_bytes", "lft_view_warp_disparity", "lft_view_render_visible")
    assert _lib.VISIBILITY_EXPORTS == names and tuple(declared) == names
    assert "Added beside ABI 5; lft_version unchanged" in " ".join(re.sub(r"^\s*\*\s?", "", line) for line in hdr.splitlines())
    assert _lib.ADDON_HEADERS["lft_hip_visibility.h"] == "VIS_" and _lib.VIS_MASK_VIEWS == 64
    assert all(k.startswith("LFT_VIS_") for k in re.findall(r"^#define (LFT_\w+)[ \t]+\S", hdr, flags=re.M))
    # the new table equals the header's prototypes
    table = {n: _lib._ADDON_SIGS[n] for n in names}
    assert table == {n: (res, args) for n, (res, args, _) in _lib._prototypes("lft_hip_visibility.h").items()}
    i, f, p = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    assert table["lft_view_visible_scratch_bytes"] == (i, [i, i, i, i, ctypes.POINTER(ctypes.c_size_t)])
    assert table["lft_view_warp_disparity"] == (i, [p, i, i, i, p, f, i, f, f, i, i, p, p, p, p])
    assert table["lft_view_render_visible"] == (i, [p, i, i, i, i, i, i, p, p, p, f, p, f, p, i, i, f, f, i, i, p, p, i, p, p, p, p])
    # the older tables keep their contents
    assert len(_lib._SIGS) == 59 and len(_lib.VIEW_EXPORTS) == 2 and len(_lib.SGM_EXPORTS) == 2
    assert _lib.VIEW_EXPORTS == ("lft_view_render_scratch_bytes", "lft_view_render") and _lib.SGM_EXPORTS == ("lft_sgm_scratch_bytes", "lft_sgm")
    assert not set(names) & (set(_lib.EXPORTS) | set(_lib.TEST_EXPORTS) | set(_lib.VIEW_EXPORTS) | set(_lib.SGM_EXPORTS) | set(_lib.STREAM_LAST))
    assert set(names) <= _lib.OPTIONAL_EXPORTS and set(names[1:]) <= _lib.ADDON_STREAM_LAST and names[0] not in _lib.ADDON_STREAM_LAST
    for other in ("lft_hip.h", "lft_hip_test.h", "lft_hip_views.h", "lft_hip_sgm.h"):
        assert "lft_view_render_visible" not in open(os.path.join(ROOT, "include", other)).read()
    assert "lft_visibility.cuh" in _lib.SOURCES
    assert [u for u in _lib.UNITS if "lft_visibility.cuh" in open(os.path.join(_lib.CSRC, u + ".hip")).read()] == ["lft_lightfield"]
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    assert _lib.lib().lft_version() == 5
    # the definition stands sentence for sentence in the header, the kernels' comment and the module docstring
    kernels = open(os.path.join(_lib.CSRC, "lft_visibility.cuh")).read()
    for text in (hdr, kernels, V.__doc__):
        flat = " ".join(re.sub(r"^\s*(//|\*|-)\s?", "", line).replace("`", "").replace("**", "").strip() for line in text.splitlines())
        flat = " ".join(flat.replace("≥", ">=").replace("·", ".").replace("−", "-").replace("Σ", "sum").replace("∈", "in").replace("[B, A, A, H, W]", "[B,A,A,H,W]").split())
        for words in ("Dv[u,v] is the map at integer view position (u,v)", "a threshold, finite, >= 0, rounded once to fp32",
                      "Dt and holes carry the same bits as the plain call", "is dropped when sy is integral", "is dropped when sx is integral",
                      "Indices are clamped into the image", "The footprint is the same for linear and cubic", "Non-finite q never occludes",
                      "All comparisons are fp32", "inside and not occluded", "over the first non-empty class in that order",
                      "Views outside the chosen class contribute nothing", "when nothing is occluded, the bits equal", "saturated at 255",
                      "The hole fill already takes the farther neighbour"):
            assert words in flat, (words, text[:40])
    assert "Per-view visibility is not tested" not in V.__doc__


def test_scratch_query():
    assert _lib.query("lft_view_visible_scratch_bytes", 2, 25, 37, 45) == 2 * 25 * 37 * 45 * 4
    assert _lib.query("lft_view_visible_scratch_bytes", 0, 3, 37, 45) == 0
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    for args, rc in (((1, 0, 4, 4), ERR_ARG), ((-1, 3, 4, 4), ERR_SHAPE), ((1, 3, 4, -4), ERR_SHAPE), ((1 << 20, 64, 1 << 20, 1 << 20), ERR_SHAPE)):
        assert L.lft_view_visible_scratch_bytes(*args, ctypes.byref(n)) == rc, args
        assert L.lft_last_error().decode().startswith("lft_view_visible_scratch_bytes:")
    assert L.lft_view_visible_scratch_bytes(1, 3, 4, 4, None) == ERR_ARG and L.lft_last_error().decode().startswith("lft_view_visible_scratch_bytes:")
    with pytest.raises(LftError, match="does not take its stream last"):
        _lib.enqueue("lft_view_visible_scratch_bytes", "cuda:0", 1, 1, 1, 1)


RENDER = dict(lf=P, cls=_lib.LF_UINT8, B=1, A=5, H=10, W=10, C=1, st=(ctypes.c_longlong * 6)(0, 500, 100, 10, 1, 0), dr=Q, dv=Q + 2048, tau=0.5,
              deltas=Q + 4096, max_delta=2.0, records=Q + 8192, T=3, taps=2, lo=-1.5, hi=2.0, near=0, fill=32, scratch=Q + 16384, views=Q + 32768,
              vcls=_lib.LF_FLOAT32, dt=Q + 65536, holes=Q + 98304, visible=Q + 131072, stream=None)
WARP = dict(dr=Q, B=1, H=10, W=10, deltas=Q + 4096, max_delta=2.0, N=25, lo=-1.5, hi=2.0, near=0, fill=32, scratch=Q + 16384, maps=Q + 32768,
            holes=Q + 98304, stream=None)
INF, NAN = float("inf"), float("nan")
# the refusals lft_view_render_visible and lft_view_warp_disparity share, by the parameters both have
SHARED = [
    (dict(B=-1), ERR_SHAPE, "negative size"), (dict(W=-4), ERR_SHAPE, "negative size"),
    (dict(fill=-1), ERR_ARG, "fill -1 outside 0 .. 64"), (dict(fill=65), ERR_ARG, "fill 65 outside 0 .. 64"),
    (dict(lo=2.0, hi=-1.5), ERR_ARG, "d_range"), (dict(lo=NAN), ERR_ARG, "d_range"), (dict(hi=INF), ERR_ARG, "d_range"), (dict(lo=-INF), ERR_ARG, "d_range"),
    (dict(near=2), ERR_ARG, "near"), (dict(near=-1), ERR_ARG, "near"), (dict(max_delta=-1.0), ERR_ARG, "max_delta"), (dict(max_delta=NAN), ERR_ARG, "max_delta"),
    (dict(max_delta=31.6), ERR_SHAPE, "reach 65"), (dict(lo=-100.0, max_delta=1.0), ERR_SHAPE, "reach 101"),
    (dict(dr=None), ERR_ARG, "null pointer"), (dict(deltas=None), ERR_ARG, "null pointer"), (dict(scratch=None), ERR_ARG, "null pointer"),
    (dict(holes=None), ERR_ARG, "null pointer"),
    (dict(scratch=Q + 16386), ERR_ARG, "scratch must be 4-byte aligned"), (dict(scratch=Q + 16386, fill=70), ERR_ARG, "fill"),
]


def refused(L, entry, good, kw, rc, words):
    assert not set(kw) - set(good), kw
    L.lft_refocus(None, 99, 1, 1, 1, 1, 1, None, None, 1, 1, None, 0, None)                  # leaves another call's message behind
    assert getattr(L, entry)(*{**good, **kw}.values()) == rc, (entry, kw)
    msg = L.lft_last_error().decode()
    assert msg.startswith(entry + ":") and words in msg and "99" not in msg, (entry, kw, msg)


def test_every_refusal_comes_before_any_device_work():
    """Each call is answered on the host (this runs without a GPU): its code, and a message that starts with the entry point."""
    L = _lib.lib()
    neg = (ctypes.c_longlong * 6)(0, 500, 100, -10, 1, 0)
    wide = (ctypes.c_longlong * 6)(0, 0, 0, 1 << 28, 1, 0)
    render = SHARED + [
        # lft_view_render's own: the rules shared with lft_refocus, the taps, the pointers, the sizes
        (dict(cls=_lib.LF_FLOAT64), ERR_ARG, "light-field class"), (dict(cls=7), ERR_ARG, "light-field class"), (dict(vcls=_lib.LF_FLOAT64), ERR_ARG, "output class"),
        (dict(vcls=9), ERR_ARG, "output class"), (dict(A=0), ERR_ARG, "angRes"), (dict(C=0), ERR_ARG, "channels"), (dict(C=5), ERR_ARG, "channels"),
        (dict(T=0), ERR_ARG, "0 slopes"), (dict(T=-2), ERR_ARG, "-2 slopes"),
        (dict(st=neg), ERR_ARG, "stride 3 is negative"), (dict(st=wide), ERR_SHAPE, "spans"), (dict(B=1 << 20, H=1 << 20, W=1 << 20), ERR_SHAPE, "2^31"),
        (dict(taps=0), ERR_ARG, "taps"), (dict(taps=3), ERR_ARG, "taps"), (dict(taps=8), ERR_ARG, "taps"), (dict(taps=1), ERR_ARG, "1 taps (2 or 4"),
        (dict(lf=None), ERR_ARG, "null pointer"), (dict(st=None), ERR_ARG, "null pointer"), (dict(records=None), ERR_ARG, "null pointer"),
        (dict(views=None), ERR_ARG, "null pointer"), (dict(dt=None), ERR_ARG, "null pointer"),
        (dict(H=(1 << 24) + 1, st=(ctypes.c_longlong * 6)(0, 0, 0, 1, 1, 0)), ERR_SHAPE, "2^24"),
        (dict(B=64, T=4096, H=2048, W=2048), ERR_SHAPE, "2^31"),
        # what the visibility test adds
        (dict(dv=None), ERR_ARG, "null pointer"), (dict(visible=None), ERR_ARG, "null pointer"),
        (dict(tau=-0.5), ERR_ARG, "tau -0.5"), (dict(tau=NAN), ERR_ARG, "tau"), (dict(tau=INF), ERR_ARG, "tau"), (dict(tau=-INF), ERR_ARG, "tau"),
        (dict(tau=-1.0, scratch=Q + 16386), ERR_ARG, "tau"),
    ]
    for kw, rc, words in render:
        refused(L, "lft_view_render_visible", RENDER, kw, rc, words)
    warp = SHARED + [
        (dict(N=0), ERR_ARG, "0 positions"), (dict(N=-3), ERR_ARG, "-3 positions"), (dict(maps=None), ERR_ARG, "null pointer"),
        (dict(H=(1 << 24) + 1), ERR_SHAPE, "2^24"), (dict(B=1 << 20, H=1 << 20, W=1 << 20), ERR_SHAPE, "2^31"),
        (dict(B=64, N=4096, H=2048, W=2048), ERR_SHAPE, "2^31"),
        (dict(N=24576, H=4096, W=4096), ERR_SHAPE, "2^40"),            # 1.5 * 2^30 blocks, 1.5 * 2^40 bytes
    ]
    for kw, rc, words in warp:
        refused(L, "lft_view_warp_disparity", WARP, kw, rc, words)
    # the largest reach and tau = 0 are accepted: what refuses these calls is the misaligned scratch behind them
    assert L.lft_view_render_visible(*{**RENDER, "max_delta": 31.5, "tau": 0.0, "scratch": Q + 16386}.values()) == ERR_ARG and b"scratch" in L.lft_last_error()
    assert L.lft_view_warp_disparity(*{**WARP, "max_delta": 31.5, "scratch": Q + 16386}.values()) == ERR_ARG and b"scratch" in L.lft_last_error()
    # empty shapes are no error and no work, null pointers included; the values are still judged
    for kw in (dict(B=0), dict(H=0), dict(W=0)):
        nulls = dict(dr=None, scratch=None, holes=None)
        assert L.lft_view_render_visible(*{**RENDER, **nulls, "lf": None, "dv": None, "views": None, "dt": None, "visible": None, **kw}.values()) == 0, kw
        assert L.lft_view_render_visible(*{**RENDER, "tau": -1.0, **kw}.values()) == ERR_ARG, kw
        assert L.lft_view_warp_disparity(*{**WARP, **nulls, "maps": None, **kw}.values()) == 0, kw
        assert L.lft_view_warp_disparity(*{**WARP, "fill": 70, **kw}.values()) == ERR_ARG, kw
    # the plain call's messages still carry its own name
    from test_views_host import render_raw
    assert render_raw(fill=65) == ERR_ARG and L.lft_last_error().decode().startswith("lft_view_render: fill 65")


def test_python_refusals_need_no_device():
    lf, dr = torch.zeros(3, 3, 6, 6), torch.zeros(6, 6)
    for vis, words in ((dict(), "tau"), (dict(tau=-1), "tau"), (dict(tau=np.nan), "tau"), (dict(tau="a"), "tau"), (dict(tau=np.inf), "tau"),
                       (dict(tau=0.5, maps=None), "visibility must be"), (0.5, "visibility must be"),
                       (dict(tau=0.5, view_disparity=np.zeros((3, 3, 6, 6), np.float32)), "view_disparity"),
                       (dict(tau=0.5, view_disparity=torch.zeros(3, 3, 6, 6, dtype=torch.float64)), "view_disparity")):
        with pytest.raises(LftError, match=words):
            V.render(lf, dr, [(1, 1)], (-1, 1), visibility=vis)
    with pytest.raises(LftError, match="no CPU path"):
        V.render(lf, dr, [(1, 1)], (-1, 1), visibility=dict(tau=0.5))
    with pytest.raises(LftError, match="no CPU path"):
        V.warp_disparity(dr, [(0, 0), (1, 2)], (-1, 1), (1, 1))
    for kw, words in ((dict(near="nearer"), "near"), (dict(fill=65), "fill"), (dict(fill=True), "fill")):
        with pytest.raises(LftError, match=words):
            V.warp_disparity(dr, [(0, 0)], (-1, 1), (1, 1), **kw)
    for bad, words in ((lambda: V.warp_disparity(dr, [], (-1, 1), (1, 1)), "targets"), (lambda: V.warp_disparity(dr, [(0, 0)], (1, -1), (1, 1)), "d_range"),
                       (lambda: V.warp_disparity(dr, [(0, 0)], (-1, 1), None), "reference"), (lambda: V.warp_disparity(dr, [(0, 0)], (-1, 1), (1,)), "reference"),
                       (lambda: V.warp_disparity(dr.double(), [(0, 0)], (-1, 1), (1, 1)), "float32"),
                       (lambda: V.warp_disparity(dr[0], [(0, 0)], (-1, 1), (1, 1)), "float32"),
                       (lambda: V.warp_disparity(dr, [(34, 1)], (-2, 2), (1, 1)), "reach 67")):
        with pytest.raises(LftError, match=words):
            bad()
    assert V.VisibleRenderResult._fields == V.RenderResult._fields + ("visible",)
    V.clear_cache()
