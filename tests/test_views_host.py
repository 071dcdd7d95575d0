"""CPU: view synthesis up to the device -- the blend tables and targets of lft_amd.views, refocus's `centre`, the new header and its
binding, every refusal of lft_view_render on the host, the Python refusals, and the numpy restatement (tests/views_util.py) on the
two scenes the GPU tests lean on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from lft_amd import _lib, refocus as R, views as V
from lft_amd._lib import LftError

import disparity_util as DU
import refocus_util as RU
import views_util as VU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = -1, -2
P, Q = 1 << 20, 2 << 20                                                       # addresses that are never dereferenced


def test_blend_tables():
    t = [(1, 2), (1.5, 2.25), (0.3, 3.9), (4.5, -0.5), (0, 0)]
    for blend in ("quad", "gaussian", "nearest"):
        if blend == "quad":
            with pytest.raises(LftError, match="every view has weight 0"):                   # a whole view step outside the grid
                V.blend_weights(5, t + [(5.0, 2)], blend)
        w = V.blend_weights(5, t, blend)
        assert w.dtype == np.float64 and np.all(w >= 0) and np.allclose(w.sum((1, 2)), 1.0, rtol=0, atol=1e-15)
    q = V.blend_weights(5, [(1, 2), (4, 0), (1.5, 2.25)])
    assert q[0, 1, 2] == 1.0 and q[0].sum() == 1.0 and q[1, 4, 0] == 1.0 and np.count_nonzero(q[:2]) == 2       # one-hot at integer targets
    assert np.count_nonzero(q[2]) == 4 and q[2, 1, 2] == 0.5 * 0.75 and q[2, 2, 3] == 0.5 * 0.25
    n = V.blend_weights(4, [(1.5, 1.5), (0.2, 2.9)], "nearest")
    assert n[0, 1, 1] == 1.0 and n[1, 0, 3] == 1.0 and np.count_nonzero(n) == 2                                   # lowest index on a tie
    g = V.blend_weights(3, [(1, 1)], "gaussian", sigma=0.5)
    assert np.isclose(g[0, 0, 1] / g[0, 1, 1], np.exp(-2.0)) and np.isclose(g[0, 0, 0] / g[0, 1, 1], np.exp(-4.0))
    ex = np.zeros((5, 5), bool)
    ex[1, 2] = True
    e = V.blend_weights(5, [(1, 2)], "gaussian", exclude=ex)
    assert e[0, 1, 2] == 0 and np.isclose(e.sum(), 1.0) and e[0, 1, 1] == e.max()
    with pytest.raises(LftError, match="every view has weight 0"):
        V.blend_weights(5, [(1, 2)], "quad", exclude=ex)
    with pytest.raises(LftError, match="every view has weight 0"):
        V.blend_weights(2, [(0, 0)], np.zeros((1, 2, 2)))
    user = np.arange(9, dtype=np.float64).reshape(1, 3, 3)
    assert np.allclose(V.blend_weights(3, [(1, 1)], user), user / 36)
    for bad in (lambda: V.blend_weights(3, [(1, 1)], "cubic"), lambda: V.blend_weights(3, [(1, 1)], np.ones((2, 3, 3))),
                lambda: V.blend_weights(3, [(1, 1)], -user), lambda: V.blend_weights(3, [(1, 1)], "gaussian", sigma=0.0),
                lambda: V.blend_weights(3, [(1, 1)], exclude=np.zeros((2, 2), bool)), lambda: V.blend_weights(3, [(1, np.nan)]),
                lambda: V.blend_weights(3, []), lambda: V.blend_weights(0, [(0, 0)])):
        with pytest.raises(LftError):
            bad()


def test_record_table_and_targets():
    t = [(1.5, 2.25), (2, 2)]
    tab = V.record_table(5, t, V.blend_weights(5, t))
    assert tab.dtype == V.RECORD and V.RECORD.itemsize == 16 and tab.shape == (2, 25)
    for n in range(25):
        u, v = divmod(n, 5)
        assert tab[0, n]["du"] == np.float32(u - 1.5) and tab[0, n]["dv"] == np.float32(v - 2.25)
    assert tab["skip"][0].sum() == 21 and tab["skip"][1].sum() == 24 and tab[1, 12]["w"] == 1.0 and tab[1, 12]["skip"] == 0
    assert np.all((tab["w"] == 0) == (tab["skip"] == 1))
    g = V.grid_targets(5, 2)
    assert g.shape == (9, 9, 2) and g[3, 8].tolist() == [1.5, 4.0] and g[0, 0].tolist() == [0, 0] and g[8, 8].tolist() == [4, 4]
    assert sum(1 for i in range(9) for j in range(9) if i % 2 or j % 2) == 56
    assert V.grid_targets(3, 1).shape == (3, 3, 2) and V.grid_targets(1, 4).shape == (1, 1, 2)
    for bad in ((5, 0), (5, 1.5), (0, 2), (5, True)):
        with pytest.raises(LftError):
            V.grid_targets(*bad)
    d = V.target_deltas(5, [(1.5, 2.25), (0.1, 4)])
    assert d.dtype == np.float32 and d.tolist() == [[-0.5, 0.25], [float(np.float32(0.1 - 2)), 2.0]]
    assert V.target_deltas(5, [(1.5, 2.25)], reference=(1, 3)).tolist() == [[0.5, -0.75]]
    assert V.splat_reach((-1.5, 2), d) == 5 and V.splat_reach((-1, 1), np.zeros((1, 2), np.float32)) == 1
    assert V.splat_reach((-1, 1), np.float32([[2, -2]])) == 3


def test_shift_table_centre_default_is_todays_table():
    """centre=None and centre=(uc, uc) give the table as it has always been: its bytes against a restatement of the original loop."""
    for A in (1, 2, 5):
        uc = (A - 1) / 2
        for interp in ("nearest", "linear", "cubic"):
            slopes = [-2.5, -0.3, 0.0, 0.75]
            want = np.zeros((len(slopes), A * A), dtype=R.RECORD)
            a = R.aperture_weights(A, "gaussian")
            for k, d in enumerate(slopes):
                axis = [R._axis(d * (i - uc), interp) for i in range(A)]
                for u in range(A):
                    for v in range(A):
                        r = want[k, u * A + v]
                        r["oy"], r["ox"], r["wy"], r["wx"], r["a"] = axis[u][0], axis[v][0], axis[u][1], axis[v][1], a[u, v]
                        r["skip"] = int(r["a"] == 0)
            assert R.shift_table(A, slopes, "gaussian", interp).tobytes() == want.tobytes()
            assert R.shift_table(A, slopes, "gaussian", interp, centre=(uc, uc)).tobytes() == want.tobytes()
    t = R.shift_table(5, [0.5], interp="linear", centre=(1, 3.5))
    assert t[0, 1 * 5 + 0]["oy"] == 0 and t[0, 1 * 5 + 0]["wy"][0] == 1.0                # u = cu: no shift
    assert t[0, 4 * 5 + 0]["oy"] == 1 and t[0, 4 * 5 + 0]["wy"][:2].tolist() == [0.5, 0.5]          # 0.5 * (4 - 1) = 1.5
    assert t[0, 0]["ox"] == -2 and t[0, 0]["wx"][:2].tolist() == [0.75, 0.25]            # 0.5 * (0 - 3.5) = -1.75
    for bad in ((1,), (1, np.inf), "ab"):
        with pytest.raises((LftError, ValueError)):
            R.shift_table(5, [0.5], centre=bad)


def test_header_declares_and_library_exports_the_view_entry_points():
    hdr = open(os.path.join(ROOT, "include", "lft_hip_views.h")).read()
    declared = set(re.findall(r"^int\s+(lft_\w+)\s*\(", hdr, flags=re.M))
    assert _lib.VIEW_EXPORTS == ("lft_view_render_scratch_bytes", "lft_view_render") and set(_lib.VIEW_EXPORTS) == declared
    assert "added beside ABI 5; lft_version unchanged" in " ".join(hdr.split()).replace("Added", "added")
    assert len(_lib._SIGS) == 59 and not set(_lib.VIEW_EXPORTS) & set(_lib.EXPORTS)       # the two older headers keep their 59 prototypes
    assert not set(_lib.VIEW_EXPORTS) & set(_lib.STREAM_LAST) and _lib.VIEW_STREAM_LAST == {"lft_view_render"}
    assert set(_lib.VIEW_EXPORTS) <= _lib.OPTIONAL_EXPORTS and _lib.UNITS == ("lft_network", "lft_lightfield", "lft_objective")
    assert "lft_views.cuh" in _lib.SOURCES
    for other in ("lft_hip.h", "lft_hip_test.h"):
        assert "lft_view_render" not in open(os.path.join(ROOT, "include", other)).read()
    users = [u for u in _lib.UNITS if "lft_views.cuh" in open(os.path.join(_lib.CSRC, u + ".hip")).read()]
    assert users == ["lft_lightfield"]
    assert (_lib.VIEW_NEAR_LARGER, _lib.VIEW_NEAR_SMALLER, _lib.VIEW_MAX_REACH, _lib.VIEW_MAX_FILL) == (0, 1, 64, 64)
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in _lib.VIEW_EXPORTS:
        assert hasattr(L, name), name
    assert _lib.lib().lft_version() == 5
    # the contract's sentences stand in the header, the kernels' comment and the module docstring
    kernels = open(os.path.join(_lib.CSRC, "lft_views.cuh")).read()
    for text in (hdr, kernels, V.__doc__):
        flat = " ".join(re.sub(r"^\s*(//|\*)\s?", "", line).replace("`", "").replace("**", "").strip() for line in text.splitlines())
        for words in ("non-finite pixels are", "sign convention is refocus's", "is dropped when py is integral", "does not depend on arrival order",
                      "Only pre-fill values are read", "which is exact", "Rows are filtered first, then columns, with explicit FMAs as in",
                      "the same quotient", "bit for bit"):
            assert words in flat.replace("`", ""), words


def test_scratch_query():
    assert _lib.query("lft_view_render_scratch_bytes", 2, 3, 37, 45) == 2 * 3 * 37 * 45 * 4
    assert _lib.query("lft_view_render_scratch_bytes", 0, 3, 37, 45) == 0
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    for args, rc in (((1, 0, 4, 4), ERR_ARG), ((-1, 3, 4, 4), ERR_SHAPE), ((1, 3, -4, 4), ERR_SHAPE), ((1 << 20, 64, 1 << 20, 1 << 20), ERR_SHAPE)):
        assert L.lft_view_render_scratch_bytes(*args, ctypes.byref(n)) == rc, args
        assert L.lft_last_error().decode().startswith("lft_view_render:")
    assert L.lft_view_render_scratch_bytes(1, 3, 4, 4, None) == ERR_ARG
    with pytest.raises(LftError, match=r"lft_view_render_scratch_bytes failed \(code -1\)"):
        _lib.query("lft_view_render_scratch_bytes", 1, 0, 4, 4)
    with pytest.raises(LftError, match="does not take its stream last"):
        _lib.enqueue("lft_view_render_scratch_bytes", "cuda:0", 1, 1, 1, 1)


GOOD = dict(lf=P, cls=_lib.LF_UINT8, B=1, A=5, H=10, W=10, C=1, st=(ctypes.c_longlong * 6)(0, 500, 100, 10, 1, 0), dr=Q, deltas=Q + 4096,
            max_delta=2.0, records=Q + 8192, T=3, taps=2, lo=-1.5, hi=2.0, near=0, fill=32, scratch=Q + 16384, views=Q + 32768,
            vcls=_lib.LF_FLOAT32, dt=Q + 65536, holes=Q + 98304, stream=None)


def render_raw(**kw):
    unknown = set(kw) - set(GOOD)
    assert not unknown, unknown
    return _lib.lib().lft_view_render(*{**GOOD, **kw}.values())


def test_every_refusal_comes_before_any_device_work():
    """Each call is answered on the host (this runs without a GPU): its code, and a message that starts with the entry point."""
    L = _lib.lib()
    neg = (ctypes.c_longlong * 6)(0, 500, 100, -10, 1, 0)
    wide = (ctypes.c_longlong * 6)(0, 0, 0, 1 << 28, 1, 0)
    inf, nan = float("inf"), float("nan")
    cases = [
        # the rules shared with lft_refocus, T in the place of the slope count
        (dict(cls=_lib.LF_FLOAT64), ERR_ARG, "light-field class"), (dict(cls=7), ERR_ARG, "light-field class"), (dict(vcls=_lib.LF_FLOAT64), ERR_ARG, "output class"),
        (dict(vcls=9), ERR_ARG, "output class"), (dict(A=0), ERR_ARG, "angRes"), (dict(C=0), ERR_ARG, "channels"), (dict(C=5), ERR_ARG, "channels"),
        (dict(T=0), ERR_ARG, "0 slopes"), (dict(T=-2), ERR_ARG, "-2 slopes"), (dict(B=-1), ERR_SHAPE, "negative size"), (dict(W=-4), ERR_SHAPE, "negative size"),
        (dict(st=neg), ERR_ARG, "stride 3 is negative"), (dict(st=wide), ERR_SHAPE, "spans"), (dict(B=1 << 20, H=1 << 20, W=1 << 20), ERR_SHAPE, "2^31"),
        # taps: 2 or 4
        (dict(taps=0), ERR_ARG, "taps"), (dict(taps=3), ERR_ARG, "taps"), (dict(taps=8), ERR_ARG, "taps"), (dict(taps=1), ERR_ARG, "1 taps (2 or 4"),
        # fill
        (dict(fill=-1), ERR_ARG, "fill -1 outside 0 .. 64"), (dict(fill=65), ERR_ARG, "fill 65 outside 0 .. 64"),
        # the range
        (dict(lo=2.0, hi=-1.5), ERR_ARG, "d_range"), (dict(lo=nan), ERR_ARG, "d_range"), (dict(hi=inf), ERR_ARG, "d_range"), (dict(lo=-inf), ERR_ARG, "d_range"),
        (dict(near=2), ERR_ARG, "near"), (dict(near=-1), ERR_ARG, "near"), (dict(max_delta=-1.0), ERR_ARG, "max_delta"), (dict(max_delta=nan), ERR_ARG, "max_delta"),
        # the reach: ceil(2 * 31.6) + 1 = 65
        (dict(max_delta=31.6), ERR_SHAPE, "reach 65"), (dict(lo=-100.0, max_delta=1.0), ERR_SHAPE, "reach 101"),
        # null pointers
        (dict(lf=None), ERR_ARG, "null pointer"), (dict(st=None), ERR_ARG, "null pointer"), (dict(dr=None), ERR_ARG, "null pointer"),
        (dict(deltas=None), ERR_ARG, "null pointer"), (dict(records=None), ERR_ARG, "null pointer"), (dict(scratch=None), ERR_ARG, "null pointer"),
        (dict(views=None), ERR_ARG, "null pointer"), (dict(dt=None), ERR_ARG, "null pointer"), (dict(holes=None), ERR_ARG, "null pointer"),
        # the scratch, and what comes before it
        (dict(scratch=Q + 16386), ERR_ARG, "scratch must be 4-byte aligned"), (dict(scratch=Q + 16386, fill=70), ERR_ARG, "fill"),
        (dict(H=(1 << 24) + 1, st=(ctypes.c_longlong * 6)(0, 0, 0, 1, 1, 0)), ERR_SHAPE, "2^24"),
        (dict(B=64, T=4096, H=2048, W=2048), ERR_SHAPE, "2^31"),
    ]
    for kw, rc, words in cases:
        L.lft_refocus(None, 99, 1, 1, 1, 1, 1, None, None, 1, 1, None, 0, None)              # leaves another call's message behind
        assert render_raw(**kw) == rc, kw
        msg = L.lft_last_error().decode()
        assert msg.startswith("lft_view_render:") and words in msg and "99" not in msg, (kw, msg)
    # the largest reach is accepted: what refuses this call is the misaligned scratch behind it
    assert render_raw(max_delta=31.5, scratch=Q + 16386) == ERR_ARG and b"scratch" in L.lft_last_error()
    # empty shapes are no error and no work, null pointers included; the values are still judged
    for kw in (dict(B=0), dict(H=0), dict(W=0)):
        assert render_raw(lf=None, dr=None, scratch=None, views=None, dt=None, holes=None, **kw) == 0, kw
        assert render_raw(fill=70, **kw) == ERR_ARG, kw


def test_python_refusals_need_no_device():
    lf, dr = torch.zeros(3, 3, 6, 6), torch.zeros(6, 6)
    with pytest.raises(LftError, match="no CPU path"):
        V.render(lf, dr, [(1, 1)], (-1, 1))
    with pytest.raises(LftError, match="torch tensor"):
        V.render(np.zeros((3, 3, 6, 6), np.float32), dr, [(1, 1)], (-1, 1))
    for kw, words in ((dict(interp="nearest"), "interp"), (dict(interp="lanczos"), "interp"), (dict(near="nearer"), "near"), (dict(fill=65), "fill"),
                      (dict(fill=-1), "fill"), (dict(fill=1.5), "fill"), (dict(fill=True), "fill"), (dict(out_dtype=torch.float16), "out_dtype"),
                      (dict(blend="box"), "blend"), (dict(sigma=-1.0, blend="gaussian"), "sigma"), (dict(exclude=np.ones((3, 3), bool)), "weight 0"),
                      (dict(reference=(1,)), "reference")):
        with pytest.raises(LftError, match=words):
            V.render(lf, dr, [(1, 1)], (-1, 1), **kw)
    for d_range in ((1, -1), (0, np.inf), (np.nan, 1), 3, (1, 2, 3)):
        with pytest.raises(LftError, match="d_range"):
            V.render(lf, dr, [(1, 1)], d_range)
    for targets in ([], [(1, np.nan)], [(1, 2, 3)], 5):
        with pytest.raises(LftError, match="targets"):
            V.render(lf, dr, targets, (-1, 1))
    with pytest.raises(LftError, match="weight 0"):
        V.render(lf, dr, [(3.5, 1)], (-1, 1))                                              # quad outside the grid
    with pytest.raises(LftError, match="reach 65"):
        V.render(lf, dr, [(33, 1)], (-2, 2), blend="gaussian")                             # 2 * 32 + 1
    with pytest.raises(LftError, match="float32"):
        V.render(lf, dr.double(), [(1, 1)], (-1, 1))
    with pytest.raises(LftError, match="float64"):
        V.render(lf.double(), dr, [(1, 1)], (-1, 1))
    with pytest.raises(LftError, match="no CPU path"):
        V.densify(lf, dr, 2, (-1, 1))
    with pytest.raises(LftError, match="no CPU path"):
        V.leave_one_out(lf, [-1.0, 0.0, 1.0])
    with pytest.raises(LftError, match="slopes"):
        V.leave_one_out(lf, [1.0, 0.0])
    V.clear_cache()


def test_restatement_on_the_plane():
    """Geometry, on the reference alone: a plane of slope d0 rendered at a fractional target is f displaced by d0 * (target - centre),
    within the linear interpolation bound max|f_yy| / 8 + max|f_xx| / 8 = (0.45^2 + 0.37^2) / 16 = 0.0213; a wrong sign is not."""
    A, H, W = 5, 40, 44
    f = lambda y, x: 0.5 + 0.5 * np.sin(0.45 * y + 0.3) * np.cos(0.37 * x - 0.2)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    worst = 0.0
    for d0 in (0.6, -1.3):
        L, _ = RU.plane(A, H, W, d0)
        Dr = np.full((H, W), d0, np.float32)
        for t in ((1.5, 2.25), (0.3, 3.9)):
            delta = V.target_deltas(A, [t])[0]
            Dt, holes = VU.fill_np(VU.splat_np(Dr, delta, (-2, 2)), Dr, (-2, 2))
            assert np.all(Dt == np.float32(d0))
            rec = V.record_table(A, [t], V.blend_weights(A, [t]))[0]
            got = VU.render_np(L[..., None], Dt, rec, 2)[..., 0]
            want = f(y - d0 * (t[0] - 2), x - d0 * (t[1] - 2))
            wrong = f(y + d0 * (t[0] - 2), x + d0 * (t[1] - 2))
            inner = (slice(4, H - 4), slice(4, W - 4))
            worst = max(worst, float(np.abs(got - want)[inner].max()))
            assert float(np.abs(got - wrong)[inner].max()) > 0.1
    print(f"plane: fp64 restatement within {worst:.4f} of f (bound 0.0213)")
    assert worst <= 0.0213


def test_restatement_on_the_two_layers():
    """Occlusion, on the reference alone: the foreground wins the splat, the holes take the background, and away from the ring
    around the box every view agrees, so the held-out view comes back to rounding."""
    A, H, W = 5, 72, 64
    L, _ = DU.two_layer(A, H, W)
    y0, y1, x0, x1 = DU.FG_BOX
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    Dr = np.where((yy >= y0) & (yy < y1) & (xx >= x0) & (xx < x1), 1.0, -1.0).astype(np.float32)
    for t in ((0, 1), (4, 4), (1, 3), (2, 2)):
        want, b5, held, fg = VU.occlusion_masks(t)
        delta = V.target_deltas(A, [t])[0]
        Dt, holes = VU.fill_np(VU.splat_np(Dr, delta, (-1, 1)), Dr, (-1, 1))
        assert np.array_equal(Dt[b5], want[b5]), t
        assert (holes.sum() > 0) == (t != (2, 2))
        ex = np.zeros((A, A), bool)
        ex[t] = True
        rec = V.record_table(A, [t], V.blend_weights(A, [t], "gaussian", exclude=ex))[0]
        assert rec["skip"].sum() == 1
        got = VU.render_np(L, Dt, rec, 2)[..., 0]
        err = np.abs(got - L[t[0], t[1], ..., 0].astype(np.float64))
        assert held.mean() >= 0.25 and (held & fg).sum() == 676
        assert float(err[held].max()) <= 1e-15 and float(err[~held].max()) > 0.1, (t, float(err[held].max()))
