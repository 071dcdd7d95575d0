"""CPU: angular tiling of a U x V field up to the device -- the origins formula against brute force, the new header and its binding,
every refusal of the entry points on the host, every Python refusal, the tool's argument parsing, and on the restatement alone
(tests/field_util.py): one window is the restatements of tests/shear_util.py and tests/blend_util.py."""
import ctypes
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import _lib, colour, field as F, scene as S
from lft_amd._lib import LftError

import blend_util as BU
import field_util as FU
import shear_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = -1, -2
P, Q, T, W, G = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20        # addresses that are never dereferenced
NAMES = ("lft_field_counts", "lft_field_divide", "lft_field_integrate")


# ---- 1. the windows ----
def test_origins_against_brute_force():
    for A in range(1, 13):
        for L in range(A, 13):
            for astride in range(1, A + 1):
                o = F.origins(L, A, astride)
                assert o == FU.origins_np(L, A, astride)
                # brute force: step by astride while the window fits, then one clamped window if the last view is not covered yet
                want = list(range(0, L - A + 1, astride))
                if want[-1] + A < L:
                    want.append(L - A)
                assert o == want, (L, A, astride)
                assert all(b > a for a, b in zip(o, o[1:])) and o[0] == 0 and o[-1] == L - A
                assert all(b - a <= A for a, b in zip(o, o[1:]))
                mult = [sum(1 for x in o if x <= p < x + A) for p in range(L)]
                assert min(mult) >= 1 and max(mult) <= -(-A // astride) + 1, (L, A, astride, mult)
                mu, mv = F.counts(L, A, A, astride)
                assert (mu, mv) == (len(o), 1)
                assert F.counts(A, L, A, astride) == (1, len(o))
    assert F.origins(5, 2, 2) == [0, 2, 3]              # the extra-multiplicity view: 3 is in two windows at astride = A
    assert F.origins(9, 5) == [0, 4] and F.origins(9, 5, 2) == [0, 2, 4] and F.origins(17, 5) == [0, 5, 10, 12]
    assert F.counts(9, 9, 5) == (2, 2) and F.counts(9, 9, 5, 2) == (3, 3) and F.counts(4, 5, 2, 1) == (3, 4)


# ---- 2. the header and its binding ----
def test_header_declares_the_exports_and_the_binding_holds_them():
    hdr = open(os.path.join(ROOT, "include", "lft_hip_field.h")).read()
    assert tuple(re.findall(r"^int\s+(lft_\w+)\s*\(", hdr, flags=re.M)) == NAMES
    assert "Added beside ABI 5; lft_version unchanged" in hdr and "#define LFT_FIELD_MAX_VIEWS 64" in hdr
    assert _lib.FIELD_EXPORTS == NAMES and _lib.ADDON_HEADERS["lft_hip_field.h"] == "FIELD_" and _lib.FIELD_MAX_VIEWS == 64
    keys = list(_lib.ADDON_HEADERS)
    assert keys[-2:] == ["lft_hip_refine.h", "lft_hip_focal.h"] and keys.index("lft_hip_field.h") == keys.index("lft_hip_blend.h") + 1 == len(keys) - 3
    assert len(_lib._SIGS) == 59 and len(_lib.UNITS) == 3
    for name in NAMES:
        assert name in _lib.OPTIONAL_EXPORTS and name not in _lib.EXPORTS
    assert set(NAMES) & _lib.ADDON_STREAM_LAST == set(NAMES[1:])
    from ctypes import c_int, c_void_p
    assert _lib._ADDON_SIGS[NAMES[0]] == (c_int, [c_int] * 4 + [c_void_p] * 2)
    assert _lib._ADDON_SIGS[NAMES[1]] == (c_int, [c_void_p] * 3 + [c_int] * 8 + [c_void_p])
    assert _lib._ADDON_SIGS[NAMES[2]] == (c_int, [c_void_p] * 5 + [c_int] * 9 + [c_void_p])
    words = {NAMES[0]: ["U", "V", "A", "astride", "mu", "mv"],
             NAMES[1]: ["field", "shear", "patches", "U", "V", "A", "astride", "h0", "w0", "patch", "stride", "stream"],
             NAMES[2]: ["sr_patches", "shear", "window", "angular", "sr_field", "U", "V", "A", "astride", "h0", "w0", "patch", "stride", "s", "stream"]}
    for name, want in words.items():
        params = re.search(name + r"\s*\(([^)]*)\)\s*;", hdr).group(1).split(",")
        assert [p.split()[-1].lstrip("*") for p in params] == want
    assert "lft_field.cuh" in _lib.SOURCES
    assert [u for u in _lib.UNITS if '"lft_field.cuh"' in open(os.path.join(_lib.CSRC, u + ".hip")).read()] == ["lft_lightfield"]
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(L, n) for n in NAMES) and _lib.lib().lft_version() == 5
    kernel = open(os.path.join(_lib.CSRC, "lft_field.cuh")).read()
    assert "k_field_divide" in kernel and "k_field_integrate" in kernel and "#pragma clang fp contract(off)" in kernel and "__fdiv_rn" in kernel
    for fn in ("reflect_idx", "fold_idx", "clamp_shear"):                   # reused, not restated
        assert not re.search(r"LFT_DEV\s+int\s+" + fn, kernel)
    assert "asm" not in kernel and "atomic" not in kernel
    # the definition's sentences stand in the header, the kernel file's comment and the module docstring
    for text in (hdr, kernel, F.__doc__):
        flat = " ".join(re.sub(r"^\s*(//|\*|-)\s?", "", line).replace("`", "").strip() for line in text.splitlines())
        flat = flat.replace("−", "-").replace("≥", ">=").replace("≤", "<=").replace("·", "*").replace(" // ", " / ")
        for words_ in ("o_i = min(i*astride, L-A)", "b = w*N + n", "ceil((L-A)/astride) + 1", "ascending wu, then wv, then ku, then kv", "ga = g[u]*g[v]",
                       "wt = ga*(win[a]*win[b])", "one rounded fp32 operation", "correctly rounded", "No sub-mosaic is materialised"):
            assert words_ in flat, words_


# ---- 3. every refusal of the entry points is answered on the host ----
def test_every_c_refusal_comes_before_any_device_work():
    _lib.build()
    L = _lib.lib()

    def refused(name, args, rc, words):
        L.lft_scene_counts(1, 1, 1, 1, None, None)      # leaves another call's message behind
        assert getattr(L, name)(*args) == rc, (name, args)
        msg = L.lft_last_error().decode()
        assert words in msg and msg.startswith(name + ":") or words in msg and ("bad scene tiling" in msg or "smaller than one patch" in msg), (args, msg)
        return msg

    # counts: host only
    mu, mv = ctypes.c_int(0), ctypes.c_int(0)
    assert L.lft_field_counts(9, 17, 5, 4, ctypes.byref(mu), ctypes.byref(mv)) == 0 and (mu.value, mv.value) == (2, 4)
    refused(NAMES[0], (9, 9, 5, 5, None, ctypes.byref(mv)), ERR_ARG, "null pointer")
    refused(NAMES[0], (9, 9, 0, 1, ctypes.byref(mu), ctypes.byref(mv)), ERR_ARG, "angRes 0")
    for U, V in ((4, 9), (9, 4), (65, 9), (9, 65)):
        refused(NAMES[0], (U, V, 5, 5, ctypes.byref(mu), ctypes.byref(mv)), ERR_SHAPE, f"a field of {U} x {V} views")
    for a in (0, 6, -1):
        refused(NAMES[0], (9, 9, 5, a, ctypes.byref(mu), ctypes.byref(mv)), ERR_SHAPE, f"angular stride {a}")

    dkeys = ("field", "shear", "patches", "U", "V", "A", "astride", "h0", "w0", "patch", "stride", "stream")
    dgood = dict(zip(dkeys, (P, Q, T, 9, 9, 5, 4, 64, 64, 32, 16, None)))
    ikeys = ("sub", "shear", "window", "angular", "out", "U", "V", "A", "astride", "h0", "w0", "patch", "stride", "s", "stream")
    igood = dict(zip(ikeys, (P, Q, W, G, T, 9, 9, 5, 4, 64, 64, 32, 16, 2, None)))
    for name, good, ptrs in ((NAMES[1], dgood, ("field", "patches")), (NAMES[2], igood, ("sub", "angular", "out"))):
        change = lambda **kw: [kw.get(k, v) for k, v in good.items()]
        for k in ptrs:
            refused(name, change(**{k: None}), ERR_ARG, "null pointer")
        refused(name, change(A=0), ERR_ARG, name + ": angRes 0")
        for kw in (dict(U=4), dict(V=4), dict(U=65), dict(V=65)):
            refused(name, change(**kw), ERR_SHAPE, name + ": a field of")
        for a in (0, 6):
            refused(name, change(astride=a), ERR_SHAPE, name + f": angular stride {a}")
        # the pointers come first, then the sizes
        refused(name, change(**{ptrs[0]: None, "stride": 0, "U": 1}), ERR_ARG, "null pointer")
        # the existing entry points' tilings, with their words -- with and without a shear / a window
        for nulls in ({}, {"shear": None}, {"shear": None, "window": None}):
            nulls = {k: v for k, v in nulls.items() if k in good}
            for kw, words in ((dict(stride=33), "bad scene tiling"), (dict(stride=0), "bad scene tiling"), (dict(h0=0), "bad scene tiling"),
                              (dict(patch=0), "bad scene tiling"), (dict(h0=8), "smaller than one patch")):
                L.lft_scene_counts(1, 1, 1, 1, None, None)
                a = change(**kw, **nulls)
                assert L.lft_scene_divide(P, T, 5, *[dict(good, **kw)[k] for k in ("h0", "w0", "patch", "stride")], None) == ERR_SHAPE
                want = L.lft_last_error().decode()
                assert words in want and refused(name, a, ERR_SHAPE, words) == want
    change = lambda **kw: [kw.get(k, v) for k, v in dgood.items()]
    refused(NAMES[1], change(patch=31), ERR_SHAPE, NAMES[1] + ": patch - stride = 15 is odd")
    assert L.lft_scene_divide_shear(P, Q, T, 5, 64, 64, 31, 16, None) == ERR_SHAPE         # the existing entry point refuses it too
    refused(NAMES[1], change(A=1, U=1, V=1, astride=1, patch=70000, stride=70000, h0=70000, w0=70000), ERR_SHAPE, "need more than 65535 blocks")
    refused(NAMES[1], change(h0=300000000, w0=64, patch=32, stride=16, shear=None), ERR_SHAPE, "need more than 65535 blocks")
    refused(NAMES[1], change(U=64, h0=65535 * 520, w0=65535, patch=65535, stride=65535, A=1, astride=1), ERR_SHAPE, "indexed beyond 2^31")
    change = lambda **kw: [kw.get(k, v) for k, v in igood.items()]
    for s in (0, 1, 3, 8, -2):
        refused(NAMES[2], change(s=s), ERR_ARG, NAMES[2] + f": scale factor {s}")
    refused(NAMES[2], change(angular=None, s=3), ERR_ARG, "null pointer")
    refused(NAMES[2], change(patch=31), ERR_SHAPE, NAMES[2] + ": patch - stride = 15 is odd")
    refused(NAMES[2], change(patch=31, shear=None), ERR_SHAPE, "patch - stride = 15 is odd")             # a window alone
    refused(NAMES[2], change(stride=23, window=None), ERR_SHAPE, "patch - stride = 9 is odd")            # a shear alone
    refused(NAMES[2], change(patch=4096, stride=4096, h0=4096, w0=4096, s=4, A=1, U=1, V=1, astride=1), ERR_SHAPE, "a window of 16384 entries (at most 8192)")
    refused(NAMES[2], change(A=1, U=1, V=1, astride=1, h0=30000, s=4), ERR_SHAPE, "an SR field mosaic of 120000 rows needs more than 65535 blocks")
    refused(NAMES[2], change(U=64, h0=600), ERR_SHAPE, "an SR field mosaic of 76800 rows")
    refused(NAMES[2], change(V=64, h0=32, w0=20000000, s=4, A=1, astride=1, U=1), ERR_SHAPE, "indexed beyond 2^31")


# ---- 4. Python refusals need no device ----
def test_python_refusals_need_no_device():
    U, V, A, patch, stride, s, h0, w0 = 9, 7, 5, 32, 16, 2, 48, 64
    assert F.counts(U, V, A, 4) == (2, 2) and S.scene_counts(h0, w0) == (3, 4)
    B = 2 * 2 * 12
    field = torch.zeros(U * h0, V * w0)
    sr = torch.zeros(B, 1, A * patch * s, A * patch * s)
    net = SimpleNamespace(angRes=A, factor=s)
    calls = (lambda **kw: F.divide(field, U, V, A, **{"astride": 4, **kw}),
             lambda **kw: F.integrate(sr, U, V, A, h0, w0, s, **{"astride": 4, **kw}),
             lambda **kw: F.super_resolve_field(net, field, U, V, **{"astride": 4, **kw}))
    for call in calls:
        for bad in (0, 6, -1, 2.0, True, "4"):
            with pytest.raises(LftError, match="astride must be None or an integer in 1 .. angRes = 5"):
                call(astride=bad)
        with pytest.raises(LftError, match=r"shear must be an int32 tensor of shape \[48\]"):
            call(shear=torch.zeros(47, dtype=torch.int32))
        with pytest.raises(LftError, match=r"shear must be an int32 tensor of shape \[48\]"):
            call(shear=torch.zeros(48))
        with pytest.raises(LftError, match="shear is on meta"):
            call(shear=torch.zeros(48, dtype=torch.int32, device="meta"))
        with pytest.raises(LftError, match="on a HIP device"):     # everything right: the device is asked for last
            call()
        with pytest.raises(LftError, match="on a HIP device"):
            call(shear=torch.zeros(48, dtype=torch.int32), astride=None)
    for call in calls[1:]:
        for bad in ("box", "Hann", 1, None, [1.0] * 5, np.ones(5, np.float32), torch.ones(5, dtype=torch.float64), torch.ones(4), torch.ones(1, 5)):
            with pytest.raises(LftError, match="angular must be one of hann, linear, flat, or a float32 tensor of shape"):
                call(angular=bad)
        with pytest.raises(LftError, match="angular is on meta"):
            call(angular=torch.ones(5, device="meta"))
        with pytest.raises(LftError, match="blend is on meta"):
            call(blend=torch.ones(64, device="meta"))
        with pytest.raises(LftError, match="blend must be None, one of hann, linear, flat"):
            call(blend="cosine")
        with pytest.raises(LftError, match="is odd"):
            call(blend="hann", stride=15)
        for kw in (dict(angular="hann"), dict(angular=torch.ones(5), blend="linear"), dict(blend=torch.ones(64), shear=torch.zeros(48, dtype=torch.int32))):
            with pytest.raises(LftError, match="on a HIP device"):
                call(**kw)
    # the views and the field's shape
    for u, v in ((4, 7), (9, 4), (65, 7)):
        with pytest.raises(LftError, match=f"a field of {u} x {v} views"):
            F.divide(field, u, v, A)
        with pytest.raises(LftError, match=f"a field of {u} x {v} views"):
            F.integrate(sr, u, v, A, h0, w0, s)
        with pytest.raises(LftError, match=f"a field of {u} x {v} views"):
            F.super_resolve_field(net, field, u, v)
    with pytest.raises(LftError, match="a field of 3 x 3 views"):
        F.counts(3, 3, 5)
    with pytest.raises(LftError, match="a field of 3 x 3 views"):
        F.origins(3, 5)
    for bad in (torch.zeros(U * h0 + 1, V * w0), torch.zeros(U * h0, V * w0 + 3), torch.zeros(0, V * w0)):
        with pytest.raises(LftError, match=r"field must be a mosaic \[U\*h0, V\*w0\] of 9 x 7 views"):
            F.divide(bad, U, V, A)
        with pytest.raises(LftError, match=r"field must be a mosaic"):
            F.super_resolve_field(net, bad, U, V)
    for bad in (torch.zeros(3, U * h0, V * w0), np.zeros((U * h0, V * w0), np.float32)):
        with pytest.raises(LftError, match="field must be a 2-D float32 tensor"):
            F.divide(bad, U, V, A)
        with pytest.raises(LftError, match="field must be a 2-D float32 tensor"):
            F.super_resolve_field(net, bad, U, V)
    with pytest.raises(LftError, match=r"sr_patches must be \[48, 1, 320, 320\] for this tiling"):
        F.integrate(sr[:47], U, V, A, h0, w0, s, astride=4)
    with pytest.raises(LftError, match=r"sr_patches must be \[72, 1, 320, 320\]"):
        F.integrate(sr, U, V, A, h0, w0, s, astride=2)
    with pytest.raises(LftError, match="scale factor must be 2 or 4, got 3"):
        F.integrate(sr, U, V, A, h0, w0, 3)
    with pytest.raises(LftError, match="scale factor must be 2 or 4"):
        F.super_resolve_field(SimpleNamespace(angRes=A, factor=3), field, U, V)
    with pytest.raises(LftError, match="bad scene tiling"):
        F.divide(field, U, V, A, 16, 32)
    # the whole field: super_resolve_scene's words
    with pytest.raises(LftError, match="shear together with ensemble is not supported"):
        F.super_resolve_field(net, field, U, V, shear=1, ensemble="flips")
    for bad in (1.5, True, "Auto", [1]):
        with pytest.raises(LftError, match="shear must be None, an integer, an int32 tensor or auto"):
            F.super_resolve_field(net, field, U, V, shear=bad)
    with pytest.raises(LftError, match="shear 5: kmax is 4"):
        F.super_resolve_field(net, field, U, V, shear=5)
    for kw in (dict(shear=2), dict(shear="auto"), dict(ensemble="flips", blend="hann"), dict(astride=1, angular="linear")):
        with pytest.raises(LftError, match="on a HIP device"):
            F.super_resolve_field(net, field, U, V, **kw)
    # the colour path
    with pytest.raises(LftError, match="views must be centre or all"):
        colour.super_resolve_lf(net, torch.zeros(9, 9, 4, 4, 3), views="every")
    with pytest.raises(LftError, match=r"a light field of shape \(9, 7, 4, 4, 3\) has 9 x 7 views"):
        colour.super_resolve_lf(net, torch.zeros(9, 7, 4, 4, 3), views="all")
    with pytest.raises(LftError, match="must be on the GPU"):
        colour.super_resolve_lf(net, torch.zeros(9, 9, 4, 4, 3), views="all")


# ---- 5. the tool ----
def test_tool_parses_views_and_hands_them_on(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import super_resolve
    from lft_amd import prepare
    net = SimpleNamespace(angRes=5, factor=2)
    got = {}
    monkeypatch.setattr(super_resolve, "load_model", lambda a, dev: got.setdefault("loaded", True) and net)
    monkeypatch.setattr(super_resolve, "load_field", lambda path, A, dev: got.update(load_A=A) or "lf")
    monkeypatch.setattr(super_resolve, "write_views", lambda *a, **kw: [])
    monkeypatch.setattr(prepare, "load_lf", lambda path: got.update(loads=got.get("loads", 0) + 1) or np.zeros(got["shape"], np.uint8))
    monkeypatch.setattr(prepare, "to_device", lambda lf, A, dev: got.update(load_A=A) or "lf")
    monkeypatch.setattr(colour, "super_resolve_lf", lambda net, lf, patch, stride, **kw: got.update(kw=kw) or torch.zeros(2, 2, 4, 4, 3))
    base = ["--path_pre_pth", "x", "--lf", "y", "--out_dir", os.devnull + "_unused", "--angRes", "5", "--scale_factor", "2"]
    monkeypatch.setattr(os, "makedirs", lambda *a, **kw: None)
    for bad in (["--angular_stride", "0"], ["--angular_stride", "6"]):
        with pytest.raises(LftError, match="astride must be None or an integer in 1 .. angRes = 5"):
            super_resolve.main(base + ["--views", "all"] + bad)
    with pytest.raises(LftError, match="--angular_window takes hann, linear, flat"):
        super_resolve.main(base + ["--views", "all", "--angular_window", "box"])
    with pytest.raises(SystemExit):
        super_resolve.main(base + ["--views", "some"])
    for orphan in (["--angular_stride", "2"], ["--angular_window", "hann"], ["--views", "centre", "--angular_stride", "5"]):
        with pytest.raises(LftError, match="--angular_stride and --angular_window belong to --views all"):
            super_resolve.main(base + orphan)
    assert not got                                      # judged before the model is loaded
    got["shape"] = (9, 7, 4, 4, 3)
    with pytest.raises(LftError, match="--views all: y holds a light field of shape"):
        super_resolve.main(base + ["--views", "all"])
    got["shape"] = (9, 9, 4, 4, 3)
    super_resolve.main(base + ["--views", "all", "--angular_stride", "2", "--angular_window", "hann", "--blend", "linear"])
    assert got["load_A"] == 9 and got["loads"] == 2 and got["kw"] == dict(ensemble=None, shear=None, blend="linear", views="all", astride=2, angular="hann")
    super_resolve.main(base + ["--views", "all"])
    assert got["kw"] == dict(ensemble=None, shear=None, views="all", astride=None, angular="flat")
    # without --views: the call it always made
    super_resolve.main(base)
    assert got["load_A"] == 5 and got["kw"] == dict(ensemble=None, shear=None)
    super_resolve.main(base + ["--views", "centre", "--shear", "2"])
    assert got["kw"] == dict(ensemble=None, shear=2)


# ---- 6. the restatement alone ----
@pytest.mark.parametrize("A,s", [(2, 2), (3, 4)])
@pytest.mark.parametrize("patch,stride", [(8, 4), (8, 6), (8, 8)])
@pytest.mark.parametrize("sheared", [False, True])
def test_one_window_is_the_scene_restatements(A, s, patch, stride, sheared):
    h0, w0 = 9, 14
    rng = np.random.default_rng([61, A, s, patch, stride, sheared])
    N = int(np.prod(SU.counts_np(h0, w0, patch, stride)))
    kmax = SU.kmax_np(A, patch, stride)
    k = rng.integers(-kmax - 1, kmax + 2, N) if sheared else None
    scene = rng.random((A * h0, A * w0), dtype=np.float32)
    cut = FU.divide_np(scene, A, A, A, A, patch, stride, k)
    assert np.array_equal(cut, SU.divide_plain_np(scene, A, patch, stride) if k is None else SU.divide_np(scene, A, patch, stride, k))
    sr = rng.random((N, A * patch * s, A * patch * s), dtype=np.float32)
    flat = np.ones(A, np.float32)
    crop, T1 = FU.integrate_np(sr, A, A, A, A, h0, w0, patch, stride, s, flat, None, k)
    assert (T1 == 1).all()
    assert np.array_equal(crop, SU.integrate_plain_np(sr, A, h0, w0, patch, stride, s) if k is None else SU.integrate_np(sr, A, h0, w0, patch, stride, s, k))
    for kind in BU.WINDOWS:
        w = BU.window_np(kind, patch * s)
        got, T = FU.integrate_np(sr, A, A, A, A, h0, w0, patch, stride, s, flat, w, k)
        want, terms = BU.blend_np(sr, A, h0, w0, patch, stride, s, w, k)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)) and np.array_equal(T, terms)


@pytest.mark.parametrize("U,V,A,astride", [(4, 5, 2, 1), (5, 3, 3, 2), (4, 4, 3, 2), (5, 5, 2, 2), (3, 3, 3, 3)])
def test_a_perfect_networks_patches_give_back_the_field(U, V, A, astride):
    h0, w0, patch, stride, s = 9, 14, 8, 4, 2
    rng = np.random.default_rng([62, U, V, A, astride])
    Gf = rng.random((U * h0 * s, V * w0 * s), dtype=np.float32)
    mu, mv = len(FU.origins_np(U, A, astride)), len(FU.origins_np(V, A, astride))
    N = int(np.prod(SU.counts_np(h0, w0, patch, stride)))
    kmax = SU.kmax_np(A, patch, stride)
    k = rng.integers(-kmax - 1, kmax + 2, mu * mv * N)
    cut = FU.cut_np(Gf, U, V, A, astride, patch, stride, s, k)
    g = (rng.random(A, dtype=np.float32) + np.float32(0.25))
    for win in (None, BU.window_np("hann", patch * s)):
        out, T = FU.integrate_np(cut, U, V, A, astride, h0, w0, patch, stride, s, g, win, k)
        assert np.abs(out.astype(np.float64) - Gf).max() <= (2 * int(T.max()) + 1) * FU.EPS * float(np.abs(Gf).max())
        if win is None:                                 # the crop: one term per window, so T is the views' multiplicity
            mult = lambda L: np.array([sum(1 for o in FU.origins_np(L, A, astride) if o <= p < o + A) for p in range(L)])
            assert np.array_equal(T.reshape(U, h0 * s, V, w0 * s)[:, 0, :, 0], mult(U)[:, None] * mult(V)[None, :])
