"""CPU tests of the three calling conventions lft_amd._lib writes once -- call, query, enqueue -- against the raw ctypes calls they
replace.  Host only: the library loads without a GPU, and every call here is answered before any device call."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest

from lft_amd import _lib

import abi_refusals_util as R

SIZE_P = ctypes.POINTER(ctypes.c_size_t)
# one accepted argument set per size query: the `good` sets of tests/abi_refusals_util.py without their size_t* outputs
QUERIES = {"lft_packed_bytes": (5, 6, 6, 2, 0), "lft_workspace_bytes": (1, 5, 6, 6, 2, 0), "lft_train_tape_bytes": (1, 2, 4, 4, 2),
           "lft_train_grad_floats": (2,), "lft_train_tape_offset": (b"feat", 1, 2, 4, 4, 2),       # not the first field, whose offset is 0
           "lft_train_grad_bucket": (2, 0), "lft_attn_maps_floats": (_lib.BLOCK_ANG, _lib.MAPS_MEAN, 1, 2, 4, 4),
           "lft_lf_loss_scratch_bytes": (1, 2, 16, 16), "lft_ssim_loss_scratch_bytes": (1, 2, 16, 16), "lft_guard_bytes": (3,),
           "lft_view_metrics_scratch_bytes": (1, 2, 16, 16), "lft_disparity_scratch_bytes": (1, 3, 10, 10, 1, 0)}
NOT_STREAM_LAST = ("lft_guard_read", "lft_train_backward_buckets", "lft_forward_profiled", "lft_kernel_time", "lft_train_step_profiled",
                   "lft_packed_bytes")


def raw(name, args):
    """(return code, values) of the hand-written convention: one c_size_t per output, passed by reference."""
    outs = [ctypes.c_size_t(0) for t in _lib._SIGS[name][1] if t is SIZE_P]
    rc = getattr(_lib.lib(), name)(*args, *[ctypes.byref(o) for o in outs])
    return rc, tuple(o.value for o in outs)


@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library from here on fails the test (it is loaded first, so that the patch is all a call could meet)."""
    def used():
        raise AssertionError("the library was reached")
    _lib.lib()
    monkeypatch.setattr(_lib, "lib", used)


def test_call_raises_with_the_entry_point_the_code_and_the_message():
    n = ctypes.c_size_t(0)
    assert _lib.call("lft_train_grad_floats", 2, ctypes.byref(n)) is None and n.value == 1_114_240
    with pytest.raises(_lib.LftError) as e:
        _lib.call("lft_train_grad_floats", 3, ctypes.byref(n))
    said = _lib.lib().lft_last_error().decode()
    assert said and str(e.value) == f"lft_train_grad_floats failed (code -2): {said}"


@pytest.mark.parametrize("name", sorted(QUERIES))
def test_query_equals_the_raw_call(name):
    types = _lib._SIGS[name][1]
    k = types.count(SIZE_P)
    assert types[-k:] == [SIZE_P] * k and k == (2 if name == "lft_train_grad_bucket" else 1)
    # the accepted set, then every refusal-table case that hands in all its outputs: the raw call's values, or LftError where it refuses
    sets = [("good", QUERIES[name])] + [(case, args[:-k]) for entry, case, args in R.cases() if entry == name and None not in args[-k:]]
    assert len(sets) > 1
    for case, args in sets:
        rc, want = raw(name, args)
        if rc == 0:
            got = _lib.query(name, *args)
            assert (got if k > 1 else (got,)) == want and all(type(v) is int for v in (got if k > 1 else (got,))), case
        else:
            with pytest.raises(_lib.LftError, match=rf"{name} failed \(code {rc}\)"):
                _lib.query(name, *args)
        assert case != "good" or (rc == 0 and any(want)), (name, rc, want)


def test_query_refuses_other_entry_points_before_the_library(no_library):
    assert {n for n, (_, types) in _lib._SIGS.items() if types and types[-1] is SIZE_P} == set(QUERIES)
    for name in ("lft_forward", "lft_scene_counts", "lft_no_such_entry"):
        with pytest.raises(_lib.LftError, match="no size query"):
            _lib.query(name, 1, 2, 3)


def test_enqueue_serves_the_entry_points_whose_last_parameter_is_the_stream(no_library):
    want = set()
    for header in ("lft_hip.h", "lft_hip_test.h"):
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", header)) as f:
            text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
        want |= {name for name, params in re.findall(r"^(?:int|const char\*)\s+(lft_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M)
                 if re.search(r"\bvoid\s*\*\s*stream\s*$", params)}
    assert _lib.STREAM_LAST == want and want <= set(_lib.EXPORTS) and len(want) >= 35
    assert {"lft_forward", "lft_scene_divide"} <= want and not want & set(NOT_STREAM_LAST)
    for name in NOT_STREAM_LAST + ("lft_status_read", "lft_no_such_entry"):
        with pytest.raises(_lib.LftError, match="does not take its stream last"):
            _lib.enqueue(name, "cuda:0", 1, 2, 3)


def test_arrays():
    t = SimpleNamespace(data_ptr=lambda: 4096, stride=lambda: (60, 12, 3, 1, 0))
    arrays = (_lib.ptr_array([t, t]), _lib.strides_array(t), _lib.strides_array(t.stride()))
    assert [(a._type_, list(a)) for a in arrays] == [(ctypes.c_void_p, [4096, 4096])] + [(ctypes.c_longlong, [60, 12, 3, 1, 0])] * 2
