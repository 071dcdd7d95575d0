"""CPU: what the C ABI answers on the host -- return code and lft_last_error() text of every argument check, in the order the
entry points make them -- is what tests/golden/abi_refusals.json recorded (tools/gen_golden_refusals.py, run before the checks
were last moved).  The calls are those of tests/abi_refusals_util.py; none reaches a device.  Also: the ctypes signatures and
constants of lft_amd._lib are what include/lft_hip.h and include/lft_hip_test.h declare."""
import json
import os

from lft_amd import _lib

import abi_refusals_util as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_refusals.json")


def test_binding_is_read_from_the_headers():
    from ctypes import POINTER, c_char_p, c_float, c_int, c_longlong, c_size_t, c_uint, c_void_p
    S = _lib._SIGS
    assert len(S) == 59 and _lib.EXPORTS == tuple(S) and set(_lib.TEST_EXPORTS) < set(S) and "lft_tail_fwd" in _lib.TEST_EXPORTS
    assert S["lft_last_error"] == (c_char_p, []) and S["lft_version"] == (c_int, [])
    assert S["lft_forward"] == (c_int, [c_void_p] * 4 + [c_int] * 6 + [c_void_p])
    assert S["lft_kernel_time"] == (c_int, [c_char_p, c_void_p, c_void_p] + [c_int] * 7 + [c_void_p, c_void_p])
    assert S["lft_adam_step"] == (c_int, [c_void_p] * 4 + [c_longlong] + [c_float] * 4 + [c_int, c_float, c_float, c_void_p])
    assert S["lft_dihedral_expand"][1][2] is c_uint and S["lft_train_grad_bucket"][1] == [c_int, c_int, POINTER(c_size_t), POINTER(c_size_t)]
    assert S["lft_train_backward_buckets"][1][-2:] == [c_void_p, c_void_p]                       # lft_bucket_fn, user
    assert (_lib.ABI_VERSION, _lib.NUM_PARAMS, _lib.STATUS_NONFINITE, _lib.GUARD_MAX_SEGMENTS, _lib.ERR_SHAPE) == (5, 78, 1001, 128, -2)
    assert _lib.OPTIONAL_EXPORTS >= set(_lib.TEST_EXPORTS + _lib.GUARD_EXPORTS + _lib.DISPARITY_EXPORTS) and "lft_forward" not in _lib.OPTIONAL_EXPORTS
    try:
        _lib._ctype("short", "lft_example")
    except _lib.LftError as e:
        assert "short" in str(e) and "lft_example" in str(e)
    else:
        raise AssertionError("an unknown scalar type must be an error, not a guess")


def test_case_table_covers_what_it_must():
    cases = U.cases()
    by_entry = {}
    for entry, case, _ in cases:
        by_entry.setdefault(entry, set()).add(case)
    assert set(by_entry) <= set(_lib.EXPORTS)
    inference = ["lft_pack_weights", "lft_forward", "lft_kernel_time", "lft_init_features_fwd", "lft_init_features_legacy_fwd", "lft_conv0_fwd",
                 "lft_ang_block_fwd", "lft_spa_block_fwd", "lft_upsample_fwd", "lft_tail_fwd"]
    for e in inference:
        assert {"bad_scale", "bad_prec", "A12"} <= by_entry[e] and any(c.startswith("null_") for c in by_entry[e]), e
    for e in ("lft_ang_block_fwd", "lft_spa_block_fwd"):
        assert {"bad_layer", "null_before_layer", "layer_before_dims"} <= by_entry[e]
    five = {"null_lf", "null_strides", "class_3", "U0", "C2", "stride0_neg", "stride4_neg", "A0", "A_gt_U", "U_minus_A_odd", "V_minus_A_odd", "A256"}
    for e in ("lft_lf_prepare", "lft_lf_luma", "lft_colour_merge"):
        assert five <= by_entry[e], e
    six = {"class_f64", "A0", "A4097", "C5", "taps3", "D0", "B_neg", "empty_B", "null_lf", "null_strides", "null_table", "stride0_neg", "stride5_neg",
           "span_rows", "too_many_blocks"}
    for e in ("lft_refocus", "lft_disparity"):
        assert six <= by_entry[e], e
    assert {f"accepts[{f}]" for f in U.TAPE_FIELDS} <= by_entry["lft_train_tape_offset"] and len(U.TAPE_FIELDS) == 8 + 4 * (8 + 11)
    assert sum(c.startswith("unknown[") for c in by_entry["lft_train_tape_offset"]) >= 3
    assert {"nparams", "param_hole", "bad_scale", "math3"} <= by_entry["lft_train_forward"]
    for e in ("lft_ema_update", "lft_adam_step_guarded"):
        assert "foreign_guard" in by_entry[e]
    for e in ("lft_lf_loss", "lft_ssim_loss"):
        assert {"dsr_is_sr", "dsr_in_hr_tail", "sr_misaligned", "scratch_misaligned"} <= by_entry[e]


def test_every_refusal_is_answered_as_recorded():
    _lib.build()
    with open(GOLDEN) as f:
        want = json.load(f)
    got = U.replay(_lib.lib())
    assert [(r["entry"], r["case"]) for r in got] == [(r["entry"], r["case"]) for r in want]      # the table and the file go together
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(want)} answers differ, the first: got {wrong[0][0]}, recorded {wrong[0][1]}"
    # the two families do differ where they always did: the same odd U - A is an argument error for prepare, a shape error for luma
    rc = {(r["entry"], r["case"]): r["rc"] for r in got}
    assert rc["lft_lf_prepare", "U_minus_A_odd"] == _lib.ERR_ARG and rc["lft_lf_luma", "U_minus_A_odd"] == _lib.ERR_SHAPE
    assert sum(r["rc"] != 0 for r in got) > 600
