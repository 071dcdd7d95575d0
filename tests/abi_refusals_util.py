"""The case table of tests/test_abi_refusals_host.py and tools/gen_golden_refusals.py: calls of the C ABI that are answered on the
host, before any device call -- an argument check refuses them, or they are a size query or an empty piece of work.  Device
pointers are addresses formed as integers and never dereferenced; what the library reads on the host before it decides (stride
arrays, crop origins, the parameter pointer array, segment tables, the 3 x 3 matrix) is real memory."""
import ctypes
from ctypes import byref, c_float, c_int, c_longlong, c_size_t, c_void_p

from lft_amd import _lib

P, Q, R = 1 << 20, 2 << 20, 3 << 20           # three far-apart, 256-byte aligned "device" addresses
NAN, INF = float("nan"), float("inf")


def _vary(entry, good, variations):
    """One case per variation: the good argument set (a dict in parameter order) with the variation's overrides."""
    for case, kw in variations.items():
        unknown = set(kw) - set(good)
        assert not unknown, (entry, case, unknown)
        yield entry, case, tuple({**good, **kw}.values())


def _ll(*v):
    return (c_longlong * len(v))(*v)


def _inference():
    dims = dict(B=1, A=5, h=6, w=6, s=2, prec=_lib.PREC_BF16)
    bad_dims = {"bad_scale": dict(s=3), "bad_prec": dict(prec=7), "A12": dict(A=12), "B0": dict(B=0), "w0": dict(w=0)}
    layer = {"bad_layer": dict(layer=4), "layer_neg": dict(layer=-1), "layer_before_dims": dict(layer=9, s=3, prec=7)}
    params = (c_void_p * 78)(*([P] * 78))
    holed = (c_void_p * 78)(*([P] * 40 + [None] + [P] * 37))
    pack = dict(params=params, nparams=78, packed=Q, A=5, h=6, w=6, s=2, prec=_lib.PREC_BF16, stream=None)
    del bad_dims["B0"]
    yield from _vary("lft_pack_weights", pack, {"null_params": dict(params=None), "null_packed": dict(packed=None), "nparams": dict(nparams=77),
                                                "param_hole": dict(params=holed), "null_before_dims": dict(packed=None, s=3), **bad_dims})
    bad_dims["B0"] = dict(B=0)
    bad_dims["too_many_tokens"] = dict(B=1024, A=11, h=64, w=64)
    bad_dims["prec_before_shape"] = dict(prec=-1, B=0, s=5)
    bad_dims["shape_before_scale"] = dict(h=0, s=5, A=12)
    bad_dims["scale_before_A"] = dict(s=5, A=12)
    fwd = dict(packed=P, lr=Q, out=R, ws=R + 4096, **dims, stream=None)
    nulls4 = {"null_packed": dict(packed=None), "null_lr": dict(lr=None), "null_out": dict(out=None), "null_ws": dict(ws=None),
              "null_before_dims": dict(ws=None, s=3, prec=9)}
    yield from _vary("lft_forward", fwd, {**nulls4, **bad_dims})
    for e in ("lft_init_features_fwd", "lft_init_features_legacy_fwd"):
        yield from _vary(e, fwd, {**nulls4, **bad_dims})
    ms = c_float(0)
    kt = dict(kernel=b"k_ang", packed=P, ws=Q, **dims, reps=3, stream=None, ms_out=byref(ms))
    yield from _vary("lft_kernel_time", kt, {"null_kernel": dict(kernel=None), "null_packed": dict(packed=None), "null_ws": dict(ws=None),
                                               "null_ms": dict(ms_out=None), "reps0": dict(reps=0), "unknown_kernel": dict(kernel=b"k_nothing"),
                                               "null_before_dims": dict(ws=None, s=3), **bad_dims})
    c0 = dict(packed=P, lr=Q, x0=R, recomputed=0, **dims, stream=None)
    yield from _vary("lft_conv0_fwd", c0, {"null_packed": dict(packed=None), "null_lr": dict(lr=None), "null_x0": dict(x0=None),
                                             "recomputed_f32": dict(recomputed=1, prec=_lib.PREC_F32), "dims_before_recomputed": dict(recomputed=1, prec=_lib.PREC_F32, s=3),
                                             "null_before_dims": dict(x0=None, A=12), **bad_dims})
    ang = dict(packed=P, layer=1, act_in=Q, act_out=R, **dims, stream=None)
    yield from _vary("lft_ang_block_fwd", ang, {"null_packed": dict(packed=None), "null_in": dict(act_in=None), "null_out": dict(act_out=None),
                                                  "null_before_layer": dict(act_out=None, layer=7), **layer, **bad_dims})
    spa = dict(packed=P, layer=1, act_in=Q, skip=None, act_out=R, ws=R + 4096, **dims, stream=None)
    yield from _vary("lft_spa_block_fwd", spa, {"null_packed": dict(packed=None), "null_in": dict(act_in=None), "null_out": dict(act_out=None),
                                                  "null_ws": dict(ws=None), "null_before_layer": dict(ws=None, layer=7), **layer, **bad_dims})
    up = dict(packed=P, act_in=Q, lr=R, out=R + 4096, ws=R + 8192, **dims, stream=None)
    yield from _vary("lft_upsample_fwd", up, {"null_packed": dict(packed=None), "null_in": dict(act_in=None), "null_lr": dict(lr=None),
                                                "null_out": dict(out=None), "null_ws": dict(ws=None), "null_before_dims": dict(ws=None, s=3), **bad_dims})
    tail = dict(packed=P, act_in=Q, skip=R, lr=R + 4096, out=R + 8192, ws=R + 12288, **dims, handoff=0, stream=None)
    yield from _vary("lft_tail_fwd", tail, {"null_packed": dict(packed=None), "null_in": dict(act_in=None), "null_skip": dict(skip=None), "null_lr": dict(lr=None),
                                              "null_out": dict(out=None), "null_ws": dict(ws=None), "null_before_dims": dict(skip=None, prec=5),
                                              "no_lane_major_bf16": dict(handoff=1), "no_lane_major_f16": dict(handoff=1, prec=_lib.PREC_F16),
                                              "no_lane_major_f32": dict(handoff=1, prec=_lib.PREC_F32, h=5, w=5),
                                              "no_lane_major_16x24": dict(handoff=1, h=16, w=24), **bad_dims})
    n = c_size_t(0)
    yield from _vary("lft_packed_bytes", dict(A=5, h=6, w=6, s=2, prec=0, out=byref(n)), {"null_out": dict(out=None), "null_before_dims": dict(out=None, s=3),
                                                                                          "bad_scale": dict(s=3), "bad_prec": dict(prec=3), "A12": dict(A=12)})
    yield from _vary("lft_workspace_bytes", dict(B=1, A=5, h=6, w=6, s=2, prec=0, out=byref(n)), {"null_out": dict(out=None), "B0": dict(B=0), "bad_scale": dict(s=3),
                                                                                                   "bad_prec": dict(prec=3), "A12": dict(A=12)})
    yield from _vary("lft_status_reset", dict(ws=P, **dims, stream=None), {"null_ws": dict(ws=None), **bad_dims})
    yield from _vary("lft_status_read", dict(ws=P, **dims, stream=None, flags=None), {"null_ws": dict(ws=None), **bad_dims})
    yield from _vary("lft_bicubic_fwd", dict(lr=P, out=Q, B=1, A=5, h=6, w=6, s=2, stream=None), {"null_lr": dict(lr=None), "null_out": dict(out=None),
                                                                                                   "bad_scale": dict(s=3), "A12": dict(A=12), "B0": dict(B=0)})
    yield from _vary("lft_mfma_selftest", dict(Am=P, Bm=P, W2=P, C=Q, D=R, prec=0, stream=None), {"null_Am": dict(Am=None), "null_D": dict(D=None),
                                                                                                   "bad_prec": dict(prec=3), "prec_neg": dict(prec=-1), "null_before_prec": dict(C=None, prec=3)})


def _five_strides():
    """lft_lf_prepare, lft_lf_luma, lft_colour_merge: the light field [U,V,H,W,C] with five strides."""
    st = _ll(9 * 20 * 20 * 3, 20 * 20 * 3, 20 * 3, 3, 1)
    lf = dict(lf=P, lf_class=_lib.LF_UINT8, U=9, V=9, H=20, W=20, C=3, strides=st, A=5)
    family = {"null_lf": dict(lf=None), "null_strides": dict(strides=None), "class_3": dict(lf_class=3), "class_neg": dict(lf_class=-1), "U0": dict(U=0),
              "V0": dict(V=0), "H0": dict(H=0), "W_neg": dict(W=-2), "C2": dict(C=2), "stride0_neg": dict(strides=_ll(-1, 1, 1, 1, 1)),
              "stride4_neg": dict(strides=_ll(1, 1, 1, 1, -7)), "A0": dict(A=0), "A_gt_U": dict(A=7, U=5), "A_gt_V": dict(A=7, V=5),
              "U_minus_A_odd": dict(U=8), "V_minus_A_odd": dict(V=6), "A256": dict(A=256, U=256, V=256), "A257": dict(A=257, U=257, V=257),
              "null_before_class": dict(lf=None, lf_class=9), "class_before_sizes": dict(lf_class=9, U=0), "sizes_before_strides": dict(C=1, strides=_ll(-1, 1, 1, 1, 1)),
              "strides_before_A": dict(strides=_ll(1, 1, -1, 1, 1), A=0), "A_before_parity": dict(A=11, U=10)}
    crops = (c_int * 4)(0, 0, 4, 4)
    outside = (c_int * 4)(0, 0, 13, 4)
    prep = dict(**lf, s=2, crops=crops, n_crops=0, crop_h=8, crop_w=8, wh=Q, ih=Q, th=4, ww=Q, iw=Q, tw=4, hr=R, lr=R + 4096, stream=None)
    # n_crops = 0: a call that passes every check launches nothing and returns 0 (A256, A257: lft_lf_prepare has no grid limit on A)
    yield from _vary("lft_lf_prepare", prep, {**family, "null_crops": dict(crops=None), "null_wh": dict(wh=None), "null_iw": dict(iw=None), "null_hr": dict(hr=None),
                                               "null_lr": dict(lr=None), "own_null_before_class": dict(hr=None, lf_class=9), "scale3": dict(s=3),
                                               "strides_before_scale": dict(s=3, strides=_ll(1, -1, 1, 1, 1)), "scale_before_A": dict(s=3, A=0),
                                               "n_crops_neg": dict(n_crops=-1), "crop_h0": dict(crop_h=0), "crop_w_gt_W": dict(crop_w=21),
                                               "crop_outside": dict(crops=outside, n_crops=2), "crop_neg": dict(crops=(c_int * 2)(-1, 0), n_crops=1),
                                               "taps_h0": dict(th=0), "taps_w19": dict(tw=19), "parity_before_crops": dict(U=8, crop_h=0),
                                               "no_crops": {}})
    luma = dict(**lf, y_out=Q, stream=None)
    yield from _vary("lft_lf_luma", luma, {**family, "null_y": dict(y_out=None), "own_null_before_class": dict(y_out=None, lf_class=9),
                                            "too_many_blocks": dict(H=1 << 20, W=1 << 20), "A256_before_blocks": dict(A=256, U=256, V=256, H=1 << 20, W=1 << 20)})
    minv = (ctypes.c_double * 9)(*range(9))
    merge = dict(**lf, s=2, sr_y=None, wh=Q, ih=Q, th=4, ww=Q, iw=Q, tw=4, minv=minv, out=R, out_class=_lib.LF_UINT8, stream=None)
    yield from _vary("lft_colour_merge", merge, {**family, "null_wh": dict(wh=None), "null_iw": dict(iw=None), "null_minv": dict(minv=None), "null_out": dict(out=None),
                                                  "own_null_before_class": dict(out=None, lf_class=9), "scale3": dict(s=3), "family_before_scale": dict(s=3, U=8),
                                                  "taps_h0": dict(th=0), "taps_w7": dict(tw=7), "scale_before_taps": dict(s=8, th=0),
                                                  "out_class_f64": dict(out_class=_lib.LF_FLOAT64), "out_class_neg": dict(out_class=-1),
                                                  "taps_before_out_class": dict(tw=0, out_class=5), "too_tall": dict(s=4, H=1 << 30), "too_wide": dict(s=4, W=1 << 30),
                                                  "too_many_tiles": dict(H=1 << 24, W=1 << 24), "out_class_before_tiles": dict(out_class=5, H=1 << 30, s=4)})


def _six_strides():
    """lft_refocus, lft_disparity: B windowed light fields [B,A,A,H,W,C] with six strides."""
    st = _ll(0, 500, 100, 10, 1, 0)
    neg = [_ll(*[(-3 if j == i else v) for j, v in enumerate((0, 500, 100, 10, 1, 0))]) for i in range(6)]
    lf = dict(lf=P, lf_class=_lib.LF_UINT8, B=1, A=5, H=10, W=10, C=1, strides=st, table=Q)
    family = {"class_f64": dict(lf_class=_lib.LF_FLOAT64), "class_7": dict(lf_class=7), "class_neg": dict(lf_class=-1), "A0": dict(A=0), "A4097": dict(A=4097),
              "C0": dict(C=0), "C5": dict(C=5), "taps0": dict(taps=0), "taps3": dict(taps=3), "taps8": dict(taps=8), "D0": dict(D=0), "D_neg": dict(D=-2),
              "B_neg": dict(B=-1), "H_neg": dict(H=-1), "W_neg": dict(W=-4), "empty_B": dict(B=0, lf=None), "empty_H": dict(H=0, strides=None),
              "empty_W": dict(W=0, table=None), "null_lf": dict(lf=None), "null_strides": dict(strides=None), "null_table": dict(table=None),
              **{f"stride{i}_neg": dict(strides=neg[i]) for i in range(6)},
              "span_rows": dict(strides=_ll(0, 0, 0, 1 << 28, 1, 0)), "span_cols": dict(strides=_ll(0, 0, 0, 1, 1 << 28, 0)),
              "span_channels": dict(C=4, strides=_ll(0, 0, 0, 1, 1, 1 << 30)),
              "too_many_blocks": dict(B=1 << 20, H=1 << 20, W=1 << 20), "too_many_blocks_D": dict(D=1 << 12, H=1 << 15, W=1 << 15),
              "class_before_A": dict(lf_class=9, A=0), "A_before_C": dict(A=0, C=9), "C_before_taps": dict(C=9, taps=3), "taps_before_D": dict(taps=3, D=0),
              "D_before_sizes": dict(D=0, B=-1), "negative_before_empty": dict(B=-1, H=0), "empty_before_null": dict(W=0, lf=None, strides=None),
              "null_before_strides": dict(table=None, strides=neg[2]), "strides_before_span": dict(strides=_ll(0, 0, -1, 1 << 28, 1, 0)),
              "span_before_blocks": dict(B=1 << 20, H=1 << 20, W=1 << 20, strides=_ll(0, 0, 0, 1 << 28, 1, 0))}
    ref = dict(**lf, D=3, taps=4, out=R, out_class=_lib.LF_FLOAT32, stream=None)
    yield from _vary("lft_refocus", ref, {**family, "out_class_f64": dict(out_class=_lib.LF_FLOAT64), "out_class_9": dict(out_class=9), "null_out": dict(out=None),
                                           "class_before_out_class": dict(lf_class=9, out_class=9), "out_class_before_A": dict(out_class=9, A=0)})
    dsp = dict(**lf, slopes=Q + 4096, D=3, taps=4, radius=2, scratch=R, disparity=R + 4096, confidence=R + 8192, index=R + 12288, cost=None, aif=None,
               aif_class=_lib.LF_FLOAT32, stream=None)
    yield from _vary("lft_disparity", dsp, {**family, "aif_class_f64": dict(aif_class=_lib.LF_FLOAT64), "aif_class_9": dict(aif_class=9),
                                             "class_before_aif_class": dict(lf_class=9, aif_class=9), "aif_class_before_A": dict(aif_class=9, A=0),
                                             "radius_neg": dict(radius=-1), "radius9": dict(radius=9), "D_before_radius": dict(D=0, radius=9),
                                             "radius_before_sizes": dict(radius=9, B=-1), "null_slopes": dict(slopes=None), "null_scratch": dict(scratch=None),
                                             "null_disparity": dict(disparity=None), "null_confidence": dict(confidence=None), "null_index": dict(index=None),
                                             "too_many_pick_blocks": dict(B=1 << 10, D=1, H=1 << 15, W=1 << 15, strides=_ll(0, 0, 0, 1 << 15, 1, 0)),
                                             "volume": dict(D=384, H=1 << 15, W=1 << 15, strides=_ll(0, 0, 0, 1 << 15, 1, 0)),
                                             "volume_aif": dict(D=96, C=4, aif=Q, H=1 << 15, W=1 << 15, strides=_ll(0, 0, 0, 1 << 15, 1, 0)),
                                             "scratch_misaligned": dict(scratch=R + 2), "volume_before_alignment": dict(D=384, H=1 << 15, W=1 << 15, scratch=R + 2,
                                                                                                                        strides=_ll(0, 0, 0, 1 << 15, 1, 0))})
    n = c_size_t(0)
    yield from _vary("lft_disparity_scratch_bytes", dict(B=1, D=3, H=10, W=10, C=1, flags=0, out=byref(n)),
                     {"null_out": dict(out=None), "C0": dict(C=0), "C5": dict(C=5), "D0": dict(D=0), "flags2": dict(flags=2), "B_neg": dict(B=-1),
                      "volume": dict(D=384, H=1 << 15, W=1 << 15), "volume_aif": dict(D=96, C=4, flags=1, H=1 << 15, W=1 << 15), "empty": dict(B=0, D=1 << 30, H=1 << 30)})


TAPE_FIELDS = (["x0", "feat", "c1", "c2", "c3", "body", "act", "skip"]
               + [f"ang{l}.{f}" for l in range(4) for f in ("n", "qk", "v", "o", "t1", "m", "hdn", "y")]
               + [f"spa{l}.{f}" for l in range(4) for f in ("tok", "n", "qk", "v", "o", "t1", "m", "hdn", "t2", "y", "petok")])
TAPE_UNKNOWN = ["bogus", "ang4.n", "spa0.zz", "ang0.tok", "spa2.", "ang1", "wp", "x0 ", "", "ang-.n", "spa1.petok2", "Ang0.n"]


def _training():
    params = (c_void_p * 78)(*([P] * 78))
    holed = (c_void_p * 78)(*([None] + [P] * 77))
    dims = dict(B=1, A=2, h=4, w=4, s=2)
    tf = dict(params=params, nparams=78, lr=P, out=Q, tape=R, **dims, math=_lib.MATH_F32, stream=None)
    yield from _vary("lft_train_forward", tf, {"null_params": dict(params=None), "null_lr": dict(lr=None), "null_out": dict(out=None), "null_tape": dict(tape=None),
                                                "nparams": dict(nparams=79), "param_hole": dict(params=holed), "bad_scale": dict(s=3), "A12": dict(A=12), "B0": dict(B=0),
                                                "math3": dict(math=3), "math_neg": dict(math=-1), "null_before_nparams": dict(tape=None, nparams=1),
                                                "nparams_before_dims": dict(nparams=1, s=3), "dims_before_math": dict(s=3, math=9)})
    tb = dict(params=params, nparams=78, lr=P, tape=R, dout=Q, grads=Q + 4096, **dims, math=_lib.MATH_F32, stream=None)
    yield from _vary("lft_train_backward", tb, {"null_dout": dict(dout=None), "null_grads": dict(grads=None), "math3": dict(math=3), "nparams": dict(nparams=0)})
    blk = dict(params=params, nparams=78, lr=P, tape=R, block=_lib.BLOCK_SPA, layer=1, d_out=Q, d_in=Q + 4096, grads=Q + 8192, **dims, math=0, stream=None)
    yield from _vary("lft_train_block_backward", blk, {"null_d_out": dict(d_out=None), "block4": dict(block=4), "block_neg": dict(block=-1), "layer4": dict(layer=4),
                                                        "layer_ignored_for_init_then_math": dict(block=_lib.BLOCK_INIT, layer=9, math=7),
                                                        "null_d_in": dict(d_in=None), "null_d_in_init_then_math": dict(block=_lib.BLOCK_INIT, d_in=None, math=7),
                                                        "block_before_layer": dict(block=9, layer=9), "layer_before_train_args": dict(layer=9, nparams=1)})
    n = c_size_t(0)
    off = dict(name=b"x0", **dims, out=byref(n))
    yield from _vary("lft_train_tape_offset", off, {"null_name": dict(name=None), "null_out": dict(out=None), "bad_scale": dict(s=3), "dims_before_name": dict(name=b"bogus", s=3),
                                                     **{f"accepts[{f}]": dict(name=f.encode()) for f in TAPE_FIELDS},
                                                     **{f"unknown[{f}]": dict(name=f.encode()) for f in TAPE_UNKNOWN}})
    yield from _vary("lft_train_tape_bytes", dict(**dims, out=byref(n)), {"null_out": dict(out=None), "bad_scale": dict(s=3), "A12": dict(A=12)})
    yield from _vary("lft_train_grad_floats", dict(s=2, out=byref(n)), {"null_out": dict(out=None), "bad_scale": dict(s=3)})
    yield from _vary("lft_train_grad_bucket", dict(s=2, bucket=0, first=byref(n), count=byref(n)), {"null_first": dict(first=None), "bad_scale": dict(s=8),
                                                                                                     "bucket3": dict(bucket=3), "bucket_neg": dict(bucket=-1)})
    yield from _vary("lft_lr_grad_bwd", dict(w0=P, dx0=Q, dout=None, d_lr=R, **dims, stream=None), {"null_w0": dict(w0=None), "null_d_lr": dict(d_lr=None), "bad_scale": dict(s=3)})
    yield from _vary("lft_attn_maps_floats", dict(block=_lib.BLOCK_ANG, heads=_lib.MAPS_MEAN, B=1, A=2, h=4, w=4, out=byref(n)),
                     {"null_out": dict(out=None), "block_init": dict(block=_lib.BLOCK_INIT), "heads2": dict(heads=2), "A12": dict(A=12)})
    yield from _vary("lft_train_attn_maps", dict(tape=P, block=_lib.BLOCK_SPA, layer=0, heads=_lib.MAPS_HEADS, maps=Q, **dims, stream=None),
                     {"null_tape": dict(tape=None), "null_maps": dict(maps=None), "block_up": dict(block=_lib.BLOCK_UPSAMPLE), "heads_neg": dict(heads=-1),
                      "layer4": dict(layer=4), "bad_scale": dict(s=3), "block_before_layer": dict(block=0, layer=4)})
    yield from _vary("lft_prod_selftest", dict(W=P, X=P, Y=Q, Yl=Q, Yr=Q, math=0, stream=None), {"null_W": dict(W=None), "math3": dict(math=3)})


def _losses_and_optimizer():
    n = c_size_t(0)
    N = 2 * 2 * 16 * 16 * 4                                                    # bytes of one [B=1, 1, A*H, A*W] fp32 image below
    lf = dict(sr=P, hr=Q, B=1, A=2, H=16, W=16, penalty=_lib.LOSS_L1, eps=1e-3, w_pix=1.0, w_epi=0.5, dsr=R, gscale=1.0, loss3=R + 8192, scratch=R + 16384,
              stream=None)
    overlap = {"dsr_is_sr": dict(dsr=P), "dsr_is_hr": dict(dsr=Q), "dsr_in_sr_tail": dict(dsr=P + N - 4), "dsr_before_sr_head": dict(dsr=P - N + 4),
               "dsr_in_hr_tail": dict(dsr=Q + N - 4), "dsr_before_hr_head": dict(dsr=Q - N + 4)}
    yield from _vary("lft_lf_loss", lf, {"null_sr": dict(sr=None), "null_hr": dict(hr=None), "null_loss3": dict(loss3=None), "null_scratch": dict(scratch=None),
                                          "sr_misaligned": dict(sr=P + 2), "hr_misaligned": dict(hr=Q + 1), "dsr_misaligned": dict(dsr=R + 3), "loss3_misaligned": dict(loss3=R + 8194),
                                          "scratch_misaligned": dict(scratch=R + 16388), "penalty3": dict(penalty=3), "penalty_neg": dict(penalty=-1),
                                          "charbonnier_eps0": dict(penalty=_lib.LOSS_CHARBONNIER, eps=0.0), "charbonnier_eps_nan": dict(penalty=_lib.LOSS_CHARBONNIER, eps=NAN),
                                          "w_pix_neg": dict(w_pix=-1.0), "w_epi_nan": dict(w_epi=NAN), "weights_zero": dict(w_pix=0.0, w_epi=0.0), "gscale_nan": dict(gscale=NAN),
                                          "B0": dict(B=0), "H0": dict(H=0), "A12": dict(A=12), "alignment_before_penalty": dict(sr=P + 2, penalty=9),
                                          "shape_before_overlap": dict(dsr=P, W=0), **overlap})
    yield from _vary("lft_lf_loss_scratch_bytes", dict(B=1, A=2, H=16, W=16, out=byref(n)), {"null_out": dict(out=None), "B0": dict(B=0), "A12": dict(A=12)})
    ss = dict(sr=P, hr=Q, B=1, A=2, H=16, W=16, ssim_range=1.0, w_ssim=0.1, dsr=R, gscale=1.0, accumulate=0, total=R + 8192, ssim_out=R + 8196, scratch=R + 16384,
              stream=None)
    yield from _vary("lft_ssim_loss", ss, {"null_sr": dict(sr=None), "null_hr": dict(hr=None), "null_total": dict(total=None), "null_ssim_out": dict(ssim_out=None),
                                            "null_scratch": dict(scratch=None), "sr_misaligned": dict(sr=P + 2), "dsr_misaligned": dict(dsr=R + 1), "total_misaligned": dict(total=R + 8193),
                                            "ssim_out_misaligned": dict(ssim_out=R + 8198), "scratch_misaligned": dict(scratch=R + 16388), "range0": dict(ssim_range=0.0),
                                            "range_inf": dict(ssim_range=INF), "w_ssim0": dict(w_ssim=0.0), "w_ssim_nan": dict(w_ssim=NAN), "gscale_nan": dict(gscale=NAN),
                                            "accumulate2": dict(accumulate=2), "B0": dict(B=0), "H10": dict(H=10), "W10": dict(W=10),
                                            "too_many_tiles": dict(B=1 << 20, A=11, H=1 << 10, W=1 << 10), "shape_before_overlap": dict(dsr=P, W=10), **overlap})
    yield from _vary("lft_ssim_loss_scratch_bytes", dict(B=1, A=2, H=16, W=16, out=byref(n)), {"null_out": dict(out=None), "H10": dict(H=10), "A0": dict(A=0)})
    yield from _vary("lft_l1_loss", dict(sr=P, hr=Q, n=64, dsr=None, gscale=1.0, loss=R, scratch=R + 4096, stream=None),
                     {"null_sr": dict(sr=None), "null_loss": dict(loss=None), "n0": dict(n=0)})
    yield from _vary("lft_adam_step", dict(p=P, g=Q, m=R, v=R + 4096, n=64, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, step=1, gscale=1.0, wd=0.0, stream=None),
                     {"null_p": dict(p=None), "n0": dict(n=0), "step0": dict(step=0), "wd_neg": dict(wd=-0.1)})
    yield from _vary("lft_guard_bytes", dict(nseg=3, out=byref(n)), {"null_out": dict(out=None), "nseg0": dict(nseg=0), "nseg129": dict(nseg=129)})
    S = _lib.GuardSegment
    segs = (S * 2)(S(0, 40, 1), S(40, 24, 0))
    gi = dict(guard=P, segs=segs, nseg=2, n=64, steps0=0, stream=None)
    yield from _vary("lft_guard_init", gi, {"null_guard": dict(guard=None), "null_segs": dict(segs=None), "guard_misaligned": dict(guard=P + 8), "nseg0": dict(nseg=0),
                                             "nseg129": dict(nseg=129), "n0": dict(n=0), "steps_neg": dict(steps0=-1), "gap": dict(segs=(S * 2)(S(0, 40, 1), S(41, 23, 1))),
                                             "count0": dict(segs=(S * 2)(S(0, 0, 1), S(0, 64, 1))), "past_n": dict(segs=(S * 2)(S(0, 40, 1), S(40, 25, 1))),
                                             "short": dict(segs=(S * 2)(S(0, 40, 1), S(40, 23, 1))), "alignment_before_nseg": dict(guard=P + 8, nseg=0)})
    # no guard block has been initialised in this process, so every address is a foreign block
    ag = dict(p=P, g=Q, m=R, v=R + 4096, n=64, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, gscale=1.0, wd=0.0, max_norm=1.0, guard=R + 8192, stream=None)
    yield from _vary("lft_adam_step_guarded", ag, {"null_p": dict(p=None), "null_guard": dict(guard=None), "g_misaligned": dict(g=Q + 2), "wd_neg": dict(wd=-1.0),
                                                    "max_norm_nan": dict(max_norm=NAN), "foreign_guard": {}, "foreign_guard_other_n": dict(n=7),
                                                    "nan_before_guard": dict(max_norm=NAN, guard=R)})
    report = _lib.GuardReport()
    yield from _vary("lft_guard_read", dict(guard=P, stream=None, host=byref(report)), {"null_guard": dict(guard=None), "null_host": dict(host=None), "foreign_guard": {}})
    em = dict(ema=P, p=Q, n=64, decay=0.999, warmup=1, step=1, guard=None, stream=None)
    yield from _vary("lft_ema_update", em, {"null_ema": dict(ema=None), "null_p": dict(p=None), "ema_misaligned": dict(ema=P + 2), "n0": dict(n=0), "overlap": dict(ema=Q + 252),
                                             "overlap_same": dict(ema=Q), "decay1": dict(decay=1.0), "decay_neg": dict(decay=-0.5), "decay_nan": dict(decay=NAN),
                                             "step0_plain": dict(step=0), "foreign_guard": dict(guard=R), "foreign_guard_step0": dict(guard=R, step=0),
                                             "decay_before_guard": dict(decay=2.0, guard=R)})


def _tiling_and_transforms():
    nu, nv = c_int(0), c_int(0)
    yield from _vary("lft_scene_counts", dict(h0=100, w0=100, patch=32, stride=16, nu=byref(nu), nv=byref(nv)),
                     {"null_nu": dict(nu=None), "stride0": dict(stride=0), "stride_gt_patch": dict(stride=33), "h0_neg": dict(h0=-1), "smaller_than_patch": dict(h0=8, stride=32)})
    yield from _vary("lft_scene_divide", dict(scene=P, patches=Q, A=5, h0=100, w0=100, patch=32, stride=16, stream=None),
                     {"null_scene": dict(scene=None), "A0": dict(A=0), "stride0": dict(stride=0)})
    yield from _vary("lft_scene_integrate", dict(sr=P, scene=Q, A=5, h0=100, w0=100, patch=32, stride=16, s=2, stream=None),
                     {"null_scene": dict(scene=None), "s0": dict(s=0), "patch0": dict(patch=0)})
    dh = dict(src=P, dst=Q, mask=0xFF, B=2, H=8, W=12, stream=None)
    bad = {"null_in": dict(src=None), "null_out": dict(dst=None), "in_place": dict(dst=P), "B0": dict(B=0), "W_neg": dict(W=-1), "too_many_blocks": dict(B=1 << 20, H=1 << 12, W=1 << 12)}
    masks = {"mask0": dict(mask=0), "mask_0x100": dict(mask=0x100), "in_place_before_mask": dict(dst=P, mask=0), "mask_before_sizes": dict(mask=0, B=0)}
    yield from _vary("lft_dihedral_expand", dh, {**bad, **masks})
    yield from _vary("lft_dihedral_merge", dh, {**bad, **masks})
    yield from _vary("lft_dihedral_batch", dict(src=P, dst=Q, codes=R, B=2, H=8, W=12, stream=None), {**bad, "null_codes": dict(codes=None), "codes_before_in": dict(codes=None, src=None)})
    yield from _vary("lft_scene_integrate_ens", dict(sr=P, scene=Q, mask=0x0F, A=5, h0=100, w0=100, patch=32, stride=16, s=2, stream=None),
                     {"null_sr": dict(sr=None), "in_place": dict(scene=P), "mask0": dict(mask=0), "A0": dict(A=0), "s0": dict(s=0), "stride0": dict(stride=0),
                      "too_many_blocks": dict(A=11, h0=1 << 20, w0=1 << 20, patch=32, stride=32, s=1)})
    n = c_size_t(0)
    yield from _vary("lft_view_metrics_scratch_bytes", dict(B=1, A=2, h=16, w=16, out=byref(n)), {"null_out": dict(out=None), "B0": dict(B=0)})
    yield from _vary("lft_view_metrics", dict(label=P, out=Q, B=1, A=2, h=16, w=16, ssim_range=2.0, psnr=R, ssim=R + 64, scratch=R + 4096, stream=None),
                     {"null_label": dict(label=None), "null_scratch": dict(scratch=None), "A0": dict(A=0), "h10": dict(h=10), "w10": dict(w=10)})


def cases():
    """[(entry point, case name, arguments)]; the names are unique per entry point."""
    out = [c for group in (_inference, _five_strides, _six_strides, _training, _losses_and_optimizer, _tiling_and_transforms) for c in group()]
    assert len({(e, c) for e, c, _ in out}) == len(out)
    return out


def replay(L):
    """Run every case on the loaded library L (lft_amd._lib.lib()): [{"entry", "case", "rc", "text"}].  text is lft_last_error()
    after a refusal -- up to the address where the message prints one, which is not the library's to choose --, the value of the
    size_t output after a successful query, and empty after any other call that returned 0."""
    records = []
    for entry, case, args in cases():
        L.lft_scene_counts(1, 1, 1, 1, None, None)                             # leaves another call's message behind
        out = [a._obj for a in args if hasattr(a, "_obj") and isinstance(a._obj, c_size_t)]
        for o in out:
            o.value = 0
        rc = getattr(L, entry)(*args)
        text = L.lft_last_error().decode().split(" 0x")[0] if rc else " ".join(str(o.value) for o in out)
        records.append({"entry": entry, "case": case, "rc": rc, "text": text})
    return records
