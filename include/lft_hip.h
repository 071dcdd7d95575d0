/* lft_hip.h -- C ABI of liblft_hip.so: the LFT forward hot path on MI355X (gfx950).
 *
 * This library replaces, for CUDA/HIP tensors, the arithmetic of the reference's
 *   model/LFT.py:52-83   get_model.forward  (and everything it calls: :86-115, :118-191, :194-238, :255-266)
 * behind the reference's own plugin surface (model.LFT.get_model(args).forward(lr)); the Python module
 * lft_amd/module.py binds these entry points with ctypes.  INTEGRATION.md shows the binding a
 * reference maintainer would add.
 *
 * Conventions
 *  - extern "C", plain pointers and ints; no torch types.  All pointers are DEVICE pointers unless noted.
 *  - The library never allocates, frees or retains device memory: the caller owns every buffer
 *    (packed weights, workspace, inputs, outputs) and sizes them with the *_bytes() queries.
 *  - Every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns without
 *    synchronising; calls are graph-capturable.
 *  - Return value: 0 ok; <0 argument error (LFT_ERR_*); >0 a hipError_t.  lft_last_error() gives a
 *    thread-local message.  Nothing is thrown across the boundary.
 *  - prec selects the MFMA operand type: LFT_PREC_F32 = exact fp32 (v_mfma_f32_32x32x2_f32),
 *    LFT_PREC_BF16 = bf16 operands / fp32 accumulate (v_mfma_f32_32x32x16_bf16), LFT_PREC_F16 = IEEE half operands /
 *    fp32 accumulate (v_mfma_f32_32x32x16_f16: same kernels, layouts and speed as bf16, 11 significant bits instead
 *    of 8, but a range of 65504 -- activations beyond it become inf; every such event reaches a LayerNorm or the output as
 *    inf / NaN, where the kernels set a sticky flag in the workspace that lft_status_read reports: an overflow is a loud error,
 *    not a silently wrong image).
 *    Activations between kernels are stored in the same type (float, __bf16 or _Float16, channels-last [B, A*A, h, w, C]).
 *  - Shapes: A = angRes (A*A <= 128 views, i.e. A = 1 .. 11: every A is tested against the oracle, 2, 3, 5 and 9 at BASELINE's
 *    view sizes, the others at small views -- tests/test_gpu_parity.py), h x w = LR view size, s = scale factor (2 or 4),
 *    channels fixed to 64 (reference option.py --channels default, LFT.py:11).
 *    View sizes: any h, w >= 1 up to the width limit -- w <= 75 in LFT_PREC_F32, w <= 347 in LFT_PREC_BF16 / LFT_PREC_F16 (the
 *    convolutions keep two image rows of a view in the 160 KiB of LDS); a wider view is refused with LFT_ERR_SHAPE before anything
 *    is launched.  Tested against the oracle, one view size per class of the kernels' tiling (the table above launch_spa1 in
 *    lft_amd/csrc/lft_network.hip): views below 128 pixels, 32- and 64-wide views with h*w % 128 == 0, ragged sizes (13x11, 17x19,
 *    35x37, 31x32), sizes that are lane-major in fp32 only (16x24, 24x16), 62x64, both sides of the k_spa1 chunk switch (53x55 |
 *    54x56 in 16 bit, 57x59 | 58x60 in fp32), and the widest views (3x75, 3x347; init_features only).
 *    Training (lft_train_*): the GEMM and weight-gradient kernels are chosen by the token count N = B*A*A*h*w and the view width;
 *    gradients are compared with float64 autograd over the oracle in every class of that dispatch (tests/train_classes.py,
 *    tests/test_gpu_train_classes.py), block by block in the three math modes: 4 096 tokens of 32-wide views (A2 2x B1 32x32),
 *    40 000 (A5 2x B16 10x10), 65 536 = the last size before the ring-fed GEMM (A8 4x B16 8x8), 72 600 (A11 2x B6 10x10; also the
 *    whole network, all 78 gradients), 76 800 = three 5x5 patches of 32x32 (A5 2x B3 32x32) and 69 192 at 4x (A6 4x B2 31x31:
 *    up-sampler and feature extractor); besides the small shapes and fixtures (<= 12 800 tokens) of tests/test_gpu_train.py.
 */
#ifndef LFT_HIP_H
#define LFT_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LFT_ABI_VERSION 5
#define LFT_PREC_F32 0
#define LFT_PREC_BF16 1
#define LFT_PREC_F16 2
#define LFT_NUM_PARAMS 78
/* GEMM arithmetic of the training step: exact fp32 MFMA, or fp32 operands split into bf16 hi + lo with three bf16
 * MFMAs per product (~2^-16 relative per product, 5x the matrix-pipe rate).  Forward and backward of one step must
 * use the same mode (the packed weights in the tape are in the mode's format). */
#define LFT_MATH_F32 0
#define LFT_MATH_BF16X3 1
#define LFT_MATH_BF16X6 2   /* fp32 operands as THREE bf16 numbers (x = a + b + c exactly), six bf16 MFMAs per product (the three smallest of the
                             * nine terms dropped: <= 2^-23 relative, fp32-class) at 6/16 of the fp32-MFMA cost; every GEMM of the step */

#define LFT_ERR_ARG (-1)         /* null pointer / bad enum */
#define LFT_ERR_SHAPE (-2)       /* shape outside what this build supports */
#define LFT_ERR_UNSUPPORTED (-3) /* valid for the reference, not implemented here yet */
#define LFT_ERR_CALLBACK (-4)    /* a caller-supplied callback asked to stop (lft_train_backward_buckets) */
/* Returned by lft_status_read (never by the enqueue-only calls): a non-finite activation or output value was seen since the last
 * lft_status_reset -- on the LFT_PREC_F16 path that is what a range overflow (|x| > 65504) turns into. */
#define LFT_STATUS_NONFINITE 1001

int lft_version(void);
const char* lft_last_error(void);

/* Size of the packed-weight buffer for a model with (A, h, w, s) and of the per-forward workspace. */
int lft_packed_bytes(int A, int h, int w, int s, int prec, size_t* out_bytes);
int lft_workspace_bytes(int B, int A, int h, int w, int s, int prec, size_t* out_bytes);

/* Re-arrange the reference's 78 fp32 parameter tensors (device pointers, in state_dict order -- the
 * order of lft_amd/params.py:param_table, which is the reference's registration order, LFT.py:23-44,
 * :125-145, :199-214) into MFMA-fragment streams, and precompute the input-independent tables
 * (angular / spatial sinusoids LFT.py:86-115, and the embedded spatial position tokens LFT.py:180).
 * `params` is a HOST array of 78 device pointers.  Must be re-run whenever a weight, h or w changes. */
int lft_pack_weights(const float* const* params, int nparams, void* packed,
                     int A, int h, int w, int s, int prec, void* stream);

/* get_model.forward (reference LFT.py:52-83).  lr: fp32 [B,1,A*h,A*w]; out: fp32 [B,1,A*h*s,A*w*s]. */
int lft_forward(const void* packed, const float* lr, float* out, void* workspace,
                int B, int A, int h, int w, int s, int prec, void* stream);

/* Sticky status word of a workspace (its last 256 bytes).  The kernels of lft_forward / the per-stage entry points that take a
 * workspace set bit 0 when a token's LayerNorm variance or an output pixel is not finite (inf / NaN): an fp16 range overflow
 * anywhere in the network, or non-finite input data.  Nothing clears it but lft_status_reset, so one read covers every
 * forward since the last reset -- also graph replays, which the host never sees individually.
 *   lft_status_reset: enqueue the clearing of the word on `stream` (call once after allocating a workspace, and after a read
 *                     that reported something).
 *   lft_status_read : copy the word to *host_flags (may be NULL), SYNCHRONISES `stream`; returns 0 when clear,
 *                     LFT_STATUS_NONFINITE when set (lft_last_error() names the cause), or an error code. */
int lft_status_reset(void* workspace, int B, int A, int h, int w, int s, int prec, void* stream);
int lft_status_read(const void* workspace, int B, int A, int h, int w, int s, int prec, void* stream, unsigned* host_flags);

/* Profiling aid, NOT for the hot path: same as lft_forward but records a HIP event on `stream` after every
 * kernel, SYNCHRONISES the stream, and returns per-kernel milliseconds (host arrays ms_out / names_out of
 * max_records entries; names are static strings).  bench.py uses it for the roofline of the dominant kernel. */
int lft_forward_profiled(const void* packed, const float* lr, float* out, void* workspace,
                         int B, int A, int h, int w, int s, int prec, void* stream,
                         int max_records, float* ms_out, const char** names_out, int* n_out);

/* Measurement aid for bench.py's roofline: mean milliseconds of ONE kernel of the forward ("k_conv64", "k_ang", "k_spa1",
 * "k_spa_b"), launched `reps` times back to back between two HIP events on `stream` -- no event between the launches,
 * so the figure is comparable with a rocprofv3 kernel trace.  The kernel reads what a previous lft_forward left in
 * `workspace`.  Synchronises `stream`. */
int lft_kernel_time(const char* kernel, const void* packed, void* workspace, int B, int A, int h, int w, int s, int prec,
                    int reps, void* stream, float* ms_out);

/* ---- per-stage entry points (unit tests, profiling).  `act` buffers are channels-last
 * [B, A*A, h, w, 64] in the activation type of `prec` (float or __bf16). ---- */

/* interpolate(), reference LFT.py:255-266: per-view bicubic of the LR mosaic. */
int lft_bicubic_fwd(const float* lr, float* out, int B, int A, int h, int w, int s, void* stream);
/* conv_init0 + conv_init + residual, reference LFT.py:65-66.  Needs the workspace for 3 temporaries. */
int lft_init_features_fwd(const void* packed, const float* lr, void* act_out, void* workspace,
                          int B, int A, int h, int w, int s, int prec, void* stream);
/* AngTrans.forward of layer `layer`, reference LFT.py:225-238. */
int lft_ang_block_fwd(const void* packed, int layer, const void* act_in, void* act_out,
                      int B, int A, int h, int w, int s, int prec, void* stream);
/* SpaTrans.forward of layer `layer`, reference LFT.py:176-191; skip (may be NULL) is added to the
 * output (the global residual of LFT.py:76 when layer == 3). */
int lft_spa_block_fwd(const void* packed, int layer, const void* act_in, const void* skip, void* act_out,
                      void* workspace, int B, int A, int h, int w, int s, int prec, void* stream);
/* upsampling + bicubic skip, reference LFT.py:79-81: act_in [B,V,h,w,64] -> out fp32 [B,1,A*h*s,A*w*s]. */
int lft_upsample_fwd(const void* packed, const void* act_in, const float* lr, float* out, void* workspace,
                     int B, int A, int h, int w, int s, int prec, void* stream);
/* ---- scene tiling around the hot path (reference utils/utils.py:91-157; caller = test.py:83-101) ----
 * lft_scene_counts   : numU, numV of LFdivide for a scene of A x A views of h0 x w0 (utils.py:95-105).
 * lft_scene_divide   : LFdivide -- scene mosaic fp32 [A*h0, A*w0] -> patches fp32 [numU*numV, 1, A*patch, A*patch]
 *                      (mirror-extended by (patch-stride)/2, zero fill beyond), ready to be fed to lft_forward as a batch.
 * lft_scene_integrate: LFintegrate + re-mosaic (test.py:97-101) -- SR patches [numU*numV, 1, A*patch*s, A*patch*s]
 *                      -> SR scene mosaic [A*h0*s, A*w0*s], keeping the central stride*s region of every patch. */
int lft_scene_counts(int h0, int w0, int patch, int stride, int* num_u, int* num_v);
int lft_scene_divide(const float* scene, float* patches, int A, int h0, int w0, int patch, int stride, void* stream);
int lft_scene_integrate(const float* sr_patches, float* sr_scene, int A, int h0, int w0, int patch, int stride, int s, void* stream);

/* ---- dihedral light-field transforms: geometric self-ensemble at inference, per-sample augmentation in training ----
 * A code t in 0..7 has three bits, applied in this order (the three coin flips of the reference's augmentation,
 * utils/utils_datasets.py:114-124): bit 0 mirrors the mosaic left-right, bit 1 up-down, bit 2 transposes it.  For x[H, W]
 *     T_t(x)[i, j] = x[fi(p), fj(q)],  (p, q) = (j, i) if bit 2 else (i, j),  fi(p) = H-1-p if bit 1 else p,  fj(q) = W-1-q if bit 0 else q;
 * T_t(x) is [W, H] when bit 2 is set.  T_t^-1 undoes the transpose first, then the mirrors (for t = 5, 6 it is not T_t).
 * A set of variants is an 8-bit mask (bit t = code t takes part, E = popcount, variants in ascending code order):
 * 0xFF = all eight, 0x0F = the four mirrors (valid for H != W), 0x01 = the identity.
 * lft_dihedral_batch : out[b] = T_(codes[b] & 7)(in[b]) -- codes: DEVICE int32 [B]; out holds B images of H*W floats each,
 *                      image b laid out [W, H] when its code transposes.
 * lft_dihedral_expand: out[b*E + k] = T_code_k(in[b]); out holds B*E images.
 * lft_dihedral_merge : out[b] = (1/E) sum_k T^-1_code_k(in[b*E + k]); H, W are those of the OUTPUT, variant k is stored [W, H]
 *                      when its code transposes.  fp32: acc = first variant, += the others in ascending code order, one
 *                      multiplication by 1.0f / E -- the same operations in torch give the same bits.
 * lft_scene_integrate_ens: lft_scene_integrate and the merge in one pass over sr_variants [N*E, 1, A*patch*s, A*patch*s] (the
 *                      E variants of patch n adjacent at n*E + k); reads only the central stride*s region of every variant.
 * in == out is refused (LFT_ERR_ARG), as are mask == 0 and mask > 0xFF; non-positive sizes give LFT_ERR_SHAPE.  H != W is valid
 * for the three lft_dihedral_* calls (a transposed image is only laid out differently); the variants of
 * lft_scene_integrate_ens are square by construction. */
int lft_dihedral_batch(const float* in, float* out, const int* codes, int B, int H, int W, void* stream);
int lft_dihedral_expand(const float* in, float* out, unsigned mask, int B, int H, int W, void* stream);
int lft_dihedral_merge(const float* in, float* out, unsigned mask, int B, int H, int W, void* stream);
int lft_scene_integrate_ens(const float* sr_variants, float* sr_scene, unsigned mask, int A, int h0, int w0, int patch, int stride, int s,
                            void* stream);

/* ---- fp32 training step (what PyTorch autograd records / replays for reference LFT.py:52-83 under train.py:89-107) ----
 * The 78 parameters are read IN PLACE (device pointers in state_dict order, HOST array), nothing is packed.
 * `tape` (lft_train_tape_bytes) holds every activation the backward pass re-reads plus its scratch; it must stay
 * untouched between lft_train_forward and lft_train_backward of the same step.
 * lft_train_forward : lr [B,1,A*h,A*w] -> out [B,1,A*h*s,A*w*s] (same function as lft_forward, unfused fp32 kernels).
 * lft_train_backward: dout [B,1,A*h*s,A*w*s] -> grads = ONE flat fp32 buffer (lft_train_grad_floats) holding the 78
 *                     parameter gradients back to back in state_dict order, fully overwritten (not accumulated).
 *                     A data-parallel job all-reduces this one buffer.  It computes no gradient for lr:
 *                     lft_train_backward_input below is the same pass plus d lr.
 *                     Every kernel of the pass runs on `stream` (its gradient tensors live in an arena of the tape and are re-used as
 *                     they die; ABI 4 still carried the second stream of round 2 as an ignored argument -- gone in ABI 5).
 * lft_train_tape_offset: float offset of a saved activation inside the tape, for tests ("feat", "ang0.y", "spa2.tok", ...). */
int lft_train_tape_bytes(int B, int A, int h, int w, int s, size_t* out_bytes);
int lft_train_grad_floats(int s, size_t* out_floats);
int lft_train_tape_offset(const char* name, int B, int A, int h, int w, int s, size_t* out_float_offset);
int lft_train_forward(const float* const* params, int nparams, const float* lr, float* out, void* tape,
                      int B, int A, int h, int w, int s, int math, void* stream);
int lft_train_backward(const float* const* params, int nparams, const float* lr, void* tape, const float* dout, float* grads,
                       int B, int A, int h, int w, int s, int math, void* stream);
/* lft_train_backward plus the gradient of the LR input: d_lr [B,1,A*h,A*w] fp32 (overwritten).  grads are bit-identical
 * to lft_train_backward's for the same tape and dout. */
int lft_train_backward_input(const float* const* params, int nparams, const float* lr, void* tape, const float* dout,
                             float* grads, float* d_lr, int B, int A, int h, int w, int s, int math, void* stream);
/* Stage entry (the _bwd counterpart of lft_bicubic_fwd + conv_init0): d_lr = conv0^T(dx0) + bicubic^T(dout).
 * dx0 [B*A*A*h*w, 64] channels-last; w0 = conv_init0.0.weight [64*9]; dout may be NULL (conv term only). */
int lft_lr_grad_bwd(const float* w0, const float* dx0, const float* dout, float* d_lr, int B, int A, int h, int w, int s, void* stream);
/* The same pass for data-parallel training (the reference's DP recipe, SURVEY.md section 8e: gradients summed over ranks):
 * the flat gradient buffer is finished in LFT_GRAD_BUCKETS contiguous ranges, in this order --
 *   bucket 0: altblock.2, altblock.3, upsampling   (after the backward of layer 2)
 *   bucket 1: altblock.0, altblock.1               (after layer 0)
 *   bucket 2: conv_init0, conv_init                (end of the pass)
 * -- and on_bucket(user, bucket, first_float, n_floats) is called ON THE HOST, from inside this call, right after the last
 * kernel writing that range has been enqueued on `stream`.  The caller orders a
 * communication stream after `stream` there and starts the bucket's all-reduce, which then runs beside the kernels of the
 * remaining buckets; or, while capturing, ends one graph and begins the next (lft_amd/train.py does the latter).  Nothing
 * enqueued after the callback touches the bucket's range.  The callback returns 0 to continue; any other value stops the pass
 * right there (nothing further is enqueued) and the call returns LFT_ERR_CALLBACK -- e.g. a failed collective or capture.  lft_train_backward is this function without notifications;
 * both produce identical bits.  lft_train_grad_bucket gives the ranges (floats) without running anything. */
#define LFT_GRAD_BUCKETS 3
typedef int (*lft_bucket_fn)(void* user, int bucket, size_t first_float, size_t n_floats);
int lft_train_backward_buckets(const float* const* params, int nparams, const float* lr, void* tape, const float* dout, float* grads,
                               int B, int A, int h, int w, int s, int math, void* stream,
                               lft_bucket_fn on_bucket, void* user);
int lft_train_grad_bucket(int s, int bucket, size_t* first_float, size_t* n_floats);
/* The backward pass of ONE block, for unit tests of the backward kernels (the `_bwd` counterparts of the per-stage forward entry
 * points above).  `tape` must hold a complete lft_train_forward of the same inputs.  The block's incoming
 * gradient d_out and outgoing gradient d_in are caller buffers; only the block's own parameter gradients are written to `grads`
 * (the flat buffer of lft_train_backward; every other range is left untouched).
 *   LFT_BLOCK_UPSAMPLE : d_out = d loss / d output image [B,1,A*h*s,A*w*s]; d_in = gradient of the body features [N,64]
 *                        (reference LFT.py:79-81; gradients of upsampling.0.weight, upsampling.3.weight)
 *   LFT_BLOCK_SPA      : SpaTrans of `layer` (LFT.py:176-191): d_out, d_in [N,64]
 *   LFT_BLOCK_ANG      : AngTrans of `layer` (LFT.py:225-238): d_out, d_in [N,64]
 *   LFT_BLOCK_INIT     : conv_init0 + conv_init + residual (LFT.py:65-66): d_out = gradient of the features [N,64]; d_in unused (may be NULL)
 * N = B*A*A*h*w tokens, channels-last [B, A*A, h, w, 64] fp32. */
#define LFT_BLOCK_UPSAMPLE 0
#define LFT_BLOCK_SPA 1
#define LFT_BLOCK_ANG 2
#define LFT_BLOCK_INIT 3
int lft_train_block_backward(const float* const* params, int nparams, const float* lr, void* tape, int block, int layer,
                             const float* d_out, float* d_in, float* grads,
                             int B, int A, int h, int w, int s, int math, void* stream);
/* ---- attention maps: the softmax weights nn.MultiheadAttention(need_weights=True) would return at reference LFT.py:183-187
 * (SpaTrans) and :230-233 (AngTrans), computed from the Q | K that lft_train_forward left in the tape.  `tape` must hold a complete
 * lft_train_forward of the same (B, A, h, w, s), in any math mode; it is only read (a backward pass after the call gives the same
 * bits as without it).  block = LFT_BLOCK_ANG or LFT_BLOCK_SPA, layer = 0..3.  heads_mode: LFT_MAPS_MEAN = averaged over the 8
 * heads (torch's default), LFT_MAPS_HEADS = one map per head (average_attn_weights=False); H below is a dimension of 8 that
 * exists only in LFT_MAPS_HEADS.  fp32 scores and softmax with the row maximum subtracted.  Layout of `maps` (fp32, fully
 * overwritten, lft_attn_maps_floats elements):
 *   LFT_BLOCK_ANG: [B, h, w, (H,) V_query, V_key], V = A*A -- the reference's (b h w) batch order;
 *   LFT_BLOCK_SPA: compact [B, V, (H,) h, w, 5, 5]: element (dy, dx) is the weight of query (y, x) on key (y+dy-2, x+dx-2), EXACTLY 0
 *                  where that key is outside the view or outside the reference's clamped window (LFT.py:155 clamps the column range
 *                  with h, not w; the window is always a subset of the centred 5x5, the dense [hw, hw] form is never built).  For
 *                  h < w a query with x - 2 >= h has an empty window: all 25 are exactly 0 -- the twin of the forward's attention
 *                  output 0 for such a query -- where torch's own need_weights path gives NaN.
 * Enqueue-only on `stream`, no allocation, no synchronisation, graph-capturable. */
#define LFT_MAPS_MEAN 0    /* averaged over the 8 heads: what nn.MultiheadAttention(need_weights=True) returns */
#define LFT_MAPS_HEADS 1   /* one map per head (average_attn_weights=False) */
int lft_attn_maps_floats(int block, int heads_mode, int B, int A, int h, int w, size_t* out_floats);
int lft_train_attn_maps(const void* tape, int block, int layer, int heads_mode, float* maps,
                        int B, int A, int h, int w, int s, void* stream);
/* Profiling aid, NOT for the hot path (bench.py's `train.roofline`): lft_train_forward + lft_train_backward on ONE stream with a HIP
 * event after every kernel; SYNCHRONISES the stream and returns per-kernel milliseconds in launch order (host arrays of max_records
 * entries, names are static strings; a step has about 450 launches). */
int lft_train_step_profiled(const float* const* params, int nparams, const float* lr, float* out, void* tape, const float* dout, float* grads,
                            int B, int A, int h, int w, int s, int math, void* stream,
                            int max_records, float* ms_out, const char** names_out, int* n_out);
/* get_loss (reference LFT.py:269-277, torch.nn.L1Loss): *loss = mean |sr - hr|; if dsr != NULL also
 * dsr = gscale * sign(sr - hr) (gscale = 1/n for d loss / d sr).  scratch1024: 1024 floats of device scratch. */
int lft_l1_loss(const float* sr, const float* hr, long long n, float* dsr, float gscale, float* loss, float* scratch1024, void* stream);
/* ---- light-field training loss: a pixel penalty plus the same penalty on the epipolar-plane-image (EPI) gradients ----
 * sr and hr are fp32 [B,1,A*H,A*W]; H x W is the HR view size; view (a1,a2) occupies rows a1*H... and columns a2*W....
 * d = sr - hr, seen as d[b,a1,y,a2,x]; n = B*A*A*H*W.  The penalty rho is chosen by an enum:
 *   LFT_LOSS_L1          rho(x) = |x|                  rho'(x) = sign(x), with rho'(0) = 0
 *   LFT_LOSS_MSE         rho(x) = x^2                  rho'(x) = 2x
 *   LFT_LOSS_CHARBONNIER rho(x) = sqrt(x^2 + eps^2)    rho'(x) = x / sqrt(x^2 + eps^2)
 * Pixel term: P = (1/n) sum rho(d).
 * EPI term, from four forward differences of d:
 *   Dx : x+1 minus x, inside a view: x = 0..W-2, never across a view border      n_x = B*A*A*H*(W-1)
 *   Dy : y+1 minus y, inside a view                                              n_y = B*A*A*(H-1)*W
 *   Dv : view a2+1 minus view a2 at the same (a1,y,x)                            n_v = B*A*(A-1)*H*W
 *   Du : view a1+1 minus view a1 at the same (a2,y,x)                            n_u = B*A*(A-1)*H*W
 * (Dv, Dx) is the gradient of the horizontal EPI (a1 and y fixed), (Du, Dy) that of the vertical EPI.  E is the mean, over the T
 * differences that exist (count above 0), of (1/n_t) sum rho(D_t d); E = 0 if T = 0.  The gradient operator is linear, so this is
 * exactly rho applied to (EPI gradient of SR - EPI gradient of HR).
 *   total = w_pix*P + w_epi*E
 *   d total / d sr = w_pix*rho'(d)/n + (w_epi/T) sum_t (1/n_t)*(rho'(D_t d at the pair ending here) - rho'(D_t d at the pair starting here)):
 * at most nine contributions per pixel.  Every n_t scales with B, so a mean over equal local shards averages to the global-batch
 * objective, as for L1.
 * lft_lf_loss: loss3[0..2] = {total, P, E}; dsr (may be NULL: values only) = gscale * d total / d sr, fully overwritten -- gscale = 1
 * gives the gradient itself, the 1/n factors are inside, unlike lft_l1_loss.  scratch: lft_lf_loss_scratch_bytes bytes of device
 * memory, 8-byte aligned.  Two launches (one stencil pass, one fold of fp64 per-block partial sums in a fixed order: no atomics,
 * bit-reproducible); no allocation, no synchronisation, graph-capturable; 16-byte accesses where the row pitch A*W and the pointers
 * allow, scalar ones otherwise; any H, W >= 1, A*A <= 128.
 * Refused before anything is launched -- LFT_ERR_ARG: null sr, hr, loss3 or scratch, misaligned pointers; an unknown penalty;
 * Charbonnier with eps <= 0 or NaN; negative or NaN weights, or both weights zero; NaN gscale; dsr overlapping sr or hr (the stencil
 * reads neighbours: in place would race).  LFT_ERR_SHAPE: non-positive sizes; A*A > 128. */
#define LFT_LOSS_L1 0
#define LFT_LOSS_MSE 1
#define LFT_LOSS_CHARBONNIER 2
int lft_lf_loss_scratch_bytes(int B, int A, int H, int W, size_t* out_bytes);
int lft_lf_loss(const float* sr, const float* hr, int B, int A, int H, int W, int penalty, float eps, float w_pix, float w_epi,
                float* dsr, float gscale, float* loss3, void* scratch, void* stream);
/* ---- structural training term: one minus the Gaussian-window SSIM, value and gradient ----
 * sr and hr are fp32 [B,1,A*H,A*W]; H x W is the HR view size; view (a1,a2) occupies rows a1*H... and columns a2*W....
 * Per view the SSIM map is exactly that of lft_view_metrics (k_view_metrics): normalised separable 11x11 Gaussian g, sigma 1.5;
 * mu = g * v, sigma^2 = (121/120) (g * v^2 - mu^2), sigma_xy likewise; C1 = (0.01 R)^2, C2 = (0.03 R)^2 with R = ssim_range;
 *   S_q = (2 mu_x mu_y + C1)(2 sigma_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(sigma_x^2 + sigma_y^2 + C2))      x = hr, y = sr
 * at the interior pixels 5 <= y < H-5, 5 <= x < W-5 only; a window never crosses a view border.  S_view is the mean of the map over
 * the interior, and
 *   S = the PLAIN mean of S_view over all B*A*A views,    Q = 1 - S.
 * This is NOT cal_metrics' "mean over the views above 0" (what fit and evaluate log per set): that rule drops views by their value
 * and is not differentiable.  Every count scales with B, so a mean over equal local shards averages to the global-batch objective,
 * as for L1 and lft_lf_loss.
 * Gradient: d S / d y(p) = (1 / (views * interior pixels)) sum_q g(q - p) [a(q) + b(q) y(p) + c(q) x(p)], with
 *   b = 2 (121/120) dS_q/d sigma_y^2,  c = (121/120) dS_q/d sigma_xy,  a = dS_q/d mu_y - b mu_y - c mu_x,
 * all zero at centres q outside the interior: three more separable filter passes.  ALL arithmetic between the fp32 loads and the fp32
 * stores is fp64, as in lft_view_metrics: E[v^2] - mu^2 cancels, and an all-fp32 evaluation is wrong by 1e-5 ... 6.5e-5 of the
 * largest gradient element on smooth inputs, where the fp64 one leaves the store rounding.
 * lft_ssim_loss: *ssim_out = S.  accumulate == 0: *total = w_ssim*Q, and dsr (may be NULL: values only) is fully overwritten with
 * gscale * w_ssim * dQ/dsr.  accumulate == 1: both are ADDED, in stream order, to what total and dsr already hold (one rounding of
 * the fp64 sum) -- this is how the term follows lft_lf_loss in a training step.  scratch: lft_ssim_loss_scratch_bytes bytes of
 * device memory, 8-byte aligned.  Two launches (one 16x16-tile stencil pass with a halo of 10, one fold of fp64 per-tile partial
 * sums in a fixed order: no atomics, bit-reproducible); no allocation, no synchronisation, graph-capturable; any row pitch and any
 * 4-byte aligned pointers: the tile loads and stores are scalar, one 64-byte row segment per 16 lanes.
 * Refused before anything is launched -- LFT_ERR_ARG: null sr, hr, total, ssim_out or scratch, misaligned pointers; ssim_range or
 * w_ssim not finite or <= 0; NaN gscale; accumulate other than 0 or 1; dsr overlapping sr or hr.  LFT_ERR_SHAPE: non-positive
 * sizes; H < 11 or W < 11 (the rule of lft_view_metrics); more than 2^31 - 1 tiles. */
int lft_ssim_loss_scratch_bytes(int B, int A, int H, int W, size_t* out_bytes);
int lft_ssim_loss(const float* sr, const float* hr, int B, int A, int H, int W, float ssim_range, float w_ssim,
                  float* dsr, float gscale, int accumulate, float* total, float* ssim_out, void* scratch, void* stream);
/* torch.optim.Adam step (train.py:77-83: betas (0.9, 0.999), eps 1e-8, weight_decay = --decay_rate, default 0) on one
 * flat fp32 buffer; step counts from 1; the gradient is multiplied by gscale first (1/world_size after a sum all-reduce),
 * then weight_decay * p is added (torch's L2 form); bias corrections are computed in double, as torch does. */
int lft_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                  int step, float gscale, float weight_decay, void* stream);
/* ---- guarded Adam step: gradient-norm clipping, non-finite gradients skipped, frozen tensors, all decided on the device ----
 * lft_adam_step applies whatever the gradient buffer holds.  lft_adam_step_guarded first measures it (one pass, fp64 sums folded
 * in a fixed order: bit-reproducible), then
 *   - a NaN / inf anywhere in a TRAINABLE segment: p, m and v keep their bits, steps_skipped += 1, Adam's step counter does not
 *     advance (the next clean call uses the same bias corrections as if the bad call had not happened);
 *   - otherwise coef = min(1, max_norm / (norm + 1e-6)) with norm = gscale * sqrt(sum of g^2 over the trainable segments), in
 *     double -- torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False)'s formula; coef = 1 when max_norm <= 0 or +inf (no
 *     clipping) --, steps_applied += 1 =: t, and lft_adam_step's update with g * gscale * coef in place of g * gscale and bias
 *     corrections 1 - beta^t formed in double, on the trainable segments only.
 * Unlike torch, which scales .grad in place, the gradient buffer is NEVER written: the clip is folded into the update.
 * Guard block: a caller-owned DEVICE buffer of lft_guard_bytes(nseg) bytes, 16-byte aligned, that lives across steps.  It holds the
 * segment table (one segment per tensor of the flat buffer: ascending, tiling [0, n) exactly; trainable = 0 freezes a tensor --
 * its p, m, v are never touched and its gradient, NaN included, takes no part in the norm or the decision, as torch ignores a
 * parameter without .grad), the counters and the report of the last step.
 *   lft_guard_init        : enqueue the writing of the block.  segs is a HOST array read before the call returns.  steps_applied0:
 *                           Adam steps already taken (0 for a fresh optimizer; resuming at step t + 1 passes t).  The library
 *                           remembers (guard address -> n, block count) on the host, so that lft_adam_step_guarded can refuse
 *                           a block it did not initialise, or another n, before anything is launched; the newest 256 blocks
 *                           are remembered.
 *   lft_adam_step_guarded : three launches on `stream`; no allocation, no synchronisation, graph-capturable -- the step number is
 *                           read from the block, so a captured call replays correctly.
 *   lft_guard_read        : copy the report to *host; SYNCHRONISES `stream`.  grad_norm, clip_coef (0 on a skipped step),
 *                           skipped_last, nonfinite_last (trainable segments) and bad_segment (first trainable segment holding a
 *                           non-finite element, -1 if none) describe the LAST call; seg_norm[i] = gscale * sqrt(sum of the finite
 *                           g^2 of segment i), frozen segments included; the three counters run since lft_guard_init.
 * LFT_ERR_ARG / LFT_ERR_SHAPE before anything is launched: null or misaligned pointers, nseg outside 1..128, a table that does not
 * tile [0, n) in ascending order with counts >= 1, a block that was not initialised, n other than lft_guard_init's, NaN max_norm. */
#define LFT_GUARD_MAX_SEGMENTS 128
typedef struct { long long first, count; int trainable; } lft_segment;
typedef struct { float grad_norm, clip_coef; int skipped_last, bad_segment; long long nonfinite_last,
                 steps_applied, steps_skipped, steps_clipped; float seg_norm[LFT_GUARD_MAX_SEGMENTS]; } lft_guard_report;
int lft_guard_bytes(int nseg, size_t* out_bytes);
int lft_guard_init(void* guard, const lft_segment* segs, int nseg, long long n, long long steps_applied0, void* stream);
int lft_adam_step_guarded(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                          float gscale, float weight_decay, float max_norm, void* guard, void* stream);
int lft_guard_read(const void* guard, void* stream, lft_guard_report* host);
/* Exponential moving average of the weights, kept beside them as one more flat fp32 buffer: ema += a * (p - ema) per element in
 * fp32, a = (float)(1 - d_t), d_t = warmup ? min(decay, (1 + t) / (10 + t)) : decay formed in double, t = Adam steps applied so
 * far, this one included.  Call it after the Adam step, on the same stream.
 *   guard != NULL : t is the block's steps_applied, read on the device (`step` is ignored; a captured call replays correctly); after
 *                   a skipped step ema keeps its bits; frozen segments are never written.  The block must have been initialised for
 *                   this n.
 *   guard == NULL : t = step (>= 1), every element of [0, n) is updated.
 * One launch; no allocation, no synchronisation, no atomics (bit-reproducible), graph-capturable.  16-byte accesses where ema and p
 * share their alignment, scalar ones otherwise.  LFT_ERR_ARG before anything is launched: null or misaligned pointers, n < 1, ema
 * and p overlapping, decay outside [0, 1) or NaN, step < 1 without a guard, a block that was not initialised or another n. */
int lft_ema_update(float* ema, const float* p, long long n, float decay, int warmup, long long step, const void* guard, void* stream);

/* ---- per-view quality metrics (reference utils/utils.py:56-88 cal_metrics, which calls scikit-image) ----
 * label, out: fp32 mosaics [B,1,A*h,A*w]; psnr, ssim: fp32 [B*A*A] in (b, u, v) order.  PSNR = 10 log10(R^2 / MSE) with
 * R = 1 when min(label view) >= 0 else 2; SSIM = mean over the view minus a 5-pixel border of the Gaussian-window
 * (sigma 1.5, 11x11, sample covariance, K1 0.01, K2 0.03) SSIM map with data range `ssim_range` (2 reproduces the
 * scikit-image releases contemporary with the reference; 1 is the physical range).  fp64 accumulation. */
int lft_view_metrics_scratch_bytes(int B, int A, int h, int w, size_t* out_bytes);
int lft_view_metrics(const float* label, const float* out, int B, int A, int h, int w, float ssim_range, float* psnr, float* ssim,
                     void* scratch, void* stream);

/* ---- data preparation (reference Generate_Data_for_Training.m / Generate_Data_for_Test.m, per sub-aperture view) ----
 * lf: the raw light field on the device in its stored class, LF[u][v][h][w][c] at element offset
 *     u*strides[0] + v*strides[1] + h*strides[2] + w*strides[3] + c*strides[4] (strides: HOST array of 5; a v7.3 .mat's
 *     reversed [C,W,H,V,U] array is read in place).  Only channels 0..2 are read; values enter as stored (uint8 as 0..255).
 * Views: the centre A x A, starting at ((U-A)/2, (V-A)/2); U-A and V-A must be even.
 * crops: HOST array of n_crops (y0, x0) origins of crop_h x crop_w regions inside every view.
 * weights_* / indices_*: MATLAB's imresize contribution tables of one crop axis (fp64 [out, taps], int32 [out, taps], device),
 *     out = ceil(crop / s) (lft_amd/prepare.py:contributions).
 * Per crop n and view (u, v), in fp64: Y = rgb2ycbcr(rgb)[..., 0], hr = single(Y), lr = single(imresize(Y, 1/s)) with the
 * rows resized first; outputs are fp32 mosaics in the MATLAB matrix orientation:
 *     hr [n_crops, A*crop_h, A*crop_w], lr [n_crops, A*ceil(crop_h/s), A*ceil(crop_w/s)]. */
#define LFT_LF_UINT8 0
#define LFT_LF_FLOAT32 1
#define LFT_LF_FLOAT64 2
int lft_lf_prepare(const void* lf, int lf_class, int U, int V, int H, int W, int C, const long long* strides, int A, int s,
                   const int* crops, int n_crops, int crop_h, int crop_w, const double* weights_h, const int* indices_h, int taps_h,
                   const double* weights_w, const int* indices_w, int taps_w, float* hr, float* lr, void* stream);

/* ---- colour path: a raw RGB light field in, super-resolved RGB views out ----
 * lf, lf_class, U, V, H, W, C, strides, A: the light field and its centre A x A views, as for lft_lf_prepare (any strides, a
 *     v7.3 .mat's reversed array read in place), with ONE difference: the values are scaled to [0, 1] first, x = double(LF) / 255
 *     for LFT_LF_UINT8 and x = double(LF) for the float classes (stored in [0, 1]); lft_lf_prepare takes them as stored.
 * Per view, in fp64: ycc = rgb2ycbcr(x) (reference utils/utils.py:160-168).
 * lft_lf_luma: y_out = single(ycc[..., 0]) as the network's input mosaic [A*H, A*W] (row u*H + h, column v*W + w).
 * lft_colour_merge: Cb and Cr are up-scaled by imresize(., s) (reference utils/imresize.py: Keys cubic a = -0.5, no antialiasing,
 *     symmetric border, rows first) with the caller's contribution tables, weights_* fp64 [s*L, taps] and indices_* int32
 *     [s*L, taps] on the device (lft_amd/colour.py:up_contributions; L = H for _h, W for _w; 1 <= taps <= 6).
 *     Y is sr_y, the fp32 mosaic [A*s*H, A*s*W] of the super-resolved luma, or with sr_y == NULL the up-scaled ycc[..., 0]: the
 *     bicubic baseline.  rgb = Minv * (255 * [Y, Cb, Cr] - [16, 128, 128]), minv: HOST array of 9 doubles, the row-major inverse
 *     of rgb2ycbcr's 3 x 3 matrix (evaluated by the caller in fp64; read before the call returns).
 *     out: [A, A, s*H, s*W, 3] interleaved RGB; out_class LFT_LF_UINT8 stores convertDouble2Byte(rgb) (clip to [0, 1], * 255,
 *     round half to even), LFT_LF_FLOAT32 stores single(rgb), unclipped.  s is 2 or 4.
 * Both calls only enqueue on `stream` (graph-capturable), allocate nothing, and refuse bad arguments with LFT_ERR_ARG or
 * LFT_ERR_SHAPE before anything is launched. */
int lft_lf_luma(const void* lf, int lf_class, int U, int V, int H, int W, int C, const long long* strides, int A, float* y_out,
                void* stream);
int lft_colour_merge(const void* lf, int lf_class, int U, int V, int H, int W, int C, const long long* strides, int A, int s,
                     const float* sr_y, const double* weights_h, const int* indices_h, int taps_h, const double* weights_w,
                     const int* indices_w, int taps_w, const double* minv, void* out, int out_class, void* stream);

/* ---- synthetic refocus: a focal stack from the views of a light field (added to ABI 5 without a new version number) ----
 *   R_d[y, x, c] = sum_{u,v} a[u,v] * S(L[u,v,:,:,c], y + d*(u-uc), x + d*(v-uc)),   uc = (A-1)/2,
 * d the slope in pixels per view step: a Lambertian plane L[u,v,y,x] = f(y - d0*(u-uc), x - d0*(v-uc)) comes back as f at d = +d0.
 * S is separable, rows (y) first, `taps` taps per axis: 1 nearest, 2 linear, 4 Keys cubic (a = -0.5).
 * lf: element (b, u, v, y, x, c) of the B light fields of A x A views, H x W pixels, C <= 4 channels at
 *     b*strides[0] + u*strides[1] + v*strides[2] + y*strides[3] + x*strides[4] + c*strides[5] (strides: HOST array of 6, >= 0):
 *     views [A, A, H, W, C] and the network's mosaic [B, 1, A*H, A*W] are both read in place.  LFT_LF_UINT8 enters as x / 255,
 *     LFT_LF_FLOAT32 as stored.
 * table: DEVICE array of D * A*A records, slope-major, views in (u, v) order (lft_amd/refocus.py:shift_table computes them in
 *     fp64 and rounds once).  Tap k of the row filter reads row clamp(y + oy + k, 0, H-1) with weight wy[k], tap k of the column
 *     filter column clamp(x + ox + k, 0, W-1) with weight wx[k]; weights beyond `taps` are ignored; a is the view's aperture
 *     weight; a view with skip != 0 is not read at all.
 * out: [B, D, H, W, C]; LFT_LF_FLOAT32 stores the fp32 sum, unclipped, LFT_LF_UINT8 clips to [0, 1], * 255, rounds half to even.
 * Sums are fp32, over the views in (u, v) order and the taps in table order, one fused multiply-add per step after a sum's first
 * product: a pixel's bits do not depend on the image around its taps or on the launch shape.  A view must span less than 2^31
 * elements (LFT_ERR_SHAPE otherwise).  The call only enqueues on `stream` (graph-capturable), allocates nothing,
 * and refuses with LFT_ERR_ARG / LFT_ERR_SHAPE before anything is launched: A < 1, C outside 1..4, taps not 1, 2 or 4, D < 1,
 * classes other than the above, negative sizes or strides, a null pointer with a non-empty shape (B, H or W == 0: no work, 0). */
typedef struct { int oy, ox; float wy[4], wx[4]; float a; int skip; } lft_refocus_record;   /* 48 bytes */
int lft_refocus(const void* lf, int lf_class, int B, int A, int H, int W, int C, const long long* strides, const void* table, int D,
                int taps, void* out, int out_class, void* stream);

/* ---- disparity from a light field: plane sweep, windowed aggregation, winner-take-all (added to ABI 5 without a new version
 * number) ----
 * Inputs are the same as for lft_refocus:
 * - B light fields of A x A views, H x W pixels, C <= 4 channels, read in place through six element strides.
 * - uint8 enters as x/255, float32 as stored.
 * - Slopes d_0 < d_1 < ... < d_{D-1} are strictly increasing; they need not be uniform.
 * - aperture, interp (1, 2 or 4 taps) and the table are those of refocus.shift_table.
 * - The sample s_k[u,v,y,x,c] = S(L[u,v,:,:,c], y + d_k(u-uc), x + d_k(v-uc)) is exactly refocus's: rows first, clamped taps,
 *   weights not renormalised.
 *
 * The outputs are defined as follows.
 *
 * 1. Moments. m_k[y,x,c] = sum_{u,v} a*s, which is the refocus stack. q_k[y,x,c] = sum_{u,v} a*s^2.
 * 2. Raw cost. V_k[y,x] = sum_c max(q_k - m_k^2, 0). This is the aperture-weighted variance of the views at slope d_k, summed
 *    over channels.
 * 3. Aggregated cost. E_k[y,x] = (2r+1)^-2 * sum_{dy,dx in [-r,r]} V_k[clamp(y+dy,0,H-1), clamp(x+dx,0,W-1)].
 *    - The radius r is in 0..8. r = 0 gives E = V.
 * 4. Index. k* = argmin_k E_k, the lowest k on an exact tie.
 * 5. Sub-sample refinement. All of it is fp32, each step a single rounded operation, with the compiler's contraction off as in
 *    k_refocus.
 *    - For 0 < k* < D-1: den = (E_{k*-1} - E_{k*}) + (E_{k*+1} - E_{k*}). Both terms are >= 0, so there is no cancellation.
 *    - delta = 0.5*(E_{k*-1} - E_{k*+1})/den if den > 0, clamped to [-0.5, 0.5]. Otherwise, and at either end of the sweep,
 *      delta = 0.
 *    - disparity = d_{k*} + delta*(d_{k*+1} - d_{k*}) for delta >= 0, and d_{k*} + delta*(d_{k*} - d_{k*-1}) for delta < 0.
 *    - The slopes are rounded once to fp32 on the host.
 * 6. Confidence. Ebar = (sum_k E_k)/D, summed in k order. conf = 1 - E_{k*}/Ebar if Ebar > 0, else 0.
 *    - A flat region, A = 1 and D = 1 all give 0.
 * 7. All-in-focus. aif[y,x,c] = m_{k*(y,x)}[y,x,c], fp32 or uint8 by refocus's rule.
 *    - m is accumulated in refocus's order: views in (u,v) order, taps in table order, explicit FMAs.
 *    - So aif equals lft_refocus's fp32 stack gathered at k*, bit for bit.
 *
 * A pixel's results must not depend on the tile, on the image around the support of its taps and window, or on the launch
 * shape. That requires a fixed aggregation order, dy then dx.
 *
 * lf, lf_class, strides, table, taps: as for lft_refocus.  slopes: DEVICE array of D floats, the slopes of the table rounded to fp32
 *     (their order is the caller's to check: the array is on the device).  radius: r.
 * scratch: DEVICE, 4-byte aligned, lft_disparity_scratch_bytes(B, D, H, W, C, flags) bytes, flags LFT_DISPARITY_AIF when aif is
 *     asked for: V [B, D, H, W] and behind it m [B, D, H, W, C], both fp32.  Its contents after the call are unspecified.
 * disparity, confidence: fp32 [B, H, W]; index: int32 [B, H, W]; cost: NULL, or fp32 [B, D, H, W] for E; aif: NULL, or
 *     [B, H, W, C] of aif_class (LFT_LF_FLOAT32 the fp32 sum, LFT_LF_UINT8 clipped to [0, 1], * 255, rounded half to even).
 * lft_disparity only enqueues on `stream` (two kernels; graph-capturable), allocates nothing, and refuses with LFT_ERR_ARG /
 * LFT_ERR_SHAPE and a message starting "lft_disparity:" before anything is launched: lft_refocus's rules, a radius outside 0..8,
 * a null scratch or a null required output with a non-empty shape (B, H or W == 0: no work, 0). */
#define LFT_DISPARITY_AIF 1
int lft_disparity_scratch_bytes(int B, int D, int H, int W, int C, int flags, size_t* out_bytes);
int lft_disparity(const void* lf, int lf_class, int B, int A, int H, int W, int C, const long long* strides, const void* table,
                  const float* slopes, int D, int taps, int radius, void* scratch, float* disparity, float* confidence, int* index,
                  float* cost, void* aif, int aif_class, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LFT_HIP_H */
