/* lft_hip_focal.h -- the focal-stack training term and the adjoint of lft_refocus, entry points of liblft_hip.so.
 * Added beside ABI 5; lft_version unchanged.  The conventions are those of lft_hip.h (plain pointers, DEVICE unless noted, enqueue
 * only, 0 / LFT_ERR_* / hipError_t, lft_last_error); a library that lacks these symbols is an older build of the same ABI.
 *
 * Refocusing is linear.  A term on the focal stack of SR - HR therefore weights an error by how much of it survives the aperture
 * sum: independent per-view errors average out by 1/A, errors that follow the scene's parallax do not.
 *
 * Inputs.
 * - sr, hr: fp32 mosaics [B,1,A*H,A*W]. View (u,v) is at rows u*H... and columns v*W....
 * - The refocus table [D, A*A] of lft_refocus_record, from refocus.shift_table(A, slopes, aperture, interp, centre).
 * - taps in {1,2,4}.
 * - 1 <= D <= LFT_FOCAL_MAX_D = 64.
 * - A*A <= 128.
 * - A penalty rho out of LFT_LOSS_L1, LFT_LOSS_MSE and LFT_LOSS_CHARBONNIER, with eps. These are the constants and the rho of
 *   lft_lf_loss.
 * - A weight w_focal > 0.
 * - gscale.
 *
 * 1. Residual stack.
 * - e = fl(sr - hr) per element, in fp32.
 * - r_k[b,y,x] is lft_refocus's fp32 output for the light field e and the same table. That means: views in (u,v) order, rows
 *   first, clamped taps, explicit FMAs, skipped views not read.
 * - r is bit for bit lft_refocus run on the materialised difference mosaic.
 *
 * 2. Value.
 * - F = (1/N) sum_{b,k,y,x} rho(r), with N = B*D*H*W.
 * - rho is evaluated in fp64 on the fp32 r.
 * - The sum is fp64, from per-block partial sums folded in a fixed order.
 * - No atomics.
 *
 * 3. Stack gradient.
 * - G_k[b,y,x] = fl32(gscale * w_focal * rho'(r)/N).
 * - rho' is evaluated in fp64 and rounded once.
 * - For L1, rho'(0) = 0.
 *
 * 4. Adjoint.  For view n = (u,v) and its pixel (y',x'):
 *   dsr[b,u,v,y',x'] = sum_k a_{k,n} * sum_{jy} wy[jy] sum_{y in Py} sum_{jx} wx[jx] sum_{x in Px} G_k[b,y,x]
 * - Py = {y in [0,H) : clamp(y + oy + jy, 0, H-1) = y'}. Px is likewise.
 * - Skipped views get 0.
 * - An interior pixel has one y per tap.
 * - A border pixel collects every y whose tap was clamped onto it.
 * - The adjoint is fp32.
 * - The order of the sums is fixed: over k, then jy, then y ascending, then jx, then x ascending; the sums over x and y are plain
 *   fp32 additions from 0, each product enters by one explicit FMA (wx into the sum over jx, wy into the sum over jy, a into the sum
 *   over k), with contraction off. Nothing depends on launch shape, tile or arrival order, there are no atomics, and two runs give
 *   the same bits.
 *
 * 5. Outputs.
 * - *focal_out = fl32(F).
 * - With accumulate == 0: *total = fl32(w_focal*F), and dsr is fully overwritten.
 * - With accumulate == 1: both are added to what total and dsr hold, in stream order. This takes one rounding each, as
 *   lft_ssim_loss does.
 * - dsr may be NULL (values only).
 * - An optional output residual: NULL, or fp32 [B,D,H,W] for r.
 * Every count scales with B. A mean over equal local shards is therefore the global-batch objective.
 *
 * lft_focal_loss: three launches -- k_focal_residual (steps 1 to 3: one lane per stack pixel, the difference formed on the fly, G
 * into the scratch), k_focal_fold (step 2's fold and step 5's values) and, unless dsr is NULL, k_focal_adjoint (step 4 as a gather,
 * one lane per mosaic pixel).  scratch: lft_focal_loss_scratch_bytes bytes of device memory, 8-byte aligned; it holds the per-block
 * sums and G.  Byte contract: sr and hr are read once per tap and active view by the lanes whose taps fall on them (TAPS^2 * 2 reads
 * per stack pixel and active view, served by the caches: the compulsory traffic is 2 * 4 * B*A*A*H*W bytes), G is written and read
 * once as 4 * B*D*H*W bytes each plus the border preimages, dsr is written (accumulate: read and written) once.
 * lft_refocus_adjoint: step 4 alone for any fp32 stack_grad [B,D,H,W] into the mosaic out [B,1,A*H,A*W] (accumulate == 1: added to
 * it, one rounding); one launch of k_focal_adjoint, no scratch.
 * All three only enqueue on `stream` (graph-capturable), allocate nothing and never synchronise.
 * Refused before anything is launched, with a message that starts with the function's name -- LFT_ERR_ARG: null sr, hr, table,
 * total, focal_out or scratch (stack_grad, table or out), pointers not 4-byte aligned, a scratch not 8-byte aligned; an unknown
 * penalty; Charbonnier with eps <= 0 or NaN; w_focal not finite or <= 0; NaN gscale; accumulate other than 0 or 1; taps not 1, 2 or
 * 4; D outside 1 .. LFT_FOCAL_MAX_D; dsr overlapping sr or hr (out overlapping stack_grad).  LFT_ERR_SHAPE: non-positive sizes;
 * A*A > 128; more than 2^31 - 1 blocks of 32 x 8 pixels. */
#ifndef LFT_HIP_FOCAL_H
#define LFT_HIP_FOCAL_H

#include "lft_hip.h"      /* LFT_LOSS_*, lft_refocus_record */

#ifdef __cplusplus
extern "C" {
#endif

#define LFT_FOCAL_MAX_D 64

int lft_focal_loss_scratch_bytes(int B, int D, int A, int H, int W, size_t* out_bytes);
int lft_focal_loss(const float* sr, const float* hr, int B, int A, int H, int W, const void* table, int D, int taps, int penalty,
                   float eps, float w_focal, float* dsr, float gscale, int accumulate, float* total, float* focal_out, float* residual,
                   void* scratch, void* stream);
int lft_refocus_adjoint(const float* stack_grad, int B, int A, int H, int W, const void* table, int D, int taps, float* out,
                        int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif
