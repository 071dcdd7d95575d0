/* lft_hip_sgm.h -- semi-global aggregation of a disparity cost volume, entry points of liblft_hip.so.
 * Added beside ABI 5; lft_version unchanged.  The conventions are those of lft_hip.h (plain pointers, DEVICE unless noted, enqueue
 * only, 0 / LFT_ERR_* / hipError_t, lft_last_error); a library that lacks these symbols is an older build of the same ABI.
 *
 * Inputs
 * - E: fp32 [B, D, H, W], the aggregated cost of lft_disparity or any other cost. It must be finite. The bit-for-bit promise is
 *   for costs >= +0.
 * - Slopes: as for lft_disparity.
 * - Host floats P1, P2 with 0 <= P1 <= P2, and gain >= 0, each rounded once to fp32.
 * - An optional guide g: fp32 [B, H, W].
 * - paths R in {4, 8}.
 * - 1 <= D <= LFT_SGM_MAX_D = 256.
 *
 * Directions, in this order; paths = 4 takes the first four. Here q = p - r is the predecessor of p on the path.
 * - r0 = (0,+1), r1 = (0,-1), r2 = (+1,0), r3 = (-1,0)
 * - r4 = (+1,+1), r5 = (-1,-1), r6 = (+1,-1), r7 = (-1,+1), each written (dy, dx).
 *
 * Recurrence. All of it is fp32, one rounded operation per step, contraction off.
 * - If q lies outside the image: L_r(p,k) = E(p,k).
 * - Otherwise:
 *   - M = min_j L_r(q,j).
 *   - P2' = P2 without a guide.
 *   - With a guide: P2' = max(P1, P2 - fl(gain*|fl(g(p) - g(q))|)).
 *   - c = fl(M + P2').
 *   - b_k = fl(min(L_r(q,k-1), L_r(q,k+1)) + P1) over the neighbours that exist. With D = 1 there is none and b is absent.
 *   - t_k = min(L_r(q,k), b_k, c).
 *   - L_r(p,k) = fl(E(p,k) + fl(t_k - M)).
 *
 * Sum. S = fl(...fl(fl(L_0 + L_1) + L_2)... + L_{R-1}) * fl(1/R). The scaling is exact for R = 4 and 8.
 *
 * Selection. Steps 4-7 of lft_disparity, word for word, applied to S in the place of E:
 * - index: the lowest k on a tie,
 * - the parabola refinement,
 * - conf = 1 - S_{k*}/Sbar,
 * - aif gathered from a stack at k*.
 *
 * Nothing may depend on launch shape, tile or arrival order. Every sum has a fixed order, and min has none to fix.
 *
 * cost: E.  C: the channels of `stack` and `aif`, 1 .. 4 (judged also without them).  slopes: DEVICE fp32 [D].
 * guide: NULL, or g; gain > 0 needs it.  stack: NULL, or fp32 [B, D, H, W, C]; required when aif is given.
 * scratch: DEVICE, 4-byte aligned, lft_sgm_scratch_bytes(B, D, H, W, paths) bytes.  Unspecified afterwards.
 * disparity, confidence: fp32 [B, H, W].  index: int32 [B, H, W].  aggregated: NULL, or fp32 [B, D, H, W] for S.
 * aif: NULL, or [B, H, W, C] of aif_class (LFT_LF_FLOAT32 the stack's value itself, LFT_LF_UINT8 by refocus's rule).
 * lft_sgm only enqueues on `stream` (two kernels; graph-capturable), allocates nothing, and refuses with LFT_ERR_ARG /
 * LFT_ERR_SHAPE and a message starting "lft_sgm:" before anything is launched: paths not 4 or 8, D outside 1 .. 256, C outside
 * 1 .. 4, a negative or non-finite p1, p2 or gain, p2 < p1, gain > 0 without a guide, aif without a stack, an unknown aif_class,
 * a negative size (LFT_ERR_SHAPE), a null cost, slopes, scratch, disparity, confidence or index with a non-empty shape (B, H or
 * W == 0: no work, 0), a misaligned scratch, a volume beyond 2^40 bytes or views beyond 2^31 pixels (LFT_ERR_SHAPE). */
#ifndef LFT_HIP_SGM_H
#define LFT_HIP_SGM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LFT_SGM_MAX_D 256
int lft_sgm_scratch_bytes(int B, int D, int H, int W, int paths, size_t* out_bytes);
int lft_sgm(const float* cost, int B, int D, int H, int W, int C, const float* slopes, int paths, float p1, float p2,
            const float* guide, float gain, const float* stack, void* scratch, float* disparity, float* confidence, int* index,
            float* aggregated, void* aif, int aif_class, void* stream);

#ifdef __cplusplus
}
#endif
#endif
