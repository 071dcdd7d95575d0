/* lft_hip_aif.h -- the all-in-focus image from the winning partial aperture, an entry point of liblft_hip.so.
 * Added beside ABI 5; lft_version unchanged.  The conventions are those of lft_hip.h (plain pointers, DEVICE unless noted, enqueue
 * only, 0 / LFT_ERR_* / hipError_t, lft_last_error); a library that lacks this symbol is an older build of the same ABI.
 *
 * lft_disparity_occ's image is gathered from m, the mean over all views, which next to a foreground edge mixes the background
 * with the foreground the far-side views see.  lft_aif_at renders the mean of the subset that won, at the slope that won.
 *
 * Inputs.
 * - The light field, layout classes, six strides, refocus table [D, A*A] of lft_refocus_record, taps in {1, 2, 4} and the centre
 *   are those of lft_refocus.
 * - subsets: DEVICE fp32 [P, A*A], the rows b_p of lft_disparity_occ. 0 <= P <= LFT_OCC_MAX_SUBSETS. subsets is NULL iff P = 0.
 * - index: int32 [B, H, W]. A value outside 0 .. D-1 is clamped into it, as in lft_occ_gather.
 * - subset: NULL, or uint8 [B, H, W]. 0 means the whole aperture. p >= 1 means row p-1 of subsets. NULL and any id above P count
 *   as 0.
 *
 * Output aif[b, y, x, c], fp32 or uint8 by rf_byte (aif_class: LFT_LF_FLOAT32, the unclipped sum, or LFT_LF_UINT8: clip to
 * [0, 1], * 255, round half to even).
 * - Let k be the clamped index and p the id of the pixel.
 * - Over the views n in (u, v) order, each view has a weight and a membership. For p = 0 the weight is w_n = a of record (k, n),
 *   and the view is skipped iff the record's skip is set. For p >= 1 the weight is w_n = b_p[n], and the view is skipped iff
 *   b_p[n] == 0 or the record's skip is set.
 * - The sample s is refocus's sample from record (k, n). It uses offsets oy, ox and clamped taps. The row pass over wy comes
 *   first, then the column pass over wx. Every step after a sum's first product is one explicit FMA, with contraction off.
 * - acc = fma(w_n, s, acc) from acc = 0.
 *
 * Consequences.
 * - p = 0: the bits of lft_refocus's stack (fp32 and uint8) at k.
 * - p >= 1: the bits of lft_refocus run with a table whose a / skip columns are b_p / b_p == 0, at k.
 * - A pixel's bits must not depend on the tile, on the launch shape, on its neighbours' k or p, or on which code path served it.
 *
 * It only enqueues on `stream` (k_aif_at, one launch; graph-capturable), allocates nothing and needs no scratch, and refuses with
 * LFT_ERR_ARG / LFT_ERR_SHAPE and a message starting "lft_aif_at:" before anything is launched: every rule of lft_refocus, in its
 * order and with its words (aif and aif_class in the place of out and out_class; D < 1 among them); then P outside
 * 0 .. LFT_OCC_MAX_SUBSETS, and subsets null with P > 0 or non-null with P = 0 (both judged for empty shapes too); then, for a
 * non-empty shape, a null index or aif, and images beyond 2^31 blocks of 32 x 8 pixels (LFT_ERR_SHAPE).  B, H or W == 0: no
 * work, 0. */
#ifndef LFT_HIP_AIF_H
#define LFT_HIP_AIF_H

#include "lft_hip_occlusion.h"      /* LFT_OCC_MAX_SUBSETS */

#ifdef __cplusplus
extern "C" {
#endif

int lft_aif_at(const void* lf, int lf_class, int B, int A, int H, int W, int C, const long long* strides, const void* table, int D,
               const float* subsets, int P, const int* index, const unsigned char* subset, int taps, void* aif, int aif_class, void* stream);

#ifdef __cplusplus
}
#endif
#endif
