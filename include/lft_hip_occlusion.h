/* lft_hip_occlusion.h -- the disparity sweep with an occlusion-aware cost from partial apertures, entry points of liblft_hip.so.
 * Added beside ABI 5; lft_version unchanged.  The conventions are those of lft_hip.h (plain pointers, DEVICE unless noted, enqueue
 * only, 0 / LFT_ERR_* / hipError_t, lft_last_error); a library that lacks these symbols is an older build of the same ABI.
 *
 * The inputs, the table, the samples s, the aperture a (fp64 on the host, sum 1) and the centre (cu, cv) are those of
 * lft_disparity. Everything below is fp32, one rounded operation per step, with contraction off.
 *
 * Subsets (host only). Let du = u - cu and dv = v - cv in fp64.
 * - "halves": the four subsets du <= 0, du >= 0, dv <= 0, dv >= 0.
 * - "quadrants": (<=,<=), (<=,>=), (>=,<=), (>=,>=) in (du, dv).
 * - A boolean array [P, A, A] with 1 <= P <= 4.
 * - A subset is kept iff at least min_views of its views have a > 0. min_views is an integer >= 2, default 2. One view has
 *   variance 0 at every slope and would win everywhere.
 * - Dropped subsets never reach the kernel. Subset ids in the outputs are positions in the kept list.
 * - If no subset is kept, raise LftError.
 * - For a kept subset p: W_p = sum_{p} a in fp64. The row b_p[u,v] = fl32(a/W_p) for members and 0 for the rest.
 * - The table [P', A*A] fp32, views in (u, v) order, is the only place these weights are rounded.
 *
 * Moments.
 * - The full aperture is unchanged: m, q, V_full exactly as today, the same FMAs in the same order. m stays refocus's stack bit
 *   for bit, and aif is still gathered from it.
 * - Per kept subset, over its members in (u, v) order:
 *   - m_p = fma(b_p, s, m_p)
 *   - q_p = fma(fl(b_p*s), s, q_p)
 *   - V_p = sum_c max(q_p - fl(m_p*m_p), 0), with c = 0 first.
 *
 * Combination.
 * - t = min_p V_p and U = fl(beta*t).
 * - V = min(V_full, U).
 * - choice = 0 if V_full <= U, else the lowest p (1-based) with V_p = t.
 * - beta is the margin: finite, >= 1, rounded once to fp32. A subset wins only where it is beta times better than the whole
 *   aperture.
 *
 * After that. Steps 3 to 7 of lft_disparity run word for word on this V, through the existing k_disparity_pick unchanged.
 *
 * New outputs.
 * - subset: uint8 [B, H, W], equal to choice at (k*, y, x).
 * - Optionally the whole choice volume, uint8 [B, D, H, W].
 * - Read together with index, subset is an occlusion-edge map: 0 where all views agree.
 *
 * No result may depend on the tile, the launch shape or the arrival order.
 *
 * lft_disparity_occ takes lft_disparity's arguments, each with lft_disparity's meaning, and
 *   subsets: DEVICE fp32 [P, A*A], the rows b_p of the kept subsets; a view is a member of p iff its entry is not 0.
 *   P: the kept subsets, 1 .. LFT_OCC_MAX_SUBSETS.  beta: the margin.
 *   subset: NULL, or uint8 [B, H, W].  choice: NULL, or uint8 [B, D, H, W].
 *   scratch: DEVICE, 4-byte aligned, lft_disparity_occ_scratch_bytes(B, D, H, W, C, flags) bytes (flags as for
 *   lft_disparity_scratch_bytes: LFT_DISPARITY_AIF when aif is given): lft_disparity's volumes and one byte per pixel and slope
 *   for the choice volume when the caller keeps none.  Unspecified afterwards.
 * It only enqueues on `stream` (k_sweep_cost_occ, k_disparity_pick and, with subset, k_occ_gather; graph-capturable), allocates
 * nothing, and refuses with LFT_ERR_ARG / LFT_ERR_SHAPE and a message starting "lft_disparity_occ:" before anything is launched:
 * every rule of lft_disparity, in its order; then P outside 1 .. 4 and a beta that is not finite or < 1 (judged for empty shapes
 * too); a null subsets table counts among the null pointers (B, H or W == 0: no work, 0).
 *
 * lft_occ_gather: subset[b, y, x] = choice[b, index[b, y, x], y, x] for any index map, such as lft_sgm's; an index outside
 * 0 .. D-1 is clamped into it.  It only enqueues (k_occ_gather), and refuses with a message starting "lft_occ_gather:" D < 1, a
 * negative size (LFT_ERR_SHAPE), maps beyond 2^31 blocks of 256 pixels (LFT_ERR_SHAPE) and, for a non-empty shape, a null
 * pointer. */
#ifndef LFT_HIP_OCCLUSION_H
#define LFT_HIP_OCCLUSION_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LFT_OCC_MAX_SUBSETS 4
int lft_disparity_occ_scratch_bytes(int B, int D, int H, int W, int C, int flags, size_t* out_bytes);
int lft_disparity_occ(const void* lf, int lf_class, int B, int A, int H, int W, int C, const long long* strides, const void* table,
                      const float* subsets, int P, float beta, const float* slopes, int D, int taps, int radius, void* scratch,
                      float* disparity, float* confidence, int* index, unsigned char* subset, unsigned char* choice, float* cost,
                      void* aif, int aif_class, void* stream);
int lft_occ_gather(const int* index, const unsigned char* choice, int B, int D, int H, int W, unsigned char* subset, void* stream);

#ifdef __cplusplus
}
#endif
#endif
