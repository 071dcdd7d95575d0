/* lft_hip_shear.h -- per-patch disparity compensation by integer shear, entry points of liblft_hip.so.
 * Added beside ABI 5; lft_version unchanged.  The conventions are those of lft_hip.h (plain pointers, DEVICE unless noted, enqueue
 * only, 0 / LFT_ERR_* / hipError_t, lft_last_error); a library that lacks these symbols is an older build of the same ABI.
 *
 * LFT's angular Transformer attends across the A x A views at the same pixel, which only works while a scene point stays within a
 * pixel or so across the views.  A shear by a whole number k of LR pixels per view step is lossless: view (u, v) of a patch is
 * cut at an offset of k*(u-u0), k*(v-u0) pixels, the network sees a light field whose residual disparity is d - k, and the SR
 * patch is put back at s*k*(u-u0), again a whole number of pixels.  No pixel is interpolated on either side.
 *
 * Let bdr = (patch - stride)/2, u0 = A / 2, du = u - u0 and dv = v - u0 (whole numbers for even A too), R = max(u0, A-1-u0), and
 * kmax = LFT_SHEAR_MAX if R = 0, else min(LFT_SHEAR_MAX, bdr / R).  Every kernel clamps k_n into [-kmax, kmax] itself: a device
 * array can hold anything, and divide and integrate must stay inverse to each other.  The sign is the disparity module's: a point
 * seen at y in view u is seen at y + d*(u'-u) in view u', so k = d aligns the views.
 *
 * Sheared divide.  Patch n = ku*nv + kv, view (u, v), pixel (y, x) of the patch.  ey = ku*stride + y, and ex likewise.  The value
 * is 0 where ey >= h0 + 2*bdr or ex >= w0 + 2*bdr: today's test, on the unsheared coordinates.  Elsewhere the value is
 * scene[u*h0 + fold(ey - bdr + k_n*du, h0), v*w0 + fold(ex - bdr + k_n*dv, w0)].  fold(i, n): m = i mod 2n (non-negative), then m
 * if m < n, else 2n-1-m.  This is reflect_idx continued to any integer; on [-n, 2n-1] the two agree.
 *
 * Sheared integrate.  SR view (u, v), SR pixel (Y, X).  ku = Y / (stride*s), i = Y - ku*stride*s, and kv, j likewise;
 * n = ku*nv + kv, as today.  The value is the SR patch n, view (u, v), at row bdr*s + i - s*k_n*du and column
 * bdr*s + j - s*k_n*dv.  With the clamp those lie inside the patch, and they never touch a zero-filled pixel.
 *
 * Vote.  index: int32 [B, H, W] and confidence: fp32 [B, H, W] (lft_disparity's maps); slopes: D whole-number slopes, DEVICE int32
 * [D], 1 <= D <= 2*LFT_SHEAR_MAX+1.  count[b, j] is the number of pixels with margin <= y < H-margin, margin <= x < W-margin,
 * clamped index equal to j, and confidence finite and >= min_confidence.  shear[b] = slopes[j*], where j* has the largest count.
 * On a tie the smallest |slope| wins, then the smaller slope.  If every count is 0 the result is 0.  Counts are integers, so arrival
 * order cannot matter.
 *
 * shear: DEVICE int32, one value per patch ([numU*numV] of lft_scene_counts).  counts: DEVICE int32 [B, D]; whatever it held is
 * gone, afterwards it holds the vote.  With every k_n = 0 the two tiling calls give the bits of lft_scene_divide and
 * lft_scene_integrate.  Byte contract of the two gathers: the plain pair's (every output element written once, one element read
 * for each), plus 4 bytes per patch.
 *
 * All three only enqueue on `stream` (k_scene_divide_shear, k_scene_integrate_shear, k_shear_vote: one launch each,
 * graph-capturable), allocate nothing and never synchronise.  Refused before anything is launched, with a message that starts with
 * the function's name -- LFT_ERR_ARG: a null pointer, A < 1, s < 1, a min_confidence that is not finite.  LFT_ERR_SHAPE: every
 * tiling lft_scene_divide refuses, with its words; a patch - stride that is odd (the border is then not the same on both sides
 * and the last row of patches is missing); each call's own launch shape (divide: A*patch or numU*numV above 65535;
 * integrate: A*h0*s above 65535), and sizes an int cannot index; negative B, H or W below 1; D outside
 * 1 .. 2*LFT_SHEAR_MAX+1; margin < 0 or 2*margin >= min(H, W).  B = 0 returns 0 and launches nothing. */
#ifndef LFT_HIP_SHEAR_H
#define LFT_HIP_SHEAR_H

#ifdef __cplusplus
extern "C" {
#endif

#define LFT_SHEAR_MAX 16

int lft_scene_divide_shear(const float* scene, const int* shear, float* patches, int A, int h0, int w0, int patch, int stride, void* stream);
int lft_scene_integrate_shear(const float* sr_patches, const int* shear, float* sr_scene, int A, int h0, int w0, int patch, int stride, int s, void* stream);
int lft_shear_vote(const int* index, const float* confidence, const int* slopes, int B, int H, int W, int D, int margin, float min_confidence, int* counts, int* shear, void* stream);

#ifdef __cplusplus
}
#endif
#endif
