/* lft_hip_field.h -- angular tiling: every view of a U x V light field through a network built for A x A views, entry points of
 * liblft_hip.so.  Added beside ABI 5; lft_version unchanged.  The conventions are those of lft_hip.h (plain pointers, DEVICE unless
 * noted, enqueue only, 0 / LFT_ERR_* / hipError_t, lft_last_error); a library that lacks these symbols is an older build of the same
 * ABI.
 *
 * Field mosaic.  A field mosaic is fp32 [U*h0, V*w0].  View (p, q) occupies rows p*h0 ... and columns q*w0 ...: the scene mosaic of
 * lft_scene_divide with two angular sizes.
 *
 * Windows along one axis of L views, with 1 <= astride <= A <= L.
 *   - m(L) = 1 if L = A, else ceil((L-A)/astride) + 1.
 *   - The origins are o_i = min(i*astride, L-A).  They are strictly increasing.  The last origin is clamped so the last view is
 *     covered.  Consecutive origins are at most A apart, so every view is covered.
 *   - mu = m(U) and mv = m(V).  Window w = wu*mv + wv has origin (o_wu, o_wv).
 *   - N = nu*nv comes from lft_scene_counts.  Batch element b = w*N + n.
 *   - A view lies in at most ceil(A/astride) + 1 windows per axis.  The +1 comes from the clamped last window: A = 2, astride = 2,
 *     L = 5 has origins 0, 2, 3, and view 3 is in two windows.
 *
 * Divide.  [U*h0, V*w0] -> [mu*mv*N, 1, A*patch, A*patch].  Element b is exactly what lft_scene_divide gives for patch n of the A x A
 * sub-mosaic of views (o_wu+u, o_wv+v).  With a non-null shear (int32 [mu*mv*N], one value per batch element, clamped to +-kmax of
 * lft_hip_shear.h) it is exactly what lft_scene_divide_shear gives with k = shear[b].  No sub-mosaic is materialised.
 *
 * Integrate.  [mu*mv*N, 1, A*pz, A*pz] -> [U*h0*s, V*w0*s], with pz = patch*s.
 *   - g is the angular table: fp32 [A], strictly positive.  win is the spatial table: either null, which means the crop, or fp32 [pz]
 *     as in lft_hip_blend.h.
 *   - The terms of output view (p, q), pixel (Y, X) are visited in ascending wu, then wv, then ku, then kv.
 *   - A window (wu, wv) takes part when 0 <= u = p - o_wu < A and 0 <= v = q - o_wv < A.  ga = g[u]*g[v], one rounded product.
 *   - With win null there is one term per window.  It is the element lft_scene_integrate would read for that window's sub-scene, or
 *     lft_scene_integrate_shear when sheared.  Its weight is wt = ga.
 *   - With win set there is one term for every (ku, kv) that lft_scene_integrate_blend counts as contributing for that window's
 *     sub-scene: the same test and the same sk_b = s*clamp(shear[b]).  Its weight is wt = ga*(win[a]*win[b]), each product rounded
 *     once.
 *   - num = num + wt*x, den = den + wt, out = num/den.  Every operation is one rounded fp32 operation, nothing is contracted, and the
 *     quotient is correctly rounded: a pixel's bits do not depend on the launch shape.  Every pixel has at least one term.
 *   - With U = V = A there is one window; with g flat that gives the bits of lft_scene_integrate, lft_scene_integrate_shear and
 *     lft_scene_integrate_blend.  With g flat and the crop, the field is the fp32 sum, in window order, of the per-window
 *     lft_scene_integrate results, divided by the fp32 count.
 *
 * field: the LR field mosaic [U*h0, V*w0]; shear: null, or int32 [mu*mv*N]; patches: [mu*mv*N, A*patch, A*patch]; sr_patches:
 * [mu*mv*N, A*pz, A*pz]; window: null, or fp32 [pz]; angular: fp32 [A]; sr_field: [U*h0*s, V*w0*s].  Byte contract of the integrate:
 * every SR patch element that shows a scene pixel read once, every field element written once, plus the tables and 4 bytes per patch.
 * Memory: mu*mv*N*(A*pz)^2*4 bytes of SR patches are live at once (for 9 x 9 views of 512 x 512, A = 5, 2x, patch 32 / stride 16: 1.7 GB
 * in the 4 windows of astride 4, 3.8 GB in the 9 windows of astride 2).
 *
 * lft_field_counts is host only.  The other two only enqueue on `stream` (k_field_divide, k_field_integrate: one launch each,
 * graph-capturable), allocate nothing and never synchronise.  Refused before anything is launched, with a message that starts with the
 * function's name -- LFT_ERR_ARG: a null pointer (shear and window may be null), A < 1, a scale factor other than 2 or 4.
 * LFT_ERR_SHAPE: U or V below A or above LFT_FIELD_MAX_VIEWS; astride < 1 or > A; every tiling the corresponding existing entry point
 * refuses, in its words (an odd patch - stride whenever shear or window is set among them); rows above 65535 (the launch's), sizes
 * an int cannot index, and a window of more than LFT_BLEND_MAX_PZ entries. */
#ifndef LFT_HIP_FIELD_H
#define LFT_HIP_FIELD_H

#ifdef __cplusplus
extern "C" {
#endif

#define LFT_FIELD_MAX_VIEWS 64

int lft_field_counts(int U, int V, int A, int astride, int* mu, int* mv);
int lft_field_divide(const float* field, const int* shear, float* patches, int U, int V, int A, int astride, int h0, int w0, int patch, int stride, void* stream);
int lft_field_integrate(const float* sr_patches, const int* shear, const float* window, const float* angular, float* sr_field, int U, int V, int A, int astride, int h0, int w0, int patch, int stride, int s, void* stream);

#ifdef __cplusplus
}
#endif
#endif
