/* lft_hip_blend.h -- windowed blending of overlapping SR patches into the SR scene, entry point of liblft_hip.so.
 * Added beside ABI 5; lft_version unchanged.  The conventions are those of lft_hip.h (plain pointers, DEVICE unless noted, enqueue
 * only, 0 / LFT_ERR_* / hipError_t, lft_last_error); a library that lacks this symbol is an older build of the same ABI.
 *
 * lft_scene_integrate keeps the central stride*s square of every SR patch and drops the rest; the kept squares meet edge to edge.
 * Here every SR patch pixel that shows a scene pixel contributes to it, weighted by a separable window over the patch.
 *
 * All sizes are in SR pixels.  pz = patch*s, S = stride*s, bdr = (pz - S)/2; (nu, nv) come from lft_scene_counts; u0 = A / 2;
 * sk_n = s*clamp(shear[n], +-kmax) with the kmax of lft_hip_shear.h, or 0 where shear is null.  Pixel (a, b) of view (u, v) of SR
 * patch n = ku*nv + kv shows scene pixel
 *     Y = ku*S + a - bdr + sk_n*(u - u0),   X = kv*S + b - bdr + sk_n*(v - u0)
 * which is lft_scene_integrate_shear's map, read backwards.  The pixel contributes iff 0 <= Y < h0*s and 0 <= X < w0*s.  That drops
 * the reflected margin and everything beyond the extended view, so no zero-filled position ever contributes.
 *
 * With the window table w[0 .. pz), fp32 and strictly positive:
 *     num = sum (w[a]*w[b]) * sub[n, u, a, v, b],   den = sum w[a]*w[b],   out = num / den
 * The sum runs over the contributing patches in ascending ku, then kv.  Every operation is one rounded fp32 operation (the
 * product of the two weights, its product with the pixel, each addition; nothing is contracted), and the division is correctly
 * rounded: a pixel's bits do not depend on the launch shape.  Every pixel has at least one term: the patch lft_scene_integrate
 * reads it from contributes, since |sk_n|*reach <= bdr.  A window that is not strictly positive may leave den = 0.
 *
 * sub: the SR patches [nu*nv, A*pz, A*pz]; shear: null, or int32 [nu*nv], the shear the patches were cut with; window: fp32 [pz];
 * out: the SR scene mosaic [A*h0*s, A*w0*s].  Byte contract: every SR patch element inside a view read once, every scene element
 * written once, plus the window and 4 bytes per patch.
 *
 * The call only enqueues on `stream` (k_scene_integrate_blend: one launch, graph-capturable), allocates nothing and never
 * synchronises.  Refused before anything is launched, with a message that starts with the function's name -- LFT_ERR_ARG: a null
 * sub, window or out, A < 1, a scale factor other than 2 or 4.  LFT_ERR_SHAPE: every tiling lft_scene_divide refuses, with its words
 * (stride > patch among them); a patch - stride that is odd; A*h0*s above 65535 (the launch's rows), sizes an int cannot index, and
 * a window of more than LFT_BLEND_MAX_PZ entries. */
#ifndef LFT_HIP_BLEND_H
#define LFT_HIP_BLEND_H

#ifdef __cplusplus
extern "C" {
#endif

#define LFT_BLEND_MAX_PZ 8192

int lft_scene_integrate_blend(const float* sr_patches, const int* shear, const float* window, float* sr_scene, int A, int h0, int w0, int patch, int stride, int s, void* stream);

#ifdef __cplusplus
}
#endif
#endif
