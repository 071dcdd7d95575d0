/* lft_hip_visibility.h -- view synthesis with a per-view visibility test, entry points of liblft_hip.so: lft_view_render
 * (lft_hip_views.h) whose render asks, per view of non-zero weight, whether that view sees the surface the target pixel shows, and
 * the warp of a disparity map to other angular positions that supplies the per-view maps.  Added beside ABI 5; lft_version
 * unchanged.  The conventions are those of lft_hip.h (plain pointers, DEVICE unless noted, enqueue only, 0 / LFT_ERR_* /
 * hipError_t, lft_last_error); a library that lacks these symbols is an older build of the same ABI.
 *
 * Inputs are those of lft_view_render, plus:
 * - Dv: the per-view disparity maps, fp32 [B,A,A,H,W]. Dv[u,v] is the map at integer view position (u,v).
 * - tau: a threshold, finite, >= 0, rounded once to fp32.
 *
 * Steps 1 (splat) and 2 (fill) are unchanged. Dt and holes carry the same bits as the plain call.
 *
 * Step 3 gains a test per view of non-zero weight. Use the same sy, sx, inside as now. Then:
 * - Footprint. iy = floor(sy), ix = floor(sx). The footprint is (iy+a, ix+b) for a, b in {0,1}.
 *   a = 1 is dropped when sy is integral. b = 1 is dropped when sx is integral. Indices are clamped into the image.
 *   The footprint is the same for linear and cubic.
 * - Occluded. For near = larger: some finite footprint value q = Dv[u,v,.,.] satisfies q > fl(d + tau). For near = smaller:
 *   q < fl(d - tau). Non-finite q never occludes. All comparisons are fp32, so a numpy float32 restatement gives the same booleans.
 * - Three classes. visible = inside and not occluded. inside. all: every view with w > 0.
 * - Output. out = sum w*s / sum w over the first non-empty class in that order. Accumulate in (u,v) order with the same FMAs as
 *   now. Views outside the chosen class contribute nothing. So when nothing is occluded, the bits equal lft_view_render's.
 * - New output visible: uint8 [B,T,H,W], the number of views in the visible class, saturated at 255.
 *
 * By default Dv is made from Dr itself: splat and fill (steps 1-2) to the A x A integer positions. The hole fill already takes the
 * farther neighbour, which is what a disocclusion needs.  A caller may pass maps of their own instead.
 *
 * lft_view_warp_disparity: steps 1 and 2 alone, for N positions.  disparity: Dr, fp32 [B,H,W].  deltas: DEVICE array of N pairs
 *     (Du, Dv) = position - reference, fp32.  max_delta, lo, hi, near, fill: as for lft_view_render.  scratch: DEVICE, 4-byte
 *     aligned, lft_view_visible_scratch_bytes(B, N, H, W) bytes, unspecified afterwards.  maps: fp32 [B,N,H,W].  holes: uint8
 *     [B,N,H,W].  Two kernels (k_view_splat, k_view_fill).  With the A*A deltas (u - ur, v - vr) in (u,v) order, maps is Dv.
 * lft_view_render_visible: lft_view_render's parameters with the same meaning, and view_disparity: Dv; tau; visible: the new
 *     output.  scratch: lft_view_visible_scratch_bytes(B, T, H, W) bytes.  Two kernels (k_view_splat, k_view_render_vis).
 * Both only enqueue on `stream` (graph-capturable), allocate nothing, and refuse with LFT_ERR_ARG / LFT_ERR_SHAPE and a message
 * starting with the function's name before anything is launched: lft_view_render's refusals (for the warp those that concern its
 * own parameters, with N < 1 in the place of the targets), plus a null view_disparity, visible or maps with a non-empty shape and a
 * negative or non-finite tau.  B, H or W == 0: no work, 0. */
#ifndef LFT_HIP_VISIBILITY_H
#define LFT_HIP_VISIBILITY_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LFT_VIS_MASK_VIEWS 64     /* the views whose visible bit k_view_render_vis keeps in registers; later ones are tested twice */
int lft_view_visible_scratch_bytes(int B, int N, int H, int W, size_t* out_bytes);
int lft_view_warp_disparity(const float* disparity, int B, int H, int W, const float* deltas, float max_delta, int N, float lo, float hi,
                            int near, int fill, void* scratch, float* maps, unsigned char* holes, void* stream);
int lft_view_render_visible(const void* lf, int lf_class, int B, int A, int H, int W, int C, const long long* strides, const float* disparity,
                            const float* view_disparity, float tau, const float* deltas, float max_delta, const void* records, int T, int taps,
                            float lo, float hi, int near, int fill, void* scratch, void* views, int views_class, float* target_disparity,
                            unsigned char* holes, unsigned char* visible, void* stream);

#ifdef __cplusplus
}
#endif
#endif
