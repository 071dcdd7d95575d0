/* lft_hip_views.h -- view synthesis entry points of liblft_hip.so: views at fractional angular positions from the A x A views of
 * a light field and a disparity map.  Added beside ABI 5; lft_version unchanged.  The conventions are those of lft_hip.h (plain
 * pointers, DEVICE unless noted, enqueue only, 0 / LFT_ERR_* / hipError_t, lft_last_error); a library that lacks these symbols is
 * an older build of the same ABI.
 *
 * Inputs:
 * - B light fields of A x A views, H x W pixels, C <= 4 channels, read in place through refocus's six element strides.
 * - uint8 enters as x/255, float32 as stored.
 * - A disparity map Dr, fp32 [B,H,W], given at the angular position reference = (ur,vr).
 * - d_range = (lo,hi), lo <= hi, rounded once to fp32. Finite Dr is clamped into it before use; non-finite pixels are skipped.
 * - T targets (ut,vt) in view-index units, fp64 on the host.
 * - The sign convention is refocus's: a point seen at y in view u is seen at y + d*(u'-u) in view u'.
 *
 * All coordinate arithmetic is fp32, one rounded operation per step, with the compiler's contraction off as in k_refocus, so a
 * numpy float32 restatement reproduces it bit for bit.
 *
 * 1. Splat. Du = fl32(ut-ur), Dv likewise. Each source pixel (y,x) with clamped d lands at py = fl(y + fl(d*Du)),
 *    px = fl(x + fl(d*Dv)) and covers (floor(py)+a, floor(px)+b) for a,b in {0,1}; a=1 is dropped when py is integral, b=1 when px
 *    is integral; pixels outside the image are dropped. Dt0[y',x'] is the nearest d among the coverers: the max for
 *    near = larger, the min for near = smaller. The result does not depend on arrival order.
 *    reach = ceil(max(|lo|,|hi|) * max(|Du|,|Dv|)) + 1; reach > 64 is refused.
 * 2. Fill. A hole is a pixel with no coverer. It takes the farther (near = larger: the smaller) of the nearest non-hole Dt0 values
 *    to its left and right in the row, each searched up to `fill` pixels (0..64); one side alone gives that one; neither: the same
 *    search up and down the column; nothing there either: clamped Dr[y,x], or the far end of d_range if that pixel is non-finite.
 *    Only pre-fill values are read. holes = 1 for filled pixels.
 * 3. Render. One 16-byte record per (target, view): {du = fl32(u-ut), dv, w, skip}, w >= 0 summing to 1 per target, computed in
 *    fp64 on the host and rounded once. For d = Dt[y,x] and each view with w > 0, in (u,v) order: sy = fl(y + fl(d*du)), sx
 *    likewise; the view is inside iff 0 <= sy <= H-1 and 0 <= sx <= W-1; iy = floor(sy), f = sy - iy, which is exact.
 *    linear: taps iy, iy+1 with weights fl(1-f), f. cubic: taps iy-1 .. iy+2 with Keys' kernel (a = -0.5) at f+1, f, 1-f, 2-f,
 *    evaluated in fp32 (in the factored forms 1 - t^2 (2.5 - 1.5 t) and -0.5 t (1 - t)^2). Taps are clamped (replicate).
 *    Rows are filtered first, then columns, with explicit FMAs as in k_refocus.
 *    out = (sum_inside w*s) / (sum_inside w); if no view is inside, the same quotient over all views with w > 0.
 *    Output is fp32 or uint8 by refocus's rule: clip, *255, round half to even.
 *
 * At an integer target whose only view of non-zero weight is that view, the output equals the input view bit for bit.
 *
 * lf, lf_class, B, A, H, W, C, strides: as for lft_refocus (H, W <= 2^24: pixel coordinates are fp32).
 * disparity: Dr.  deltas: DEVICE array of T pairs (Du, Dv), fp32.  max_delta: HOST value, the largest |Du|, |Dv| of the array,
 *     from which the reach is taken (a smaller value than the truth loses coverers, it reads nothing out of bounds).
 * records: DEVICE array of T * A*A lft_view_record, target-major, views in (u, v) order; skip marks a view of weight 0, which is
 *     never read.  taps: 2 (linear) or 4 (cubic).  near: LFT_VIEW_NEAR_LARGER or LFT_VIEW_NEAR_SMALLER.  fill: 0 .. 64.
 * scratch: DEVICE, 4-byte aligned, lft_view_render_scratch_bytes(B, T, H, W) bytes: the pre-fill map.  Unspecified afterwards.
 * views: [B, T, H, W, C] of views_class (LFT_LF_FLOAT32 the quotient itself, LFT_LF_UINT8 clipped to [0, 1], * 255, rounded half
 *     to even).  target_disparity: fp32 [B, T, H, W], Dt after the fill.  holes: uint8 [B, T, H, W].
 * lft_view_render only enqueues on `stream` (two kernels; graph-capturable), allocates nothing, and refuses with LFT_ERR_ARG /
 * LFT_ERR_SHAPE and a message starting "lft_view_render:" before anything is launched: lft_refocus's rules with T in the place of
 * the slope count, taps not 2 or 4, fill outside 0 .. 64, lo > hi or a non-finite end, a negative or non-finite max_delta, a reach
 * above 64 (LFT_ERR_SHAPE), an unknown `near`, a null disparity, deltas, records, scratch or output with a non-empty shape (B, H or
 * W == 0: no work, 0), a misaligned scratch. */
#ifndef LFT_HIP_VIEWS_H
#define LFT_HIP_VIEWS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LFT_VIEW_NEAR_LARGER 0
#define LFT_VIEW_NEAR_SMALLER 1
#define LFT_VIEW_MAX_REACH 64
#define LFT_VIEW_MAX_FILL 64
typedef struct { float du, dv, w; int skip; } lft_view_record;   /* 16 bytes */
int lft_view_render_scratch_bytes(int B, int T, int H, int W, size_t* out_bytes);
int lft_view_render(const void* lf, int lf_class, int B, int A, int H, int W, int C, const long long* strides, const float* disparity,
                    const float* deltas, float max_delta, const void* records, int T, int taps, float lo, float hi, int near, int fill,
                    void* scratch, void* views, int views_class, float* target_disparity, unsigned char* holes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
