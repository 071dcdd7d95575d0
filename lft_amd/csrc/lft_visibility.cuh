// lft_visibility.cuh -- view synthesis with a per-view visibility test: lft_view_render (lft_views.cuh) whose step 3 asks, per view of
// non-zero weight, whether that view sees the surface the target pixel shows, and the warp of a disparity map to other angular
// positions that supplies the per-view maps.
//
// Inputs are those of lft_view_render, plus:
// - Dv: the per-view disparity maps, fp32 [B,A,A,H,W]. Dv[u,v] is the map at integer view position (u,v).
// - tau: a threshold, finite, >= 0, rounded once to fp32.
//
// Steps 1 (splat) and 2 (fill) are unchanged. Dt and holes carry the same bits as the plain call.
//
// Step 3 gains a test per view of non-zero weight. Use the same sy, sx, inside as now. Then:
// - Footprint. iy = floor(sy), ix = floor(sx). The footprint is (iy+a, ix+b) for a, b in {0,1}.
//   a = 1 is dropped when sy is integral. b = 1 is dropped when sx is integral. Indices are clamped into the image.
//   The footprint is the same for linear and cubic.
// - Occluded. For near = larger: some finite footprint value q = Dv[u,v,.,.] satisfies q > fl(d + tau). For near = smaller:
//   q < fl(d - tau). Non-finite q never occludes. All comparisons are fp32, so a numpy float32 restatement gives the same booleans.
// - Three classes. visible = inside and not occluded. inside. all: every view with w > 0.
// - Output. out = sum w*s / sum w over the first non-empty class in that order. Accumulate in (u,v) order with the same FMAs as
//   now. Views outside the chosen class contribute nothing. So when nothing is occluded, the bits equal lft_view_render's.
// - New output visible: uint8 [B,T,H,W], the number of views in the visible class, saturated at 255.
//
// By default Dv is made from Dr itself: splat and fill (steps 1-2) to the A x A integer positions. The hole fill already takes the
// farther neighbour, which is what a disocclusion needs.
//
//   k_view_fill        one pixel per lane over (batch element, 32 x 8 tile, target): vw_pixel and vw_fill_store of lft_views.cuh --
//                      the fill on the keys k_view_splat left, written to the maps and the holes -- with no render.
//   k_view_render_vis  k_view_render's launch shape (vw_pixel), its fill (vw_fill_store: k_view_render's vw_fill and stores) and its
//                      sample (vw_sample, the one k_view_render calls).  Two passes over the records of the
//                      target.  The first needs only Dt, the record and four dwords of Dv per view -- the footprint's dropped
//                      members repeat a kept one, so the four loads are unconditional --; it counts the visible and the inside
//                      views, which fixes the class, and keeps the visible bits of the first 64 views in a register pair.  The
//                      second loads the TAPS^2 * C colour taps of the views of the chosen class only, every load of one view
//                      unconditional behind the one per-view test; past the 64th view the test is taken again from Dv, so there
//                      is no limit on A.  No LDS, no barrier.
#pragma once
#include "lft_views.cuh"

namespace {

constexpr int kVsMask = 64;         // the views whose visible bit stays in registers between the passes

struct FillArgs {
    const uint32_t* keys;            // [B, N, H, W]
    const float* dr;                 // [B, H, W]
    float lo, hi;
    int neg, fill;
    int H, W, N, rtiles_x, rtiles;   // tiles of kRfTile x kVwRows
    float* maps;                     // [B, N, H, W]
    uint8_t* holes;                  // [B, N, H, W]
};

struct VisArgs {
    RenderArgs r;
    const float* dv;                 // [B, A*A, H, W]
    float tau;
    uint8_t* visible;                // [B, T, H, W]
};

__global__ __launch_bounds__(256) void k_view_fill(FillArgs a) {
    int b, t, y, x;
    if (!vw_pixel(a.N, a.rtiles_x, a.rtiles, a.H, a.W, b, t, y, x)) return;
    const size_t plane = (size_t)a.H * a.W, tp = ((size_t)b * a.N + t) * plane;
    vw_fill_store(a.keys + tp, a.dr + (size_t)b * plane, y, x, a.H, a.W, a.fill, a.neg, a.lo, a.hi, a.maps + tp, a.holes + tp);
}

// the two clamped indices of one axis of the footprint at the sample position s: floor(s), and floor(s) + 1 unless s is integral
__device__ __forceinline__ void vs_axis(float s, int n, int& i0, int& i1) {
    const float fl = floorf(s);
    const int i = (int)fminf(fmaxf(fl, -4.0f), (float)n + 4.0f);      // beyond the clamp both are the border pixel
    i0 = min(max(i, 0), n - 1);
    i1 = min(max(s != fl ? i + 1 : i, 0), n - 1);
}

// whether the view whose map is dvn hides the surface at disparity threshold thr from the sample position (sy, sx)
__device__ __forceinline__ bool vs_occluded(const float* dvn, float sy, float sx, int H, int W, float thr, int neg) {
    int y0, y1, x0, x1;
    vs_axis(sy, H, y0, y1);
    vs_axis(sx, W, x0, x1);
    const float q00 = dvn[(size_t)y0 * W + x0], q01 = dvn[(size_t)y0 * W + x1], q10 = dvn[(size_t)y1 * W + x0], q11 = dvn[(size_t)y1 * W + x1];
    const float inf = __builtin_inff();
    if (neg) {                                                       // non-finite values never occlude
        const float m = fminf(fminf(vw_finite(q00) ? q00 : inf, vw_finite(q01) ? q01 : inf), fminf(vw_finite(q10) ? q10 : inf, vw_finite(q11) ? q11 : inf));
        return m < thr;
    }
    const float m = fmaxf(fmaxf(vw_finite(q00) ? q00 : -inf, vw_finite(q01) ? q01 : -inf), fmaxf(vw_finite(q10) ? q10 : -inf, vw_finite(q11) ? q11 : -inf));
    return m > thr;
}

template <typename T, int C, int TAPS>
__global__ __launch_bounds__(256) void k_view_render_vis(VisArgs va) {
#pragma clang fp contract(off)
    const RenderArgs& a = va.r;
    int b, t, y, x;
    if (!vw_pixel(a.D, a.rtiles_x, a.rtiles, a.H, a.W, b, t, y, x)) return;          // no barrier below
    const size_t plane = (size_t)a.H * a.W, tp = ((size_t)b * a.D + t) * plane, o = tp + (size_t)y * a.W + x;
    const float d = vw_fill_store(a.keys + tp, a.dr + (size_t)b * plane, y, x, a.H, a.W, a.fill, a.neg, a.lo, a.hi, a.dt + tp, a.holes + tp);

    // ---- first pass: the classes
    const int nv = a.A * a.A;
    const int* recs = a.table + (size_t)t * nv * kVwRec;
    const float* dvb = va.dv + (size_t)b * nv * plane;
    const float fy = (float)y, fx = (float)x, ymax = (float)(a.H - 1), xmax = (float)(a.W - 1);
    const float thr = a.neg ? d - va.tau : d + va.tau;
    unsigned long long seen = 0ull;                                  // bit n: view n < kVsMask is visible
    int n_vis = 0, n_in = 0;
    for (int n = 0; n < nv; ++n) {
        if (recs[n * kVwRec + 3]) continue;                          // the same for every lane
        const float* rf = reinterpret_cast<const float*>(recs + n * kVwRec);
        const float sy = fy + d * rf[0], sx = fx + d * rf[1];
        const bool inside = sy >= 0.0f && sy <= ymax && sx >= 0.0f && sx <= xmax;
        const bool occluded = vs_occluded(dvb + (size_t)n * plane, sy, sx, a.H, a.W, thr, a.neg);        // loaded whether inside or not
        const bool vis = inside && !occluded;
        n_in += inside ? 1 : 0;
        n_vis += vis ? 1 : 0;
        if (n < kVsMask) seen |= (unsigned long long)(vis ? 1 : 0) << n;
    }
    va.visible[o] = (uint8_t)min(n_vis, 255);
    const int cls = n_vis ? 0 : n_in ? 1 : 2;                        // visible, inside, all

    // ---- second pass: the render over the chosen class
    const T* lfb = static_cast<const T*>(a.lf) + b * a.st[0];
    float num[C], den = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) num[c] = 0.0f;
    for (int n = 0; n < nv; ++n) {
        if (recs[n * kVwRec + 3]) continue;
        const float* rf = reinterpret_cast<const float*>(recs + n * kVwRec);
        const float w = rf[2];
        const float sy = fy + d * rf[0], sx = fx + d * rf[1];
        bool member = true;
        if (cls == 1) member = sy >= 0.0f && sy <= ymax && sx >= 0.0f && sx <= xmax;
        if (cls == 0) {
            if (n < kVsMask) member = (seen >> n) & 1ull;
            else member = sy >= 0.0f && sy <= ymax && sx >= 0.0f && sx <= xmax && !vs_occluded(dvb + (size_t)n * plane, sy, sx, a.H, a.W, thr, a.neg);
        }
        if (!member) continue;
        float s[C];
        vw_sample<T, C, TAPS>(a, lfb, n, sy, sx, s);
        den = den + w;
#pragma unroll
        for (int c = 0; c < C; ++c) num[c] = __fmaf_rn(w, s[c], num[c]);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float v = num[c] / den;
        if (a.out_f32) static_cast<float*>(a.out)[o * C + c] = v;
        else static_cast<uint8_t*>(a.out)[o * C + c] = rf_byte(v);
    }
}

// the instantiation for an input type, channel count (1 .. 4) and tap count (2, 4)
template <typename T>
inline void (*render_vis_kernel(int C, int taps))(VisArgs) {
    static void (*const k[4][2])(VisArgs) = {{k_view_render_vis<T, 1, 2>, k_view_render_vis<T, 1, 4>},
                                             {k_view_render_vis<T, 2, 2>, k_view_render_vis<T, 2, 4>},
                                             {k_view_render_vis<T, 3, 2>, k_view_render_vis<T, 3, 4>},
                                             {k_view_render_vis<T, 4, 2>, k_view_render_vis<T, 4, 4>}};
    return k[C - 1][taps == 4 ? 1 : 0];
}

}  // namespace
