// lft_aif.cuh -- the all-in-focus image from the winning partial aperture: the occlusion-aware sweep (lft_occlusion.cuh) finds the
// background's slope next to a foreground edge by scoring a half or a quadrant of the aperture, but its image is still gathered
// from m, the mean over all views, which mixes the background with the foreground the far-side views see.  The image below is the
// mean of the subset that won, at the slope that won: one gather pass over the views.
//
// Inputs.
// - The light field, layout classes, six strides, refocus table [D, A*A] of lft_refocus_record, taps in {1, 2, 4} and the centre
//   are those of lft_refocus.
// - subsets: DEVICE fp32 [P, A*A], the rows b_p of lft_disparity_occ. 0 <= P <= LFT_OCC_MAX_SUBSETS. subsets is NULL iff P = 0.
// - index: int32 [B, H, W]. A value outside 0 .. D-1 is clamped into it, as in lft_occ_gather.
// - subset: NULL, or uint8 [B, H, W]. 0 means the whole aperture. p >= 1 means row p-1 of subsets. NULL and any id above P count
//   as 0.
//
// Output aif[b, y, x, c], fp32 or uint8 by rf_byte.
// - Let k be the clamped index and p the id of the pixel.
// - Over the views n in (u, v) order, each view has a weight and a membership. For p = 0 the weight is w_n = a of record (k, n),
//   and the view is skipped iff the record's skip is set. For p >= 1 the weight is w_n = b_p[n], and the view is skipped iff
//   b_p[n] == 0 or the record's skip is set.
// - The sample s is refocus's sample from record (k, n). It uses offsets oy, ox and clamped taps. The row pass over wy comes
//   first, then the column pass over wx. Every step after a sum's first product is one explicit FMA, with contraction off.
// - acc = fma(w_n, s, acc) from acc = 0.
//
// Consequences.
// - p = 0: the bits of lft_refocus's stack (fp32 and uint8) at k.
// - p >= 1: the bits of lft_refocus run with a table whose a / skip columns are b_p / b_p == 0, at k.
// - A pixel's bits must not depend on the tile, on the launch shape, on its neighbours' k or p, or on which code path served it.
//
//   k_aif_at  one launch; one workgroup per (batch element, 32 x 8 tile) as in k_view_render, the ids dealt XCD-aware (xcd_tile),
//             one pixel per lane, a wave two rows of 32 pixels, C accumulators in registers.  No LDS, no barrier, no scratch.  Per
//             view that is not skipped TAPS^2 * C plain loads at the lane's own offset, then aif_view: the row pass, the column pass
//             and the FMA above.  k_refocus's window pipeline does not serve here, the slope differs per pixel; the arithmetic and
//             its order are k_refocus's.
//             A record is 12 dwords per view, more than the pixel's taps.  Where every active lane of a wave holds the same
//             (k, p) -- the common case away from depth edges -- the wave reads the records and b_p through a wave-uniform
//             address (scalar loads, one per wave) and a skipped view is one scalar branch; a mixed wave reads them per lane and
//             skips under the lane mask.  Both paths are the one aif_walk with other pointers, so both give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lft_views.cuh"

namespace {

struct AifArgs {
    const void* lf;
    long long st[3];                 // element strides of (b, u, v)
    int sy, sx, sc;                  // element strides of (y, x, c): a view spans less than 2^31 elements
    int A, H, W, D, tiles_x, tiles;  // tiles: of kRfTile x kRfTile (fill_windowed); the launch uses rtiles
    const int* table;                // [D, A*A] records
    const float* subsets;            // [P, A*A] b_p, or null with P = 0
    int P;
    const int* index;                // [B, H, W]
    const uint8_t* subset;           // [B, H, W] or null
    int rtiles_x, rtiles;            // tiles of kRfTile x kVwRows
    void* out;                       // [B, H, W, C]
    int out_f32;
};

// What a lane keeps of record (k, n) and of b_p[n]: the first taps' offsets, the TAPS weights of either pass, the view's weight
// and whether it is skipped.
template <int TAPS> struct AifRec { int oy, ox; float wy[TAPS], wx[TAPS], w; bool skip; };

// Record n of the table row `recs`, with the weight and membership of the subset row bp (null: the whole aperture).  With
// wave-uniform pointers these are scalar loads and `skip` is one value for the wave.
template <int TAPS>
__device__ __forceinline__ AifRec<TAPS> aif_rec(const int* recs, const float* bp, int n) {
    const int* rec = recs + n * kRfRec;
    const float* rf = reinterpret_cast<const float*>(rec);
    AifRec<TAPS> r;
    r.oy = rec[0]; r.ox = rec[1];
#pragma unroll
    for (int k = 0; k < TAPS; ++k) { r.wy[k] = rf[2 + k]; r.wx[k] = rf[6 + k]; }
    r.w = bp ? bp[n] : rf[10];
    r.skip = rec[11] != 0 || (bp && r.w == 0.0f);
    return r;
}

// One view's term of one pixel: acc[c] = fma(w, s[c], acc[c]), s refocus's sample of the view at vb by the record r.  Per column
// tap its row pass, then its term of the column pass, as vw_sample; the taps are clamped into the view (replicate).
template <typename T, int C, int TAPS>
__device__ __forceinline__ void aif_view(const AifArgs& a, const T* vb, int y, int x, const AifRec<TAPS>& r, float (&acc)[C]) {
#pragma clang fp contract(off)
    // the first tap, kept within 8 pixels of the view: taps beyond clamp to the same pixel either way
    const int ry = (int)min(max((long long)y + r.oy, -8LL), (long long)a.H + 7);
    const int rx = (int)min(max((long long)x + r.ox, -8LL), (long long)a.W + 7);
    int oy[TAPS], ox[TAPS];
#pragma unroll
    for (int k = 0; k < TAPS; ++k) {
        oy[k] = min(max(ry + k, 0), a.H - 1) * a.sy;
        ox[k] = min(max(rx + k, 0), a.W - 1) * a.sx;
    }
    float s[C];
#pragma unroll
    for (int k = 0; k < TAPS; ++k) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float t = r.wy[0] * rf_x<T>(vb[oy[0] + ox[k] + c * a.sc]);
#pragma unroll
            for (int j = 1; j < TAPS; ++j) t = __fmaf_rn(r.wy[j], rf_x<T>(vb[oy[j] + ox[k] + c * a.sc]), t);
            s[c] = k ? __fmaf_rn(r.wx[k], t, s[c]) : r.wx[0] * t;
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = __fmaf_rn(r.w, s[c], acc[c]);
}

// The walk over the views of one pixel, written once for both paths.
template <typename T, int C, int TAPS>
__device__ __forceinline__ void aif_walk(const AifArgs& a, const T* lfb, int y, int x, const int* recs, const float* bp, float (&acc)[C]) {
    const int nv = a.A * a.A;
    for (int n = 0; n < nv; ++n) {
        const AifRec<TAPS> r = aif_rec<TAPS>(recs, bp, n);
        if (!r.skip) aif_view<T, C, TAPS>(a, lfb + (n / a.A) * a.st[1] + (n % a.A) * a.st[2], y, x, r, acc);
    }
}

template <typename T, int C, int TAPS>
__global__ __launch_bounds__(256) void k_aif_at(AifArgs a) {
    const int tid = threadIdx.x;
    const int bid = xcd_tile(blockIdx.x, gridDim.x);
    const int tile = bid % a.rtiles, b = bid / a.rtiles;
    const int y = (tile / a.rtiles_x) * kVwRows + tid / kRfTile, x = (tile % a.rtiles_x) * kRfTile + tid % kRfTile;
    if (y >= a.H || x >= a.W) return;                                // no barrier below
    const size_t o = (size_t)b * a.H * a.W + (size_t)y * a.W + x;
    const int k = min(max(a.index[o], 0), a.D - 1);
    int p = a.subset ? (int)a.subset[o] : 0;
    if (p > a.P) p = 0;

    const size_t row = (size_t)a.A * a.A;                            // records of a slope, weights of a subset
    const T* lfb = static_cast<const T*>(a.lf) + b * a.st[0];
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0f;

    const int k0 = __builtin_amdgcn_readfirstlane(k), p0 = __builtin_amdgcn_readfirstlane(p);
    if (__all(k == k0 && p == p0))       // one (k, p) for the wave: uniform addresses, and a skipped view is one scalar branch
        aif_walk<T, C, TAPS>(a, lfb, y, x, a.table + k0 * row * kRfRec, p0 ? a.subsets + (p0 - 1) * row : nullptr, acc);
    else                                 // a mixed wave: per-lane addresses, a view skipped under the lane mask
        aif_walk<T, C, TAPS>(a, lfb, y, x, a.table + k * row * kRfRec, p ? a.subsets + (p - 1) * row : nullptr, acc);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (a.out_f32) static_cast<float*>(a.out)[o * C + c] = acc[c];
        else static_cast<uint8_t*>(a.out)[o * C + c] = rf_byte(acc[c]);
    }
}

// the instantiation for an input type, channel count (1 .. 4) and tap count (1, 2, 4)
template <typename T>
inline void (*aif_kernel(int C, int taps))(AifArgs) {
    static void (*const k[4][3])(AifArgs) = {{k_aif_at<T, 1, 1>, k_aif_at<T, 1, 2>, k_aif_at<T, 1, 4>},
                                             {k_aif_at<T, 2, 1>, k_aif_at<T, 2, 2>, k_aif_at<T, 2, 4>},
                                             {k_aif_at<T, 3, 1>, k_aif_at<T, 3, 2>, k_aif_at<T, 3, 4>},
                                             {k_aif_at<T, 4, 1>, k_aif_at<T, 4, 2>, k_aif_at<T, 4, 4>}};
    return k[C - 1][taps == 4 ? 2 : taps - 1];
}

}  // namespace
