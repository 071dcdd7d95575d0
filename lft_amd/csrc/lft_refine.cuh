// lft_refine.cuh -- refinement of a selected disparity map: the cross-view consistency check (lft_disp_check), the farther-neighbour
// fill (lft_disp_fill) and the guided weighted median (lft_disp_wmedian).  Declared in include/lft_hip_refine.h.
//
// Common rules.  near is LFT_VIEW_NEAR_LARGER or LFT_VIEW_NEAR_SMALLER.  All floating-point comparisons are fp32.  Coordinates are
// fp32, one rounded operation per step, contraction off.  No result depends on tile, launch shape or arrival order.
//
// 1. Check.  Dr fp32 [B,H,W] at the reference position, Dv fp32 [B,N,H,W] at N other positions, deltas N pairs (Du, Dv) = position -
//    reference, tau >= 0.  Per pixel (y,x) with d = Dr[y,x], over the views in order n = 0..N-1:
//    - py = fl(y + fl(d*Du)), and px likewise.
//    - Footprint: (floor(py)+a, floor(px)+b) for a, b in {0,1}.  a = 1 is dropped when py is integral, b = 1 when px is integral.
//      Positions outside the image are dropped, not clamped; that is decided in fp32 before any conversion to int, so a huge or
//      non-finite py is simply outside.
//    - Let Q be the finite values Dv[n, ., .] on the footprint.  View n falls in the first class that applies:
//      agree: some q in Q has fl(d - tau) <= q <= fl(d + tau).
//      occluded: some q in Q is nearer than the band: q > fl(d + tau) for near = larger, q < fl(d - tau) for near = smaller.
//      conflict: Q is non-empty, so every q is farther than the band: the view looks through the surface the map claims.
//      unseen: Q is empty.
//    Outputs uint8 [B,H,W]: agree and conflict, the counts of those views; valid = finite(d) && agree >= min_agree && conflict <=
//    max_conflict.  A non-finite d gives 0, 0, 0.
// 2. Fill.  A pixel is good iff valid != 0 (a null valid: all) and D is finite there.  A good pixel passes through bit for bit, with
//    holes = 0.  Any other pixel takes the farther (near = larger: the smaller) of the nearest good values to its left and to its right
//    in the row, each side searched up to reach pixels; one side alone gives that one; neither: the same search up and down the
//    column.  A pixel that got a value has holes = 1.  If nothing is found, out has the bits of D and holes = 2.  Only input values
//    are read: a filled pixel never feeds another.
// 3. Weighted median.  guide uint8 [B,H,W,C], table uint16 [1024], radius r.  The window of p is every q = p + (dy,dx) with |dy|, |dx|
//    <= r that lies inside the image; positions outside are dropped.  q is a sample iff it is good.  Its weight is the integer w_q =
//    table[min(1023, sum_c |g_c(p) - g_c(q)|)].  T = sum w_q over the samples, at most 225*65535, so 2T fits 32 bits.  T = 0: out has
//    the bits of D[p] and flag = 2.  Otherwise out = min{ v : 2 * sum_{q: D[q] <= v} w_q >= T } over the sample values v, the lower
//    weighted median, and flag = 0 if p was good, else 1.  The sums are integers, so the definition has no order to fix and is
//    exact.  Values are compared as numbers: where -0 and +0 both occur, either may come back.
//
//   k_disp_check    one pixel per lane, 256 consecutive pixels of a map per workgroup.  Per view the lane reads the two deltas
//                   (wave-uniform) and the up to four footprint values of Dv at its own offset; three booleans and two counters
//                   in registers.  No LDS, no barrier.
//   k_disp_fill     one pixel per lane over (batch element, 32 x 8 tile).  A good pixel copies; any other runs vw_search of
//                   lft_views.cuh -- the search k_view_fill runs on its pre-fill keys -- on keys made on the fly from D and valid
//                   (vw_key of d, of -d for near = smaller; 0 for a pixel that is not good).  No LDS, no barrier.
//   k_disp_wmedian  one workgroup per (batch element, 32 x 16 tile of outputs), two outputs per lane.  The tile with its halo of r
//                   goes to LDS once: D as vw_key's order-preserving 32-bit keys, 0 for a pixel that is no sample or lies outside the
//                   image; the guide as one packed dword per pixel, unused channels 0, so that sum_c |dg_c| is one sum-of-absolute-
//                   differences instruction on packed bytes; the 2 KiB table beside them as dwords (12.8 KiB at r = 7).  No sort:
//                   the lower weighted median is the smallest key K with 2 * sum_{key <= K} w >= T.  A first pass over the window gives
//                   T and the smallest and largest key of non-zero weight, L and U: the answer is a sample key in [L, U].  Each further
//                   pass picks a split L <= M < U, sums the weights of the keys <= M and keeps the largest key <= M and the smallest
//                   key > M that it meets.  2 * sum >= T: the answer is <= M, so U becomes that largest key; else L becomes that
//                   smallest key.  Either way a pass removes at least one distinct value, and L == U ends it (a constant window: no
//                   pass at all).  Any split keeps the result; it only sets the number of passes.  The bit split is at the highest
//                   bit in which L and U differ (M = the common prefix, that bit 0, ones below): at most 32 passes.  The interpolating
//                   split is where half of T would fall if the weight between L and U lay evenly over the keys, computed in fp32 and
//                   clamped into [L, U - 1], so its rounding cannot reach the result.  Up to r = 3 every pass splits by bits; above,
//                   even passes interpolate and odd passes split by bits, which bounds the passes at 64 whatever the values.  The
//                   Measured (5 x 5 views of 512 x 512 x 3, the noisy two-layer scene): 0.65 ms at r = 7 and 0.118 ms at r = 3.  A first
//                   version, bits alone at every radius and a branch round the entries of no weight, took 0.95 ms and 0.067 ms: r = 7
//                   gained, r = 3 lost, and the cause of the loss was not separated.  The weights are recomputed
//                   per pass from LDS: 225 of them do not fit a lane's registers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lft_views.cuh"

namespace {

constexpr int kRnMaxViews = 128;     // the views of one check
constexpr int kRnMaxRadius = 7;      // largest window radius of the median
constexpr int kRnMaxFill = kVwMaxFill;
constexpr int kRnTable = 1024;       // entries of the weight table
constexpr int kRnTileW = 32, kRnTileH = 16;     // outputs of one workgroup of k_disp_wmedian
constexpr int kRnBitsOnly = 3;       // up to this radius k_disp_wmedian splits by bits alone

struct CheckArgs {
    const float* dr;                 // [B, H, W]
    const float* dv;                 // [B, N, H, W]
    const float* deltas;             // [N, 2]
    float tau;
    int neg, min_agree, max_conflict;
    int H, W, N, per;                // per: workgroups per map
    uint8_t* valid;                  // [B, H, W] each
    uint8_t* agree;
    uint8_t* conflict;
};

struct DispFillArgs {
    const float* d;                  // [B, H, W]
    const uint8_t* valid;            // [B, H, W] or null
    int reach, neg;
    int H, W, rtiles_x, rtiles;      // tiles of kRfTile x kVwRows
    float* out;                      // [B, H, W]
    uint8_t* holes;                  // [B, H, W]
};

struct MedianArgs {
    const float* d;                  // [B, H, W]
    const uint8_t* valid;            // [B, H, W] or null
    const uint8_t* guide;            // [B, H, W, C]
    const uint16_t* table;           // [kRnTable]
    int H, W, C, tiles_x, tiles;     // tiles of kRnTileW x kRnTileH
    float* out;                      // [B, H, W]
    uint8_t* flags;                  // [B, H, W]
};

__global__ __launch_bounds__(256) void k_disp_check(CheckArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.x / a.per;
    const size_t plane = (size_t)a.H * a.W, i = (size_t)(blockIdx.x % a.per) * 256 + threadIdx.x;
    if (i >= plane) return;                                          // no barrier below
    const int y = (int)(i / a.W), x = (int)(i % a.W);
    const size_t o = (size_t)b * plane + i;
    const float d = a.dr[o];
    if (!vw_finite(d)) {
        a.valid[o] = 0; a.agree[o] = 0; a.conflict[o] = 0;
        return;
    }
    const float lo = d - a.tau, hi = d + a.tau;
    const float fy = (float)y, fx = (float)x, ymax = (float)(a.H - 1), xmax = (float)(a.W - 1);
    const float* dvb = a.dv + (size_t)b * a.N * plane;
    int n_agree = 0, n_conflict = 0;
    for (int n = 0; n < a.N; ++n) {
        const float py = fy + d * a.deltas[2 * n], px = fx + d * a.deltas[2 * n + 1];
        const float y0 = floorf(py), x0 = floorf(px);
        const float* dvn = dvb + (size_t)n * plane;
        bool agree = false, nearer = false, any = false;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const float yy = y0 + (float)p;
            if (!((p == 0 || py != y0) && yy >= 0.0f && yy <= ymax)) continue;      // dropped, in fp32: a NaN is outside
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float xx = x0 + (float)q;
                if (!((q == 0 || px != x0) && xx >= 0.0f && xx <= xmax)) continue;
                const float v = dvn[(size_t)(int)yy * a.W + (int)xx];
                if (!vw_finite(v)) continue;
                any = true;
                agree |= v >= lo && v <= hi;
                nearer |= a.neg ? v < lo : v > hi;
            }
        }
        n_agree += agree ? 1 : 0;
        n_conflict += !agree && !nearer && any ? 1 : 0;
    }
    a.agree[o] = (uint8_t)n_agree;                                   // N <= 128
    a.conflict[o] = (uint8_t)n_conflict;
    a.valid[o] = n_agree >= a.min_agree && n_conflict <= a.max_conflict ? 1 : 0;
}

// the key of a pixel of the map at d (its plane) under the mask at valid (its plane, or null): 0 unless the pixel is good
__device__ __forceinline__ uint32_t rn_key(const float* d, const uint8_t* valid, size_t i, int neg) {
    if (valid && !valid[i]) return 0u;
    const float v = d[i];
    return vw_finite(v) ? vw_key(neg ? -v : v) : 0u;
}

__global__ __launch_bounds__(256) void k_disp_fill(DispFillArgs a) {
    int b, t, y, x;
    if (!vw_pixel(1, a.rtiles_x, a.rtiles, a.H, a.W, b, t, y, x)) return;
    const size_t plane = (size_t)a.H * a.W, o = (size_t)b * plane + (size_t)y * a.W + x;
    const float* d = a.d + (size_t)b * plane;
    const uint8_t* valid = a.valid ? a.valid + (size_t)b * plane : nullptr;
    uint32_t v = reinterpret_cast<const uint32_t*>(d)[(size_t)y * a.W + x];      // the bits, whatever they are
    int hole = 0;
    if (!rn_key(d, valid, (size_t)y * a.W + x, a.neg)) {
        const uint32_t found = vw_search([&](int yy, int xx) { return rn_key(d, valid, (size_t)yy * a.W + xx, a.neg); }, y, x, a.H, a.W, a.reach);
        hole = found ? 1 : 2;
        if (found) v = __float_as_uint(a.neg ? -vw_unkey(found) : vw_unkey(found));
    }
    reinterpret_cast<uint32_t*>(a.out)[o] = v;
    a.holes[o] = (uint8_t)hole;
}

template <int R>
__global__ __launch_bounds__(256) void k_disp_wmedian(MedianArgs a) {
    constexpr int LW = kRnTileW + 2 * R, LH = kRnTileH + 2 * R;
    __shared__ uint32_t keys[LH * LW];
    __shared__ uint32_t gd[LH * LW];
    __shared__ uint32_t tab[kRnTable / 2];
    const int tid = threadIdx.x;
    const int bid = xcd_tile(blockIdx.x, gridDim.x);
    const int tile = bid % a.tiles, b = bid / a.tiles;
    const int y0 = (tile / a.tiles_x) * kRnTileH, x0 = (tile % a.tiles_x) * kRnTileW;
    const size_t plane = (size_t)a.H * a.W;
    const float* d = a.d + (size_t)b * plane;
    const uint8_t* valid = a.valid ? a.valid + (size_t)b * plane : nullptr;
    const uint8_t* guide = a.guide + (size_t)b * plane * a.C;
    for (int i = tid; i < kRnTable / 2; i += 256) tab[i] = (uint32_t)a.table[2 * i] | ((uint32_t)a.table[2 * i + 1] << 16);
    for (int i = tid; i < LH * LW; i += 256) {
        const int y = y0 - R + i / LW, x = x0 - R + i % LW;
        uint32_t k = 0u, g = 0u;
        if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
            const size_t p = (size_t)y * a.W + x;
            k = rn_key(d, valid, p, 0);
            for (int c = 0; c < a.C; ++c) g |= (uint32_t)guide[p * a.C + c] << (8 * c);
        }
        keys[i] = k;
        gd[i] = g;
    }
    __syncthreads();

    // the weight of window entry j seen from a pixel whose packed guide is gp: 0 for an entry that is no sample
    auto weight = [&](int j, uint32_t gp, uint32_t& k) {
        k = keys[j];
        const uint32_t s = min(__builtin_amdgcn_sad_u8(gp, gd[j], 0u), (uint32_t)(kRnTable - 1));
        const uint32_t w = (tab[s >> 1] >> (16 * (s & 1))) & 0xffffu;
        return k ? w : 0u;
    };
#pragma unroll 1
    for (int half = 0; half < kRnTileW * kRnTileH / 256; ++half) {
        const int ty = half * (256 / kRnTileW) + tid / kRnTileW, tx = tid % kRnTileW;
        const int y = y0 + ty, x = x0 + tx;
        if (y >= a.H || x >= a.W) continue;                          // no barrier below
        const int c0 = (ty + R) * LW + tx + R;                       // the pixel itself; its window starts R rows and columns before
        const uint32_t gp = gd[c0], own = keys[c0];
        uint32_t T = 0u, L = 0xffffffffu, U = 0u;
        for (int dy = -R; dy <= R; ++dy)
            for (int dx = -R; dx <= R; ++dx) {
                uint32_t k;
                const uint32_t w = weight(c0 + dy * LW + dx, gp, k);
                T += w;
                if (w) { L = min(L, k); U = max(U, k); }
            }
        const size_t o = (size_t)b * plane + (size_t)y * a.W + x;
        if (T == 0u) {
            reinterpret_cast<uint32_t*>(a.out)[o] = reinterpret_cast<const uint32_t*>(d)[(size_t)y * a.W + x];      // the bits, whatever they are
            a.flags[o] = 2;
            continue;
        }
        uint32_t below = 0u, upto = T;                               // the weight of the keys < L, and of the keys <= U
#pragma unroll 1
        for (int pass = 0; L != U; ++pass) {
            uint32_t M;                                              // any L <= M < U keeps the result; the choice sets the number of passes
            if (R <= kRnBitsOnly || (pass & 1)) {
                const uint32_t low = 0x7fffffffu >> __clz(L ^ U);    // ones below the highest bit in which L and U differ
                M = (L & ~low) | low;                                // L's bit there is 0, U's is 1
            } else {                                                 // where half of T falls between L and U if the weight lay evenly over the keys
                const float share = (0.5f * (float)T - (float)below) / (float)(upto - below);
                const float at = fminf(fmaxf(share * (float)(U - L), 0.0f), 4294967040.0f);
                M = L + min((uint32_t)at, U - L - 1u);
            }
            uint32_t sum = 0u, le = 0u, gt = 0xffffffffu;
            for (int dy = -R; dy <= R; ++dy)
                for (int dx = -R; dx <= R; ++dx) {
                    uint32_t k;
                    const uint32_t w = weight(c0 + dy * LW + dx, gp, k);
                    const bool lower = k <= M;
                    sum += lower ? w : 0u;
                    le = max(le, w && lower ? k : 0u);
                    gt = min(gt, w && !lower ? k : 0xffffffffu);
                }
            if (2u * sum >= T) { U = le; upto = sum; }
            else { L = gt; below = sum; }
        }
        a.out[o] = vw_unkey(L);
        a.flags[o] = own ? 0 : 1;
    }
}

}  // namespace
