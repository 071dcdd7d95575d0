// lft_disparity.cuh -- disparity from a light field: a plane sweep over the slopes, windowed aggregation, winner-take-all.
//
// Inputs are the same as for lft_refocus:
// - B light fields of A x A views, H x W pixels, C <= 4 channels, read in place through six element strides.
// - uint8 enters as x/255, float32 as stored.
// - Slopes d_0 < d_1 < ... < d_{D-1} are strictly increasing; they need not be uniform.
// - aperture, interp (1, 2 or 4 taps) and the table are those of refocus.shift_table.
// - The sample s_k[u,v,y,x,c] = S(L[u,v,:,:,c], y + d_k(u-uc), x + d_k(v-uc)) is exactly refocus's: rows first, clamped taps,
//   weights not renormalised.
//
// The outputs are defined as follows.
//
// 1. Moments. m_k[y,x,c] = sum_{u,v} a*s, which is the refocus stack. q_k[y,x,c] = sum_{u,v} a*s^2.
// 2. Raw cost. V_k[y,x] = sum_c max(q_k - m_k^2, 0). This is the aperture-weighted variance of the views at slope d_k, summed
//    over channels.
// 3. Aggregated cost. E_k[y,x] = (2r+1)^-2 * sum_{dy,dx in [-r,r]} V_k[clamp(y+dy,0,H-1), clamp(x+dx,0,W-1)].
//    - The radius r is in 0..8. r = 0 gives E = V.
// 4. Index. k* = argmin_k E_k, the lowest k on an exact tie.
// 5. Sub-sample refinement. All of it is fp32, each step a single rounded operation, with the compiler's contraction off as in
//    k_refocus.
//    - For 0 < k* < D-1: den = (E_{k*-1} - E_{k*}) + (E_{k*+1} - E_{k*}). Both terms are >= 0, so there is no cancellation.
//    - delta = 0.5*(E_{k*-1} - E_{k*+1})/den if den > 0, clamped to [-0.5, 0.5]. Otherwise, and at either end of the sweep,
//      delta = 0.
//    - disparity = d_{k*} + delta*(d_{k*+1} - d_{k*}) for delta >= 0, and d_{k*} + delta*(d_{k*} - d_{k*-1}) for delta < 0.
//    - The slopes are rounded once to fp32 on the host.
// 6. Confidence. Ebar = (sum_k E_k)/D, summed in k order. conf = 1 - E_{k*}/Ebar if Ebar > 0, else 0.
//    - A flat region, A = 1 and D = 1 all give 0.
// 7. All-in-focus. aif[y,x,c] = m_{k*(y,x)}[y,x,c], fp32 or uint8 by refocus's rule.
//    - m is accumulated in refocus's order: views in (u,v) order, taps in table order, explicit FMAs.
//    - So aif equals lft_refocus's fp32 stack gathered at k*, bit for bit.
//
// A pixel's results must not depend on the tile, on the image around the support of its taps and window, or on the launch
// shape. That requires a fixed aggregation order, dy then dx.
//
//   k_sweep_cost      k_refocus's grid and window pipeline (lft_refocus.cuh: one workgroup per (batch element, 32 x 32 tile, slope),
//                     the slope fastest, ids XCD-aware; per view of non-zero weight the window to registers and LDS, the row pass,
//                     the column pass, the next view's loads in flight meanwhile), the column pass feeding two accumulators per
//                     element: m = fma(a, s, m) exactly as k_refocus, q = fma(a*s, s, q).  After the last view the per-element
//                     max(q - fl(m*m), 0) goes to LDS -- the element-indexed layout has a pixel's channels next to each other --
//                     and each lane adds the channels of four pixels, c = 0 first.  V leaves as fp32 into the caller's volume
//                     [B, D, H, W]; with a stack pointer m leaves too, [B, D, H, W, C], for the all-in-focus gather.
//                     The body is sweep_cost<T, C, TAPS, OCC>, written once for this kernel and for k_sweep_cost_occ
//                     (lft_occlusion.cuh, which describes what OCC adds); k_refocus keeps its own copy of the pipeline, see below.
//   k_disparity_pick  one workgroup per (batch element, 16 x 16 tile), one pixel per lane: four times the workgroups of the sweep,
//                     because each walks the D slopes one after the other behind two barriers and only other workgroups hide
//                     that.  Per slope the V tile with a halo of r (clamped coordinates)
//                     goes to LDS; the box sum is direct, not a sliding one: per column the 2r+1 rows added from dy = -r up, then
//                     per pixel the 2r+1 column sums from dx = -r up, times fl(1/(2r+1)^2).  Each lane keeps for its pixel the
//                     best E and its k, the E before it, the E after it (caught by a pending flag), the last E and the running
//                     sum; after the last slope it refines and writes disparity, confidence, index, and gathers aif from the
//                     stack.  E goes out per slope when the caller asks for it.
//   DpSelect, dp_gather_aif   steps 4-7 for one pixel, written once here: the state a lane keeps (step(k, E) per slope, finish
//                     after the last) and the gather.  k_disparity_pick and k_sgm_pick (lft_sgm.cuh) both run them.
// Nothing here depends on which tile a pixel falls in: every sum has a fixed order and a fixed set of terms per pixel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lft_refocus.cuh"

namespace {

constexpr int kDpMaxR = 8;                                           // largest aggregation radius
constexpr int kDpTile = 16;                                          // tile of k_disparity_pick: one pixel per lane
constexpr int kDpCols = kDpTile + 2 * kDpMaxR;                       // rows and columns of a V tile with the largest halo (32)
constexpr int kDpPitch = 48;                                         // LDS pitch: the 16-pixel rows of a wave fall on disjoint banks
static_assert(kDpCols == 32 && kDpPitch >= kDpCols, "k_disparity_pick deals its lanes as 32 columns by 8 rows");

struct SweepArgs {
    const void* lf;
    long long st[3];                 // element strides of (b, u, v)
    int sy, sx, sc;                  // element strides of (y, x, c): a view spans less than 2^31 elements
    int A, H, W, D, tiles_x, tiles;
    const int* table;                // [D, A*A] records
    float* vol;                      // [B, D, H, W]     V
    float* stack;                    // [B, D, H, W, C]  m, or null
};

struct PickArgs {
    const float* vol;                // [B, D, H, W]
    const float* stack;              // [B, D, H, W, C], read when aif is set
    const float* slopes;             // [D]
    int H, W, D, C, r, tiles_x, tiles;   // tiles of kDpTile
    float* disparity;                // [B, H, W]
    float* confidence;               // [B, H, W]
    int* index;                      // [B, H, W]
    float* cost;                     // [B, D, H, W] or null
    void* aif;                       // [B, H, W, C] or null
    int aif_f32;
};

constexpr int kOccMaxP = 4;                                          // LFT_OCC_MAX_SUBSETS of include/lft_hip_occlusion.h

// The body of k_sweep_cost (OCC false; the last four arguments are not read) and of k_sweep_cost_occ (lft_occlusion.cuh; OCC true:
// subsets [P, A*A], 1 <= P <= kOccMaxP, the margin beta and the choice volume [B, D, H, W] or null): the window pipeline and both
// tails, written once.  What the subsets add stands under `if constexpr (OCC)`.  Sharing moved instructions in all 48 kernels (no
// scratch, LDS equal, no occupancy step crossed) but not the time: parent against shared, alternating in fresh processes on an
// MI355X, maps_ms 0.5075 .. 0.5114 against 0.5084 .. 0.5125, halves_ms 1.0218 .. 1.0238 against 1.0175 .. 1.0206, quadrants_ms
// 0.9922 .. 0.9980 against 0.9876 .. 0.9918 (profiles/sweep_refactor_ab.txt; uint8, C = 3, linear only).
template <typename T, int C, int TAPS, bool OCC>
__device__ __forceinline__ void sweep_cost(const SweepArgs& a, const float* subsets, int P, float beta, uint8_t* choice) {
#pragma clang fp contract(off)
    // the window pipeline below is k_refocus's, statement for statement, up to the second accumulator.  Of k_refocus it is a copy
    // on purpose: one inlined function serving both changed k_refocus's instructions and cost its linear stack 0.8 %
    constexpr int NR = kRfTile + TAPS - 1;
    constexpr int RW = NR * C;
    constexpr int NE = NR * RW;
    constexpr int RP = 256 / RW, NLD = (NR + RP - 1) / RP;
    static_assert(RP >= 1, "a window row is loaded by one pass of the workgroup");
    constexpr int OW = kRfTile * C, NACC = kRfTile * OW / 256;
    constexpr int NITEM = (kRfTile / kRfRows) * RW;
    constexpr int NPIX = kRfTile * kRfTile / 256;                    // pixels per lane of the channel sum
    __shared__ float win[NE];
    __shared__ float tmp[kRfTile * RW];                              // row pass of the window; at the end the per-element variances
    static_assert(kRfTile * RW >= kRfTile * OW, "the variances of a tile fit the row-pass buffer");

    const int tid = threadIdx.x;
    const int bid = xcd_tile(blockIdx.x, gridDim.x);
    const int d = bid % a.D, tile = (bid / a.D) % a.tiles, b = bid / (a.D * a.tiles);
    const int y0 = (tile / a.tiles_x) * kRfTile, x0 = (tile % a.tiles_x) * kRfTile;
    const int ny = min(kRfTile, a.H - y0), nx = min(kRfTile, a.W - x0);
    const int nv = a.A * a.A;
    const int* recs = a.table + (size_t)d * nv * kRfRec;
    const T* lfb = static_cast<const T*>(a.lf) + b * a.st[0];

    const int prow = tid / RW, pj = tid % RW, pxw = pj / C, pc = pj % C;
    T stage[NLD];
    float m[NACC], q[NACC], mp[OCC ? kOccMaxP : 1][NACC], qp[OCC ? kOccMaxP : 1][NACC];
#pragma unroll
    for (int r = 0; r < NACC; ++r) {
        m[r] = 0.0f; q[r] = 0.0f;
        if constexpr (OCC) {
#pragma unroll
            for (int p = 0; p < kOccMaxP; ++p) { mp[p][r] = 0.0f; qp[p][r] = 0.0f; }
        }
    }

    auto next_active = [&](int n) {
        while (n < nv && recs[n * kRfRec + 11]) ++n;
        return n;
    };
    auto fetch = [&](int n) {
        const int by = (int)min(max((long long)y0 + recs[n * kRfRec], -64LL), (long long)a.H + 63);
        const int bx = (int)min(max((long long)x0 + recs[n * kRfRec + 1], -64LL), (long long)a.W + 63);
        const T* vb = lfb + (n / a.A) * a.st[1] + (n % a.A) * a.st[2];
        const int coff = min(max(bx + pxw, 0), a.W - 1) * a.sx + pc * a.sc;
#pragma unroll
        for (int r = 0; r < NLD; ++r) {
            const int row = prow + RP * r;
            if (prow < RP && row < NR) stage[r] = vb[min(max(by + row, 0), a.H - 1) * a.sy + coff];
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int r = 0; r < NLD; ++r) {
            const int row = prow + RP * r;
            if (prow < RP && row < NR) win[row * RW + pj] = rf_x<T>(stage[r]);
        }
    };

    int cur = next_active(0);
    if (cur < nv) { fetch(cur); commit(); }
    __syncthreads();
    while (cur < nv) {
        const int nxt = next_active(cur + 1);
        if (nxt < nv) fetch(nxt);
        const float* wf = reinterpret_cast<const float*>(recs + cur * kRfRec);
        float wy[TAPS], wx[TAPS];
#pragma unroll
        for (int k = 0; k < TAPS; ++k) { wy[k] = wf[2 + k]; wx[k] = wf[6 + k]; }
        const float aw = wf[10];

        for (int i = tid; i < NITEM; i += 256) {
            const int yg = (i / RW) * kRfRows, j = i % RW;
            float w[kRfRows + TAPS - 1];
#pragma unroll
            for (int p = 0; p < kRfRows + TAPS - 1; ++p) w[p] = win[(yg + p) * RW + j];
#pragma unroll
            for (int p = 0; p < kRfRows; ++p) {
                float s = wy[0] * w[p];
#pragma unroll
                for (int k = 1; k < TAPS; ++k) s = __fmaf_rn(wy[k], w[p + k], s);
                tmp[(yg + p) * RW + j] = s;
            }
        }
        __syncthreads();
        float sv[OCC ? NACC : 1];                                    // this view's samples: every subset it belongs to reads them
#pragma unroll
        for (int r = 0; r < NACC; ++r) {
            const int i = tid + 256 * r;
            const float* t = tmp + (i / OW) * RW + i % OW;
            float s = wx[0] * t[0];
#pragma unroll
            for (int k = 1; k < TAPS; ++k) s = __fmaf_rn(wx[k], t[k * C], s);
            if constexpr (OCC) sv[r] = s;
            m[r] = __fmaf_rn(aw, s, m[r]);
            q[r] = __fmaf_rn(aw * s, s, q[r]);
        }
        if constexpr (OCC) {
#pragma unroll
            for (int p = 0; p < kOccMaxP; ++p) {
                if (p >= P) break;
                const float bw = subsets[p * nv + cur];              // the same for every lane: a scalar load and a scalar branch
                if (bw != 0.0f) {
#pragma unroll
                    for (int r = 0; r < NACC; ++r) {
                        mp[p][r] = __fmaf_rn(bw, sv[r], mp[p][r]);
                        qp[p][r] = __fmaf_rn(bw * sv[r], sv[r], qp[p][r]);
                    }
                }
            }
        }
        if (nxt < nv) commit();
        __syncthreads();
        cur = nxt;
    }

    // every lane is past the last column pass: tmp takes the variances, element-indexed, pitch OW (of one moment pair at a time with subsets)
    const size_t pix = ((size_t)b * a.D + d) * a.H * a.W;             // first pixel of this (b, slope) plane
    const int nb = nx * C;
    if constexpr (!OCC) {
#pragma unroll
        for (int r = 0; r < NACC; ++r) {
            const int i = tid + 256 * r, y = i / OW, e = i % OW;
            tmp[i] = fmaxf(q[r] - m[r] * m[r], 0.0f);                    // the square rounded on its own: one view (a = 1) gives exactly 0
            if (a.stack && y < ny && e < nb) a.stack[(pix + (size_t)(y0 + y) * a.W + x0) * C + e] = m[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < NPIX; ++r) {
            const int i = tid + 256 * r, y = i / kRfTile, x = i % kRfTile;
            float v = tmp[i * C];
#pragma unroll
            for (int c = 1; c < C; ++c) v += tmp[i * C + c];
            if (y < ny && x < nx) a.vol[pix + (size_t)(y0 + y) * a.W + x0 + x] = v;
        }
    } else {
        auto channel_sum = [&](const float* mm, const float* qq, float* v) {   // V of this lane's NPIX pixels; ends behind a barrier
#pragma clang fp contract(off)
#pragma unroll
            for (int r = 0; r < NACC; ++r) tmp[tid + 256 * r] = fmaxf(qq[r] - mm[r] * mm[r], 0.0f);   // the square rounded on its own
            __syncthreads();
#pragma unroll
            for (int r = 0; r < NPIX; ++r) {
                const int i = tid + 256 * r;
                float s = tmp[i * C];
#pragma unroll
                for (int c = 1; c < C; ++c) s += tmp[i * C + c];
                v[r] = s;
            }
            __syncthreads();                                             // the next pair's variances overwrite tmp
        };
        if (a.stack) {
#pragma unroll
            for (int r = 0; r < NACC; ++r) {
                const int i = tid + 256 * r, y = i / OW, e = i % OW;
                if (y < ny && e < nb) a.stack[(pix + (size_t)(y0 + y) * a.W + x0) * C + e] = m[r];
            }
        }
        float vfull[NPIX], t[NPIX], vp[NPIX];
        int arg[NPIX];
#pragma unroll
        for (int r = 0; r < NPIX; ++r) { t[r] = 0.0f; arg[r] = 0; }
        channel_sum(m, q, vfull);
#pragma unroll
        for (int p = 0; p < kOccMaxP; ++p) {
            if (p >= P) break;                                           // uniform: every lane meets the same barriers
            channel_sum(mp[p], qp[p], vp);
#pragma unroll
            for (int r = 0; r < NPIX; ++r)
                if (p == 0 || vp[r] < t[r]) { t[r] = vp[r]; arg[r] = p + 1; }   // strict: the lowest p wins an exact tie
        }
#pragma unroll
        for (int r = 0; r < NPIX; ++r) {
            const int i = tid + 256 * r, y = i / kRfTile, x = i % kRfTile;
            if (y < ny && x < nx) {
                const size_t o = pix + (size_t)(y0 + y) * a.W + x0 + x;
                const float U = beta * t[r];
                const bool whole = vfull[r] <= U;
                a.vol[o] = whole ? vfull[r] : U;
                if (choice) choice[o] = whole ? (uint8_t)0 : (uint8_t)arg[r];
            }
        }
    }
}

template <typename T, int C, int TAPS>
__global__ __launch_bounds__(256) void k_sweep_cost(SweepArgs a) { sweep_cost<T, C, TAPS, false>(a, nullptr, 0, 0.0f, nullptr); }

// The selection (steps 4-7) of one pixel, written once: k_disparity_pick feeds it E_k, k_sgm_pick (lft_sgm.cuh) S_k, in k order.
// It keeps the best value and its k, the value before it, the value after it (caught by the pending flag), the last value and the
// running sum.
struct DpSelect {
    float best = 0.0f, before = 0.0f, after = 0.0f, last = 0.0f, sum = 0.0f;
    int bk = 0;
    bool pending = true;

    __device__ __forceinline__ void step(int k, float E) {
#pragma clang fp contract(off)
        sum = k ? sum + E : E;
        if (k == 0 || E < best) {                                    // strict: the lowest k wins an exact tie
            before = last; best = E; bk = k; pending = true;
        } else if (pending) {
            after = E; pending = false;
        }
        last = E;
    }
    // after the last of the D values: refines, writes disparity, confidence and index at pixel o of [B, H, W]; returns k*
    __device__ __forceinline__ int finish(const float* slopes, int D, float* disparity, float* confidence, int* index, size_t o) const {
#pragma clang fp contract(off)
        float delta = 0.0f;
        if (bk > 0 && !pending) {                                    // pending: no slope after the best one, bk == D - 1
            const float den = (before - best) + (after - best);
            if (den > 0.0f) delta = fminf(fmaxf((0.5f * (before - after)) / den, -0.5f), 0.5f);
        }
        const float dk = slopes[bk];
        float disp = dk;
        if (delta > 0.0f) disp = dk + delta * (slopes[bk + 1] - dk);
        else if (delta < 0.0f) disp = dk + delta * (dk - slopes[bk - 1]);
        const float mean = sum / (float)D;
        disparity[o] = disp;
        confidence[o] = mean > 0.0f ? 1.0f - best / mean : 0.0f;
        index[o] = bk;
        return bk;
    }
};
// step 7 at pixel o of [B, H, W]: mk, the pixel's C channels of the stack at k*, to aif as fp32 or as bytes (rf_byte)
__device__ __forceinline__ void dp_gather_aif(const float* mk, int C, void* aif, int aif_f32, size_t o) {
    for (int c = 0; c < C; ++c) {
        if (aif_f32) static_cast<float*>(aif)[o * C + c] = mk[c];
        else static_cast<uint8_t*>(aif)[o * C + c] = rf_byte(mk[c]);
    }
}

__global__ __launch_bounds__(256) void k_disparity_pick(PickArgs a) {
#pragma clang fp contract(off)
    __shared__ float vt[kDpCols * kDpPitch];                         // V_k of the tile and its halo
    __shared__ float cs[kDpTile * kDpPitch];                         // per column the sum over dy

    const int tid = threadIdx.x;
    const int lx = tid % kDpCols, ly = tid / kDpCols;                // the two LDS stages: 32 columns by 8 rows per pass
    const int px = tid % kDpTile, py = tid / kDpTile;                // this lane's pixel of the tile
    const int tile = blockIdx.x % a.tiles, b = blockIdx.x / a.tiles;
    const int y0 = (tile / a.tiles_x) * kDpTile, x0 = (tile % a.tiles_x) * kDpTile;
    const bool live = y0 + py < a.H && x0 + px < a.W;
    const int r = a.r, n = 2 * r + 1, pw = kDpTile + 2 * r;          // pw <= kDpCols
    const float inv = 1.0f / (float)(n * n);
    const size_t plane = (size_t)a.H * a.W;
    const int gx = min(max(x0 - r + lx, 0), a.W - 1);                // this lane's column of the halo, clamped into the image

    DpSelect sel;
    for (int k = 0; k < a.D; ++k) {
        const float* v = a.vol + ((size_t)b * a.D + k) * plane;
        if (lx < pw)
            for (int j = ly; j < pw; j += 256 / kDpCols) vt[j * kDpPitch + lx] = v[(size_t)min(max(y0 - r + j, 0), a.H - 1) * a.W + gx];
        __syncthreads();
        if (lx < pw)
            for (int y = ly; y < kDpTile; y += 256 / kDpCols) {
                float s = vt[y * kDpPitch + lx];
                for (int dy = 1; dy < n; ++dy) s += vt[(y + dy) * kDpPitch + lx];
                cs[y * kDpPitch + lx] = s;
            }
        __syncthreads();                                             // the next slope's vt is written behind this barrier, its cs behind the next
        float s = cs[py * kDpPitch + px];
        for (int dx = 1; dx < n; ++dx) s += cs[py * kDpPitch + px + dx];
        const float E = s * inv;
        if (a.cost && live) a.cost[((size_t)b * a.D + k) * plane + (size_t)(y0 + py) * a.W + x0 + px] = E;
        sel.step(k, E);
    }
    if (!live) return;

    const size_t at = (size_t)(y0 + py) * a.W + x0 + px, o = (size_t)b * plane + at;
    const int bk = sel.finish(a.slopes, a.D, a.disparity, a.confidence, a.index, o);
    if (a.aif) dp_gather_aif(a.stack + (((size_t)b * a.D + bk) * plane + at) * a.C, a.C, a.aif, a.aif_f32, o);
}

// the instantiation for an input type, channel count (1 .. 4) and tap count (1, 2, 4)
template <typename T>
inline void (*sweep_kernel(int C, int taps))(SweepArgs) {
    static void (*const k[4][3])(SweepArgs) = {{k_sweep_cost<T, 1, 1>, k_sweep_cost<T, 1, 2>, k_sweep_cost<T, 1, 4>},
                                               {k_sweep_cost<T, 2, 1>, k_sweep_cost<T, 2, 2>, k_sweep_cost<T, 2, 4>},
                                               {k_sweep_cost<T, 3, 1>, k_sweep_cost<T, 3, 2>, k_sweep_cost<T, 3, 4>},
                                               {k_sweep_cost<T, 4, 1>, k_sweep_cost<T, 4, 2>, k_sweep_cost<T, 4, 4>}};
    return k[C - 1][taps == 4 ? 2 : taps - 1];
}

}  // namespace
