// lft_occlusion.cuh -- the plane sweep's cost from partial apertures: next to a foreground edge the views on the far side of the
// edge see the foreground at the background's true slope, the variance of all views is large there and a wrong slope wins.  The
// views of one side of the aperture still agree, so the cost below also scores a slope by the variance of up to four subsets of
// the views and lets a subset win where it is much better than the whole aperture.
//
// The inputs, the table, the samples s, the aperture a (fp64 on the host, sum 1) and the centre (cu, cv) are those of
// lft_disparity. Everything below is fp32, one rounded operation per step, with contraction off.
//
// Subsets (host only). Let du = u - cu and dv = v - cv in fp64.
// - "halves": the four subsets du <= 0, du >= 0, dv <= 0, dv >= 0.
// - "quadrants": (<=,<=), (<=,>=), (>=,<=), (>=,>=) in (du, dv).
// - A boolean array [P, A, A] with 1 <= P <= 4.
// - A subset is kept iff at least min_views of its views have a > 0. min_views is an integer >= 2, default 2. One view has
//   variance 0 at every slope and would win everywhere.
// - Dropped subsets never reach the kernel. Subset ids in the outputs are positions in the kept list.
// - If no subset is kept, raise LftError.
// - For a kept subset p: W_p = sum_{p} a in fp64. The row b_p[u,v] = fl32(a/W_p) for members and 0 for the rest.
// - The table [P', A*A] fp32, views in (u, v) order, is the only place these weights are rounded.
//
// Moments.
// - The full aperture is unchanged: m, q, V_full exactly as today, the same FMAs in the same order. m stays refocus's stack bit
//   for bit, and aif is still gathered from it.
// - Per kept subset, over its members in (u, v) order:
//   - m_p = fma(b_p, s, m_p)
//   - q_p = fma(fl(b_p*s), s, q_p)
//   - V_p = sum_c max(q_p - fl(m_p*m_p), 0), with c = 0 first.
//
// Combination.
// - t = min_p V_p and U = fl(beta*t).
// - V = min(V_full, U).
// - choice = 0 if V_full <= U, else the lowest p (1-based) with V_p = t.
// - beta is the margin: finite, >= 1, rounded once to fp32. A subset wins only where it is beta times better than the whole
//   aperture.
//
// After that. Steps 3 to 7 of lft_disparity run word for word on this V, through the existing k_disparity_pick unchanged.
//
// New outputs.
// - subset: uint8 [B, H, W], equal to choice at (k*, y, x).
// - Optionally the whole choice volume, uint8 [B, D, H, W].
// - Read together with index, subset is an occlusion-edge map: 0 where all views agree.
//
// No result may depend on the tile, the launch shape or the arrival order.
//
//   k_sweep_cost_occ  k_sweep_cost's grid and window pipeline (lft_disparity.cuh), a copy for the reason given there, with 1 + P'
//                     accumulator pairs per element.  The tile stays 32 x 32 and a lane keeps 4C elements: 2 * 4C * 5 = 160
//                     accumulators at C = 4 and four subsets, which a workgroup of 256 lanes (one wave per SIMD, up to 512
//                     registers each) holds without scratch; what is given up is occupancy, not the window's reuse.  The column
//                     pass first leaves its 4C samples in registers, then walks the subsets: a view's membership is the same for
//                     every lane (b_p[view] != 0, read through a uniform address), so each subset is one scalar branch round an
//                     unrolled loop over statically indexed registers.  After the last view the channel sums go through the
//                     row-pass LDS buffer one moment pair after the other -- the whole aperture first, then the subsets in order,
//                     each between two barriers -- and a lane keeps for its four pixels V_full, the running minimum t and the
//                     subset that set it (strictly smaller replaces: the lowest p wins a tie).  V leaves as fp32, choice as one
//                     byte per pixel and slope.
//   k_occ_gather      one lane per pixel: subset[b, y, x] = choice[b, index[b, y, x], y, x], the index clamped into 0 .. D-1.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lft_disparity.cuh"

namespace {

constexpr int kOccMaxP = 4;                                          // LFT_OCC_MAX_SUBSETS of include/lft_hip_occlusion.h

struct SweepOccArgs {
    SweepArgs s;                     // the plain sweep's arguments; vol takes V = min(V_full, U)
    const float* subsets;            // [P, A*A] b_p, 0 for the views outside the subset
    int P;                           // kept subsets, 1 .. kOccMaxP
    float beta;
    uint8_t* choice;                 // [B, D, H, W] or null
};

struct OccGatherArgs {
    const int* index;                // [B, H, W]
    const uint8_t* choice;           // [B, D, H, W]
    uint8_t* subset;                 // [B, H, W]
    int D;
    size_t plane, n;                 // H * W, B * H * W
};

template <typename T, int C, int TAPS>
__global__ __launch_bounds__(256) void k_sweep_cost_occ(SweepOccArgs oa) {
#pragma clang fp contract(off)
    const SweepArgs& a = oa.s;
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
    const int P = oa.P;

    const int prow = tid / RW, pj = tid % RW, pxw = pj / C, pc = pj % C;
    T stage[NLD];
    float m[NACC], q[NACC], mp[kOccMaxP][NACC], qp[kOccMaxP][NACC];
#pragma unroll
    for (int r = 0; r < NACC; ++r) {
        m[r] = 0.0f; q[r] = 0.0f;
#pragma unroll
        for (int p = 0; p < kOccMaxP; ++p) { mp[p][r] = 0.0f; qp[p][r] = 0.0f; }
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
        float sv[NACC];                                              // this view's samples: every subset it belongs to reads them
#pragma unroll
        for (int r = 0; r < NACC; ++r) {
            const int i = tid + 256 * r;
            const float* t = tmp + (i / OW) * RW + i % OW;
            float s = wx[0] * t[0];
#pragma unroll
            for (int k = 1; k < TAPS; ++k) s = __fmaf_rn(wx[k], t[k * C], s);
            sv[r] = s;
            m[r] = __fmaf_rn(aw, s, m[r]);
            q[r] = __fmaf_rn(aw * s, s, q[r]);
        }
#pragma unroll
        for (int p = 0; p < kOccMaxP; ++p) {
            if (p >= P) break;
            const float bw = oa.subsets[p * nv + cur];               // the same for every lane: a scalar load and a scalar branch
            if (bw != 0.0f) {
#pragma unroll
                for (int r = 0; r < NACC; ++r) {
                    mp[p][r] = __fmaf_rn(bw, sv[r], mp[p][r]);
                    qp[p][r] = __fmaf_rn(bw * sv[r], sv[r], qp[p][r]);
                }
            }
        }
        if (nxt < nv) commit();
        __syncthreads();
        cur = nxt;
    }

    // every lane is past the last column pass: tmp takes the variances of one moment pair at a time, element-indexed, pitch OW
    const size_t pix = ((size_t)b * a.D + d) * a.H * a.W;             // first pixel of this (b, slope) plane
    const int nb = nx * C;
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
            const float U = oa.beta * t[r];
            const bool whole = vfull[r] <= U;
            a.vol[o] = whole ? vfull[r] : U;
            if (oa.choice) oa.choice[o] = whole ? (uint8_t)0 : (uint8_t)arg[r];
        }
    }
}

__global__ __launch_bounds__(256) void k_occ_gather(OccGatherArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const size_t b = i / a.plane, at = i % a.plane;
    const int k = min(max(a.index[i], 0), a.D - 1);
    a.subset[i] = a.choice[(b * a.D + k) * a.plane + at];
}

// the instantiation for an input type, channel count (1 .. 4) and tap count (1, 2, 4)
template <typename T>
inline void (*sweep_occ_kernel(int C, int taps))(SweepOccArgs) {
    static void (*const k[4][3])(SweepOccArgs) = {{k_sweep_cost_occ<T, 1, 1>, k_sweep_cost_occ<T, 1, 2>, k_sweep_cost_occ<T, 1, 4>},
                                                  {k_sweep_cost_occ<T, 2, 1>, k_sweep_cost_occ<T, 2, 2>, k_sweep_cost_occ<T, 2, 4>},
                                                  {k_sweep_cost_occ<T, 3, 1>, k_sweep_cost_occ<T, 3, 2>, k_sweep_cost_occ<T, 3, 4>},
                                                  {k_sweep_cost_occ<T, 4, 1>, k_sweep_cost_occ<T, 4, 2>, k_sweep_cost_occ<T, 4, 4>}};
    return k[C - 1][taps == 4 ? 2 : taps - 1];
}

}  // namespace
