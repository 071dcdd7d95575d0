// lft_sgm.cuh -- semi-global aggregation of a disparity cost volume (lft_sgm, declared in include/lft_hip_sgm.h).
//
// Inputs
// - E: fp32 [B, D, H, W], the aggregated cost of lft_disparity or any other cost. It must be finite. The bit-for-bit promise is
//   for costs >= +0.
// - Slopes: as for lft_disparity.
// - Host floats P1, P2 with 0 <= P1 <= P2, and gain >= 0, each rounded once to fp32.
// - An optional guide g: fp32 [B, H, W].
// - paths R in {4, 8}.
// - 1 <= D <= LFT_SGM_MAX_D = 256.
//
// Directions, in this order; paths = 4 takes the first four. Here q = p - r is the predecessor of p on the path.
// - r0 = (0,+1), r1 = (0,-1), r2 = (+1,0), r3 = (-1,0)
// - r4 = (+1,+1), r5 = (-1,-1), r6 = (+1,-1), r7 = (-1,+1), each written (dy, dx).
//
// Recurrence. All of it is fp32, one rounded operation per step, contraction off.
// - If q lies outside the image: L_r(p,k) = E(p,k).
// - Otherwise:
//   - M = min_j L_r(q,j).
//   - P2' = P2 without a guide.
//   - With a guide: P2' = max(P1, P2 - fl(gain*|fl(g(p) - g(q))|)).
//   - c = fl(M + P2').
//   - b_k = fl(min(L_r(q,k-1), L_r(q,k+1)) + P1) over the neighbours that exist. With D = 1 there is none and b is absent.
//   - t_k = min(L_r(q,k), b_k, c).
//   - L_r(p,k) = fl(E(p,k) + fl(t_k - M)).
//
// Sum. S = fl(...fl(fl(L_0 + L_1) + L_2)... + L_{R-1}) * fl(1/R). The scaling is exact for R = 4 and 8.
//
// Selection. Steps 4-7 of lft_disparity, word for word, applied to S in the place of E:
// - index: the lowest k on a tie,
// - the parabola refinement,
// - conf = 1 - S_{k*}/Sbar,
// - aif gathered from a stack at k*.
//
// Nothing may depend on launch shape, tile or arrival order. Every sum has a fixed order, and min has none to fix.
//
//   k_sgm_scan   every direction in one launch, each writing its own volume L_r [B, D, H, W] into the scratch; no direction reads
//                what another writes.  A neighbour that does not exist is +inf: min ignores it, and inf + P1 loses against c.
//                - The six directions with dy != 0 (workgroups first in the grid: they run longest).  One workgroup per 64
//                  adjacent lines; a lane owns the line c and walks t = 0 .. H-1 with y = t (dy > 0) or H-1-t and x = c + dx*t,
//                  so a row's loads and stores are contiguous across the lanes.  A line that enters through the left or right
//                  edge becomes active late and starts from E; the workgroup walks only the rows where one of its lines is inside.
//                  The D slopes are dealt to the four waves in contiguous segments of ceil(D/4); a lane keeps its segment of
//                  L_r(q,.) in registers (KC of them, the kernel's template argument) and the E of the next PF rows in a register
//                  ring, loaded PF rows ahead.  Per row the waves exchange through LDS, double-buffered behind one barrier, the
//                  first and last L of each segment (the neighbours across a segment border) and the segment minima (M).
//                  Every load is unconditional, so that a row's loads issue back to back and only their use waits: a register
//                  past the segment re-reads the segment's last slope and is set to +inf, a lane outside the image reads pixel 0.
//                - The two horizontal directions.  One wave per image row (four rows per workgroup), lanes over k (k = lane + 64 j),
//                  walking x up or down.  [D x chunk] tiles of E come in with lanes along x, are scanned column by column out of LDS
//                  (odd pitch: no bank conflict), overwritten in place with L_r and leave with lanes along x again.  k-1 and k+1
//                  come from the neighbouring lanes by shuffles, M from a cross-lane minimum (DPP within rows of 16 lanes, then
//                  the four rows).
//   k_sgm_pick   one pixel per lane: per slope the R volumes added in direction order and scaled and fed to the selection that
//                k_disparity_pick uses (DpSelect and dp_gather_aif of lft_disparity.cuh), no box sum and no LDS.  S goes out
//                per slope when the caller asks for it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lft_disparity.cuh"   // the selection: DpSelect, dp_gather_aif

namespace {

constexpr int kSgMaxD = 256;                                         // LFT_SGM_MAX_D
constexpr int kSgLines = 64;                                         // lines of a workgroup of the non-horizontal directions
constexpr int kSgSegs = 4;                                           // its waves: segments of the D slopes
constexpr int kSgRows = 4;                                           // rows of a workgroup of the horizontal directions: one per wave
constexpr int kSgTile = 2304;                                        // floats of a row's [D x chunk] tile: 64 x 33, 128 x 17, 256 x 9
constexpr int kSgGuide = 40;                                         // floats of a row's guide chunk: the pixel before it and <= 32 pixels
constexpr int kSgRowLds = kSgTile + kSgGuide;
constexpr int kSgLds = kSgRows * kSgRowLds;                          // floats of LDS; the line workgroups use the first 1536
constexpr int kSgBatch = 8;                                          // loads of a tile in flight per lane
static_assert(kSgLds >= 2 * kSgSegs * 3 * kSgLines, "edges and minima of the line workgroups, double-buffered");
static_assert(64 * 33 <= kSgTile && 128 * 17 <= kSgTile && 256 * 9 <= kSgTile && 33 <= kSgGuide, "the three chunk widths fit");

struct SgmScanArgs {
    const float* cost;               // [B, D, H, W]     E
    const float* guide;              // [B, H, W] or null
    float* paths;                    // [R, B, D, H, W]  L_r
    int B, D, H, W, R, kc;           // kc = ceil(D / kSgSegs)
    float p1, p2, gain;
    int start[9];                    // per batch element: workgroups start[i] .. start[i+1] serve the i-th direction of the grid
};

struct SgmPickArgs {
    const float* paths;              // [R, B, D, H, W]
    const float* stack;              // [B, D, H, W, C], read when aif is set
    const float* slopes;             // [D]
    int H, W, D, C, R, per;          // per: workgroups per batch element
    size_t vol;                      // B * D * H * W
    float* disparity;                // [B, H, W]
    float* confidence;               // [B, H, W]
    int* index;                      // [B, H, W]
    float* aggregated;               // [B, D, H, W] or null
    void* aif;                       // [B, H, W, C] or null
    int aif_f32;
};

// The order of the directions in the grid: the lines that walk the image's height first, the rows last.
__device__ inline int sg_order(int i) { return i < 6 ? i + 2 : i - 6; }

template <int CTRL> __device__ inline float sg_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// The minimum of a wave in every lane.  quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror: each step folds the
// other half of a group of 2, 4, 8, 16 lanes in; min does not mind that the last two are mirrors, not butterflies.
__device__ inline float sg_wave_min(float v) {
    v = fminf(v, sg_dpp<0xB1>(v));
    v = fminf(v, sg_dpp<0x4E>(v));
    v = fminf(v, sg_dpp<0x141>(v));
    v = fminf(v, sg_dpp<0x140>(v));
    const int i = __float_as_int(v);
    const float a = __int_as_float(__builtin_amdgcn_readlane(i, 0)), b = __int_as_float(__builtin_amdgcn_readlane(i, 16));
    const float c = __int_as_float(__builtin_amdgcn_readlane(i, 32)), d = __int_as_float(__builtin_amdgcn_readlane(i, 48));
    return fminf(fminf(a, b), fminf(c, d));
}

// P2' of a step from the guide at p and at q
__device__ inline float sg_p2(const SgmScanArgs& a, float gp, float gq) {
#pragma clang fp contract(off)
    const float d = fabsf(gp - gq);
    const float s = a.gain * d;
    return fmaxf(a.p1, a.p2 - s);
}

// ---- the six directions with dy != 0: 64 lines per workgroup, a lane per line, a wave per segment of the slopes ----
template <int KC, int PF, bool G>
__device__ inline void sg_lines(const SgmScanArgs& a, float* lds, int b, int r, int group) {
#pragma clang fp contract(off)
    const float inf = __builtin_huge_valf();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = a.H, W = a.W, D = a.D;
    const int dy = (r & 1) ? -1 : 1;                                 // r2 r4 r6 walk down, r3 r5 r7 up
    const int dx = r < 4 ? 0 : ((r == 4 || r == 7) ? 1 : -1);
    const int nlines = W + (dx ? H - 1 : 0);
    const int shift = dx > 0 ? -(H - 1) : 0;                         // line id -> c, the x of the line at t = 0
    const int cA = group * kSgLines + shift, cB = min(group * kSgLines + kSgLines - 1, nlines - 1) + shift;
    int t0 = 0, t1 = H - 1;                                          // the rows where a line of this workgroup is inside the image
    if (dx > 0) { t0 = max(0, -cB); t1 = min(H - 1, W - 1 - cA); }
    if (dx < 0) { t0 = max(0, cA - (W - 1)); t1 = min(H - 1, cB); }
    const int c = group * kSgLines + lane + shift;
    const bool line = group * kSgLines + lane < nlines;

    const size_t plane = (size_t)H * W;
    const int k0 = wave * a.kc, nk = min(max(D - k0, 0), a.kc);      // this wave's slopes k0 .. k0 + nk - 1
    const int jl = max(nk - 1, 0);                                   // the last register that holds a slope
    const float* E = a.cost + ((size_t)b * D + min(k0, D - 1)) * plane;       // an empty segment reads the last slope and keeps nothing
    float* Lr = a.paths + (((size_t)r * a.B + b) * D + k0) * plane;
    const float* g = G ? a.guide + (size_t)b * plane : nullptr;

    float* edge = lds;                                               // [2][kSgSegs][2][64]: first and last L of a segment
    float* pmin = lds + 2 * kSgSegs * 2 * kSgLines;                  // [2][kSgSegs][64]: the minimum of a segment

    auto inside = [&](int t) { const int x = c + dx * t; return line && t <= t1 && x >= 0 && x < W; };
    auto before = [&](int t) { const int x = c + dx * (t - 1); return inside(t) && t > 0 && x >= 0 && x < W; };      // q is inside too
    auto pixel = [&](int t) { return inside(t) ? (size_t)(dy > 0 ? t : H - 1 - t) * W + (c + dx * t) : (size_t)0; };
    const ptrdiff_t back = -((ptrdiff_t)dy * W + dx);                 // from p to q

    float L[KC], e[PF][KC], gp[PF], gq[PF];                         // gp, gq: the guide at p and at q of a row of the ring
#pragma unroll
    for (int j = 0; j < KC; ++j) L[j] = inf;
#pragma unroll
    for (int p = 0; p < PF; ++p) {
        const size_t pix = pixel(t0 + p);
#pragma unroll
        for (int j = 0; j < KC; ++j) e[p][j] = E[(size_t)min(j, jl) * plane + pix];
        if constexpr (G) {
            gp[p] = g[pix];
            gq[p] = g[before(t0 + p) ? pix + back : 0];
        }
    }

    int cur = 0;
    for (int tb = t0; tb <= t1; tb += PF) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int t = tb + p;
            if (t > t1) break;                                       // the same for the whole workgroup
            const bool act = inside(t);
            const bool prev = before(t);
            // what the other waves left behind the last barrier; at t0 nothing yet, and no lane has a predecessor
            const float* eg = edge + cur * (kSgSegs * 2 * kSgLines);
            const float* pm = pmin + cur * (kSgSegs * kSgLines);
            const float below = eg[(max(wave - 1, 0) * 2 + 1) * kSgLines + lane], above = eg[(min(wave + 1, kSgSegs - 1) * 2) * kSgLines + lane];
            const float lo = wave > 0 ? below : inf, hi = wave < kSgSegs - 1 ? above : inf;
            const float M = fminf(fminf(pm[lane], pm[kSgLines + lane]), fminf(pm[2 * kSgLines + lane], pm[3 * kSgLines + lane]));
            float cM = M + a.p2;
            if constexpr (G) cM = M + sg_p2(a, gp[p], gq[p]);
            float left = lo, nm = inf, last = inf, keep[KC];         // keep: what goes to L_r, the last slope's value repeated
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const float own = L[j];
                float right = hi;
                if (j + 1 < KC) right = j + 1 < nk ? L[j + 1] : hi;
                const float bk = fminf(left, right) + a.p1;
                const float tk = fminf(fminf(own, bk), cM);
                const float step = e[p][j] + (tk - M);
                float v = prev ? step : e[p][j];
                keep[j] = j < nk ? v : keep[j > 0 ? j - 1 : 0];
                v = j < nk ? v : inf;
                L[j] = v;
                left = own;
                nm = fminf(nm, v);
                last = j == a.kc - 1 ? v : last;
            }
            if (act && nk > 0) {                                     // one masked run of stores: a register past the segment
                const size_t pix = pixel(t);                         // writes the segment's last slope once more
#pragma unroll
                for (int j = 0; j < KC; ++j) Lr[(size_t)min(j, jl) * plane + pix] = keep[j];
            }
            float* out = edge + (cur ^ 1) * (kSgSegs * 2 * kSgLines);
            out[(wave * 2) * kSgLines + lane] = L[0];                // +inf while the segment is empty
            out[(wave * 2 + 1) * kSgLines + lane] = last;            // +inf unless the segment is full: else no slope follows it
            pmin[(cur ^ 1) * (kSgSegs * kSgLines) + wave * kSgLines + lane] = nm;
            {                                                        // this slot of the ring: the row PF ahead
                const size_t pix = pixel(t + PF);
#pragma unroll
                for (int j = 0; j < KC; ++j) e[p][j] = E[(size_t)min(j, jl) * plane + pix];
                if constexpr (G) {
                    gp[p] = g[pix];
                    gq[p] = g[before(t + PF) ? pix + back : 0];
                }
            }
            __syncthreads();
            cur ^= 1;
        }
    }
}

// ---- the two horizontal directions: a wave per row, lanes over the slopes ----
__device__ inline void sg_rows(const SgmScanArgs& a, float* lds, int b, int r, int group) {
#pragma clang fp contract(off)
    const float inf = __builtin_huge_valf();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = a.H, W = a.W, D = a.D;
    const int y = group * kSgRows + wave;
    const bool live = y < H;
    const int kpl = (D + 63) / 64;                                   // slopes per lane
    const int sh = D <= 64 ? 5 : D <= 128 ? 4 : 3, CH = 1 << sh, pitch = CH + 1;      // pixels per tile: 32, 16, 8
    const size_t plane = (size_t)H * W;
    const size_t row = (size_t)(live ? y : 0) * W;                   // a wave past the last row reads row 0 and stores nothing
    const float* E = a.cost + (size_t)b * D * plane + row;
    float* Lr = a.paths + ((size_t)r * a.B + b) * D * plane + row;
    const bool guided = a.guide != nullptr;
    const float* g = guided ? a.guide + (size_t)b * plane + row : E;
    float* tile = lds + wave * kSgRowLds;
    float* gb = tile + kSgTile;                                      // gb[i + 1]: the guide at step t0 + i; gb[0]: at the step before
    auto xof = [&](int t) { return r ? W - 1 - t : t; };             // r1 walks x down

    float L[4] = {inf, inf, inf, inf};
    float M = 0.0f;
    for (int t0 = 0; t0 < W; t0 += CH) {
        const int n = min(CH, W - t0);
        for (int base = 0; base < D * CH; base += 64 * kSgBatch) {   // unconditional loads, clamped into the row: they issue back to back
            float v[kSgBatch];
#pragma unroll
            for (int u = 0; u < kSgBatch; ++u) {
                const int idx = base + 64 * u + lane;
                v[u] = E[(size_t)min(idx >> sh, D - 1) * plane + xof(min(t0 + (idx & (CH - 1)), W - 1))];
            }
#pragma unroll
            for (int u = 0; u < kSgBatch; ++u) {
                const int idx = base + 64 * u + lane, k = idx >> sh, i = idx & (CH - 1);
                if (k < D && i < n) tile[k * pitch + i] = v[u];
            }
        }
        const float gval = g[xof(min(t0 + lane, W - 1))];
        if (lane < n) gb[lane + 1] = gval;
        __syncthreads();
        for (int i = 0; i < n; ++i) {
            const bool prev = t0 + i > 0;
            const float cM = M + (guided ? sg_p2(a, gb[i + 1], gb[i]) : a.p2);
            float lf[4], rt[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < kpl) {                                       // the same for every lane: the shuffles run in full waves
                    const float up = __shfl_up(L[j], 1), dn = __shfl_down(L[j], 1);
                    float wl = inf, wr = inf;
                    if (j > 0) wl = __shfl(L[j - 1], 63);
                    if (j + 1 < 4) { if (j + 1 < kpl) wr = __shfl(L[j + 1], 0); }
                    lf[j] = lane == 0 ? wl : up;
                    rt[j] = lane == 63 ? wr : dn;
                }
            float nm = inf;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < kpl) {
                    const int k = lane + 64 * j;
                    float v = inf;                                   // a slope past the last: never a neighbour, never the minimum
                    if (k < D) {
                        v = tile[k * pitch + i];
                        if (prev) {
                            const float bk = fminf(lf[j], rt[j]) + a.p1;
                            const float tk = fminf(fminf(L[j], bk), cM);
                            v = v + (tk - M);
                        }
                        tile[k * pitch + i] = v;
                    }
                    L[j] = v;
                    nm = fminf(nm, v);
                }
            M = sg_wave_min(nm);
        }
        if (lane == 0) gb[0] = gb[n];
        __syncthreads();
        if (live)
            for (int idx = lane; idx < D * CH; idx += 64) {
                const int k = idx >> sh, i = idx & (CH - 1);
                if (i < n) Lr[(size_t)k * plane + xof(t0 + i)] = tile[k * pitch + i];
            }
        __syncthreads();                                             // the next chunk overwrites the tile
    }
}

template <int KC, int PF, bool G>
__global__ __launch_bounds__(256) void k_sgm_scan(SgmScanArgs a) {
    __shared__ float lds[kSgLds];
    const int per = a.start[a.R];
    const int b = blockIdx.x / per, id = blockIdx.x % per;
    int i = 0;
    while (id >= a.start[i + 1]) ++i;
    const int r = sg_order(i + (a.R == 4 && i >= 2 ? 4 : 0));         // four paths: r2, r3, then the rows
    if (r >= 2) sg_lines<KC, PF, G>(a, lds, b, r, id - a.start[i]);
    else sg_rows(a, lds, b, r, id - a.start[i]);
}

__global__ __launch_bounds__(256) void k_sgm_pick(SgmPickArgs a) {
#pragma clang fp contract(off)
    const size_t plane = (size_t)a.H * a.W;
    const int b = blockIdx.x / a.per;
    const size_t px = (size_t)(blockIdx.x % a.per) * 256 + threadIdx.x;
    if (px >= plane) return;
    const float inv = 1.0f / (float)a.R;

    DpSelect sel;
    for (int k = 0; k < a.D; ++k) {
        const size_t at = ((size_t)b * a.D + k) * plane + px;
        float s = a.paths[at];
        for (int r = 1; r < a.R; ++r) s = s + a.paths[(size_t)r * a.vol + at];
        const float E = s * inv;
        if (a.aggregated) a.aggregated[at] = E;
        sel.step(k, E);
    }

    const size_t o = (size_t)b * plane + px;
    const int bk = sel.finish(a.slopes, a.D, a.disparity, a.confidence, a.index, o);
    if (a.aif) dp_gather_aif(a.stack + (((size_t)b * a.D + bk) * plane + px) * a.C, a.C, a.aif, a.aif_f32, o);
}

}  // namespace
