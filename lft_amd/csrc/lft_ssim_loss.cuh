// Structural training term (lft_ssim_loss; the definition is in include/lft_hip.h): Q = 1 - S, S the plain mean over all views of the
// Gaussian-window SSIM of k_view_metrics (lft_metrics.cuh), and its gradient with respect to sr.
//
//   k_ssim_loss<GRAD> : one workgroup per 16x16 pixel tile of one view.  It stages the 36x36 surroundings (halo 10) of sr and hr as
//                       fp32, filters the five moment maps at the 26x26 window centres around the tile (rows first, into LDS, then
//                       columns, in registers), forms S_q and the coefficient maps a, b, c there -- zero outside the view's interior
//                       --, filters those back to the 16x16 pixels and writes dsr = k * (A + B*sr + C*hr).  Only the tile's own 16x16
//                       centres enter its partial sum of S, so no centre is counted twice.  GRAD = false (dsr == NULL): only the
//                       tile's own centres are evaluated and nothing is filtered back.
//   k_ssim_loss_fold  : one workgroup adds the per-tile partials in a fixed order and writes or accumulates {total, S}.
// Everything between the fp32 loads and the fp32 stores is fp64: sigma^2 = E[x^2] - mu^2 cancels, and an fp32 evaluation is wrong by
// up to 6.5e-5 of the largest gradient element on smooth inputs.  No atomics, every sum in index order: the same bits every run.
// The window up to S at one centre is lft_ssim_window.cuh's, shared with k_view_metrics; the sums fold through BlockSum (lft_common.cuh).
//
// LDS: 2 x 36x36 fp32 + 5 x 36x26 fp64 + 3 x 26x26 fp64 = 64 032 bytes, two workgroups per CU.  The row-filtered coefficient maps
// (3 x 26x16 fp64) reuse the moment rows.  Rows of 26 and 16 doubles are contiguous in a lane's neighbourhood: a wave's 8-byte reads
// walk consecutive addresses, which the 64-bank 8-byte read path serves without conflicts.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lft_ssim_window.cuh"

namespace {

constexpr int kSsimTile = 16;
constexpr int kSsimC = kSsimTile + 2 * kSsimR;      // 26 window centres per side reach the tile's pixels
constexpr int kSsimIn = kSsimC + 2 * kSsimR;        // 36 input pixels per side reach those centres
constexpr int kSsimThreads = 256;

struct SsimArgs {
    int A, H, W, tiles_x, ntiles;
    int accumulate;
    double C1, C2;
    double k;                                       // gscale * w_ssim * dQ/dS / (views * interior pixels), the sign included
};
struct SsimFoldArgs {
    double inv_count;                               // 1 / (views * interior pixels)
    double w;
    int accumulate;
};

template <bool GRAD>
__global__ __launch_bounds__(kSsimThreads) void k_ssim_loss(const float* __restrict__ sr, const float* __restrict__ hr, float* __restrict__ dsr,
                                                            SsimArgs p, double* __restrict__ part) {
    __shared__ float tx[kSsimIn][kSsimIn], ty[kSsimIn][kSsimIn];              // x = hr, y = sr
    __shared__ double hz[5][kSsimIn][kSsimC];
    __shared__ double co[GRAD ? 3 : 1][GRAD ? kSsimC : 1][GRAD ? kSsimC : 1];
    __shared__ double gs[kSsimTaps];
    __shared__ BlockSum<double, 1, kSsimThreads / 64> red;
    const int tid = threadIdx.x;
    const int H = p.H, W = p.W, A = p.A;
    const long long view = (long long)blockIdx.x / p.ntiles;                  // (b*A + a1)*A + a2
    const int tile = (int)((long long)blockIdx.x - view * p.ntiles);
    const int ty0 = (tile / p.tiles_x) * kSsimTile, tx0 = (tile % p.tiles_x) * kSsimTile;
    const int a2 = (int)(view % A), a1 = (int)((view / A) % A);
    const long long b = view / ((long long)A * A);
    const long long pitch = (long long)A * W;
    const long long base = (b * A * H + (long long)a1 * H) * pitch + (long long)a2 * W;
    if (tid < kSsimTaps) gs[tid] = ssim_gauss_raw(tid - kSsimR);
    for (int i = tid; i < kSsimIn * kSsimIn; i += kSsimThreads) {
        const int r = i / kSsimIn, c = i % kSsimIn;
        const int yy = ty0 - 2 * kSsimR + r, xx = tx0 - 2 * kSsimR + c;
        const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;               // outside values only reach centres outside the interior
        const long long o = base + (long long)yy * pitch + xx;
        tx[r][c] = in ? hr[o] : 0.0f;
        ty[r][c] = in ? sr[o] : 0.0f;
    }
    __syncthreads();
    double g[kSsimTaps];
    ssim_gauss(g, [&](int i) { return gs[i]; });
    ssim_moment_rows<kSsimIn, kSsimC, kSsimIn, kSsimThreads>(tx, ty, hz, g, tid);
    __syncthreads();
    double ssum = 0.0;
    for (int i = tid; i < kSsimC * kSsimC; i += kSsimThreads) {               // along the columns, then S_q and a, b, c at centre (r, c)
        const int r = i / kSsimC, c = i % kSsimC;
        const int cy = ty0 - kSsimR + r, cx = tx0 - kSsimR + c;
        const bool own = r >= kSsimR && r < kSsimR + kSsimTile && c >= kSsimR && c < kSsimR + kSsimTile;
        const bool interior = cy >= kSsimR && cy < H - kSsimR && cx >= kSsimR && cx < W - kSsimR;
        double ca = 0.0, cb = 0.0, cc = 0.0;
        if (interior && (GRAD || own)) {
            const SsimAt q = ssim_at(hz, r, c, g, p.C1, p.C2);
            if (own) ssum += q.S;
            if constexpr (GRAD) {
                const double d_mu = 2.0 * q.A2 * (q.mx - q.my * (q.A1 / q.B1)) / (q.B1 * q.B2);      // dS/d mu_y at fixed variances
                const double d_vy = -q.S / q.B2, d_vxy = 2.0 * q.A1 / (q.B1 * q.B2);                 // dS/d sigma_y^2, dS/d sigma_xy
                cb = 2.0 * kSsimCov * d_vy;
                cc = kSsimCov * d_vxy;
                ca = d_mu - cb * q.my - cc * q.mx;
            }
        }
        if constexpr (GRAD) { co[0][r][c] = ca; co[1][r][c] = cb; co[2][r][c] = cc; }
    }
    if constexpr (GRAD) {
        __syncthreads();                                                      // every read of hz is done: its memory takes the row pass
        double (*h2)[kSsimC][kSsimTile] = reinterpret_cast<double (*)[kSsimC][kSsimTile]>(&hz[0][0][0]);
        for (int i = tid; i < kSsimC * kSsimTile; i += kSsimThreads) {
            const int r = i / kSsimTile, c = i % kSsimTile;
            double s0 = 0, s1 = 0, s2 = 0;
            for (int k = 0; k < kSsimTaps; ++k) { s0 += g[k] * co[0][r][c + k]; s1 += g[k] * co[1][r][c + k]; s2 += g[k] * co[2][r][c + k]; }
            h2[0][r][c] = s0; h2[1][r][c] = s1; h2[2][r][c] = s2;
        }
        __syncthreads();
        const int ly = tid / kSsimTile, lx = tid % kSsimTile, y = ty0 + ly, x = tx0 + lx;
        if (y < H && x < W) {
            double s0 = 0, s1 = 0, s2 = 0;
            for (int k = 0; k < kSsimTaps; ++k) { s0 += g[k] * h2[0][ly + k][lx]; s1 += g[k] * h2[1][ly + k][lx]; s2 += g[k] * h2[2][ly + k][lx]; }
            const double yv = ty[ly + 2 * kSsimR][lx + 2 * kSsimR], xv = tx[ly + 2 * kSsimR][lx + 2 * kSsimR];
            const double v = p.k * (s0 + s1 * yv + s2 * xv);
            const long long o = base + (long long)y * pitch + x;
            dsr[o] = p.accumulate ? (float)((double)dsr[o] + v) : (float)v;
        }
    }
    red.put(&ssum, tid);
    __syncthreads();
    if (tid == 0) part[blockIdx.x] = red.get(0);
}

__global__ __launch_bounds__(kSsimThreads) void k_ssim_loss_fold(const double* __restrict__ part, long long nb, SsimFoldArgs f,
                                                                 float* __restrict__ total, float* __restrict__ ssim_out) {
    __shared__ BlockSum<double, 1, kSsimThreads / 64> red;
    if (blockIdx.x != 0) return;
    const int tid = threadIdx.x;
    double s = 0.0;
    for (long long b = tid; b < nb; b += kSsimThreads) s += part[b];
    red.put(&s, tid);
    __syncthreads();
    if (tid == 0) {
        const double S = red.get(0) * f.inv_count, term = f.w * (1.0 - S);
        *ssim_out = (float)S;
        *total = f.accumulate ? (float)((double)*total + term) : (float)term;
    }
}

}  // namespace
