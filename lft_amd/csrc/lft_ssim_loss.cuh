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
//
// LDS: 2 x 36x36 fp32 + 5 x 36x26 fp64 + 3 x 26x26 fp64 = 64 032 bytes, two workgroups per CU.  The row-filtered coefficient maps
// (3 x 26x16 fp64) reuse the moment rows.  Rows of 26 and 16 doubles are contiguous in a lane's neighbourhood: a wave's 8-byte reads
// walk consecutive addresses, which the 64-bank 8-byte read path serves without conflicts.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kSsimTile = 16, kSsimR = 5;
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
    __shared__ double gs[2 * kSsimR + 1];
    __shared__ double red[kSsimThreads / 64];
    const int tid = threadIdx.x;
    const int H = p.H, W = p.W, A = p.A;
    const long long view = (long long)blockIdx.x / p.ntiles;                  // (b*A + a1)*A + a2
    const int tile = (int)((long long)blockIdx.x - view * p.ntiles);
    const int ty0 = (tile / p.tiles_x) * kSsimTile, tx0 = (tile % p.tiles_x) * kSsimTile;
    const int a2 = (int)(view % A), a1 = (int)((view / A) % A);
    const long long b = view / ((long long)A * A);
    const long long pitch = (long long)A * W;
    const long long base = (b * A * H + (long long)a1 * H) * pitch + (long long)a2 * W;
    if (tid < 2 * kSsimR + 1) { const int k = tid - kSsimR; gs[tid] = exp(-0.5 * k * k / (1.5 * 1.5)); }
    for (int i = tid; i < kSsimIn * kSsimIn; i += kSsimThreads) {
        const int r = i / kSsimIn, c = i % kSsimIn;
        const int yy = ty0 - 2 * kSsimR + r, xx = tx0 - 2 * kSsimR + c;
        const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;               // outside values only reach centres outside the interior
        const long long o = base + (long long)yy * pitch + xx;
        tx[r][c] = in ? hr[o] : 0.0f;
        ty[r][c] = in ? sr[o] : 0.0f;
    }
    __syncthreads();
    double g[2 * kSsimR + 1];
    {
        double s = 0.0;
        for (int k = 0; k < 2 * kSsimR + 1; ++k) s += gs[k];
        for (int k = 0; k < 2 * kSsimR + 1; ++k) g[k] = gs[k] / s;
    }
    for (int i = tid; i < kSsimIn * kSsimC; i += kSsimThreads) {              // the five moment maps along the rows
        const int r = i / kSsimC, c = i % kSsimC;
        double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
        for (int k = 0; k < 2 * kSsimR + 1; ++k) {
            const double x = tx[r][c + k], y = ty[r][c + k];
            sx += g[k] * x; sy += g[k] * y; sxx += g[k] * x * x; syy += g[k] * y * y; sxy += g[k] * x * y;
        }
        hz[0][r][c] = sx; hz[1][r][c] = sy; hz[2][r][c] = sxx; hz[3][r][c] = syy; hz[4][r][c] = sxy;
    }
    __syncthreads();
    double ssum = 0.0;
    for (int i = tid; i < kSsimC * kSsimC; i += kSsimThreads) {               // along the columns, then S_q and a, b, c at centre (r, c)
        const int r = i / kSsimC, c = i % kSsimC;
        const int cy = ty0 - kSsimR + r, cx = tx0 - kSsimR + c;
        const bool own = r >= kSsimR && r < kSsimR + kSsimTile && c >= kSsimR && c < kSsimR + kSsimTile;
        const bool interior = cy >= kSsimR && cy < H - kSsimR && cx >= kSsimR && cx < W - kSsimR;
        double ca = 0.0, cb = 0.0, cc = 0.0;
        if (interior && (GRAD || own)) {
            double m[5] = {0, 0, 0, 0, 0};
            for (int k = 0; k < 2 * kSsimR + 1; ++k)
                for (int q = 0; q < 5; ++q) m[q] += g[k] * hz[q][r + k][c];
            const double cov = 121.0 / 120.0;
            const double mx = m[0], my = m[1];
            const double vx = cov * (m[2] - mx * mx), vy = cov * (m[3] - my * my), vxy = cov * (m[4] - mx * my);
            const double A1 = 2 * mx * my + p.C1, A2 = 2 * vxy + p.C2, B1 = mx * mx + my * my + p.C1, B2 = vx + vy + p.C2;
            const double S = (A1 * A2) / (B1 * B2);
            if (own) ssum += S;
            if constexpr (GRAD) {
                const double d_mu = 2.0 * A2 * (mx - my * (A1 / B1)) / (B1 * B2);      // dS/d mu_y at fixed variances
                const double d_vy = -S / B2, d_vxy = 2.0 * A1 / (B1 * B2);             // dS/d sigma_y^2, dS/d sigma_xy
                cb = 2.0 * cov * d_vy;
                cc = cov * d_vxy;
                ca = d_mu - cb * my - cc * mx;
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
            for (int k = 0; k < 2 * kSsimR + 1; ++k) { s0 += g[k] * co[0][r][c + k]; s1 += g[k] * co[1][r][c + k]; s2 += g[k] * co[2][r][c + k]; }
            h2[0][r][c] = s0; h2[1][r][c] = s1; h2[2][r][c] = s2;
        }
        __syncthreads();
        const int ly = tid / kSsimTile, lx = tid % kSsimTile, y = ty0 + ly, x = tx0 + lx;
        if (y < H && x < W) {
            double s0 = 0, s1 = 0, s2 = 0;
            for (int k = 0; k < 2 * kSsimR + 1; ++k) { s0 += g[k] * h2[0][ly + k][lx]; s1 += g[k] * h2[1][ly + k][lx]; s2 += g[k] * h2[2][ly + k][lx]; }
            const double yv = ty[ly + 2 * kSsimR][lx + 2 * kSsimR], xv = tx[ly + 2 * kSsimR][lx + 2 * kSsimR];
            const double v = p.k * (s0 + s1 * yv + s2 * xv);
            const long long o = base + (long long)y * pitch + x;
            dsr[o] = p.accumulate ? (float)((double)dsr[o] + v) : (float)v;
        }
    }
    for (int off = 32; off > 0; off >>= 1) ssum += __shfl_xor(ssum, off);     // wave64 butterfly: the same order every run
    if ((tid & 63) == 0) red[tid >> 6] = ssum;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < kSsimThreads / 64; ++w) t += red[w];
        part[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kSsimThreads) void k_ssim_loss_fold(const double* __restrict__ part, long long nb, SsimFoldArgs f,
                                                                 float* __restrict__ total, float* __restrict__ ssim_out) {
    __shared__ double red[kSsimThreads / 64];
    if (blockIdx.x != 0) return;
    const int tid = threadIdx.x;
    double s = 0.0;
    for (long long b = tid; b < nb; b += kSsimThreads) s += part[b];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < kSsimThreads / 64; ++w) t += red[w];
        const double S = t * f.inv_count, term = f.w * (1.0 - S);
        *ssim_out = (float)S;
        *total = f.accumulate ? (float)((double)*total + term) : (float)term;
    }
}

}  // namespace
