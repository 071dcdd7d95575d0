// lft_focal.cuh -- the focal-stack training term (lft_focal_loss) and the adjoint of lft_refocus (lft_refocus_adjoint); the
// definition, as in include/lft_hip_focal.h:
//
// Inputs.
// - sr, hr: fp32 mosaics [B,1,A*H,A*W]. View (u,v) is at rows u*H... and columns v*W....
// - The refocus table [D, A*A] of lft_refocus_record, from refocus.shift_table(A, slopes, aperture, interp, centre).
// - taps in {1,2,4}.
// - 1 <= D <= LFT_FOCAL_MAX_D = 64.
// - A*A <= 128.
// - A penalty rho out of LFT_LOSS_L1, LFT_LOSS_MSE and LFT_LOSS_CHARBONNIER, with eps. These are the constants and the rho of
//   lft_lf_loss.
// - A weight w_focal > 0.
// - gscale.
//
// 1. Residual stack.
// - e = fl(sr - hr) per element, in fp32.
// - r_k[b,y,x] is lft_refocus's fp32 output for the light field e and the same table. That means: views in (u,v) order, rows
//   first, clamped taps, explicit FMAs, skipped views not read.
// - r is bit for bit lft_refocus run on the materialised difference mosaic.
//
// 2. Value.
// - F = (1/N) sum_{b,k,y,x} rho(r), with N = B*D*H*W.
// - rho is evaluated in fp64 on the fp32 r.
// - The sum is fp64, from per-block partial sums folded in a fixed order.
// - No atomics.
//
// 3. Stack gradient.
// - G_k[b,y,x] = fl32(gscale * w_focal * rho'(r)/N).
// - rho' is evaluated in fp64 and rounded once.
// - For L1, rho'(0) = 0.
//
// 4. Adjoint.  For view n = (u,v) and its pixel (y',x'):
//   dsr[b,u,v,y',x'] = sum_k a_{k,n} * sum_{jy} wy[jy] sum_{y in Py} sum_{jx} wx[jx] sum_{x in Px} G_k[b,y,x]
// - Py = {y in [0,H) : clamp(y + oy + jy, 0, H-1) = y'}. Px is likewise.
// - Skipped views get 0.
// - An interior pixel has one y per tap.
// - A border pixel collects every y whose tap was clamped onto it.
// - The adjoint is fp32.
// - The order of the sums is fixed: over k, then jy, then y ascending, then jx, then x ascending; the sums over x and y are plain
//   fp32 additions from 0, each product enters by one explicit FMA (wx into the sum over jx, wy into the sum over jy, a into the sum
//   over k), with contraction off. Nothing depends on launch shape, tile or arrival order, there are no atomics, and two runs give
//   the same bits.
//
// 5. Outputs.
// - *focal_out = fl32(F).
// - With accumulate == 0: *total = fl32(w_focal*F), and dsr is fully overwritten.
// - With accumulate == 1: both are added to what total and dsr hold, in stream order. This takes one rounding each, as
//   lft_ssim_loss does.
// - dsr may be NULL (values only).
// - An optional output residual: NULL, or fp32 [B,D,H,W] for r.
// Every count scales with B. A mean over equal local shards is therefore the global-batch objective.
//
//   k_focal_residual<PEN, TAPS> : steps 1 to 3.  One lane per stack pixel, a workgroup per (batch element, 32 x 8 tile, slope), the
//                                 slope fastest and the ids dealt XCD-aware as in k_refocus.  (k, n) is the same for the whole
//                                 workgroup, so a record is a scalar load.  Per active view a lane reads the TAPS x TAPS pixels of
//                                 sr and of hr its taps touch (a wave's 64 lanes are two row segments of 32 consecutive pixels),
//                                 forms e there and filters as k_refocus does: the column of row sums, then the sum over the
//                                 columns, then acc = fma(a, s, acc).  Lanes beyond the view compute on clamped coordinates and
//                                 store nothing.  r goes to `residual`, G to the scratch, rho(r) into one fp64 sum per workgroup.
//   k_focal_fold                : one workgroup adds the per-block sums in index order and writes or accumulates {total, F}.
//   k_focal_adjoint<TAPS>       : step 4 as a gather.  One lane per mosaic pixel, a workgroup per (batch element, view, 32 x 8
//                                 tile): tiles lie inside one view, so (k, n) is wave-uniform and a record is a scalar load.  It
//                                 loops over k.  The preimage loops are bounded, for the whole workgroup, by min(|o| + TAPS, extent)
//                                 where the tile touches the view's first or last row (column) and by 1 elsewhere; every
//                                 iteration loads from a clamped address and selects afterwards (no branch around a load).
// The sampling rule is refocus's (rf_x of lft_refocus.cuh reads an element, kRfRec is the record's size); rho and rho' are
// lft_loss.cuh's, in fp64.  No LDS beyond the block sum, no atomics.  Every element offset is formed in 64 bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lft_refocus.cuh"
#include "lft_loss.cuh"

namespace {

constexpr int kFocalTileX = 32, kFocalTileY = 8, kFocalThreads = kFocalTileX * kFocalTileY;

struct FocalArgs {
    int A, H, W, D, tiles_x, tiles;
    const int* table;                // [D, A*A] records
    double eps2;                     // Charbonnier: eps * eps
    double c;                        // gscale * w_focal / N
    int accumulate;
};
struct FocalFoldArgs {
    double inv_n, w;
    int accumulate;
};

// tap j of an axis reads clamp(p + o + j, 0, n - 1)
__device__ __forceinline__ int focal_tap(int p, int o, int j, int n) { return (int)min(max((long long)p + o + j, 0LL), (long long)n - 1); }

template <int PEN, int TAPS>
__global__ __launch_bounds__(kFocalThreads) void k_focal_residual(const float* __restrict__ sr, const float* __restrict__ hr, FocalArgs a,
                                                                  float* __restrict__ residual, float* __restrict__ G, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ BlockSum<double, 1, kFocalThreads / 64> red;
    const int tid = threadIdx.x;
    const int bid = xcd_tile(blockIdx.x, gridDim.x);
    const int d = bid % a.D, tile = (bid / a.D) % a.tiles, b = bid / (a.D * a.tiles);
    const int y = (tile / a.tiles_x) * kFocalTileY + tid / kFocalTileX, x = (tile % a.tiles_x) * kFocalTileX + tid % kFocalTileX;
    const bool in = y < a.H && x < a.W;
    const int yc = min(y, a.H - 1), xc = min(x, a.W - 1);
    const int nv = a.A * a.A;
    const int* recs = a.table + (size_t)d * nv * kRfRec;
    const size_t pitch = (size_t)a.A * a.W, image = (size_t)a.A * a.H * pitch;
    float acc = 0.0f;
    for (int n = 0; n < nv; ++n) {
        const int* rec = recs + n * kRfRec;
        if (rec[11]) continue;
        const float* wf = reinterpret_cast<const float*>(rec);
        const size_t vb = (size_t)b * image + (size_t)(n / a.A) * a.H * pitch + (size_t)(n % a.A) * a.W;
        size_t ro[TAPS];
        int xx[TAPS];
#pragma unroll
        for (int j = 0; j < TAPS; ++j) {
            ro[j] = vb + (size_t)focal_tap(yc, rec[0], j, a.H) * pitch;
            xx[j] = focal_tap(xc, rec[1], j, a.W);
        }
        float t[TAPS];
#pragma unroll
        for (int jx = 0; jx < TAPS; ++jx) {                          // the row pass at the columns this pixel's taps read
            float s = wf[2] * (rf_x<float>(sr[ro[0] + xx[jx]]) - rf_x<float>(hr[ro[0] + xx[jx]]));
#pragma unroll
            for (int jy = 1; jy < TAPS; ++jy) s = __fmaf_rn(wf[2 + jy], rf_x<float>(sr[ro[jy] + xx[jx]]) - rf_x<float>(hr[ro[jy] + xx[jx]]), s);
            t[jx] = s;
        }
        float s = wf[6] * t[0];
#pragma unroll
        for (int jx = 1; jx < TAPS; ++jx) s = __fmaf_rn(wf[6 + jx], t[jx], s);
        acc = __fmaf_rn(wf[10], s, acc);
    }
    double rho = 0.0;
    if (in) {
        const size_t o = (((size_t)b * a.D + d) * a.H + y) * a.W + x;
        const double r = (double)acc;
        rho = loss_rho<PEN, double>(r, a.eps2);
        if (residual) residual[o] = acc;
        if (G) G[o] = (float)(a.c * loss_drho<PEN, double>(r, a.eps2));
    }
    red.put(&rho, tid);
    __syncthreads();
    if (tid == 0) part[bid] = red.get(0);
}

__global__ __launch_bounds__(kFocalThreads) void k_focal_fold(const double* __restrict__ part, long long nb, FocalFoldArgs f,
                                                              float* __restrict__ total, float* __restrict__ focal_out) {
    __shared__ BlockSum<double, 1, kFocalThreads / 64> red;
    if (blockIdx.x != 0) return;
    const int tid = threadIdx.x;
    double s = 0.0;
    for (long long b = tid; b < nb; b += kFocalThreads) s += part[b];
    red.put(&s, tid);
    __syncthreads();
    if (tid == 0) {
        const double F = red.get(0) * f.inv_n, term = f.w * F;
        *focal_out = (float)F;
        *total = f.accumulate ? (float)((double)*total + term) : (float)term;
    }
}

// the preimage of p' under tap j of an axis of extent n with offset o: the p in [lo, hi] (empty if lo > hi)
__device__ __forceinline__ void focal_preimage(int p, int o, int j, int n, int& lo, int& hi) {
    const long long c = (long long)p - o - j;
    lo = p == 0 ? 0 : (int)min(max(c, 0LL), (long long)n);            // the first pixel: every p whose tap falls at or before it
    hi = p == n - 1 ? n - 1 : (int)min(max(c, -1LL), (long long)n - 1);   // the last pixel: every p whose tap falls at or behind it
}

template <int TAPS>
__global__ __launch_bounds__(kFocalThreads) void k_focal_adjoint(const float* __restrict__ G, FocalArgs a, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const int nv = a.A * a.A;
    const int tile = blockIdx.x % a.tiles, n = (blockIdx.x / a.tiles) % nv, b = blockIdx.x / (a.tiles * nv);
    const int y0 = (tile / a.tiles_x) * kFocalTileY, x0 = (tile % a.tiles_x) * kFocalTileX;
    const int y = y0 + tid / kFocalTileX, x = x0 + tid % kFocalTileX;
    const bool in = y < a.H && x < a.W;
    const int yc = min(y, a.H - 1), xc = min(x, a.W - 1);
    const bool edge_y = y0 == 0 || y0 + kFocalTileY >= a.H, edge_x = x0 == 0 || x0 + kFocalTileX >= a.W;    // the tile holds a border pixel
    const size_t plane = (size_t)a.H * a.W;
    float v = 0.0f;
    for (int k = 0; k < a.D; ++k) {
        const int* rec = a.table + ((size_t)k * nv + n) * kRfRec;
        if (rec[11]) continue;
        const float* wf = reinterpret_cast<const float*>(rec);
        const int oy = rec[0], ox = rec[1];
        const int ny = edge_y ? (int)min((long long)a.H, llabs((long long)oy) + TAPS) : 1;
        const int nx = edge_x ? (int)min((long long)a.W, llabs((long long)ox) + TAPS) : 1;
        const float* Gk = G + ((size_t)b * a.D + k) * plane;
        int xlo[TAPS], xhi[TAPS];
#pragma unroll
        for (int jx = 0; jx < TAPS; ++jx) focal_preimage(xc, ox, jx, a.W, xlo[jx], xhi[jx]);
        float sk = 0.0f;
#pragma unroll
        for (int jy = 0; jy < TAPS; ++jy) {
            int ylo, yhi;
            focal_preimage(yc, oy, jy, a.H, ylo, yhi);
            float sy = 0.0f;
            for (int iy = 0; iy < ny; ++iy) {
                const int yy = ylo + iy;
                const float* row = Gk + (size_t)min(yy, a.H - 1) * a.W;
                float sx = 0.0f;
#pragma unroll
                for (int jx = 0; jx < TAPS; ++jx) {
                    float s = 0.0f;
                    for (int ix = 0; ix < nx; ++ix) {
                        const int xx = xlo[jx] + ix;
                        const float g = row[min(xx, a.W - 1)];
                        s = xx <= xhi[jx] ? s + g : s;
                    }
                    sx = __fmaf_rn(wf[6 + jx], s, sx);
                }
                sy = yy <= yhi ? sy + sx : sy;
            }
            sk = __fmaf_rn(wf[2 + jy], sy, sk);
        }
        v = __fmaf_rn(wf[10], sk, v);
    }
    if (in) {
        const size_t o = (((size_t)b * a.A + n / a.A) * a.H + y) * ((size_t)a.A * a.W) + (size_t)(n % a.A) * a.W + x;
        out[o] = a.accumulate ? out[o] + v : v;
    }
}

}  // namespace
