// lft_prepare.cuh -- the per-view arithmetic of the reference's data scripts (Generate_Data_for_Training.m:47-58,
// Generate_Data_for_Test.m:57-66) on the GPU: RGB -> Y (rgb2ycbcr, no input scaling) and MATLAB's antialiased bicubic
// imresize(Y, 1/s) of every crop of every centre view, all in fp64, one rounding to fp32 at the end.
//
// Grid: x = LR output tile (kPrepTileHr / s outputs per side, i.e. a 32 x 32 HR region), y = view (u*A + v), z = crop of
// this launch.  A workgroup stages Y of the input rows / columns its tile's taps touch in LDS (the RGB of that region is read
// once), runs the H pass into an LDS intermediate, then the W pass, and writes its HR and LR regions.  The contribution
// tables come from the caller (lft_amd/prepare.py:contributions); their indices are clamped into the crop, and a table whose
// taps span more than the LDS region falls back to reading Y from global memory with the same arithmetic.
// Sums run tap by tap in table order with contraction off, so the result does not depend on the tile or the launch shape.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kPrepCrops = 96;       // crop origins per launch, passed by value in the kernel arguments
constexpr int kPrepSpan = 56;        // staged Y region: at most kPrepSpan rows x kPrepSpan columns (32 + 18 taps + slack)
constexpr int kPrepTileHr = 32;      // HR extent of a tile; LR tile = 32 / s
constexpr int kPrepMaxTaps = 18;     // ceil(4 s) + 2 for s = 4, before all-zero tap columns are dropped

struct PrepCrops {
    int y0[kPrepCrops];
    int x0[kPrepCrops];
};
struct PrepArgs {
    const void* lf;
    long long st[5];                 // element strides of [U, V, H, W, C]
    int u0, v0, A, s, ch, cw, oh, ow, ph, pw, n0;
    const double* wh; const int* ih; // [oh, ph]
    const double* ww; const int* iw; // [ow, pw]
    float* hr;                       // [N, A*ch, A*cw]
    float* lr;                       // [N, A*oh, A*ow]
};

template <typename T>
__device__ __forceinline__ double prep_y(const T* p, long long sc) {
#pragma clang fp contract(off)
    const double r = (double)p[0], g = (double)p[sc], b = (double)p[2 * sc];
    return (((65.481 * r + 128.553 * g) + 24.966 * b) + 16.0) / 255.0;      // reference utils/utils.py:163, then / 255
}

template <typename T>
struct PrepView {
    const T* base;                   // (u, v, y0, x0) of the crop
    long long sh, sw, sc;
    const double* ys;                // staged Y, or nullptr
    int r0, c0, nr, nc;
    __device__ __forceinline__ double y(int r, int c) const {
        const int rr = r - r0, cc = c - c0;
        if (ys && rr >= 0 && rr < nr && cc >= 0 && cc < nc) return ys[rr * nc + cc];
        return prep_y(base + r * sh + c * sw, sc);
    }
    // H pass of LR row o at crop column c: sum over the taps of the row table, in order
    __device__ __forceinline__ double hsum(const PrepArgs& a, int o, int c) const {
#pragma clang fp contract(off)
        const double* w = a.wh + (size_t)o * a.ph;
        const int* ix = a.ih + (size_t)o * a.ph;
        double acc = w[0] * y(min(max(ix[0], 0), a.ch - 1), c);
        for (int k = 1; k < a.ph; ++k) acc = acc + w[k] * y(min(max(ix[k], 0), a.ch - 1), c);
        return acc;
    }
};

template <typename T>
__global__ __launch_bounds__(256) void k_lf_prepare(PrepArgs a, PrepCrops crops) {
#pragma clang fp contract(off)
    __shared__ double ys[kPrepSpan * kPrepSpan];
    __shared__ double ts[kPrepTileHr / 2 * kPrepSpan];
    __shared__ int rng[4];
    const int tid = threadIdx.x, TO = kPrepTileHr / a.s;
    const int tiles_x = (a.ow + TO - 1) / TO;
    const int oy0 = (blockIdx.x / tiles_x) * TO, ox0 = (blockIdx.x % tiles_x) * TO;
    const int ny = min(TO, a.oh - oy0), nx = min(TO, a.ow - ox0);
    const int u = blockIdx.y / a.A, v = blockIdx.y % a.A, n = blockIdx.z;
    const int cy = crops.y0[n], cx = crops.x0[n];

    PrepView<T> V;
    V.base = static_cast<const T*>(a.lf) + (a.u0 + u) * a.st[0] + (a.v0 + v) * a.st[1] + cy * a.st[2] + cx * a.st[3];
    V.sh = a.st[2]; V.sw = a.st[3]; V.sc = a.st[4];
    V.ys = nullptr; V.r0 = V.c0 = 0; V.nr = V.nc = 0;

    // rows / columns of the crop that this tile's taps read
    if (tid < 4) rng[tid] = (tid & 1) ? -1 : 0x7fffffff;
    __syncthreads();
    for (int i = tid; i < ny * a.ph; i += 256) {
        const int r = min(max(a.ih[(size_t)(oy0 + i / a.ph) * a.ph + i % a.ph], 0), a.ch - 1);
        atomicMin(&rng[0], r); atomicMax(&rng[1], r);
    }
    for (int i = tid; i < nx * a.pw; i += 256) {
        const int c = min(max(a.iw[(size_t)(ox0 + i / a.pw) * a.pw + i % a.pw], 0), a.cw - 1);
        atomicMin(&rng[2], c); atomicMax(&rng[3], c);
    }
    __syncthreads();
    const int r0 = rng[0], nr = rng[1] - r0 + 1, c0 = rng[2], nc = rng[3] - c0 + 1;
    const bool staged = nr <= kPrepSpan && nc <= kPrepSpan;
    if (staged) {
        for (int i = tid; i < nr * nc; i += 256) ys[i] = prep_y(V.base + (r0 + i / nc) * V.sh + (c0 + i % nc) * V.sw, V.sc);
        V.ys = ys; V.r0 = r0; V.c0 = c0; V.nr = nr; V.nc = nc;
    }
    __syncthreads();

    // H pass into LDS: ts[oy][c - c0] for the tile's rows and every column the W pass reads
    const bool tstaged = nc <= kPrepSpan;
    if (tstaged)
        for (int i = tid; i < ny * nc; i += 256) ts[(i / nc) * kPrepSpan + i % nc] = V.hsum(a, oy0 + i / nc, c0 + i % nc);
    __syncthreads();

    const int n_all = a.n0 + n;
    if (tid < ny * nx) {                                            // W pass: one LR output per thread (TO*TO <= 256)
        const int oy = tid / nx, ox = tid % nx;
        const double* w = a.ww + (size_t)(ox0 + ox) * a.pw;
        const int* ix = a.iw + (size_t)(ox0 + ox) * a.pw;
        double acc = 0.0;
        for (int k = 0; k < a.pw; ++k) {
            const int c = min(max(ix[k], 0), a.cw - 1);
            const double t = tstaged ? ts[oy * kPrepSpan + (c - c0)] : V.hsum(a, oy0 + oy, c);
            acc = k == 0 ? w[k] * t : acc + w[k] * t;
        }
        const size_t row = (size_t)n_all * a.A * a.oh + (size_t)u * a.oh + oy0 + oy;
        a.lr[row * ((size_t)a.A * a.ow) + (size_t)v * a.ow + ox0 + ox] = (float)acc;
    }
    // HR: Y of the tile's HR region (rows oy0*s .. (oy0+ny)*s, clipped to the crop)
    const int hy0 = oy0 * a.s, hx0 = ox0 * a.s;
    const int hny = min(ny * a.s, a.ch - hy0), hnx = min(nx * a.s, a.cw - hx0);
    for (int i = tid; i < hny * hnx; i += 256) {
        const int r = hy0 + i / hnx, c = hx0 + i % hnx;
        const size_t row = (size_t)n_all * a.A * a.ch + (size_t)u * a.ch + r;
        a.hr[row * ((size_t)a.A * a.cw) + (size_t)v * a.cw + c] = (float)V.y(r, c);
    }
}

}  // namespace
