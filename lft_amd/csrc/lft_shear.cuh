// lft_shear.cuh -- per-patch disparity compensation by integer shear: scene tiling whose cut moves with the view
// (lft_scene_divide_shear, lft_scene_integrate_shear) and the vote that chooses each patch's shear from a disparity sweep
// (lft_shear_vote).  Declared in include/lft_hip_shear.h.
#pragma once
#include "lft_scene.cuh"      // reflect_idx, which fold continues; the plain gathers these two follow

namespace {

// ------------------------------------------------------------------------------------------
// LFT's angular Transformer attends across the A x A views at the same pixel, which only works while a scene point stays within a
// pixel or so across the views.  A shear by a whole number k of LR pixels per view step is lossless: view (u, v) of a patch is
// cut at an offset of k*(u-u0), k*(v-u0) pixels, the network sees a light field whose residual disparity is d - k, and the SR
// patch is put back at s*k*(u-u0), again a whole number of pixels.  No pixel is interpolated on either side.
//
// Let bdr = (patch - stride)/2, u0 = A / 2, du = u - u0 and dv = v - u0 (whole numbers for even A too), R = max(u0, A-1-u0), and
// kmax = LFT_SHEAR_MAX if R = 0, else min(LFT_SHEAR_MAX, bdr / R).  Every kernel clamps k_n into [-kmax, kmax] itself: a device
// array can hold anything, and divide and integrate must stay inverse to each other.  The sign is the disparity module's: a point
// seen at y in view u is seen at y + d*(u'-u) in view u', so k = d aligns the views.
//
// Sheared divide.  Patch n = ku*nv + kv, view (u, v), pixel (y, x) of the patch.  ey = ku*stride + y, and ex likewise.  The value
// is 0 where ey >= h0 + 2*bdr or ex >= w0 + 2*bdr: today's test, on the unsheared coordinates.  Elsewhere the value is
// scene[u*h0 + fold(ey - bdr + k_n*du, h0), v*w0 + fold(ex - bdr + k_n*dv, w0)].  fold(i, n): m = i mod 2n (non-negative), then m
// if m < n, else 2n-1-m.  This is reflect_idx continued to any integer; on [-n, 2n-1] the two agree.
//
// Sheared integrate.  SR view (u, v), SR pixel (Y, X).  ku = Y / (stride*s), i = Y - ku*stride*s, and kv, j likewise;
// n = ku*nv + kv, as today.  The value is the SR patch n, view (u, v), at row bdr*s + i - s*k_n*du and column
// bdr*s + j - s*k_n*dv.  With the clamp those lie inside the patch, and they never touch a zero-filled pixel.
//
// Vote.  count[b, j] is the number of pixels with margin <= y < H-margin, margin <= x < W-margin, clamped index equal to j, and
// confidence finite and >= min_confidence.  shear[b] = slopes[j*], where j* has the largest count.  On a tie the smallest |slope|
// wins, then the smaller slope.  If every count is 0 the result is 0.  Counts are integers, so arrival order cannot matter.
//
// Both tiling kernels are pure gathers (one thread per output element) whose reads along x are contiguous for every k, HBM-bound
// like the plain pair; their byte contract is the plain pair's plus 4 bytes per patch.
// ------------------------------------------------------------------------------------------
LFT_DEV int fold_idx(int i, int n) {                // reflect_idx continued to any integer: period 2n, edge repeated
    if (i >= -n && i < 2 * n) return reflect_idx(i, n);     // at most one reflection: every read unless the view is smaller than the border
    int m = i % (2 * n);
    m = m < 0 ? m + 2 * n : m;
    return m < n ? m : 2 * n - 1 - m;
}
LFT_DEV int clamp_shear(int k, int kmax) { return k < -kmax ? -kmax : k > kmax ? kmax : k; }

__global__ __launch_bounds__(256) void k_scene_divide_shear(const float* __restrict__ scene, const int* __restrict__ shear,
                                                            float* __restrict__ patches, int A, int h0, int w0, int patch, int stride,
                                                            int nv, int kmax) {
    // grid: k_scene_divide's -- x over the A*patch columns, y = row of the patch mosaic, z = patch index ku*nv + kv.  A workgroup
    // serves one patch and one mosaic row: k_n and the source row come from blockIdx alone (a wave-uniform address, scalar work).
    const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y, n = blockIdx.z;
    const int P = A * patch;
    if (X >= P) return;
    const int k = clamp_shear(shear[n], kmax), u0 = A / 2;
    const int bdr = (patch - stride) / 2, ku = n / nv, kv = n - ku * nv;
    const int u = Y / patch, y = Y - u * patch, v = X / patch, x = X - v * patch;
    const int ey = ku * stride + y, ex = kv * stride + x;
    float val = 0.0f;                                   // beyond the extended view: zero fill, judged on the unsheared coordinates
    if (ey < h0 + 2 * bdr && ex < w0 + 2 * bdr)
        val = scene[(size_t)(u * h0 + fold_idx(ey - bdr + k * (u - u0), h0)) * (A * w0) + v * w0 + fold_idx(ex - bdr + k * (v - u0), w0)];
    patches[((size_t)n * P + Y) * P + X] = val;
}
__global__ __launch_bounds__(256) void k_scene_integrate_shear(const float* __restrict__ sub, const int* __restrict__ shear,
                                                               float* __restrict__ out, int A, int pz, int stride, int h0, int w0, int nv,
                                                               int s, int kmax) {
    // grid: k_scene_integrate's -- x over the A*w0 columns of the SR scene mosaic, y = its rows; pz, stride, h0, w0 are in SR
    // pixels.  A row of the grid crosses patches, so k_n is read per lane (the lanes of one patch share the address).
    const int Xm = blockIdx.x * 256 + threadIdx.x, Ym = blockIdx.y;
    if (Xm >= A * w0) return;
    const int bdr = (pz - stride) / 2, u0 = A / 2;
    const int u = Ym / h0, Y = Ym - u * h0, v = Xm / w0, X = Xm - v * w0;
    const int ku = Y / stride, i = Y - ku * stride, kv = X / stride, j = X - kv * stride;
    const int n = ku * nv + kv, sk = s * clamp_shear(shear[n], kmax);
    const int P = A * pz;
    out[(size_t)Ym * (A * w0) + Xm] = sub[((size_t)n * P + u * pz + bdr + i - sk * (u - u0)) * P + v * pz + bdr + j - sk * (v - u0)];
}

struct VoteArgs {
    const int* index; const float* confidence; const int* slopes;
    int H, W, D, margin; float min_confidence;
    int* counts; int* shear;
};
constexpr int kShearMax = 16;                       // LFT_SHEAR_MAX of the header (asserted where both are seen)
constexpr int kVoteMaxD = 2 * kShearMax + 1;
__global__ __launch_bounds__(256) void k_shear_vote(const VoteArgs a) {
    // One workgroup per batch element (a patch's maps are small): its pixels in strides of 256, the counts in LDS by integer
    // atomics, then the counts written out whole -- nothing to zero beforehand -- and the selection by lane 0.
    __shared__ int hist[kVoteMaxD];
    const int b = blockIdx.x, t = threadIdx.x;
    if (t < kVoteMaxD) hist[t] = 0;
    __syncthreads();
    const int rw = a.W - 2 * a.margin;
    const long long pixels = (long long)(a.H - 2 * a.margin) * rw;
    const size_t map = (size_t)b * a.H * a.W;
    for (long long p = t; p < pixels; p += 256) {
        const int y = (int)(p / rw), x = (int)(p - (long long)y * rw);
        const size_t at = map + (size_t)(y + a.margin) * a.W + (x + a.margin);
        const float c = a.confidence[at];
        if (isfinite(c) && c >= a.min_confidence) {
            const int j = a.index[at];
            atomicAdd(&hist[j < 0 ? 0 : j > a.D - 1 ? a.D - 1 : j], 1);
        }
    }
    __syncthreads();
    if (t < a.D) a.counts[(size_t)b * a.D + t] = hist[t];
    if (t == 0) {
        int best = 0, slope = 0;                        // every count 0: the result is 0
        for (int j = 0; j < a.D; ++j) {
            const int c = hist[j], sj = a.slopes[j];
            const long long mag = sj < 0 ? -(long long)sj : sj, held = slope < 0 ? -(long long)slope : slope;
            if (c > best || (c == best && c > 0 && (mag < held || (mag == held && sj < slope)))) { best = c; slope = sj; }
        }
        a.shear[b] = slope;
    }
}

}  // namespace
