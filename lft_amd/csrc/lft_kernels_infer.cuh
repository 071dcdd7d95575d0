// lft_kernels_infer.cuh -- the kernels that are no templates and that only the inference unit launches: weight copies and
// compositions of the packing plan, k_spa_b's geometry table, the bicubic skip on its own.  A __global__ function that is no
// template is emitted by every unit that sees it, so these stand apart from the templates of lft_kernels_a.cuh / _b.cuh, which the
// training unit includes too.
#pragma once
#include "lft_kernels_b.cuh"

namespace {

__global__ void k_copy_f32(const float* __restrict__ src, float* __restrict__ dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
// w0 [64][9], w1 [64][64][9] -> w01 [64][kW01K] fp32 (pack time; k_pack rounds it to ConvLrOp)
__global__ void k_compose_w01(const float* __restrict__ w0, const float* __restrict__ w1, float* __restrict__ w01) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 64 * kW01K) return;
    const int rho = idx / kW01K, k = idx - rho * kW01K;
    float v = 0.0f;
    if (k < 81) {
        const int o = conv01_row_channel(rho), t1 = k / 9, t0 = k - 9 * t1;
        for (int c = 0; c < 64; ++c) v += w1[o * 576 + c * 9 + t1] * w0[c * 9 + t0];
    }
    w01[idx] = v;
}
// The 16-bit part B folds the 1x1x1 conv into the FFN's second Linear (k_spa_b): wl [64][128], w2 [128][256] -> wlw2 [64][256]
// fp32, summed in channel order (pack time; k_pack rounds it once to the operand type)
__global__ void k_compose_wlw2(const float* __restrict__ wl, const float* __restrict__ w2, float* __restrict__ wlw2) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 64 * 256) return;
    const int o = idx >> 8, k = idx & 255;
    float v = 0.0f;
    for (int c = 0; c < 128; ++c) v += wl[o * 128 + c] * w2[c * 256 + k];
    wlw2[idx] = v;
}
__global__ __launch_bounds__(256) void k_spa_b_geom(unsigned* __restrict__ tab, int h, int w) {
    const int tiles_x = (w + kAttTX - 1) / kAttTX;
    const int tile = blockIdx.x, tx = tile % tiles_x, ty = tile / tiles_x;
    const int lane = threadIdx.x & 63, r = lane & 31, wave = threadIdx.x >> 6;
    const int y0 = ty * kAttTY, x0 = tx * kAttTX, bxl = 8 * wave;
    const int qy = y0 + ((r >> 2) & 3);
    int dofs[kAdPerWave], kb[2], vb[2];
    unsigned ymask, xs[2];
    spa_b_dma_offsets<true>(wave, lane, y0, x0, h, w, dofs);
    spa_b_window_masks(lane, qy, y0, x0, bxl, h, w, ymask, xs);
    spa_b_read_bases(lane, bxl, kb, vb);
    unsigned* dst = tab + ((size_t)(tile * 4 + wave) * kSpaBGeomPieces * 64 + lane) * 4;
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[(i >> 2) * 256 + (i & 3)] = (unsigned)dofs[i];
    dst[512] = (unsigned)dofs[8];
    dst[513] = (unsigned)kb[0] | ((unsigned)kb[1] << 16);
    dst[514] = (unsigned)vb[0] | ((unsigned)vb[1] << 16);
    dst[515] = ymask | (xs[0] << 8) | (xs[1] << 16);
}
// The per-view bicubic skip on its own (lft_bicubic_fwd: unit tests of reference LFT.py:255-266).
__global__ __launch_bounds__(256) void k_bicubic(const float* __restrict__ lr, float* __restrict__ out, int B, int A, int h, int w, int s) {
    // grid: x = 256-pixel column groups, y = HR mosaic row, z = batch
    const int HR_H = A * h * s, HR_W = A * w * s;
    const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y, b = blockIdx.z;
    if (X >= HR_W) return;
    const int a1 = Y / (h * s), a2 = X / (w * s);
    const float* view = lr + (size_t)b * (A * h) * (A * w) + (size_t)(a1 * h) * (A * w) + a2 * w;
    out[((size_t)b * HR_H + Y) * HR_W + X] = bicubic_at(view, A * w, h, w, Y - a1 * h * s, X - a2 * w * s, s);
}

}  // namespace
