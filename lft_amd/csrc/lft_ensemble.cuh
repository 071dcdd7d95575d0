// ------------------------------------------------------------------------------------------
// Dihedral light-field transforms (geometric self-ensemble at inference, per-sample augmentation in training).
// A code t in 0..7: bit 0 mirrors the mosaic left-right, bit 1 up-down, bit 2 transposes it, applied in that order -- the three
// coin flips of the reference's augmentation (utils/utils_datasets.py:114-124).  For x[H, W]:
//     T_t(x)[i, j] = x[fi(p), fj(q)],  (p, q) = (j, i) if bit 2 else (i, j),  fi(p) = H-1-p if bit 1,  fj(q) = W-1-q if bit 0
// and T_t(x) is [W, H] when bit 2 is set.  T_t^-1 undoes the transpose first, then the mirrors:
//     T_t^-1(y)[a, b] = y[fi(a), fj(b)]            (bit 2 clear, y stored [H, W])
//     T_t^-1(y)[a, b] = y[fj(b), fi(a)]            (bit 2 set,   y stored [W, H])
// The forward transform is the inverse of the inverse code (bits 0 and 1 swapped when bit 2 is set: 5 <-> 6, the rest are
// involutions), so ONE tile gather -- tile_inv -- serves all three kernels.
//
// All kernels: fp32 gathers, 256 threads = 32 lanes x 8 rows on a 32x32 tile, one code per block (no divergence on the code), the
// image index folded into grid x.  A mirrored read walks a 128-byte run downwards (still one run per 32 lanes); a transposed read
// is staged through LDS [32][33]: the global read runs along the STORED rows of the variant, the LDS read along its columns
// (pitch 33: conflict-free), so both sides of a transposing code move whole 128-byte runs.  Ragged edges are guarded.
// The merge adds the variants in ascending code order and multiplies once by 1.0f / E -- nothing a compiler could contract
// into an FMA -- so the same operations in torch give the same bits.
// ------------------------------------------------------------------------------------------
#pragma once
#include "lft_common.cuh"

namespace {

constexpr int DH_TILE = 32;

LFT_DEV int dihedral_nth_code(unsigned mask, int k) {      // code of the k-th set bit of mask (ascending); k < popcount(mask)
    int code = 0;
    for (unsigned m = mask & 0xFFu; m; m >>= 1, ++code)
        if ((m & 1u) && k-- == 0) break;
    return code;
}
LFT_DEV int dihedral_inverse_code(int code) {
    return (code & 4) ? (4 | ((code & 1) << 1) | ((code >> 1) & 1)) : code;
}

// v[r] = T_code^-1(y)[a0 + ty + 8 r, b0 + tx] for r = 0..3, where the result image is H x W and only na x nb elements of the tile
// (na, nb <= 32) are wanted: the others are neither read nor defined.  Every thread of the block must call it (barriers).
LFT_DEV void tile_inv(const float* __restrict__ y, int code, int H, int W, int a0, int b0, int na, int nb,
                      float (*tile)[DH_TILE + 1], float v[4]) {
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const bool lr = code & 1, ud = code & 2;
    if (!(code & 4)) {
        const int b = b0 + tx, col = lr ? W - 1 - b : b;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = a0 + ty + 8 * r, row = ud ? H - 1 - a : a;
            if (ty + 8 * r < na && tx < nb) v[r] = y[(size_t)row * W + col];
        }
        return;
    }
    // y is stored [W, H]: lanes run along its rows (index fi(a)), the 8 thread rows along fj(b)
    const int a = a0 + tx, col = ud ? H - 1 - a : a;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = b0 + ty + 8 * r, row = lr ? W - 1 - b : b;
        if (ty + 8 * r < nb && tx < na) tile[ty + 8 * r][tx] = y[(size_t)row * H + col];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (ty + 8 * r < na && tx < nb) v[r] = tile[tx][ty + 8 * r];
    __syncthreads();                                        // the next variant refills the tile
}

// out[j] = T_code(j)(in[j / rep]) for images of H x W floats; code(j) = codes[j] & 7 (device array, rep = 1: per-sample
// augmentation) or, with codes == nullptr, the (j % rep)-th code of mask (rep = E: expansion into adjacent variants).
// grid x = images * tiles, tiles = ceil(H/32) * ceil(W/32) (the same count for [H, W] and [W, H] outputs).
__global__ __launch_bounds__(256) void k_dihedral(const float* __restrict__ in, float* __restrict__ out, const int* __restrict__ codes,
                                                  unsigned mask, int rep, int H, int W) {
    __shared__ float tile[DH_TILE][DH_TILE + 1];
    const unsigned tiles = (unsigned)((H + DH_TILE - 1) / DH_TILE) * (unsigned)((W + DH_TILE - 1) / DH_TILE);
    const unsigned img = blockIdx.x / tiles, t = blockIdx.x - img * tiles;
    const int code = codes ? (codes[img] & 7) : dihedral_nth_code(mask, (int)(img % (unsigned)rep));
    const int Ho = (code & 4) ? W : H, Wo = (code & 4) ? H : W;
    const unsigned tc = (unsigned)((Wo + DH_TILE - 1) / DH_TILE);
    const int a0 = (int)(t / tc) * DH_TILE, b0 = (int)(t % tc) * DH_TILE;
    const int na = min(DH_TILE, Ho - a0), nb = min(DH_TILE, Wo - b0);
    const size_t hw = (size_t)H * W;
    float v[4];
    tile_inv(in + (size_t)(img / (unsigned)rep) * hw, dihedral_inverse_code(code), Ho, Wo, a0, b0, na, nb, tile, v);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    float* o = out + (size_t)img * hw;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (ty + 8 * r < na && tx < nb) o[(size_t)(a0 + ty + 8 * r) * Wo + b0 + tx] = v[r];
}

// out[n] = (1/E) sum_k T^-1_code_k(in[n*E + k]), out [B, H, W]; variant k is stored [W, H] when its code transposes.
// grid x = B * tiles of the output.
__global__ __launch_bounds__(256) void k_dihedral_merge(const float* __restrict__ in, float* __restrict__ out, unsigned mask, int E,
                                                        int H, int W) {
    __shared__ float tile[DH_TILE][DH_TILE + 1];
    const unsigned tc = (unsigned)((W + DH_TILE - 1) / DH_TILE), tiles = (unsigned)((H + DH_TILE - 1) / DH_TILE) * tc;
    const unsigned n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int a0 = (int)(t / tc) * DH_TILE, b0 = (int)(t % tc) * DH_TILE;
    const int na = min(DH_TILE, H - a0), nb = min(DH_TILE, W - b0);
    const size_t hw = (size_t)H * W;
    const float* y = in + (size_t)n * E * hw;
    float acc[4], v[4];
    int code = 0, k = 0;
    for (unsigned m = mask & 0xFFu; m; m >>= 1, ++code) {
        if (!(m & 1u)) continue;
        if (k == 0) {
            tile_inv(y, code, H, W, a0, b0, na, nb, tile, acc);
        } else {
            tile_inv(y + (size_t)k * hw, code, H, W, a0, b0, na, nb, tile, v);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] += v[r];
        }
        ++k;
    }
    const float inv = 1.0f / (float)E;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    float* o = out + (size_t)n * hw;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (ty + 8 * r < na && tx < nb) o[(size_t)(a0 + ty + 8 * r) * W + b0 + tx] = acc[r] * inv;
}

// LFintegrate + re-mosaic (k_scene_integrate) and the merge in one pass: only the central S x S region (S = stride * s) of every
// view of every variant is read -- a quarter of the data at patch 32 / stride 16 -- and every SR scene pixel is written once.
// A block takes one 32x32 tile of the S x S region of one (patch, view): its source in every variant is then ONE rectangle of one
// P x P mosaic (P = A * pz), read through T^-1 like the merge; the part of the region beyond the scene (the last patch row /
// column overhangs) is neither read nor written.  pz, S, h0, w0 in SR pixels.
// grid x = patches * A * A * ceil(S/32)^2.
__global__ __launch_bounds__(256) void k_scene_integrate_ens(const float* __restrict__ sub, float* __restrict__ out, unsigned mask, int E,
                                                             int A, int pz, int S, int h0, int w0, int nv) {
    __shared__ float tile[DH_TILE][DH_TILE + 1];
    const unsigned ts = (unsigned)((S + DH_TILE - 1) / DH_TILE);
    unsigned t = blockIdx.x;
    const int tj = (int)(t % ts); t /= ts;
    const int ti = (int)(t % ts); t /= ts;
    const int v_ = (int)(t % (unsigned)A); t /= (unsigned)A;
    const int u_ = (int)(t % (unsigned)A); t /= (unsigned)A;
    const int ku = (int)(t / (unsigned)nv), kv = (int)(t % (unsigned)nv);
    const int i0 = ti * DH_TILE, j0 = tj * DH_TILE;                    // tile origin inside the region
    const int Y0 = ku * S + i0, X0 = kv * S + j0;                      // ... and inside the SR view
    const int na = min(min(DH_TILE, S - i0), h0 - Y0), nb = min(min(DH_TILE, S - j0), w0 - X0);
    if (na <= 0 || nb <= 0) return;                                    // block-uniform: the whole tile overhangs the scene
    const int bdr = (pz - S) / 2, P = A * pz;
    const int a0 = u_ * pz + bdr + i0, b0 = v_ * pz + bdr + j0;
    const size_t pp = (size_t)P * P;
    const float* y = sub + (size_t)t * E * pp;
    float acc[4], v[4];
    int code = 0, k = 0;
    for (unsigned m = mask & 0xFFu; m; m >>= 1, ++code) {
        if (!(m & 1u)) continue;
        if (k == 0) {
            tile_inv(y, code, P, P, a0, b0, na, nb, tile, acc);
        } else {
            tile_inv(y + (size_t)k * pp, code, P, P, a0, b0, na, nb, tile, v);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] += v[r];
        }
        ++k;
    }
    const float inv = 1.0f / (float)E;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (ty + 8 * r < na && tx < nb)
            out[(size_t)(u_ * h0 + Y0 + ty + 8 * r) * ((size_t)A * w0) + (size_t)v_ * w0 + X0 + tx] = acc[r] * inv;
}

}  // namespace
