// lft_colour.cuh -- the colour path around the network: a raw RGB light field in, super-resolved RGB views out.
//
// Per sub-aperture view, in fp64 with MATLAB's conventions: x = double(LF) (/ 255 for uint8: UNLIKE lft_lf_prepare the input is
// scaled to [0, 1], which is what the network was trained on), ycc = rgb2ycbcr(x) (reference utils/utils.py:160-168, the operation
// order of prep_y for every channel), Cb and Cr up-scaled by imresize(., s) (reference utils/imresize.py, the up-scaling branch:
// Keys cubic a = -0.5, no antialiasing, rows first), rgb = Minv * (255 * [Y, Cb, Cr] - [16, 128, 128]) with Minv the fp64 inverse
// of rgb2ycbcr's matrix, and convertDouble2Byte (imresize.py:141-144: clip to [0, 1], * 255, round half to even).
//
//   k_lf_luma       single(Y) of the centre views as the network's input mosaic [A*H, A*W].
//   k_colour_merge  grid: x = HR tile (32 x 32) of a view, y = view (u*A + v).  A workgroup reads the RGB of the LR region its
//                   tile's taps touch once, stages Cb and Cr (and Y without sr_y: the bicubic baseline) in LDS, runs the row pass
//                   into an LDS intermediate, then the column pass, takes Y from its sr_y tile, inverts, and writes interleaved
//                   RGB [A, A, s*H, s*W, 3] as uint8 or as the unquantised fp32.  The tile's output is assembled in LDS so that
//                   lanes store whole dwords of consecutive addresses.  Neither the LR nor the HR chroma reaches memory.
// The contribution tables come from the caller (lft_amd/colour.py:up_contributions); their indices are clamped into the view, and
// a table whose taps span more than the LDS region falls back to reading the view from global memory with the same arithmetic.
// Sums run tap by tap in table order with contraction off, so the result does not depend on the tile or the launch shape.
// COPIES KEPT: the resampler and the rgb2ycbcr rows also stand in lft_prepare.cuh, the byte-row store in
// lft_refocus.cuh; through shared helpers k_colour_merge<uint8> was slower in every round (0.2750-0.2764 ms against 0.2740-0.2747).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kColTile = 32;         // HR extent of a tile
constexpr int kColSpan = 24;         // staged LR region: at most kColSpan rows x kColSpan columns (32 / 2 + 6 taps + slack)
constexpr int kColMaxTaps = 6;       // ceil(4) + 2, before all-zero tap columns are dropped (4 are left for s = 2 and 4)
constexpr int kColSlots = 28;        // store slots per tile row: up to 24 whole dwords, then one slot each for head and tail bytes

struct LumaArgs {
    const void* lf;
    long long st[5];                 // element strides of [U, V, H, W, C]
    int u0, v0, A, H, W;
    float* y;                        // [A*H, A*W]
};
struct ColourArgs {
    const void* lf;
    long long st[5];
    int u0, v0, A, s, H, W, ph, pw;
    const float* sr_y;               // [A*s*H, A*s*W], or nullptr: Y is up-scaled like the chroma
    const double* wh; const int* ih; // [s*H, ph]
    const double* ww; const int* iw; // [s*W, pw]
    double minv[9];                  // row-major inverse of rgb2ycbcr's matrix
    void* out;                       // [A, A, s*H, s*W, 3]
    int out_f32;
};

template <typename T> __device__ __forceinline__ double col_x(T v) { return (double)v; }
template <> __device__ __forceinline__ double col_x<uint8_t>(uint8_t v) { return (double)v / 255.0; }

// channel ch of rgb2ycbcr(x) at one pixel (reference utils/utils.py:163-165, then / 255)
template <typename T>
__device__ __forceinline__ double col_ycc(const T* p, long long sc, int ch) {
#pragma clang fp contract(off)
    const double r = col_x<T>(p[0]), g = col_x<T>(p[sc]), b = col_x<T>(p[2 * sc]);
    if (ch == 0) return (((65.481 * r + 128.553 * g) + 24.966 * b) + 16.0) / 255.0;
    if (ch == 1) return (((-37.797 * r - 74.203 * g) + 112.0 * b) + 128.0) / 255.0;
    return (((112.0 * r - 93.786 * g) - 18.214 * b) + 128.0) / 255.0;
}

template <typename T>
__global__ __launch_bounds__(256) void k_lf_luma(LumaArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)a.H * a.W) return;
    const int h = (int)(i / a.W), w = (int)(i % a.W), u = blockIdx.y / a.A, v = blockIdx.y % a.A;
    const T* p = static_cast<const T*>(a.lf) + (a.u0 + u) * a.st[0] + (a.v0 + v) * a.st[1] + h * a.st[2] + w * a.st[3];
    a.y[((size_t)u * a.H + h) * ((size_t)a.A * a.W) + (size_t)v * a.W + w] = (float)col_ycc(p, a.st[4], 0);
}

template <typename T>
struct ColView {
    const T* base;                   // (u, v, 0, 0) of the view
    long long sh, sw, sc;
    const double* zs;                // staged planes [3][nr * nc] (plane stride kColSpan * kColSpan), or nullptr
    int r0, c0, nr, nc;
    __device__ __forceinline__ double val(int ch, int r, int c) const {
        const int rr = r - r0, cc = c - c0;
        if (zs && rr >= 0 && rr < nr && cc >= 0 && cc < nc) return zs[ch * kColSpan * kColSpan + rr * nc + cc];
        return col_ycc(base + r * sh + c * sw, sc, ch);
    }
    // row pass of HR row o at LR column c: sum over the taps of the row table, in order
    __device__ __forceinline__ double hsum(const ColourArgs& a, int ch, int o, int c) const {
#pragma clang fp contract(off)
        const double* w = a.wh + (size_t)o * a.ph;
        const int* ix = a.ih + (size_t)o * a.ph;
        double acc = w[0] * val(ch, min(max(ix[0], 0), a.H - 1), c);
        for (int k = 1; k < a.ph; ++k) acc = acc + w[k] * val(ch, min(max(ix[k], 0), a.H - 1), c);
        return acc;
    }
};

template <typename T>
__global__ __launch_bounds__(256) void k_colour_merge(ColourArgs a) {
#pragma clang fp contract(off)
    __shared__ double zs[3 * kColSpan * kColSpan];
    __shared__ double ts[3 * kColTile * kColSpan];
    __shared__ float ob[kColTile * kColTile * 3];                   // the tile's output: fp32, or bytes in its first quarter
    __shared__ int rng[4];
    const int tid = threadIdx.x;
    const int OH = a.s * a.H, OW = a.s * a.W;
    const int tiles_x = (OW + kColTile - 1) / kColTile;
    const int oy0 = (blockIdx.x / tiles_x) * kColTile, ox0 = (blockIdx.x % tiles_x) * kColTile;
    const int ny = min(kColTile, OH - oy0), nx = min(kColTile, OW - ox0);
    const int u = blockIdx.y / a.A, v = blockIdx.y % a.A;
    const int ch0 = a.sr_y ? 1 : 0;                                 // first channel to up-scale

    ColView<T> V;
    V.base = static_cast<const T*>(a.lf) + (a.u0 + u) * a.st[0] + (a.v0 + v) * a.st[1];
    V.sh = a.st[2]; V.sw = a.st[3]; V.sc = a.st[4];
    V.zs = nullptr; V.r0 = V.c0 = 0; V.nr = V.nc = 0;

    // rows / columns of the view that this tile's taps read
    if (tid < 4) rng[tid] = (tid & 1) ? -1 : 0x7fffffff;
    __syncthreads();
    for (int i = tid; i < ny * a.ph; i += 256) {
        const int r = min(max(a.ih[(size_t)(oy0 + i / a.ph) * a.ph + i % a.ph], 0), a.H - 1);
        atomicMin(&rng[0], r); atomicMax(&rng[1], r);
    }
    for (int i = tid; i < nx * a.pw; i += 256) {
        const int c = min(max(a.iw[(size_t)(ox0 + i / a.pw) * a.pw + i % a.pw], 0), a.W - 1);
        atomicMin(&rng[2], c); atomicMax(&rng[3], c);
    }
    __syncthreads();
    const int r0 = rng[0], nr = rng[1] - r0 + 1, c0 = rng[2], nc = rng[3] - c0 + 1;
    const bool staged = nr <= kColSpan && nc <= kColSpan;
    if (staged) {
        for (int i = tid; i < nr * nc; i += 256) {
            const T* p = V.base + (r0 + i / nc) * V.sh + (c0 + i % nc) * V.sw;
            for (int ch = ch0; ch < 3; ++ch) zs[ch * kColSpan * kColSpan + i] = col_ycc(p, V.sc, ch);
        }
        V.zs = zs; V.r0 = r0; V.c0 = c0; V.nr = nr; V.nc = nc;
    }
    __syncthreads();

    // row pass into LDS: ts[ch][oy][c - c0] for the tile's rows and every column the column pass reads
    const bool tstaged = nc <= kColSpan;
    if (tstaged)
        for (int i = tid; i < (3 - ch0) * ny * nc; i += 256) {
            const int ch = ch0 + i / (ny * nc), oy = (i / nc) % ny, cc = i % nc;
            ts[(ch * kColTile + oy) * kColSpan + cc] = V.hsum(a, ch, oy0 + oy, c0 + cc);
        }
    __syncthreads();

    // column pass, inverse transform, quantisation: the tile's pixels, interleaved, into LDS
    const size_t view = (size_t)u * a.A + v;
    uint8_t* ob8 = reinterpret_cast<uint8_t*>(ob);
    for (int p = tid; p < ny * nx; p += 256) {
        const int oy = p / nx, ox = p % nx;
        const double* w = a.ww + (size_t)(ox0 + ox) * a.pw;
        const int* ix = a.iw + (size_t)(ox0 + ox) * a.pw;
        double z[3];
        for (int ch = ch0; ch < 3; ++ch) {
            double acc = 0.0;
            for (int k = 0; k < a.pw; ++k) {
                const int c = min(max(ix[k], 0), a.W - 1);
                const double t = tstaged ? ts[(ch * kColTile + oy) * kColSpan + (c - c0)] : V.hsum(a, ch, oy0 + oy, c);
                acc = k == 0 ? w[k] * t : acc + w[k] * t;
            }
            z[ch] = acc;
        }
        if (a.sr_y) z[0] = (double)a.sr_y[((size_t)u * OH + oy0 + oy) * ((size_t)a.A * OW) + (size_t)v * OW + ox0 + ox];
        const double e0 = 255.0 * z[0] - 16.0, e1 = 255.0 * z[1] - 128.0, e2 = 255.0 * z[2] - 128.0;
        for (int j = 0; j < 3; ++j) {
            const double c = (a.minv[3 * j] * e0 + a.minv[3 * j + 1] * e1) + a.minv[3 * j + 2] * e2;
            if (a.out_f32) ob[p * 3 + j] = (float)c;
            else ob8[p * 3 + j] = (uint8_t)(int)rint(255.0 * fmin(fmax(c, 0.0), 1.0));    // convertDouble2Byte
        }
    }
    __syncthreads();

    const int nb = nx * 3;                                          // elements of one tile row, contiguous in the output
    if (a.out_f32) {
        float* o = static_cast<float*>(a.out);
        for (int i = tid; i < ny * nb; i += 256)
            o[((view * OH + oy0 + i / nb) * OW + ox0) * 3 + i % nb] = ob[i];
        return;
    }
    // bytes: the 4-byte-aligned middle of every row goes out as whole dwords, the up to 3 bytes before and after it one by one
    for (int i = tid; i < ny * kColSlots; i += 256) {
        const int row = i / kColSlots, k = i % kColSlots;
        uint8_t* g = static_cast<uint8_t*>(a.out) + ((view * OH + oy0 + row) * OW + ox0) * 3;
        const uint8_t* l = ob8 + row * nb;
        const int head = min(nb, (int)((4 - (reinterpret_cast<uintptr_t>(g) & 3)) & 3)), ndw = (nb - head) / 4;
        if (k < ndw) {
            const uint8_t* q = l + head + 4 * k;
            *reinterpret_cast<uint32_t*>(g + head + 4 * k) = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
        } else if (k == kColSlots - 2) {
            for (int j = 0; j < head; ++j) g[j] = l[j];
        } else if (k == kColSlots - 1) {
            for (int j = head + 4 * ndw; j < nb; ++j) g[j] = l[j];
        }
    }
}

}  // namespace
