// lft_refocus.cuh -- synthetic refocus: a focal stack from the A x A views of a light field by shift-and-add.
//
//   R_d[y, x, c] = sum_{u,v} a[u,v] * S(L[u,v,:,:,c], y + d*(u-uc), x + d*(v-uc)),   uc = (A-1)/2,
//
// d the slope in pixels per view step.  Every view's shift is constant, so S is a separable FIR of TAPS = 1 (nearest), 2 (linear)
// or 4 (Keys cubic) taps whose coefficients depend on (slope, view) only: the caller's table (lft_amd/refocus.py:shift_table, the
// record below) holds them, computed in fp64 and rounded once to fp32.  Tap indices are clamped into the view (replicate).
//
//   k_refocus  one launch per focal stack; 1-D grid over (batch element, output tile 32 x 32, slope), the slope fastest and the
//              ids dealt XCD-aware (xcd_tile), so that the slopes of one tile, which read overlapping windows, follow each other
//              on one L2.  Per view of non-zero weight the workgroup reads the (32 + TAPS - 1)^2 window its taps touch -- whole
//              window rows, element by element as the interleaved channels lie, lane j at element j of a row, as many rows per
//              pass as fit 256 lanes -- into registers, and from there as fp32 into LDS.  The row pass (taps over y) writes an
//              LDS intermediate, the column pass (taps over x) accumulates a * s into 4*C registers per lane.
//              The loads of the next view's window are issued before the current
//              view is filtered and land in LDS after its row pass, when no lane reads the window any more: one window buffer
//              is enough for the overlap.  fp32 output goes out from the registers (lanes at consecutive addresses), uint8 is
//              assembled in LDS and stored as whole dwords (k_colour_merge's scheme).  No temporaries in memory.
// Both passes index LDS by ELEMENT (x*C + c), lane i at element i of a row: consecutive lanes hit consecutive banks for any C
// (a lane-per-pixel layout at C = 3 would stride 3 banks and need padding), apart from the one lane group per row where the
// item index wraps to the next row.
// Sums run over the views in (u, v) order and over the taps in table order, every step after a sum's first product one explicit
// fused multiply-add (the compiler's own contraction is off): a pixel's bits do not depend on the tile, the image size around it
// or the launch shape.
// Shared with the other light-field kernels from here: rf_x (an input element as fp32) and rf_byte (the uint8 output rule), each
// written once.  The window pipeline of k_refocus is not shared: k_sweep_cost (lft_disparity.cuh) holds a copy, on a measurement
// (DESIGN.md section 10).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lft_common.cuh"

namespace {

constexpr int kRfTile = 32;          // output tile
constexpr int kRfRec = 12;           // dwords per table record (lft_refocus_record of include/lft_hip.h)
constexpr int kRfRows = 4;           // output rows per row-pass item: 4 + TAPS - 1 LDS reads for 4 results
constexpr int kRfSlots = 34;         // store slots per uint8 tile row: up to 32 whole dwords, then one each for head and tail bytes

struct RefocusArgs {
    const void* lf;
    long long st[3];                 // element strides of (b, u, v)
    int sy, sx, sc;                  // element strides of (y, x, c): a view spans less than 2^31 elements
    int A, H, W, D, tiles_x, tiles;
    const int* table;                // [D, A*A] records
    void* out;                       // [B, D, H, W, C]
    int out_f32;
};

template <typename T> __device__ __forceinline__ float rf_x(T v) { return (float)v; }
// v / 255, correctly rounded for every byte (tests/test_gpu_refocus.py::test_identities): the product with fl(1/255) and one
// correction step, a third of the instructions of the division
template <> __device__ __forceinline__ float rf_x<uint8_t>(uint8_t v) {
    const float b = (float)v, r = 1.0f / 255.0f, q = b * r;
    return __fmaf_rn(__fmaf_rn(-q, 255.0f, b), r, q);
}
// the byte of a value: convertDouble2Byte's rule in fp32 -- clip to [0, 1], * 255, round half to even.  The one place it is written:
// refocus, the all-in-focus gather of both picks and both renders store their uint8 output through it
__device__ __forceinline__ uint8_t rf_byte(float v) { return (uint8_t)(int)rintf(255.0f * fminf(fmaxf(v, 0.0f), 1.0f)); }

template <typename T, int C, int TAPS>
__global__ __launch_bounds__(256) void k_refocus(RefocusArgs a) {
#pragma clang fp contract(off)
    constexpr int NR = kRfTile + TAPS - 1;                           // window rows (and pixels per window row)
    constexpr int RW = NR * C;                                       // elements of a window row
    constexpr int NE = NR * RW;                                      // window elements
    constexpr int RP = 256 / RW, NLD = (NR + RP - 1) / RP;           // window rows per pass of the 256 lanes; passes
    static_assert(RP >= 1, "a window row is loaded by one pass of the workgroup");
    constexpr int OW = kRfTile * C, NACC = kRfTile * OW / 256;       // elements of an output row; accumulators per lane (4*C)
    constexpr int NITEM = (kRfTile / kRfRows) * RW;                  // row-pass items
    __shared__ float win[NE];                                        // the current view's window; at the end the uint8 tile
    __shared__ float tmp[kRfTile * RW];                              // row pass of the window
    static_assert(NE * 4 >= kRfTile * kRfTile * C, "the uint8 tile is assembled in the window buffer");

    const int tid = threadIdx.x;
    const int bid = xcd_tile(blockIdx.x, gridDim.x);
    const int d = bid % a.D, tile = (bid / a.D) % a.tiles, b = bid / (a.D * a.tiles);
    const int y0 = (tile / a.tiles_x) * kRfTile, x0 = (tile % a.tiles_x) * kRfTile;
    const int ny = min(kRfTile, a.H - y0), nx = min(kRfTile, a.W - x0);
    const int nv = a.A * a.A;
    const int* recs = a.table + (size_t)d * nv * kRfRec;
    const T* lfb = static_cast<const T*>(a.lf) + b * a.st[0];

    const int prow = tid / RW, pj = tid % RW, pxw = pj / C, pc = pj % C;     // this lane's row of a pass and element of the row
    T stage[NLD];
    float acc[NACC];
#pragma unroll
    for (int r = 0; r < NACC; ++r) acc[r] = 0.0f;

    auto next_active = [&](int n) {                                  // the first view >= n of non-zero weight
        while (n < nv && recs[n * kRfRec + 11]) ++n;
        return n;
    };
    auto fetch = [&](int n) {                                        // view n's window -> registers
        // the window's origin, kept within 64 pixels of the view: rows and columns beyond clamp to the same pixel either way
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
    auto commit = [&]() {                                            // registers -> LDS, as fp32
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
        if (nxt < nv) fetch(nxt);                                    // in flight while this view is filtered
        const float* wf = reinterpret_cast<const float*>(recs + cur * kRfRec);
        float wy[TAPS], wx[TAPS];
#pragma unroll
        for (int k = 0; k < TAPS; ++k) { wy[k] = wf[2 + k]; wx[k] = wf[6 + k]; }
        const float aw = wf[10];

        // row pass: tmp[y][j] = sum_k wy[k] * win[y + k][j]
        for (int i = tid; i < NITEM; i += 256) {
            const int yg = (i / RW) * kRfRows, j = i % RW;
            float w[kRfRows + TAPS - 1];
#pragma unroll
            for (int q = 0; q < kRfRows + TAPS - 1; ++q) w[q] = win[(yg + q) * RW + j];
#pragma unroll
            for (int q = 0; q < kRfRows; ++q) {
                float s = wy[0] * w[q];
#pragma unroll
                for (int k = 1; k < TAPS; ++k) s = __fmaf_rn(wy[k], w[q + k], s);
                tmp[(yg + q) * RW + j] = s;
            }
        }
        __syncthreads();
        // column pass: acc[y][e] += a * sum_k wx[k] * tmp[y][e + k*C], e = x*C + c
#pragma unroll
        for (int r = 0; r < NACC; ++r) {
            const int i = tid + 256 * r;
            const float* t = tmp + (i / OW) * RW + i % OW;
            float s = wx[0] * t[0];
#pragma unroll
            for (int k = 1; k < TAPS; ++k) s = __fmaf_rn(wx[k], t[k * C], s);
            acc[r] = __fmaf_rn(aw, s, acc[r]);
        }
        if (nxt < nv) commit();                                      // every lane is past the row pass: the window is free
        __syncthreads();
        cur = nxt;
    }

    const size_t obase = ((size_t)b * a.D + d) * a.H * a.W * C;      // elements
    const int nb = nx * C;                                           // elements of one tile row, contiguous in the output
    if (a.out_f32) {
        float* o = static_cast<float*>(a.out) + obase;
#pragma unroll
        for (int r = 0; r < NACC; ++r) {
            const int i = tid + 256 * r, y = i / OW, e = i % OW;
            if (y < ny && e < nb) o[((size_t)(y0 + y) * a.W + x0) * C + e] = acc[r];
        }
        return;
    }
    // bytes: convertDouble2Byte's rule in fp32, the tile assembled in LDS
    uint8_t* ob8 = reinterpret_cast<uint8_t*>(win);
#pragma unroll
    for (int r = 0; r < NACC; ++r) {
        const int i = tid + 256 * r, y = i / OW, e = i % OW;
        if (y < ny && e < nb) ob8[y * nb + e] = rf_byte(acc[r]);
    }
    __syncthreads();
    // the 4-byte-aligned middle of every row goes out as whole dwords, the up to 3 bytes before and after it one by one
    for (int i = tid; i < ny * kRfSlots; i += 256) {
        const int row = i / kRfSlots, k = i % kRfSlots;
        uint8_t* g = static_cast<uint8_t*>(a.out) + obase + ((size_t)(y0 + row) * a.W + x0) * C;
        const uint8_t* l = ob8 + row * nb;
        const int head = min(nb, (int)((4 - (reinterpret_cast<uintptr_t>(g) & 3)) & 3)), ndw = (nb - head) / 4;
        if (k < ndw) {
            const uint8_t* q = l + head + 4 * k;
            *reinterpret_cast<uint32_t*>(g + head + 4 * k) = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
        } else if (k == kRfSlots - 2) {
            for (int j = 0; j < head; ++j) g[j] = l[j];
        } else if (k == kRfSlots - 1) {
            for (int j = head + 4 * ndw; j < nb; ++j) g[j] = l[j];
        }
    }
}

// the instantiation for an input type, channel count (1 .. 4) and tap count (1, 2, 4)
template <typename T>
inline void (*refocus_kernel(int C, int taps))(RefocusArgs) {
    static void (*const k[4][3])(RefocusArgs) = {{k_refocus<T, 1, 1>, k_refocus<T, 1, 2>, k_refocus<T, 1, 4>},
                                                 {k_refocus<T, 2, 1>, k_refocus<T, 2, 2>, k_refocus<T, 2, 4>},
                                                 {k_refocus<T, 3, 1>, k_refocus<T, 3, 2>, k_refocus<T, 3, 4>},
                                                 {k_refocus<T, 4, 1>, k_refocus<T, 4, 2>, k_refocus<T, 4, 4>}};
    return k[C - 1][taps == 4 ? 2 : taps - 1];
}

}  // namespace
