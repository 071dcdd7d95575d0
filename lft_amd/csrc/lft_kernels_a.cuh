// lft_kernels_a.cuh -- weight packing, position tables, initial convolutions, angular Transformer.
#pragma once
#include "lft_common.cuh"

namespace {

// ------------------------------------------------------------------------------------------
// Weight packing.  A stream is a sequence of fragments in exactly the order a kernel consumes
// them.  One PackOp describes ntiles x ksteps fragments (nt-major) cut from a row-major fp32 matrix:
//   frag(nt, ks)[lane = 32h + r][j] = scale * src[(row0 + 32 nt + r) * ld + (k0 + 16 ks + kk(h, j)) * kmul + kadd]
// kmap 0: natural kk = 8h + j (operand loaded from memory); kmap 1: acc order (see lft_common.cuh).
// kind 1 (UPM) builds the "overlap-add" matrix of the final 3x3 convolution instead (see k_up); kind 2 its transpose.
// ------------------------------------------------------------------------------------------
struct PackOp {
    const float* src;
    int kind, row0, nrows, ntiles, ld, kmul, kadd, k0, ksteps, kmap, frag0, s;
    float scale;
    int order;     // 0: nt-major (frag = nt * ksteps + ks); 1: groups of 4 output tiles, inside a group ks-major (wfrag_index): the
                   // fragments one workgroup of the training GEMM consumes are then ONE contiguous stream in consumption order
};
// Fragment (ot, ks) of a matrix of OT output tiles packed with order 1: groups of four tiles (the last one may hold fewer),
// group g at 4 g KS, inside it k-step-major.
__host__ __device__ __forceinline__ int wfrag_index(int OT, int KS, int ot, int ks) {
    const int g = ot >> 2, G = OT - 4 * g < 4 ? OT - 4 * g : 4;
    return 4 * g * KS + ks * G + (ot & 3);
}
__host__ __device__ __forceinline__ void wfrag_coords(int OT, int KS, int lf, int order, int& nt, int& ks) {
    if (!order) { nt = lf / KS; ks = lf % KS; return; }
    const int gl = (OT - 1) >> 2, g = lf / (4 * KS) < gl ? lf / (4 * KS) : gl, G = OT - 4 * g < 4 ? OT - 4 * g : 4, rem = lf - 4 * g * KS;
    ks = rem / G; nt = 4 * g + rem % G;
}
constexpr int LFT_PACK_MAXOPS = 40;
struct PackArgs {
    int nops;
    PackOp op[LFT_PACK_MAXOPS];
};

// Row n = (I+1)*(s+2) + (J+1), I,J in [-1, s]: HR position relative to the s x s block of one LR pixel.
// Column kk = c*s*s + i*s + j: PixelShuffle source channel (reference LFT.py:41).  Entry = W3[c][i-I+1][j-J+1]
// when that tap exists: out[Y] = sum_dy W3[dy+1] F[Y+dy]  (reference LFT.py:43, cross-correlation, pad 1).
LFT_DEV float upm_entry(const float* __restrict__ w3, int n, int kk, int s) {
    const int I = n / (s + 2) - 1, J = n % (s + 2) - 1;
    const int c = kk / (s * s), i = (kk / s) % s, j = kk % s;
    const int dy = i - I, dx = j - J;
    if (dy < -1 || dy > 1 || dx < -1 || dx > 1) return 0.0f;
    return w3[c * 9 + (dy + 1) * 3 + (dx + 1)];
}

template <typename T>
__global__ __launch_bounds__(64) void k_pack(PackArgs args, T* __restrict__ dst) {
    const int f = blockIdx.x, lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    int oi = 0;
    for (int i = 0; i < args.nops; ++i)
        if (f >= args.op[i].frag0) oi = i;
    const PackOp& op = args.op[oi];
    int nt, ks;
    wfrag_coords(op.ntiles, op.ksteps, f - op.frag0, op.order, nt, ks);
    const int n = 32 * nt + r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int kk = op.k0 + 16 * ks + (op.kmap ? 8 * (j >> 2) + 4 * h + (j & 3) : 8 * h + j);
        float v = 0.0f;
        if (n < op.nrows) {
            if (op.kind == 0) v = op.scale * op.src[(size_t)(op.row0 + n) * op.ld + kk * op.kmul + op.kadd];
            else if (op.kind == 1) v = upm_entry(op.src, n, kk, op.s);
            else v = kk < (op.s + 2) * (op.s + 2) ? upm_entry(op.src, kk, n, op.s) : 0.0f;   // kind 2: the transposed matrix (rows = PixelShuffle channels)
        }
        if constexpr (sizeof(T) == 4) dst[(((size_t)f * 2 + (j >> 2)) * 64 + lane) * 4 + (j & 3)] = (T)v;   // two 1 KiB pieces
        else dst[((size_t)f * 64 + lane) * 8 + j] = (T)v;
    }
}

// Sinusoid position tables (reference LFT.py:91-115): channel c < 32 -> sin(l / T^(2c/64)),
// c >= 32 -> cos(l / T^(2(c-32)/64)).  Angular table [V][64] fp32; spatial image [h*w][64] = (PE_h[y]+PE_w[x])/2.
LFT_DEV float pe_value(int l, int c) {
    const int m = c & 31;
    const float g = (float)pow(10000.0, (double)(2 * m) / 64.0);
    const float p = (float)l / g;
    return (c < 32) ? (float)sin((double)p) : (float)cos((double)p);
}
// Angular table: lane-major fp32 (see load_lane_major_raw): [view tile][k = 0..3][lane][8].
template <typename T>
__global__ void k_pe_tables(float* __restrict__ ang_pe, T* __restrict__ spa_img, int V, int h, int w) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int ntile = (V + 31) / 32;
    if (idx < ntile * 2048) {
        const int e = idx & 7, lane = (idx >> 3) & 63, k = (idx >> 9) & 3, ct = idx >> 11;
        const int view = ct * 32 + (lane & 31), nt = k >> 1, g = 2 * (k & 1) + (e >> 2);
        const int ch = 32 * nt + 8 * g + 4 * (lane >> 5) + (e & 3);
        ang_pe[idx] = view < V ? pe_value(view, ch) : 0.0f;
    }
    if (idx < h * w * 64) {
        const int p = idx >> 6, c = idx & 63;
        spa_img[idx] = (T)((pe_value(p / w, c) + pe_value(p % w, c)) / 2.0f);
    }
}

// ------------------------------------------------------------------------------------------
// conv_init0: 1 -> 64 channels, per-view 3x3, zero pad per view (reference LFT.py:23-25,65).
// Reads the LR mosaic [B,1,A*h,A*w] (view (a1,a2) is the block at rows a1*h.., cols a2*w.. -- LFT.py:58),
// writes channels-last tokens [B,V,h,w,64].  One thread = 8 channels of one token.
// ------------------------------------------------------------------------------------------
constexpr int kConv0Tok = 128;          // tokens per workgroup
// View (a1, a2) of image b inside the LR mosaic [B,1,A*h,A*w]; row stride A*w.
LFT_DEV const float* lr_view(const float* __restrict__ lr, int im, int A, int h, int w) {
    const int V = A * A, b = im / V, v = im - b * V, a1 = v / A, a2 = v - a1 * A;
    return lr + (size_t)b * (A * h) * (A * w) + (size_t)(a1 * h) * (A * w) + a2 * w;
}
// The nine taps of one token, branch-free: all are loaded from clamped (readable) positions and masked at use -- a conditional
// load is a masked branch per tap, nine dependent round trips instead of nine loads in flight.
LFT_DEV void conv0_taps_load(const float* __restrict__ img, int ldi, int y, int x, int h, int w, float (&val)[9]) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {                                           // clamped (readable) positions; masked at use
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        val[t] = img[min(max(yy, 0), h - 1) * ldi + min(max(xx, 0), w - 1)];
    }
}
template <typename T>
__global__ __launch_bounds__(256) void k_conv0(const float* __restrict__ lr, const float* __restrict__ w0,
                                               T* __restrict__ out, int B, int A, int h, int w) {
    // grid: x = kConv0Tok-token groups of one view image, y = image (b, v).  32-bit index math only.
    // The 64 x 9 weights, 72 of them per thread: the kernel was bound by these LDS reads (72 ds_read_b32 per thread, 2-way
    // bank conflicts).  9 taps padded to 12 floats per channel = three 16-byte reads; channel groups 100 floats apart put the
    // eight distinct addresses of a 16-lane group on disjoint banks.
    __shared__ __attribute__((aligned(16))) float wl[8 * 100];
    const int hw = h * w, im = blockIdx.y;
    const int cg = threadIdx.x & 7;
    const float* img = lr_view(lr, im, A, h, w);
    // kConv0Tok tokens per workgroup, 32 per pass: the weight staging and the barrier above are paid once per 128 tokens
    // (3 200 workgroups of 32 tokens spent most of their time in that prologue).
    // The kernel is a latency chain, not a throughput problem (13 MB out, 60 MFLOP): round 4 issues the taps of ALL passes before
    // the first use -- one memory round trip per workgroup instead of one per pass (four, each behind the previous pass's compute).
    constexpr int NP = kConv0Tok / 32;
    float val[NP][9];
#pragma unroll
    for (int pass = 0; pass < NP; ++pass) {
        const int p = min(blockIdx.x * kConv0Tok + pass * 32 + (int)(threadIdx.x >> 3), hw - 1);
        const int y = p / w, x = p - y * w;
        conv0_taps_load(img, A * w, y, x, h, w, val[pass]);
    }
    {   // all three loads of a thread in flight before the first LDS write (as a load / wait / write loop: three serialised round trips)
        float wv[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) wv[k] = w0[min((int)threadIdx.x + 256 * k, 575)];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = (int)threadIdx.x + 256 * k, ch = i / 9, t = i - ch * 9;
            if (i < 576) wl[(ch >> 3) * 100 + (ch & 7) * 12 + t] = wv[k];
        }
    }
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < NP; ++pass) {
        // The empty asm names a pass's nine values at once: it keeps hipcc from sinking the loads back under their conditions.
        asm volatile("" : "+v"(val[pass][0]), "+v"(val[pass][1]), "+v"(val[pass][2]), "+v"(val[pass][3]), "+v"(val[pass][4]), "+v"(val[pass][5]),
                          "+v"(val[pass][6]), "+v"(val[pass][7]), "+v"(val[pass][8]));
        const int p = blockIdx.x * kConv0Tok + pass * 32 + (threadIdx.x >> 3);
        if (p >= hw) return;
        const int y = p / w, x = p - y * w;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
            val[pass][t] = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? val[pass][t] : 0.0f;
        }
        f32x4 o[2];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const f32x4* wq = reinterpret_cast<const f32x4*>(wl + cg * 100 + c * 12);
            const f32x4 w03 = wq[0], w47 = wq[1], w8 = wq[2];
            float a = 0.0f;                                              // same order of additions as before: bit-identical results
#pragma unroll
            for (int t = 0; t < 4; ++t) a += w03[t] * val[pass][t];
#pragma unroll
            for (int t = 0; t < 4; ++t) a += w47[t] * val[pass][4 + t];
            a += w8[0] * val[pass][8];
            o[c >> 2][c & 3] = a;
        }
        T* row = out + ((size_t)im * hw + p) * 64 + cg * 8;
        if constexpr (sizeof(T) == 2) {                              // one 16-byte store per thread: a wave writes 1 KiB of whole lines
            typename H16<T>::v8 v;
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = (T)o[c >> 2][c & 3];
            store_raw16(reinterpret_cast<char*>(row), __builtin_bit_cast(raw16, v));
        } else {
            store4(row, o[0]);
            store4(row + 4, o[1]);
        }
    }
}

// ------------------------------------------------------------------------------------------
// Per-view 3x3 convolution, 64 -> 32*NT channels, as an implicit GEMM.  A workgroup owns 128
// consecutive tokens of one view image (4 waves x 32 tokens); K = 9 taps x 64 channels = 36 k-steps.
//  * input: the 128 tokens plus a halo of w+1 tokens on either side are brought into LDS ONCE (each token row is
//    re-read by up to 9 taps) by LDS-DMA: no registers, no round trip before the data is needed, and it
//    shares one wait with the first weight chunks.  LDS-DMA writes lane-linear 1 KiB pieces, so rows are
//    unpadded (128 B bf16 / 256 B fp32) and bank conflicts are removed by an XOR swizzle applied on the
//    per-lane SOURCE address and again on the read (16-byte piece c of slot s lives at piece c ^ f(s)):
//    conflict-free for every tile alignment (checked exhaustively offline; unswizzled it is 8- / 16-way).
//    Tokens outside the image are fetched from a clamped address and never used: the lane predicate zeroes
//    them, as it does at the left/right image border (per-view zero padding, reference LFT.py:24,27,167).
//  * weights: the fragment stream ((tap*4 + ks) * NT + nt) arrives through the workgroup's LDS ring.
// ------------------------------------------------------------------------------------------
template <typename T, int NW = 4> struct ConvIn {     // NW waves x 32 tokens per workgroup tile
    static constexpr int ROW_BYTES = 64 * (int)sizeof(T);
    static constexpr int PPR = ROW_BYTES / 16;                       // 16-byte pieces per token row (8 / 16)
    static constexpr int SLOTS_PER_DMA = 1024 / ROW_BYTES;           // token rows per 1 KiB LDS-DMA piece (8 / 4)
    static __host__ __device__ int slots(int w) { return 32 * NW + 2 + 2 * w; }
    static __host__ __device__ int dma_pieces(int w) { return (slots(w) + SLOTS_PER_DMA - 1) / SLOTS_PER_DMA; }
    static __host__ __device__ int bytes(int w) { return dma_pieces(w) * 1024; }
    static __device__ __forceinline__ int swz(int slot) { return sizeof(T) == 2 ? ((slot >> 1) & 7) : (slot & 15); }
};

// Issues the DMA only; the caller waits (vmcnt) and publishes (barrier) before the first read.
template <typename T, int NW = 4>
LFT_DEV void stage_conv_input(const T* __restrict__ img, int p0, int hw, int w, char* lds_in) {
    using CI = ConvIn<T, NW>;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int npieces = CI::dma_pieces(w);
    LFT_NOTE_ASM_("DMA", kNoteConvIn, 0);
    for (int piece = wave; piece < npieces; piece += NW) {
        const int slot = piece * CI::SLOTS_PER_DMA + lane / CI::PPR, cpos = lane % CI::PPR;
        const int q = min(max(p0 - w - 1 + slot, 0), hw - 1);                       // clamped: out-of-image rows are masked at use
        const char* src = reinterpret_cast<const char*>(img) + ((size_t)q * CI::ROW_BYTES + ((cpos ^ CI::swz(slot)) * 16));
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(lds_in + piece * 1024), 16, 0, 0);
    }
}
LFT_DEV void wait_staged() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }   // own DMA pieces and early loads landed

// tl = token index inside the workgroup tile (0..127); (y, x) its image coordinates.
// Taps that fall outside the image (per-view zero padding) read a row of zeros (`zero_row`, kConvZeroRow bytes the caller
// cleared before publishing the tile) instead of being masked in registers: one select on the row address per tap
// instead of one per fragment register (16 v_cndmask per tap).
constexpr int kConvZeroRow = 256;
LFT_DEV void clear_zero_row(char* zero_row) {                          // call before the barrier that publishes the input tile
    if (threadIdx.x < kConvZeroRow / 16) store_raw16(zero_row + threadIdx.x * 16, raw16{0u, 0u, 0u, 0u});
}
template <int NT, typename T, int NW, typename Ring>
LFT_DEV void conv3x3_tile(const char* lds_in, const char* zero_row, int tl, int y, int x, bool ok, int h, int w, int hh,
                          Ring& ring, f32x16 (&acc)[NT]) {
    using CI = ConvIn<T, NW>;
    static_assert(CI::ROW_BYTES <= kConvZeroRow, "zero row too short");
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        const int yy = y + dy, xx = x + dx;
        const bool inb = ok && yy >= 0 && yy < h && xx >= 0 && xx < w;
        const int slot = tl + w + 1 + dy * w + dx;
        const char* row = inb ? lds_in + slot * CI::ROW_BYTES : zero_row;
        const int sw = inb ? CI::swz(slot) : 0;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            Frag<T> b;
            if constexpr (sizeof(T) == 2) {
                b.v = __builtin_bit_cast(typename H16<T>::v8, load_raw16(row + (((2 * ks + hh) ^ sw) * 16)));
            } else {
                b.lo = __builtin_bit_cast(f32x4, load_raw16(row + (((4 * ks + 2 * hh) ^ sw) * 16)));
                b.hi = __builtin_bit_cast(f32x4, load_raw16(row + (((4 * ks + 2 * hh + 1) ^ sw) * 16)));
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) mma(ring.next(), b, acc[nt]);
        }
    }
}
template <int NT> LFT_DEV void lrelu_acc(f32x16 (&a)[NT]) {            // LeakyReLU(0.2)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 16; ++i) a[nt][i] = lrelu02_fast(a[nt][i]);
}

// A workgroup's tile of NW x 32 consecutive tokens of one view image, and this lane's place in it (k_conv64, k_conv64_lr,
// k_conv0_recomputed, k_spa1).  Lane = token r of wave `wave` (MFMA column), hh its row half.  Neighbouring tiles share halo rows,
// so xcd_tile puts them on one XCD.  SWAVE: the wave index as a scalar, for a loop that strides by it (k_conv64_lr).
template <int NW, bool SWAVE = false> struct ViewTile {
    int lane, r, hh, wave, hw, im, p0, tl, p, t0, nvalid;
    bool ok;
    __device__ __forceinline__ ViewTile(int h, int w) {
        constexpr int TT = 32 * NW;                                       // tokens per workgroup tile
        lane = threadIdx.x & 63; r = lane & 31; hh = lane >> 5;
        wave = SWAVE ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : threadIdx.x >> 6;
        hw = h * w;
        const int tpi = (hw + TT - 1) / TT, bid = xcd_tile(blockIdx.x, gridDim.x);
        im = bid / tpi; p0 = (bid % tpi) * TT;
        tl = wave * 32 + r; p = p0 + tl;                                  // token inside the tile, inside the image
        ok = p < hw;
        t0 = p0 + wave * 32; nvalid = max(0, min(32, hw - t0));           // this wave's 32 consecutive tokens
    }
    __device__ __forceinline__ size_t tile_off(int ch) const { return ((size_t)im * hw + min(t0, hw - 1)) * ch; }   // of [token][ch]
};

// conv_init[i]: 64 -> 64 + LeakyReLU(0.2); the last one adds conv_init0's output (reference LFT.py:26-33,66).
// A workgroup = NW waves x 32 consecutive tokens of one view image; all its waves share one weight ring, so the
// packed weights are streamed into the CU once per 32*NW tokens.
constexpr int kNwConv = 4;
constexpr int kConv64Chunk = 12;   // 72 fragments: 6 chunks of 12, 3-slot ring = 36 KiB (bf16) so two workgroups share a CU

// ------------------------------------------------------------------------------------------
// The 16-bit front end computes conv_init0 where its output is consumed, from the LR pixels, instead of writing
// x0 to memory and reading it twice.  conv_init0 (1 -> 64) has no bias and no activation (reference LFT.py:23-25,65),
// so with lr~ = the view's LR image, zero outside it:
//   x0(q)[c] = sum_t0 w0[c,t0] lr~(q+t0)
//   a(p)[o]  = sum_t1 [p+t1 inside the view] sum_c w1[o,c,t1] x0(p+t1)[c]
//            = sum_(t1,t0) [p+t1 inside the view] W01[o,t1,t0] lr~(p+t1+t0),   W01[o,t1,t0] = sum_c w1[o,c,t1] w0[c,t0]
// The bracket is the per-view zero padding of x0 in front of conv_init.0; it is applied to the B operand, so there are
// no border classes.  K = 81 (k = 9 t1 + t0) padded to 96 = 6 k-steps x 2 row tiles = one kConv64Chunk of fragments.
// Operand type of THIS product: IEEE half in both 16-bit precisions (ConvLrOp).  x0 used to be formed in fp32, so a filter
// whose taps nearly cancel on a smooth image (what training produces) kept its small response exactly; composed, the
// cancellation happens inside the product, on ROUNDED pixels and ROUNDED W01 entries, and 8 significant bits quantise
// a [0, 1] image like an 8-bit file (bf16 forward on trained weights: 0.027 dB from the oracle where 0.014 dB is the level
// of the other sites).  11 bits keep the first product at the fp16 path's level; LR pixels and W01 entries are far inside
// the half range (|lr| > 65504 would overflow).  The result is rounded to T where ta used to be stored, as before.
typedef f16_t ConvLrOp;
// ------------------------------------------------------------------------------------------
constexpr int kW01K = 96, kW01Frags = 12;
// Row rho of the composed matrix holds output channel conv01_row_channel(rho) (bits 2 and 3 exchanged): the accumulator
// of the W01 product, taken as fragments (acc_frags), then holds channels 16 ks + 8 h + j in element j of fragment ks
// -- the natural order of a token row in memory, so conv_init.2 consumes the tile with the stream it always had.
__host__ __device__ __forceinline__ int conv01_row_channel(int rho) { return (rho & ~12) | ((rho & 4) << 1) | ((rho & 8) >> 1); }
// LR pixels of a workgroup tile in LDS: the image rows of the tile's slots plus two rows above and below, two zero
// columns left and right; everything outside the view is stored as zero (lr~), so a 5 x 5 patch is 25 unconditional reads.
template <int NW> struct LrStage {
    static __host__ __device__ int width(int w) { return w + 4; }
    static __host__ __device__ int max_rows(int w) { return (32 * NW + 2 * w + 1) / w + 6; }    // slots span at most (TT + 2w + 1) / w + 2 rows
    static __host__ __device__ int bytes(int w) { return (max_rows(w) * width(w) * 4 + 15) & ~15; }
};
// conv_init0's weights in LDS as [tap][64] (kConv0WBytes), and conv_init0 for one token in accumulator layout with the
// arithmetic of k_conv0: the same fp32 order of additions, rounded to T and widened back -- bit-identical to the x0 it stores.
constexpr int kConv0WBytes = 9 * 64 * 4;
LFT_DEV void conv0_w_stage(const float* __restrict__ w0, float* wl) {       // the caller's barrier publishes it
    float wv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) wv[k] = w0[min((int)threadIdx.x + 256 * k, 575)];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = (int)threadIdx.x + 256 * k, ch = i / 9, t = i - ch * 9;
        if (i < 576) wl[t * 64 + ch] = wv[k];
    }
}
template <typename T>
LFT_DEV void conv0_token_acc(const float (&tap)[9], const float* wl, int y, int x, int h, int w, int hh, f32x16 (&rr)[2]) {
    float val[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        val[t] = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? tap[t] : 0.0f;
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 wq[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) wq[t] = __builtin_bit_cast(f32x4, load_raw16(reinterpret_cast<const char*>(wl + t * 64 + 32 * nt + 8 * g + 4 * hh)));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float a = 0.0f;                                              // k_conv0's order of additions
#pragma unroll
                for (int t = 0; t < 9; ++t) a += wq[t][j] * val[t];
                rr[nt][4 * g + j] = (float)(T)a;
            }
        }
}
struct ConvLr { const float* lr; const float* w0; int A; };   // RES == 2: LR mosaic, conv_init0 weights (fp32), angular resolution

// Dynamic LDS of k_conv64 and k_conv64_lr, byte offsets: weight ring | input tile | NW tile I/O scratches | zero row | extra.
// extra: conv_init0's weights (k_conv64<T, 2>) or the staged LR pixels (k_conv64_lr); one size, total_lr, serves both.
template <typename T, int NW = kNwConv> struct ConvLds {
    static constexpr int in = WRing<T, kConv64Chunk, NW>::LDS_BYTES;
    static __host__ __device__ int scr(int w, int wave) { return in + ConvIn<T, NW>::bytes(w) + wave * TileIO<2, T>::BYTES; }
    static __host__ __device__ int zero_row(int w) { return scr(w, NW); }
    static __host__ __device__ int extra(int w) { return zero_row(w) + kConvZeroRow; }
    static __host__ __device__ int total(int w) { return extra(w); }
    static __host__ __device__ int total_lr(int w) { return extra(w) + (LrStage<NW>::bytes(w) > kConv0WBytes ? LrStage<NW>::bytes(w) : kConv0WBytes); }
};

// RES: 0 no residual; 1 the residual tile is read from `res`; 2 the residual is conv_init0 of the LR pixels, recomputed
// (16-bit front end: x0 is never written).
template <typename T, int RES, int NW = kNwConv>
__global__ __launch_bounds__(64 * NW) void k_conv64(const T* __restrict__ in, T* __restrict__ out, const T* __restrict__ res,
                                                   const T* __restrict__ wstream, int nimg, int h, int w, ConvLr cl) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using L = ConvLds<T, NW>;
    const ViewTile<NW> t(h, w);
    const size_t tile_off = t.tile_off(64);
    char* lds_in = smem + L::in;
    char* scr = smem + L::scr(w, t.wave);                                             // wave-private tile I/O scratch
    char* zero_row = smem + L::zero_row(w);
    float* wl = reinterpret_cast<float*>(smem + L::extra(w));                         // RES == 2 only
    const int pc = min(t.p, t.hw - 1), yc = pc / w, xc = pc - yc * w;
    f32x16 rr[2];
    float tap[9];
    if constexpr (RES == 1) load_tile<2, T>(res + tile_off, t.nvalid, t.lane, rr, scr);   // first: its latency hides under the tile
    if constexpr (RES == 2) conv0_taps_load(lr_view(cl.lr, t.im, cl.A, h, w), cl.A * w, yc, xc, h, w, tap);
    WRing<T, kConv64Chunk, NW> ring;
    ring.init(wstream, smem, 72);
    stage_conv_input<T, NW>(in + (size_t)t.im * t.hw * 64, t.p0, t.hw, w, lds_in);
    clear_zero_row(zero_row);
    if constexpr (RES == 2) conv0_w_stage(cl.w0, wl);
    wait_staged();
    __syncthreads();                                                                 // ... and everybody else's
    LFT_NOTE_ASM_("USE", kNoteConvIn, 0);
    if constexpr (RES == 2) conv0_token_acc<T>(tap, wl, yc, xc, h, w, t.hh, rr);
    f32x16 acc[2];
    zero_acc<2>(acc);
    conv3x3_tile<2, T, NW>(lds_in, zero_row, t.tl, t.p / w, t.p % w, t.ok, h, w, t.hh, ring, acc);
    lrelu_acc<2>(acc);
    if constexpr (RES != 0) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[nt] += rr[nt];
    }
    store_tile<2, T>(out + tile_off, t.nvalid, t.lane, acc, scr);
}

// conv_init.0 composed with conv_init0, then conv_init.2: LR mosaic -> tb (16-bit precisions).  Same tile as k_conv64; the
// conv-input tile of conv_init.2 (ConvIn::slots(w) token rows, swizzled as conv3x3_tile reads them) is COMPUTED here
// instead of fetched: per 32 slots one masked B operand from the staged LR pixels, 12 half-precision MFMAs against W01, LeakyReLU,
// four 16-byte LDS stores per lane.  The column tiles of 32 slots are spread over the NW waves.  Stream: the 12 W01
// fragments (nt-major), then conv_init.2's 72 -- W01 is the first chunk of the ring, taken into registers by every wave.
// Slots outside the view and tokens beyond hw hold values of clamped positions; conv3x3_tile never uses them.
template <typename T, int NW = kNwConv>
__global__ __launch_bounds__(64 * NW) void k_conv64_lr(const float* __restrict__ lr, T* __restrict__ out, const T* __restrict__ wstream,
                                                      int A, int nimg, int h, int w) {
    static_assert(sizeof(T) == 2, "16-bit operand types only");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using CI = ConvIn<T, NW>;
    using L = ConvLds<T, NW>;
    constexpr int TT = 32 * NW;
    const ViewTile<NW, true> vt(h, w);
    char* lds_in = smem + L::in;
    char* scr = smem + L::scr(w, vt.wave);
    char* zero_row = smem + L::zero_row(w);
    float* lrs = reinterpret_cast<float*>(smem + L::extra(w));
    WRing<T, kConv64Chunk, NW> ring;
    ring.init(wstream, smem, kW01Frags + 72);
    // LR pixels: rows y_first - 2 .. y_last + 2 of the view, columns -2 .. w + 1
    const int nslots = CI::slots(w), LW = LrStage<NW>::width(w);
    const int y_first = max(vt.p0 - w - 1, 0) / w, y_last = min(vt.p0 + TT + w, vt.hw - 1) / w;
    {
        const float* img = lr_view(lr, vt.im, A, h, w);
        const int n = (y_last - y_first + 5) * LW, ldi = A * w;
        for (int i = threadIdx.x; i < n; i += 64 * NW) {
            const int row = i / LW, yy = y_first - 2 + row, xx = i - row * LW - 2;
            const float v = img[min(max(yy, 0), h - 1) * ldi + min(max(xx, 0), w - 1)];
            lrs[i] = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? v : 0.0f;
        }
    }
    clear_zero_row(zero_row);
    Frag<ConvLrOp> wf[kW01Frags];                                      // packed as ConvLrOp whatever T is: same 1 KiB pieces
#pragma unroll
    for (int i = 0; i < kW01Frags; ++i) wf[i].v = __builtin_bit_cast(H16<ConvLrOp>::v8, ring.next().v);   // the ring's first barrier also publishes the LR pixels
    for (int ct = vt.wave; ct * 32 < nslots; ct += NW) {
        const int slot = ct * 32 + vt.r;
        const int q = min(max(vt.p0 - w - 1 + slot, 0), vt.hw - 1), y = q / w, x = q - y * w;
        const float* pl = lrs + (y - y_first) * LW + x;                 // lr~(y - 2 + a, x - 2 + b) = pl[a * LW + b]
        float P[5][5];
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int b = 0; b < 5; ++b) P[a][b] = pl[a * LW + b];
        bool m[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
            m[t] = yy >= 0 && yy < h && xx >= 0 && xx < w;
        }
        auto masked = [&](int k) -> float {                             // B[k = 9 t1 + t0][slot]; k is a constant after unrolling
            if (k >= 81) return 0.0f;
            const int t1 = k / 9, t0 = k % 9;
            return m[t1] ? P[t1 / 3 + t0 / 3][t1 % 3 + t0 % 3] : 0.0f;
        };
        f32x16 a01[2];
        zero_acc<2>(a01);
#pragma unroll
        for (int ks = 0; ks < kW01K / 16; ++ks) {
            Frag<ConvLrOp> b;
#pragma unroll
            for (int j = 0; j < 8; ++j) b.v[j] = (ConvLrOp)(vt.hh ? masked(16 * ks + 8 + j) : masked(16 * ks + j));
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) mma(wf[nt * (kW01K / 16) + ks], b, a01[nt]);
        }
        lrelu_acc<2>(a01);
        Frag<T> of[4];
        acc_frags<2, T>(a01, of);
        if (slot < nslots) {
            char* row = lds_in + slot * CI::ROW_BYTES;
            const int sw = CI::swz(slot);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) store_raw16(row + (((2 * ks + vt.hh) ^ sw) * 16), __builtin_bit_cast(raw16, of[ks].v));
        }
    }
    wg_barrier_keep_vm();                                              // the computed tile is published (lgkmcnt(0) inside)
    f32x16 acc[2];
    zero_acc<2>(acc);
    conv3x3_tile<2, T, NW>(lds_in, zero_row, vt.tl, vt.p / w, vt.p % w, vt.ok, h, w, vt.hh, ring, acc);
    lrelu_acc<2>(acc);
    store_tile<2, T>(out + vt.tile_off(64), vt.nvalid, vt.lane, acc, scr);
}
// Test hook (lft_conv0_fwd): the residual tile k_conv64<T, 2> computes, written out as tokens [ntok][64].
template <typename T, int NW = kNwConv>
__global__ __launch_bounds__(64 * NW) void k_conv0_recomputed(T* __restrict__ out, int nimg, int h, int w, ConvLr cl) {
    __shared__ __attribute__((aligned(16))) char sm[kConv0WBytes + NW * TileIO<2, T>::BYTES];
    const ViewTile<NW> t(h, w);
    const int pc = min(t.p, t.hw - 1), yc = pc / w, xc = pc - yc * w;
    float* wl = reinterpret_cast<float*>(sm);
    float tap[9];
    conv0_taps_load(lr_view(cl.lr, t.im, cl.A, h, w), cl.A * w, yc, xc, h, w, tap);
    conv0_w_stage(cl.w0, wl);
    __syncthreads();
    f32x16 rr[2];
    conv0_token_acc<T>(tap, wl, yc, xc, h, w, t.hh, rr);
    store_tile<2, T>(out + t.tile_off(64), t.nvalid, t.lane, rr, sm + kConv0WBytes + t.wave * TileIO<2, T>::BYTES);
}

// ------------------------------------------------------------------------------------------
// Angular Transformer block, fully fused (reference AngTrans.forward, LFT.py:225-238).
// One wave = one spatial position (b, y, x); its V <= 32 views sit on the 32 MFMA columns.
//   n = LN(x + PE_v); Q = n Wq^T, K = n Wk^T (PE'd, normalised) ; V = x Wv^T (raw tokens, LFT.py:230-232)
//   per head (8 x 8 channels): S^T[kv, q] = K Q^T  -> softmax over kv -> O^T += V^T P^T
//   t = x + O Wo^T ;  t += W2 relu(W1 LN'(t))
// Everything stays in registers: Q^T/K^T accumulators are re-used as MFMA operands; V is produced
// with the operand roles swapped (tokens as A, weight as B) so that it lands view-on-row, which is
// what the P.V product needs as its A operand.  Heads are separated by zeroing half of a k-step
// (QK^T: 16 k values = 2 heads) or whole fragments by lane (P.V: 32 output rows = 4 heads).
// The softmax scale 1/sqrt(8) and log2(e) are folded into the packed Wq; exp2 is used.
// Stream: Wq[2x4] Wk[2x4] Wv[2x4] Wo[2x4] W1[4x4] W2[2x8]  (64 fragments) -- small enough to live
// in LDS for the whole kernel: a persistent workgroup DMAs it once and then walks over positions.
// ------------------------------------------------------------------------------------------
// The steps k_ang and k_ang_multi share, each written once.  A kernel hands over its operands through accessors: wfrag(f) is
// fragment f of the weight stream (k_ang: from LDS; k_ang_multi: from LDS or, fp32, from L2), vfrag(j, s2) the V operand of
// key tile j (k_ang: its own accumulators; k_ang_multi: what the waves published in LDS).  No helper holds a barrier.
constexpr int kLdsParams = 1024;   // 256 LayerNorm floats
// Dynamic LDS of both kernels, byte offsets: the 64 weight fragments (WLDS) | LayerNorm parameters | KV published K / V
// fragments | one tile I/O scratch per wave.  k_ang: <T, true, 0, 4>.
template <typename T, bool WLDS, int KV, int NWAVE> struct AngLds {
    static constexpr int FB = 1024 * FragInfo<T>::PIECES;              // bytes of one fragment
    static constexpr int ln = WLDS ? 64 * FB : 0, kv = ln + kLdsParams, scr = kv + KV * FB, total = scr + NWAVE * TileIO<2, T>::BYTES;
};
template <int NT_OUT, int KS, typename T, typename WF>
LFT_DEV void linear_frags(const WF& wfrag, int f0, const Frag<T> (&x)[KS], f32x16 (&y)[NT_OUT]) {
#pragma unroll
    for (int nt = 0; nt < NT_OUT; ++nt)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) mma(wfrag(f0 + nt * KS + ks), x[ks], y[nt]);
}
// n = LN(x + PE) of a tile of 32 views; nf: n as operand (Q, K), xf: the raw tokens as operand (V, reference LFT.py:230-232).
// pe: this tile's piece of the lane-major position table.
template <typename T>
LFT_DEV void ang_prologue(const f32x16 (&x)[2], const float* __restrict__ pe, bool ok, const float* lds_ln, int lane, int hh,
                          unsigned& bad, Frag<T> (&nf)[4], Frag<T> (&xf)[4]) {
    typename RawPiece<float>::type pr[8];
    load_lane_major_raw<2, float>(pe, lane, pr);
    f32x16 n[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) n[nt] = x[nt];
    add_acc_raw<2, float>(n, pr, ok);
    layernorm_acc<2, sizeof(T) == 2>(n, lds_ln, lds_ln + 64, hh, bad);
    acc_frags<2, T>(n, nf);
    acc_frags<2, T>(x, xf);
}
// Softmax numerators of one head over CT score tiles, in place; only the last tile has a compile-time live count (registers
// LASTLIVE .. 15 of it are a view for no lane: probability 0 without computing it).  m: start value of the row maximum.  The
// kernels are bound by vector-instruction issue: subtract and sum as register pairs (v_pk_add_f32).  The row sum is left to the
// caller in two parts, the pair sums and -- returned -- the last probability of an odd LASTLIVE (0 for an even one).
template <int CT, int LASTLIVE>
LFT_DEV float ang_softmax(f32x16 (&S)[CT], float m, f32x2& sum2) {
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
        for (int i = 0; i < (j == CT - 1 ? LASTLIVE : 16); ++i) m = fmaxf(m, S[j][i]);
    m = xhalf_max(m);
    const f32x2 mm = {m, m};
    float odd = 0.0f;
    sum2 = f32x2{0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < CT; ++j) {
        const int live = j == CT - 1 ? LASTLIVE : 16;
#pragma unroll
        for (int i = 0; i + 1 < live; i += 2) {
            f32x2 d = f32x2{S[j][i], S[j][i + 1]} - mm;
            d[0] = fast_exp2(d[0]); d[1] = fast_exp2(d[1]);
            S[j][i] = d[0]; S[j][i + 1] = d[1];
            sum2 += d;
        }
        if (live & 1) odd = S[j][live - 1] = fast_exp2(S[j][live - 1] - m);
#pragma unroll
        for (int i = live; i < 16; ++i) S[j][i] = 0.0f;
    }
    return odd;
}
// O^T of head hd in a fresh accumulator: with V's 32 channels (4 heads) as the A operand every row of the product is computed,
// the head's own 8 rows = registers 4*(hd&3)..+3 are kept, normalised by the row sum -- cheaper than zeroing the other heads'
// channels of V per head (8 v_cndmask per head and fragment in kernels bound by vector-instruction issue).
template <int CT, typename T, typename VF>
LFT_DEV void ang_pv_keep(const VF& vfrag, const f32x16 (&S)[CT], float sum, int hd, f32x16& o) {
    const float inv = sizeof(T) == 2 ? fast_rcp(xhalf_sum(sum)) : 1.0f / xhalf_sum(sum);
    f32x16 oh;
#pragma unroll
    for (int i = 0; i < 16; ++i) oh[i] = 0.0f;
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) mma(vfrag(j, s2), acc_to_frag(S[j], s2, T()), oh);
#pragma unroll
    for (int i = 0; i < 4; ++i) o[4 * (hd & 3) + i] = oh[4 * (hd & 3) + i] * inv;
}
// The per-token tail, in place: x = x + O Wo^T; x += W2 relu(W1 LN'(x)).  FAST2: the second LayerNorm in its fast form.
template <typename T, bool FAST2, typename WF>
LFT_DEV void ang_tail(const WF& wfrag, const f32x16 (&o)[2], const float* lds_ln, int hh, unsigned& bad, f32x16 (&x)[2]) {
    Frag<T> of[4], nf[4], hf[8];
    acc_frags<2, T>(o, of);
    linear_frags<2, 4, T>(wfrag, 24, of, x);
    f32x16 n[2], hid[4];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) n[nt] = x[nt];
    layernorm_acc<2, FAST2>(n, lds_ln + 128, lds_ln + 192, hh, bad);
    acc_frags<2, T>(n, nf);
    zero_acc<4>(hid);
    linear_frags<4, 4, T>(wfrag, 32, nf, hid);
    acc_frags_relu<4>(hid, hf);
    linear_frags<2, 8, T>(wfrag, 48, hf, x);
}

// NLIVE: accumulator registers 0 .. NLIVE-1 of a score tile can hold an existing view (register i <-> view rows
// acc_row(i, 0) and acc_row(i, 1)); for V <= 25 (5 x 5) registers 13..15 are rows 25-27 / 29-31, never a view: the
// softmax skips them at compile time (the kernel is bound by vector-instruction issue, not by the matrix pipe).
template <typename T, int NLIVE = 16>
__global__ __launch_bounds__(256, 2) void k_ang(const T* __restrict__ X, T* __restrict__ Y, const T* __restrict__ ws,
                                             const float* __restrict__ ln, const float* __restrict__ pe,
                                             int V, int hw, int npix, unsigned* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int FB = 1024 * FragInfo<T>::PIECES;
    const int lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned bad = 0;                                                  // non-finite activation seen (layernorm_acc)
    {
        const char* g = reinterpret_cast<const char*>(ws);
        LFT_NOTE_ASM_("DMA", kNoteAngW, 0);
#pragma unroll
        for (int i = 0; i < 16 * FragInfo<T>::PIECES; ++i) {
            const int piece = wave * 16 * FragInfo<T>::PIECES + i;
            glds_piece(g + piece * 1024, smem + piece * 1024, lane);
        }
    }
    using L = AngLds<T, true, 0, 4>;
    float* lds_ln = reinterpret_cast<float*>(smem + L::ln);
    const auto wfrag = [&](int f) { return frag_from_pieces(smem + f * FB, lane, T()); };
    LFT_STAMP(0);
    const raw16 lnv = params_load(ln, 256);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // own LDS-DMA pieces landed, then publish (see WRing::next)
    params_store(lds_ln, 256, lnv);
    __syncthreads();
    LFT_NOTE_ASM_("USE", kNoteAngW, 0);
    LFT_STAMP(1);
    [[maybe_unused]] int stamp_it = 0;                                     // diagnostic build: second tile's stamps go to slots 7..11
    const bool ok = r < V;
    f32x16 negmask;                                                                       // 0 for key rows < V, -inf beyond
#pragma unroll
    for (int i = 0; i < 16; ++i) negmask[i] = acc_row(i, hh) >= V ? -INFINITY : 0.0f;
    char* scr = smem + L::scr + wave * TileIO<2, T>::BYTES;                                 // wave-private tile I/O scratch
    const size_t vstride = (size_t)hw * 64 * sizeof(T);                                   // one view to the next, same position
    for (int pix = blockIdx.x * 4 + wave; pix < npix; pix += gridDim.x * 4) {
        asm volatile("" ::: "memory");    // keep the (loop-invariant) LDS weight reads inside the loop: hoisted, they cost 256+ VGPRs
        const int b = pix / hw, p = pix % hw;
        const size_t off0 = (((size_t)b * V) * hw + p) * 64;                              // view 0 of this position

        f32x16 x[2];
        load_tile<2, T>(X + off0, V, lane, x, scr, vstride);                              // rows = views: 8 lanes x 16 B per row
        LFT_STAMP_IT(2, 5 * stamp_it);
        Frag<T> nf[4], xf[4];
        ang_prologue<T>(x, pe, ok, lds_ln, lane, hh, bad, nf, xf);

        f32x16 q[2], k[2], v[2], o[2];
        zero_acc<2>(q); zero_acc<2>(k); zero_acc<2>(v);
        linear_frags<2, 4, T>(wfrag, 0, nf, q);
        linear_frags<2, 4, T>(wfrag, 8, nf, k);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)           // V[view, ch] = sum_k x[view, k] Wv[ch, k]: tokens are the A operand
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) mma(xf[ks], wfrag(16 + nt * 4 + ks), v[nt]);

        LFT_STAMP_IT(3, 5 * stamp_it);
#pragma unroll
        for (int hd = 0; hd < 8; ++hd) {
            const int nt = hd >> 2, s = (hd >> 1) & 1, half = hd & 1;
            f32x16 S[1] = {negmask};                               // rows of non-existent views start at -inf: no per-head masking
            mma(frag_half(acc_to_frag(k[nt], s, T()), half), acc_to_frag(q[nt], s, T()), S[0]);   // S^T[kv, q]
            // Inherited, and not the same in k_ang_multi: the row maximum starts at the first score (there: -inf), and an odd
            // last probability joins the row sum after the two pair sums (there: before).
            f32x2 sum2;
            const float odd = ang_softmax<1, NLIVE>(S, S[0][0], sum2);
            float sum = sum2[0] + sum2[1];
            if constexpr (NLIVE & 1) sum += odd;
            ang_pv_keep<1, T>([&](int, int s2) { return acc_to_frag(v[nt], s2, T()); }, S, sum, hd, o[nt]);
        }

        LFT_STAMP_IT(4, 5 * stamp_it);
        ang_tail<T, sizeof(T) == 2>(wfrag, o, lds_ln, hh, bad, x);
        LFT_STAMP_IT(5, 5 * stamp_it);
        store_tile<2, T>(Y + off0, V, lane, x, scr, vstride);
        LFT_STAMP_IT(6, 5 * stamp_it);
        stamp_it = 1;
    }
    publish_status(status, bad);
}

// ------------------------------------------------------------------------------------------
// Angular block for more than 32 views (e.g. 9x9 = 81 views, BASELINE configs[4]).  A workgroup of CT waves
// owns one spatial position; wave c holds views 32c .. 32c+31 on its MFMA columns and does everything that is
// per-token (LN, projections, out_proj, FFN) exactly as k_ang.  For the attention each wave publishes its K and V
// operand fragments (8 per wave) in LDS; after a barrier every wave runs its 32 queries against all CT key tiles:
// per head CT score tiles (softmax over up to 32*CT keys: registers + one lane^32 exchange) and 2*CT P.V MFMAs.
// WLDS: weights LDS-resident (bf16); the fp32 parity build reads them from L2 (128 KiB would not leave room).
// ------------------------------------------------------------------------------------------
// NG positions share one workgroup (NG * CT waves) and therefore one LDS copy of the weights: more waves per CU for the
// same LDS (9x9, bf16: 2 x 3 waves and 113 KiB instead of 3 waves and 89 KiB).  All groups run the loop in lock-step.
// LASTLIVE: score registers of the LAST key tile that can hold an existing view (as NLIVE in k_ang): 9 x 9 views on three
// tiles leave 17 rows in the last one -- registers 9 .. 15 are never a view and are skipped at compile time.
template <typename T, int CT, bool WLDS, int NG, int LASTLIVE = 16>
__global__ __launch_bounds__(64 * CT * NG) void k_ang_multi(const T* __restrict__ X, T* __restrict__ Y, const T* __restrict__ ws,
                                                            const float* __restrict__ ln, const float* __restrict__ pe,
                                                            int V, int hw, int npix, unsigned* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int FB = 1024 * FragInfo<T>::PIECES;
    const int lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
    unsigned bad = 0;                                                  // non-finite activation seen (layernorm_acc)
    const int wave_all = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = wave_all / CT, wave = wave_all % CT;             // position group, column tile inside the position
    using L = AngLds<T, WLDS, NG * CT * 8, NG * CT>;
    char* lds_w = smem;                                            // 64 weight fragments when WLDS
    float* lds_ln = reinterpret_cast<float*>(smem + L::ln);
    char* lds_kv = smem + L::kv + (size_t)grp * CT * 8 * FB;          // per group [CT][8] fragments: K (nt, s) then V (nt, s)
    char* scr = smem + L::scr + wave_all * TileIO<2, T>::BYTES;       // wave-private tile I/O scratch
    if (WLDS) {
        const char* g = reinterpret_cast<const char*>(ws);
        for (int piece = wave_all; piece < 64 * FragInfo<T>::PIECES; piece += CT * NG) glds_piece(g + piece * 1024, lds_w + piece * 1024, lane);
    }
    if (threadIdx.x < 64) {
        const int i = threadIdx.x * 4;
        store_raw16(reinterpret_cast<char*>(lds_ln + i), load_raw16(reinterpret_cast<const char*>(ln + i)));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    auto wfrag = [&](int f) -> Frag<T> {
        if (WLDS) return frag_from_pieces(lds_w + f * FB, lane, T());
        return load_wfrag(ws, f, lane);
    };
    const int view = wave * 32 + r;
    const bool ok = view < V;
    const int nrows = max(0, min(32, V - wave * 32));                // views of this column tile
    const size_t vstride = (size_t)hw * 64 * sizeof(T);              // one view to the next, same position
    // 0 / -inf start value of the LAST key tile's scores (the host picks CT = ceil(V / 32): every earlier tile is full)
    f32x16 negmask;
#pragma unroll
    for (int i = 0; i < 16; ++i) negmask[i] = (32 * (CT - 1) + acc_row(i, hh) >= V) ? -INFINITY : 0.0f;
    for (int base = blockIdx.x * NG; base < npix; base += gridDim.x * NG) {
        asm volatile("" ::: "memory");
        const bool active = base + grp < npix;                        // a trailing group repeats the last position and stores nothing
        const int pix = min(base + grp, npix - 1);
        const int b = pix / hw, p = pix % hw;
        const size_t off = (((size_t)b * V + min(wave * 32, V - 1)) * hw + p) * 64;   // first view of this column tile
        f32x16 x[2];
        if constexpr (sizeof(T) == 2) load_tile<2, T>(X + off, nrows, lane, x, scr, vstride);   // rows = views, coalesced through the scratch
        else load_acc<2, T>(X + (((size_t)b * V + min(view, V - 1)) * hw + p) * 64, ok, hh, x);   // fp32 build: already register-bound, keep the direct form
        Frag<T> nf[4], xf[4];
        ang_prologue<T>(x, pe + (size_t)wave * 2048, ok, lds_ln, lane, hh, bad, nf, xf);
        f32x16 q[2], o[2];
        zero_acc<2>(q);
        {
            f32x16 k[2], v[2];
            zero_acc<2>(k); zero_acc<2>(v);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    mma(wfrag(nt * 4 + ks), nf[ks], q[nt]);
                    mma(wfrag(8 + nt * 4 + ks), nf[ks], k[nt]);
                    mma(xf[ks], wfrag(16 + nt * 4 + ks), v[nt]);      // V[view, ch]: tokens are the A operand
                }
            __syncthreads();                                            // previous position's fragments fully consumed
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const Frag<T> kf = acc_to_frag(k[nt], s2, T()), vf = acc_to_frag(v[nt], s2, T());
                    char* dk = lds_kv + ((wave * 8 + nt * 2 + s2) * FB);
                    char* dv = lds_kv + ((wave * 8 + 4 + nt * 2 + s2) * FB);
                    if constexpr (sizeof(T) == 4) {
                        store_raw16(dk + lane * 16, __builtin_bit_cast(raw16, kf.lo)); store_raw16(dk + 1024 + lane * 16, __builtin_bit_cast(raw16, kf.hi));
                        store_raw16(dv + lane * 16, __builtin_bit_cast(raw16, vf.lo)); store_raw16(dv + 1024 + lane * 16, __builtin_bit_cast(raw16, vf.hi));
                    } else {
                        store_raw16(dk + lane * 16, __builtin_bit_cast(raw16, kf.v));
                        store_raw16(dv + lane * 16, __builtin_bit_cast(raw16, vf.v));
                    }
                }
            __syncthreads();                                            // all K / V fragments of this position published
        }
#pragma unroll
        for (int hd = 0; hd < 8; ++hd) {
            const int nt = hd >> 2, s = (hd >> 1) & 1, half = hd & 1;
            const Frag<T> qf = acc_to_frag(q[nt], s, T());
            f32x16 S[CT];
#pragma unroll
            for (int j = 0; j < CT; ++j) {
                if (j == CT - 1) S[j] = negmask;
                else {
#pragma unroll
                    for (int i = 0; i < 16; ++i) S[j][i] = 0.0f;
                }
                mma(frag_half(frag_from_pieces(lds_kv + (j * 8 + nt * 2 + s) * FB, lane, T()), half), qf, S[j]);   // S^T[kv, q]
            }
            // Inherited, and not the same in k_ang: the row maximum starts at -inf (there: the first score), and an odd last
            // probability joins the first pair sum before the two are added (there: after).
            f32x2 sum2;
            const float odd = ang_softmax<CT, LASTLIVE>(S, -INFINITY, sum2);
            if constexpr (LASTLIVE & 1) sum2[0] += odd;
            ang_pv_keep<CT, T>([&](int j, int s2) { return frag_from_pieces(lds_kv + (j * 8 + 4 + nt * 2 + s2) * FB, lane, T()); },
                               S, sum2[0] + sum2[1], hd, o[nt]);
        }
        // The second LayerNorm in its exact form in every precision, where k_ang (and the first one here) take the fast form in
        // 16 bit: inherited from the copy this kernel began as, not a decision.
        ang_tail<T, false>(wfrag, o, lds_ln, hh, bad, x);
        if constexpr (sizeof(T) == 2) store_tile<2, T>(Y + off, active ? nrows : 0, lane, x, scr, vstride);
        else store_acc<2, T>(Y + (((size_t)b * V + min(view, V - 1)) * hw + p) * 64, ok && active, hh, x);
    }
    publish_status(status, bad);
}

}  // namespace
