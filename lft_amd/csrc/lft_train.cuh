// lft_train.cuh -- fp32 training kernels (forward with a saved-activation tape + backward) for the LFT network.
//
// The reference trains in fp32 through PyTorch autograd (train.py:74-107: net(data) -> L1Loss -> loss.backward() ->
// Adam).  This file is the MI355X counterpart of what autograd records and replays for model/LFT.py:52-83:
// every linear map of the network as an exact-fp32 MFMA product in the "token on lane" layout of lft_common.cuh,
//   k_lin    Y = act(X W^T) (+R)        any of the network's Linear / 1x1 / 3x3-per-view convolutions, and -- with
//                                       transposed weight strides and flipped taps -- their input gradients
//   k_wgrad  dW = dY^T X                split over token chunks (deterministic two-stage reduction)
// plus the small VALU kernels around them (LayerNorm, both attentions, activations, up-sampler tail).
// The GEMMs come in three arithmetics (LFT_MATH_F32 / _BF16X3 / _BF16X6).  The kernels are written once, over the product policy
// Prod<MM> below: it owns the operand type of a mode, its packed fragment size, the split of fp32 values into the mode's parts,
// the fragment loads, the lane shift and the MFMA sequence of one product.  A kernel never branches on the mode; another product
// scheme or piece layout is a change to (or another specialisation of) Prod.
// Weights change every step: at the start of a step both orientations (W for the forward, W^T for the input gradients)
// are re-packed into fragment order by k_pack (9 MB, microseconds) so that every weight read is a coalesced 1 KiB piece.
// All tensors are fp32 channels-last [token][channel]; token = ((b*V + v)*h + y)*w + x.
#pragma once
#include "lft_common.cuh"
#include "lft_kernels_b.cuh"   // asm-issued loads with counted waits (ld16_async_ofs, wait_vm_q), cubic_coef
#include "lft_win_attn.cuh"

namespace {

// ------------------------------------------------------------------------------------------
// Product policy.  The GEMM kernels below (k_lin, k_linr, k_wgrad, k_pack_split) are templates over the math mode MM and never
// look at it themselves: Prod<MM> is the only place that knows how a mode represents an operand and multiplies two of them.
//   Op                 the operand of one 16-deep k-step (8 values per lane), in the mode's representation
//   FRAG_BYTES         bytes of one packed weight fragment: 1 KiB lane-linear pieces, one per bf16 part (two for fp32)
//   elem / put         one float -> the mode's parts of it; such an element -> position j of an Op
//   split              a whole fp32 fragment -> Op (elem + put eight times; the identity for fp32)
//   store_w            an element -> the packed fragment in memory (k_pack_split; fp32 fragments are written by k_pack)
//   load_w / load_w_lds  the packed fragment from the global stream / from an LDS ring slot
//   shift<DIR>         lane_shift1 on every piece: the operand of the neighbouring token
//   mul(w, x, acc)     acc += w x; the order of the MFMAs is pinned by the gradient fixtures
//   keep               empty asm over every piece: pins the compiler's wait for the operand's loads where it stands (k_linr)
// All members are forced inline; the mode is a template argument everywhere, never a runtime value.
// ------------------------------------------------------------------------------------------
// One token to the left / right inside a wave's 32-token row (lanes 0-31 and 32-63 hold the two k-halves of the same tokens):
// DIR = +1: lane r takes lane r + 1 (v_mov_dpp wave_shl:1), DIR = -1: lane r - 1 (wave_shr:1); the row's first / last token takes 0
// (the lane the shift would pull across the two halves, or from outside the wave).
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
template <int DIR> LFT_DEV u32x4_t lane_shift1_u(u32x4_t u, bool edge) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int s = __builtin_amdgcn_update_dpp(0, (int)u[i], DIR > 0 ? 0x130 : 0x138, 0xf, 0xf, true);
        u[i] = edge ? 0u : (unsigned)s;
    }
    return u;
}
template <int DIR> LFT_DEV bf16x8 lane_shift1(bf16x8 v, bool edge) { return __builtin_bit_cast(bf16x8, lane_shift1_u<DIR>(__builtin_bit_cast(u32x4_t, v), edge)); }
template <int DIR> LFT_DEV f32x4 lane_shift1(f32x4 v, bool edge) { return __builtin_bit_cast(f32x4, lane_shift1_u<DIR>(__builtin_bit_cast(u32x4_t, v), edge)); }
LFT_DEV bf16x8 load_piece(const char* p) { return __builtin_bit_cast(bf16x8, load_raw16(p)); }

template <int MM> struct Prod;          // MM: 0 exact fp32 MFMA, 1 split-bf16 (3 products), 2 bf16x6 (6 products, fp32-class)
// P::split for the split modes: every value of the fragment through the element pair
template <typename P> LFT_DEV typename P::Op split_elems(const Frag<float>& f) {
    typename P::Op r;
#pragma unroll
    for (int j = 0; j < 8; ++j) P::put(r, j, P::elem(j < 4 ? f.lo[j] : f.hi[j - 4]));
    return r;
}

// Exact fp32 (LFT_MATH_F32): v_mfma_f32_32x32x2_f32, 157 TFLOP/s peak.  The operand is the fp32 fragment itself.
template <> struct Prod<0> {
    using Op = Frag<float>;
    using Elem = float;
    static constexpr int FRAG_BYTES = 2048;
    LFT_DEV Elem elem(float x) { return x; }
    LFT_DEV void put(Op& o, int j, Elem e) { if (j < 4) o.lo[j] = e; else o.hi[j - 4] = e; }
    LFT_DEV const Op& split(const Frag<float>& f) { return f; }        // by reference: no copy of the operand is made
    LFT_DEV Op load_w_lds(const char* base) {
        Op r;
        r.lo = __builtin_bit_cast(f32x4, load_raw16(base));
        r.hi = __builtin_bit_cast(f32x4, load_raw16(base + 1024));
        return r;
    }
    LFT_DEV Op load_w(const float* __restrict__ stream, int f, int lane) { return load_wfrag(stream, f, lane); }
    template <int DIR> LFT_DEV Op shift(const Op& x, bool edge) {
        Op r;
        r.lo = lane_shift1<DIR>(x.lo, edge); r.hi = lane_shift1<DIR>(x.hi, edge);
        return r;
    }
    LFT_DEV void mul(const Op& w, const Op& x, f32x16& acc) { mma(w, x, acc); }
    LFT_DEV void keep(const Op& x) { asm volatile("" :: "v"(x.lo), "v"(x.hi)); }
};

// Split-bf16 products ("bf16x3", LFT_MATH_BF16X3).  The fp32 MFMA is 16x slower than the bf16 one, so an fp32 operand x is split
// into two bf16 numbers x = hi + lo (+ O(2^-17 x)) and a product is
//   a * b ~= ah*bh + ah*bl + al*bh            (3 MFMAs, fp32 accumulate; the dropped al*bl is O(2^-18 a b))
// i.e. fp32 operands with ~2^-16 relative error per product at 3/16 of the fp32-MFMA cost.
// Packed weights in this mode: fragment f = [1 KiB hi piece][1 KiB lo piece] (same 2 KiB as an fp32 fragment).
struct Frag2 { Frag<bf16_t> hi, lo; };
template <> struct Prod<1> {
    using Op = Frag2;
    struct Elem { bf16_t hi, lo; };
    static constexpr int FRAG_BYTES = 2048;
    LFT_DEV Elem elem(float x) {
        Elem e;
        e.hi = (bf16_t)x;
        e.lo = (bf16_t)(x - (float)e.hi);
        return e;
    }
    LFT_DEV void put(Op& o, int j, const Elem& e) { o.hi.v[j] = e.hi; o.lo.v[j] = e.lo; }
    LFT_DEV Op split(const Frag<float>& f) { return split_elems<Prod>(f); }
    LFT_DEV void store_w(bf16_t* frag, int i, const Elem& e) { frag[i] = e.hi; frag[512 + i] = e.lo; }   // i = 8 lane + j
    LFT_DEV Op load_w_lds(const char* base) {
        Op r;
        r.hi.v = load_piece(base); r.lo.v = load_piece(base + 1024);
        return r;
    }
    LFT_DEV Op load_w(const float* __restrict__ stream, int f, int lane) {
        return load_w_lds(reinterpret_cast<const char*>(stream) + (size_t)f * FRAG_BYTES + lane * 16);
    }
    template <int DIR> LFT_DEV Op shift(const Op& x, bool edge) {
        Op r;
        r.hi.v = lane_shift1<DIR>(x.hi.v, edge); r.lo.v = lane_shift1<DIR>(x.lo.v, edge);
        return r;
    }
    LFT_DEV void mul(const Op& w, const Op& x, f32x16& acc) {
        mma(w.lo, x.hi, acc);
        mma(w.hi, x.lo, acc);
        mma(w.hi, x.hi, acc);
    }
    LFT_DEV void keep(const Op& x) { asm volatile("" :: "v"(x.hi.v), "v"(x.lo.v)); }
};

// "bf16x6" (LFT_MATH_BF16X6): an fp32 number IS the sum of three bf16 numbers, x = a + b + c exactly (8 + 8 + 8 significant bits;
// each remainder is exact in fp32), so a product is the sum of nine bf16 products of which the three smallest (b c', c b', c c':
// <= 2^-23 |x y| together) are dropped:
//   x * y ~= a a' + (a b' + b a') + (a c' + c a' + b b')        6 MFMAs, fp32 accumulate, smallest terms first
// -- fp32-class products (the fp32 MFMA rounds its product to 2^-24) at 6/16 of the fp32-MFMA cost.
// Packed weights in this mode: fragment f = [1 KiB a][1 KiB b][1 KiB c] (3 KiB; the fp32 and split-bf16 fragments are 2 KiB).
struct Frag3 { Frag<bf16_t> a, b, c; };
template <> struct Prod<2> {
    using Op = Frag3;
    struct Elem { bf16_t a, b, c; };
    static constexpr int FRAG_BYTES = 3072;
    LFT_DEV Elem elem(float x) {
        Elem e;
        e.a = (bf16_t)x;
        const float r1 = x - (float)e.a;
        e.b = (bf16_t)r1;
        e.c = (bf16_t)(r1 - (float)e.b);
        return e;
    }
    LFT_DEV void put(Op& o, int j, const Elem& e) { o.a.v[j] = e.a; o.b.v[j] = e.b; o.c.v[j] = e.c; }
    LFT_DEV Op split(const Frag<float>& f) { return split_elems<Prod>(f); }
    LFT_DEV void store_w(bf16_t* frag, int i, const Elem& e) { frag[i] = e.a; frag[512 + i] = e.b; frag[1024 + i] = e.c; }
    LFT_DEV Op load_w_lds(const char* base) {
        Op r;
        r.a.v = load_piece(base); r.b.v = load_piece(base + 1024); r.c.v = load_piece(base + 2048);
        return r;
    }
    LFT_DEV Op load_w(const float* __restrict__ stream, int f, int lane) {
        return load_w_lds(reinterpret_cast<const char*>(stream) + (size_t)f * FRAG_BYTES + lane * 16);
    }
    template <int DIR> LFT_DEV Op shift(const Op& x, bool edge) {
        Op r;
        r.a.v = lane_shift1<DIR>(x.a.v, edge); r.b.v = lane_shift1<DIR>(x.b.v, edge); r.c.v = lane_shift1<DIR>(x.c.v, edge);
        return r;
    }
    LFT_DEV void mul(const Op& w, const Op& x, f32x16& acc) {
        mma(w.c, x.a, acc);
        mma(w.a, x.c, acc);
        mma(w.b, x.b, acc);
        mma(w.b, x.a, acc);
        mma(w.a, x.b, acc);
        mma(w.a, x.a, acc);
    }
    LFT_DEV void keep(const Op& x) { asm volatile("" :: "v"(x.a.v), "v"(x.b.v), "v"(x.c.v)); }
};

// k_pack's twin for the split modes (MM = 1, 2): same PackOp description (natural k order), every value written as the mode's parts.
template <int MM>
__global__ __launch_bounds__(64) void k_pack_split(PackArgs args, float* __restrict__ dst) {
    using P = Prod<MM>;
    const int f = blockIdx.x, lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    int oi = 0;
    for (int i = 0; i < args.nops; ++i)
        if (f >= args.op[i].frag0) oi = i;
    const PackOp& op = args.op[oi];
    int nt, ks;
    wfrag_coords(op.ntiles, op.ksteps, f - op.frag0, op.order, nt, ks);
    const int n = 32 * nt + r;
    bf16_t* d = reinterpret_cast<bf16_t*>(dst) + (size_t)f * (P::FRAG_BYTES / 2);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int kk = op.k0 + 16 * ks + 8 * h + j;
        float v = 0.0f;
        if (n < op.nrows) {
            if (op.kind == 0) v = op.scale * op.src[(size_t)(op.row0 + n) * op.ld + kk * op.kmul + op.kadd];
            else if (op.kind == 1) v = upm_entry(op.src, n, kk, op.s);
            else v = kk < (op.s + 2) * (op.s + 2) ? upm_entry(op.src, kk, n, op.s) : 0.0f;
        }
        P::store_w(d, lane * 8 + j, P::elem(v));
    }
}

// Test-only (lft_prod_selftest): the policy in isolation, one wave.  Wp = one packed fragment of W [32][16] (k_pack / k_pack_split),
// X [32 tokens][16]; Y [token][o] = X W^T, Yr / Yl the same product with the operand of the token to the right / left (zero at the edge).
template <int MM>
__global__ __launch_bounds__(64) void k_prod_selftest(const float* __restrict__ Wp, const float* __restrict__ X,
                                                      float* __restrict__ Y, float* __restrict__ Yl, float* __restrict__ Yr) {
    using P = Prod<MM>;
    const int lane = threadIdx.x, r = lane & 31, kh = lane >> 5;
    const Frag<float> xf = load_row8(X + r * 16 + 8 * kh, true, 0.0f);
    const auto& x = P::split(xf);
    const typename P::Op w = P::load_w(Wp, 0, lane), xr = P::template shift<1>(x, r == 31), xl = P::template shift<-1>(x, r == 0);
    f32x16 acc[3];
    zero_acc<3>(acc);
    P::mul(w, x, acc[0]);
    P::mul(w, xl, acc[1]);
    P::mul(w, xr, acc[2]);
    float* const out[3] = {Y, Yl, Yr};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < 16; ++i) out[k][r * 32 + acc_row(i, kh)] = acc[k][i];
}

// ------------------------------------------------------------------------------------------
// Generic linear / per-view 3x3 convolution on MFMA.
//   Y[t][o] = act( sum_tap sum_i W(o, i, tap) * X[shift_tap(t)][i] ) (+ R[t][o])
// taps == 1: plain Linear.  taps == 9: tap -> (dy, dx) = (tap/3 - 1, tap%3 - 1), the source token is
// (y + dy, x + dx) of the same view image (zero outside: per-view zero padding, reference LFT.py:24,28,167);
// flip negates the offset, which together with the transposed packing turns the kernel into the convolution's input gradient.
// A wave owns 32 tokens x NT*32 output channels (blockIdx.y selects the channel group).
// ------------------------------------------------------------------------------------------
struct LinP {
    const float* X; int ldx;
    const float* Wp; int OT, KS, ot0; // packed fragments of the whole view (k_pack order 1, natural k order): frag (tap, ot, ks) at tap*OT*KS + wfrag_index(OT, KS, ot, ks); ot0 = first output tile of this call
    const float* R; int ldr;          // optional: accumulator initialised with R (residual, or Y itself to accumulate)
    float* Y; int ldy;
    const float* M; int ldm, mact;    // optional backward-of-activation epilogue: Y = acc * act'(M), M = the saved activation OUTPUT (mact 1 relu, 2 lrelu)
    int taps, flip, act;              // act: 0 none, 1 relu, 2 leaky relu 0.2
    int h, w;
    long long N;
    int gy;                           // k_linr: output groups (workgroups per 128 tokens)
};

// TILED (plain Linears at small batch): the 32 input rows of a wave, consecutive in memory, are fetched in coalesced
// 64-channel chunks through the scratch instead of one 32-byte piece per lane and k-step -- fewer, fuller memory
// requests when there are too few waves to hide latency; at large batch the direct form's higher occupancy wins.
template <int NT, int MM, bool TILED>      // MM: the math mode, see Prod
__global__ __launch_bounds__(256, 3) void k_lin(const LinP p) {
    using P = Prod<MM>;
    constexpr int SCR = TileIO<(NT > 2 ? NT : 2), float>::BYTES;          // output tile or a 64-channel input chunk
    __shared__ __attribute__((aligned(16))) char scr_all[4 * SCR];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, kh = lane >> 5;
    char* scr = scr_all + wave * SCR;
    const long long t0 = ((long long)blockIdx.x * 4 + wave) * 32;
    if (t0 >= p.N) return;
    const int nvalid = (int)min((long long)32, p.N - t0);
    const int otl = blockIdx.y * NT, o0 = otl * 32, ot0 = p.ot0 + otl;     // otl: tile inside this call's output block (Y / R / M columns), ot0: tile of the view
    const long long t = min(t0 + r, p.N - 1);
    const int hw = p.h * p.w;
    const int pix = (int)(t % hw), y = pix / p.w, x = pix - y * p.w;
    f32x16 acc[NT];
    if (p.R) load_tile<NT, float>(p.R + t0 * p.ldr + o0, nvalid, lane, acc, scr, (size_t)p.ldr * 4);
    else zero_acc<NT>(acc);
    if constexpr (TILED) {
        // plain Linear: the wave's 32 input rows are consecutive in memory -> coalesced 64-channel chunks through the scratch
        for (int k0 = 0; k0 < p.KS; k0 += 4) {
            Frag<float> b[4];
            load_tile_frags_s<4, float>(p.X + t0 * p.ldx + 16 * k0, (size_t)p.ldx * 4, nvalid, lane, b, scr);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const auto& x = P::split(b[ks]);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) P::mul(P::load_w(p.Wp, wfrag_index(p.OT, p.KS, ot0 + nt, k0 + ks), lane), x, acc[nt]);
            }
        }
    } else
    for (int tap = 0; tap < p.taps; ++tap) {
        int dy = 0, dx = 0;
        if (p.taps == 9) { dy = tap / 3 - 1; dx = tap % 3 - 1; if (p.flip) { dy = -dy; dx = -dx; } }
        const bool ok = (t0 + r < p.N) && (y + dy >= 0) && (y + dy < p.h) && (x + dx >= 0) && (x + dx < p.w);
        const float* row = p.X + (ok ? (t + dy * p.w + dx) : t) * p.ldx + 8 * kh;
        const int fbase = tap * p.OT * p.KS;
        for (int ks = 0; ks < p.KS; ++ks) {
            const Frag<float> b = load_row8(row + 16 * ks, ok, 0.0f);
            const auto& x = P::split(b);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) P::mul(P::load_w(p.Wp, fbase + wfrag_index(p.OT, p.KS, ot0 + nt, ks), lane), x, acc[nt]);
        }
    }
    // The epilogue (activation, derivative mask, output tile) is the same in k_lin and k_linr and is written out in both: as a
    // shared inlined helper its blocks land in front of the main loop in the function's layout and hipcc allocates differently
    // (VGPR counts moved in 21 of the 33 instantiations, the 3x3 row kernels gained up to 93 register moves).
    if (p.act) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float v = acc[nt][i];
                acc[nt][i] = v > 0.0f ? v : (p.act == 1 ? 0.0f : 0.2f * v);
            }
    }
    if (p.M) {                                                           // dZ = dY * act'(Z), sign(Z) read off the saved act(Z)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {                                // one 32-channel tile at a time: 16 live registers, not 16 NT
            f32x16 mk[1];
            load_tile<1, float>(p.M + t0 * p.ldm + o0 + 32 * nt, nvalid, lane, mk, scr, (size_t)p.ldm * 4);
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[nt][i] = mk[0][i] > 0.0f ? acc[nt][i] : (p.mact == 1 ? 0.0f : 0.2f * acc[nt][i]);
        }
    }
    store_tile<NT, float>(p.Y + t0 * p.ldy + o0, nvalid, lane, acc, scr, (size_t)p.ldy * 4);
}

// ------------------------------------------------------------------------------------------
// k_lin with the weights through LDS.  The four waves of a workgroup (32 tokens each) multiply by the SAME NT x KS (x taps)
// fragments; read per wave from L2 they are 4 KB per token against 1 KB of activations in and 1 KB out (a knock-out build
// without the weight reads ran the family 20 % faster, one without the MFMAs not at all).  Here the group's fragments -- one
// contiguous stream in consumption order (k_pack order 1) -- pass once per workgroup through the 3-slot LDS ring of the inference
// kernels (as WRing: one chunk = one k-step's NT fragments, LDS-DMA two k-steps ahead, one barrier per k-step), and the activation
// rows of the NEXT k-step are in flight while this one is multiplied.
// Ordering (vmcnt retires in issue order).  The rows are ordinary loads: hipcc waits for them itself, so whatever it does with
// the registers is safe (rows loaded from inline asm were COPIED in front of the asm wait that was to guard them).  Rows of
// k-step s are issued in iteration s - 1, i.e. after the DMA of chunk s (behind barrier s - 2) and before that of chunk s + 1:
// the compiler's wait for them -- pinned in front of barrier s -- therefore also covers this wave's pieces of chunk s, and
// the ring needs no wait of its own.
// LDS: ring slots 0, 1 | slot 2 overlaid by the waves' tile scratch -- the scratch is used before barrier 0 (residual tile)
// and after the last k-step (activation-derivative tile, output tile); slot 2 is first written by the DMA behind barrier 0.
// Requires: the call's output block is one packed group (NT == its tile count, first tile a multiple of 4); taps == 9: OT == NT.
// ------------------------------------------------------------------------------------------
// KS3 > 0 (= KS, 4 or 8): a per-view 3x3 convolution on 32-wide views, where a wave's 32 tokens are ONE image row.  The KS row
// fragments of an input row (dy) are loaded ONCE and serve its three taps: the neighbours to the left and right are the same
// registers one lane over (Prod::shift), the image's left / right border is the shift's zero.  Input rows come from L2 three
// times instead of nine and the split into bf16 pairs is done once per row fragment instead of once per tap -- in the SAME step
// order (tap row, tap column, k-step) and with the same operand values as the generic form, so the results are bit-identical.
// acc += (the NT packed fragments of one published chunk of k_linr's LDS ring; base = the chunk's slot + this lane's 16 bytes) x
template <typename P, int NT>
LFT_DEV void mul_chunk(const char* base, const typename P::Op& x, f32x16 (&acc)[NT]) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) P::mul(P::load_w_lds(base + nt * P::FRAG_BYTES), x, acc[nt]);
}
template <int NT, int MM, int KS3 = 0>     // MM as k_lin
__global__ __launch_bounds__(256, 3) void k_linr(const LinP p) {
    using P = Prod<MM>;
    constexpr int FB = P::FRAG_BYTES;                                     // bytes per packed fragment
    constexpr int CHUNK = NT * FB, NPIECE = CHUNK / 1024;                 // bytes / 1 KiB pieces of weights per k-step
    // pieces per wave and chunk: NPIECE / 4, except bf16x6 with two output tiles (6 pieces): waves 0, 1 move two, waves 2, 3 one
    constexpr bool EVEN = NPIECE % 4 == 0;
    constexpr int PPW = EVEN ? NPIECE / 4 : 2;
    constexpr int SCR = TileIO<NT, float>::BYTES;
    static_assert(NT == 2 || NT == 4, "two or four output tiles");
    __shared__ __attribute__((aligned(16))) char lds[2 * CHUNK + (4 * SCR > CHUNK ? 4 * SCR : CHUNK)];
    const int lane = threadIdx.x & 63, r = lane & 31, kh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char* scr = lds + 2 * CHUNK + wave * SCR;
    // 1-D grid: the p.gy workgroups (output groups) that read the same 128 tokens get ids 8 apart = the same XCD at about the
    // same time: the second reader of the rows hits in that XCD's L2 (as grid (tokens, group) they were a launch apart)
    const int grp8 = (int)blockIdx.x / (8 * p.gy), rem = (int)blockIdx.x % (8 * p.gy);
    const long long tile = (long long)grp8 * 8 + (rem & 7);
    const int by = rem >> 3;
    const long long t0w = (tile * 4 + wave) * 32;
    if (tile * 128 >= p.N) return;                                       // (whole workgroup: the last group of 8 may be short)
    const bool active = t0w < p.N;                                       // a wave past the end still runs the ring protocol (barriers, DMA share)
    const long long t0 = active ? t0w : 0;
    const int nvalid = active ? (int)min((long long)32, p.N - t0) : 0;
    const int otl = by * NT, o0 = otl * 32, ot0 = p.ot0 + otl;
    const long long t = min(t0 + r, p.N - 1);
    const int hw = p.h * p.w;
    const int pix = (int)(t % hw), y = pix / p.w, x = pix - y * p.w;
    const int S = p.taps * p.KS;                                         // k-steps = ring chunks
    // the ring: chunk c (the NT fragments of k-step c) in slot c % 3; every wave moves PPW pieces of it.  The DMA is issued from
    // inline asm: hipcc does not know it, so its waits for the row loads are computed without it (stricter, never unsafe) and
    // it does not guard the ring's LDS reads with a vmcnt(0) of its own (it did, with the builtin form)
    const int my_first = EVEN ? wave * PPW : (wave < 2 ? 2 * wave : 2 + wave), my_count = EVEN ? PPW : (wave < 2 ? 2 : 1);   // wave-uniform
    const char* wsrc = reinterpret_cast<const char*>(p.Wp) + (size_t)wfrag_index(p.OT, p.KS, ot0, 0) * FB + my_first * 1024 + lane * 16;
    auto issue_w = [&](int c, int slot) {
        if (c >= S) return;
#pragma unroll
        for (int i = 0; i < PPW; ++i)
            if (EVEN || i < my_count) glds16_asm(wsrc + (size_t)c * CHUNK + i * 1024, lds + slot * CHUNK + (my_first + i) * 1024);
    };
    issue_w(0, 0);
    issue_w(1, 1);
    f32x16 acc[NT];
    if (p.R) load_tile<NT, float>(p.R + t0 * p.ldr + o0, nvalid, lane, acc, scr, (size_t)p.ldr * 4);
    else zero_acc<NT>(acc);
    if constexpr (KS3 > 0) {
        const bool lane_ok = t0w + r < p.N, e_lo = r == 0, e_hi = r == 31;
        int cs = 0, slot = 0;
        for (int dyi = 0; dyi < 3; ++dyi) {
            const int dy = p.flip ? 1 - dyi : dyi - 1;
            const bool okr = lane_ok && (y + dy >= 0) && (y + dy < p.h);
            const float* row = p.X + (okr ? t + dy * p.w : t) * p.ldx + 8 * kh;
            Frag<float> xr[KS3];
#pragma unroll
            for (int ks = 0; ks < KS3; ++ks) xr[ks] = load_row8(row + 16 * ks, true, 0.0f);
            typename P::Op xs[KS3];
#pragma unroll
            for (int ks = 0; ks < KS3; ++ks) xs[ks] = P::split(okr ? xr[ks] : frag_zero(0.0f));
            for (int dxi = 0; dxi < 3; ++dxi) {
                const int dx = p.flip ? 1 - dxi : dxi - 1;               // uniform
#pragma unroll
                for (int ks = 0; ks < KS3; ++ks) {
                    // this wave's pieces of chunk cs have landed (only those of chunk cs + 1 may still be in flight: the counted wait
                    // of WRing), then the barrier publishes the chunk and retires chunk cs - 1
                    wait_vmcnt(cs + 1 < S ? my_count : 0);
                    wg_barrier_keep_vm();
                    issue_w(cs + 2, slot == 0 ? 2 : slot - 1);
                    const typename P::Op b = dx > 0 ? P::template shift<1>(xs[ks], e_hi) : dx < 0 ? P::template shift<-1>(xs[ks], e_lo) : xs[ks];
                    mul_chunk<P>(lds + slot * CHUNK + lane * 16, b, acc);
                    ++cs;
                    slot = slot == 2 ? 0 : slot + 1;
                }
            }
        }
    } else {
    // cursor of the next row load: (tap, k-step); past the last k-step it stays there (one redundant, cached reload)
    int ctap = 0, cks = 0;
    auto load_x = [&](bool& ok) -> Frag<float> {                         // raw rows; zeroed by `ok` where they are consumed (a select here would pull the wait up to here)
        int dy = 0, dx = 0;
        if (p.taps == 9) { dy = ctap / 3 - 1; dx = ctap % 3 - 1; if (p.flip) { dy = -dy; dx = -dx; } }
        ok = (t0w + r < p.N) && (y + dy >= 0) && (y + dy < p.h) && (x + dx >= 0) && (x + dx < p.w);
        const float* row = p.X + (ok ? (t + dy * p.w + dx) : t) * p.ldx + 8 * kh + 16 * cks;
        if (cks + 1 < p.KS) ++cks; else if (ctap + 1 < p.taps) { cks = 0; ++ctap; }
        return load_row8(row, true, 0.0f);
    };
    int cs = 0, slot = 0;                                                // current k-step and its ring slot
    auto step = [&](const Frag<float>& xraw, bool ok) {
        const Frag<float> xz = ok ? xraw : frag_zero(0.0f);
        const auto& xs = P::split(xz);
        P::keep(xs);                                                     // (the compiler's wait for the rows sits here, in front of the barrier)
        wg_barrier_keep_vm();                                            // chunk cs published by every wave, chunk cs - 1 retired
        issue_w(cs + 2, slot == 0 ? 2 : slot - 1);                       // into the slot chunk cs - 1 vacated
        mul_chunk<P>(lds + slot * CHUNK + lane * 16, xs, acc);
        ++cs;
        slot = slot == 2 ? 0 : slot + 1;
    };
    bool oka, okb;
    Frag<float> xa = load_x(oka), xb;
    for (int s = 0; s < S; s += 2) {                                    // S is even (KS is); two register sets, no copy between them
        xb = load_x(okb);                                                // rows of k-step s + 1: in flight under this step's MFMAs
        step(xa, oka);
        xa = load_x(oka);
        step(xb, okb);
    }
    }
    wg_barrier_keep_vm();                                                // every wave is done with the ring: slot 2 is scratch again
    if (p.act) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float v = acc[nt][i];
                acc[nt][i] = v > 0.0f ? v : (p.act == 1 ? 0.0f : 0.2f * v);
            }
    }
    if (p.M) {                                                           // dZ = dY * act'(Z), sign(Z) read off the saved act(Z)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {                                // one 32-channel tile at a time: 16 live registers, not 16 NT
            f32x16 mk[1];
            load_tile<1, float>(p.M + t0 * p.ldm + o0 + 32 * nt, nvalid, lane, mk, scr, (size_t)p.ldm * 4);
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[nt][i] = mk[0][i] > 0.0f ? acc[nt][i] : (p.mact == 1 ? 0.0f : 0.2f * acc[nt][i]);
        }
    }
    store_tile<NT, float>(p.Y + t0 * p.ldy + o0, nvalid, lane, acc, scr, (size_t)p.ldy * 4);
}

// ------------------------------------------------------------------------------------------
// Weight gradient: part[chunk][o*so + i*si + tap*st] = sum_{t in chunk} dY[t][o] * X[shift_tap(t)][i]
// MFMA with k = token: A[m = o][k] = dY[t0 + k][o], B[k][n = i] = X[shift(t0 + k)][i]; both operands are read
// straight from the channels-last tensors (lanes = consecutive channels of one token: 128-byte segments).
// A wave owns one 32-row block of dY channels, one tap, NI 32-column blocks of X channels and one token chunk.
// grid: 1-D over (chunk, (o tile, i group), tap row), see the kernel.   k_reduce_all then sums the chunks in a fixed order.
// ------------------------------------------------------------------------------------------
struct WgP {
    const float* dY; int ldy;
    const float* X; int ldx;
    float* part; long long wsize;     // floats per chunk image of the weight
    int so, si, st;
    int Co, Ci, taps;
    int h, w;
    long long N, chunk_len;           // chunk_len % 64 == 0: four waves x 16-token k-steps
    int igroups;
    int nch, gy;                      // token chunks; workgroups per chunk and tap row (output tiles x input groups)
};

// TX = 3: the wave owns a whole ROW of taps (dy fixed by blockIdx.z, dx = -1, 0, +1): the dY fragment is loaded (and
// split) once for three products and the three shifted X rows are neighbours in memory.
// The 4 waves of a workgroup split the chunk's tokens and add their accumulators through LDS, in a fixed order:
// one partial image per workgroup (a quarter of the partial-sum traffic for the same number of waves in flight).
template <int NI, int MM, int TX>      // MM: the math mode, see Prod
__global__ __launch_bounds__(256, TX == 3 ? 2 : 3) void k_wgrad(const WgP p) {
    using P = Prod<MM>;
    extern __shared__ __attribute__((aligned(16))) float wred[];        // [3 waves][TX * NI tiles][16][64]
    const int lane = threadIdx.x & 63, r = lane & 31, kh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // 1-D grid: the gy (x 3 tap rows) workgroups that read the SAME token chunk get workgroup ids 8 apart -- ids are dealt round
    // robin to the 8 XCDs, so they run on one XCD at about the same time and the chunk's second .. last reader hits in its L2
    // (as grid (chunk, tile, tap row) they were a whole launch apart: every tile and tap row re-read its operands from HBM)
    const int per = p.gy * (TX == 3 ? 3 : 1);
    const int grp = (int)blockIdx.x / (8 * per), rem = (int)blockIdx.x % (8 * per);
    const int chunk = grp * 8 + (rem & 7), sub_id = rem >> 3;
    if (chunk >= p.nch) return;                                         // (whole workgroup: the last group of 8 may be short)
    const int by = sub_id % p.gy, bz = sub_id / p.gy;
    const int ot = by / p.igroups, ig = by % p.igroups;
    const int o0 = ot * 32, i0 = ig * NI * 32;
    const long long sub = p.chunk_len >> 2;                              // chunk_len % 64 == 0
    const long long ta = (long long)chunk * p.chunk_len + wave * sub, tb = min(ta + sub, p.N);
    const int hw = p.h * p.w;
    const int dy = TX == 3 ? bz - 1 : 0;
    f32x16 acc[TX][NI];
#pragma unroll
    for (int tx = 0; tx < TX; ++tx) zero_acc<NI>(acc[tx]);
    // Addressing: wave-uniform anchors (scalar registers) + one 32-bit byte offset per lane, advanced by 16 tokens per step; the
    // lane's image position (ys, xs) is advanced the same way -- the 64-bit token arithmetic (a division per fragment element:
    // ~1 000 of the loop's 1 600 instructions around 12 MFMAs) happens once per wave.  Lanes outside the chunk or the image read
    // the anchor's own row and are zeroed.
    const int nsub = (int)max(0LL, tb - ta);
    const int pre = TX == 3 ? p.w + 1 : 0;                              // the X anchor lies `pre` tokens before the wave's first token
    const char* ya = reinterpret_cast<const char*>(p.dY) + (ta * p.ldy + o0) * 4;
    const char* xa = reinterpret_cast<const char*>(p.X) + ((ta - pre) * p.ldx + i0) * 4;
    const unsigned safe_x = ((unsigned)pre * p.ldx + r) * 4u, safe_y = r * 4u;
    unsigned vy = ((unsigned)(8 * kh) * p.ldy + r) * 4u, vx = ((unsigned)(8 * kh + pre) * p.ldx + r) * 4u;
    int rl = 8 * kh, ys = 0, xs = 0;
    if constexpr (TX == 3) { const int pix = (int)((ta + 8 * kh) % hw); ys = pix / p.w; xs = pix - ys * p.w; }
    // 3x3 on 32-wide views: a 16-token step lies in one half of ONE image row, every step is full (N, the chunk and the wave's
    // share are multiples of 16).  A lane's three tap fragments X[t + j - 1], X[t + j], X[t + j + 1] (j = 0..7) are ten values:
    // eight centre ones, a left and a right neighbour -- 10 loads instead of 24, each value is split ONCE into the mode's element
    // (Prod::elem) and the three fragments are gathered from the ten elements (in the bf16 modes: two packings of the same bf16
    // pairs, even pairs (c0,c1).. for the centre tap, odd pairs (L,c0),(c1,c2)..,(c7,R) for the other two).  Same values, same MFMA order as the general form below: bit-identical.
    bool fast3 = false;
    if constexpr (TX == 3) fast3 = p.w == 32 && nsub % 16 == 0 && ta % 16 == 0;
    if (fast3) {
        if constexpr (TX == 3) {
            const int pix0 = (int)(ta % hw);
            int yw = pix0 / 32, xb = pix0 % 32;                             // wave-uniform: image row and half (0 / 16) of the step
            for (int step = 0; step * 16 < nsub; ++step) {
                const bool okrow = (yw + dy >= 0) && (yw + dy < p.h);       // uniform
                const bool okl = okrow && (xb + 8 * kh > 0), okr = okrow && (xb + 8 * kh + 8 < 32);
                Frag<float> a;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float av = *reinterpret_cast<const float*>(ya + vy + (unsigned)(j * p.ldy) * 4u);
                    if (j < 4) a.lo[j] = av; else a.hi[j - 4] = av;
                }
                float v[NI][10];                                            // [0] = left neighbour, [1..8] = centre, [9] = right neighbour
#pragma unroll
                for (int e = 0; e < 10; ++e) {
                    const bool ok = e == 0 ? okl : e == 9 ? okr : okrow;
                    const float* xr = reinterpret_cast<const float*>(xa + (ok ? vx + (unsigned)((e - 1 + dy * 32) * p.ldx) * 4u : safe_x));
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni) { const float t = xr[32 * ni]; v[ni][e] = ok ? t : 0.0f; }
                }
                vy += 16u * p.ldy * 4u; vx += 16u * p.ldx * 4u;
                xb += 16;
                if (xb == 32) { xb = 0; if (++yw == p.h) yw = 0; }
                const auto& a_op = P::split(a);
                typename P::Elem el[NI][10];
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                    for (int e = 0; e < 10; ++e) el[ni][e] = P::elem(v[ni][e]);
#pragma unroll
                for (int tx = 0; tx < 3; ++tx)
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni) {
                        typename P::Op b;
#pragma unroll
                        for (int j = 0; j < 8; ++j) P::put(b, j, el[ni][j + tx]);
                        P::mul(a_op, b, acc[tx][ni]);
                    }
            }
        }
    } else
    for (int step = 0; step * 16 < nsub; ++step) {
        Frag<float> a, b[TX][NI];
        int y = ys, x = xs;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool in = rl + j < nsub;
            const bool okrow = in && (y + dy >= 0) && (y + dy < p.h);
            const float av = *reinterpret_cast<const float*>(ya + (in ? vy + (unsigned)(j * p.ldy) * 4u : safe_y));
            if (j < 4) a.lo[j] = in ? av : 0.0f; else a.hi[j - 4] = in ? av : 0.0f;
#pragma unroll
            for (int tx = 0; tx < TX; ++tx) {
                const int dx = TX == 3 ? tx - 1 : 0;
                const bool ok = TX == 3 ? okrow && (x + dx >= 0) && (x + dx < p.w) : in;
                const float* xr = reinterpret_cast<const float*>(xa + (ok ? vx + (unsigned)((j + dy * p.w + dx) * p.ldx) * 4u : safe_x));
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) {
                    const float bv = xr[32 * ni];
                    const float bz = TX == 3 ? (ok ? bv : 0.0f) : bv;   // plain: a row outside the chunk meets a zeroed dY element (the anchor row read instead is finite data)
                    if (j < 4) b[tx][ni].lo[j] = bz; else b[tx][ni].hi[j - 4] = bz;
                }
            }
            if constexpr (TX == 3) { if (++x == p.w) { x = 0; if (++y == p.h) y = 0; } }
        }
        rl += 16; vy += 16u * p.ldy * 4u; vx += 16u * p.ldx * 4u;
        if constexpr (TX == 3) {
            xs += 16;
            while (xs >= p.w) { xs -= p.w; if (++ys == p.h) ys = 0; }
        }
        const auto& a_op = P::split(a);
#pragma unroll
        for (int tx = 0; tx < TX; ++tx)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) P::mul(a_op, P::split(b[tx][ni]), acc[tx][ni]);
    }
    if (wave) {
#pragma unroll
        for (int tx = 0; tx < TX; ++tx)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int i = 0; i < 16; ++i) wred[(((wave - 1) * TX * NI + tx * NI + ni) * 16 + i) * 64 + lane] = acc[tx][ni][i];
    }
    __syncthreads();
    if (wave) return;
#pragma unroll
    for (int w2 = 0; w2 < 3; ++w2)
#pragma unroll
        for (int tx = 0; tx < TX; ++tx)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[tx][ni][i] += wred[((w2 * TX * NI + tx * NI + ni) * 16 + i) * 64 + lane];
#pragma unroll
    for (int tx = 0; tx < TX; ++tx) {
        const int tap = TX == 3 ? bz * 3 + tx : 0;
        float* dst = p.part + (long long)chunk * p.wsize + (size_t)tap * p.st;
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int i = 0; i < 16; ++i)
                dst[(size_t)(o0 + acc_row(i, kh)) * p.so + (size_t)(i0 + 32 * ni + r) * p.si] = acc[tx][ni][i];
    }
}

// All partial-sum reductions of one backward pass in ONE launch: every producer (weight-gradient workgroups, LayerNorm
// backward workgroups, the two tail kernels) leaves its partials in its own region of the partial buffer, and a table of
// segments tells this kernel what to sum where.  dst[i] = sum_c part[off + c*stride + i] (+ a second chained partial
// set: the position-token contribution to the embedding weight).  Fixed summation order: deterministic.
struct RedSeg { long long part_off, part2_off, dst_off; int nch, nch2, n, stride, blk0; };
constexpr int kRedMax = 80;
struct RedTab { int nseg, nblk; RedSeg s[kRedMax]; };
__global__ __launch_bounds__(256) void k_reduce_all(const RedTab tab, const float* __restrict__ part, float* __restrict__ grads) {
    __shared__ float red[4][64];
    int lo = 0, hi = tab.nseg - 1;                                      // last segment whose first block <= blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab.s[mid].blk0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const RedSeg& sg = tab.s[lo];
    const int xl = threadIdx.x & 63, yl = threadIdx.x >> 6;
    const int i = ((int)blockIdx.x - sg.blk0) * 64 + xl;
    float s0 = 0.0f, s1 = 0.0f;
    if (i < sg.n) {
        const float* p1 = part + sg.part_off + i;
        int c = yl;
        for (; c + 28 < sg.nch; c += 32) {                              // eight loads in flight; each accumulator sees its chunks in the same order as before
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = p1[(long long)(c + 4 * k) * sg.stride];
#pragma unroll
            for (int k = 0; k < 8; k += 2) { s0 += v[k]; s1 += v[k + 1]; }
        }
        for (; c + 4 < sg.nch; c += 8) { s0 += p1[(long long)c * sg.stride]; s1 += p1[(long long)(c + 4) * sg.stride]; }
        if (c < sg.nch) s0 += p1[(long long)c * sg.stride];
        const float* p2 = part + sg.part2_off + i;
        for (c = yl; c < sg.nch2; c += 4) s1 += p2[(long long)c * sg.stride];
    }
    red[yl][xl] = s0 + s1;
    __syncthreads();
    if (yl == 0 && i < sg.n) grads[sg.dst_off + i] = (red[0][xl] + red[1][xl]) + (red[2][xl] + red[3][xl]);
}

// ------------------------------------------------------------------------------------------
// Plain position tables (reference LFT.py:86-115): angular [V][64], spatial [h*w][64].
// ------------------------------------------------------------------------------------------
__global__ void k_pe_plain(float* __restrict__ ang, float* __restrict__ spa, int V, int h, int w) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < V * 64) ang[idx] = pe_value(idx >> 6, idx & 63);
    if (idx < h * w * 64) {
        const int pp = idx >> 6, c = idx & 63;
        spa[idx] = (pe_value(pp / w, c) + pe_value(pp % w, c)) / 2.0f;
    }
}

// ------------------------------------------------------------------------------------------
// LayerNorm over C channels (C = 64 or 128), input u = X (+ pe): pe_mode 0 none, 1 angular pe[v][c] with
// v = (t / hw) % V, 2 spatial-token pe[t % hw][c].  16 lanes per token, C/16 channels per lane.
// Backward: du = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dY * gamma; out = (add ? add : 0) + du;
// per-block partial sums of dgamma = sum dY * xhat and dbeta = sum dY go to pgb[block][2C].
// ------------------------------------------------------------------------------------------
template <int C>
LFT_DEV void ln_load(const float* __restrict__ X, const float* __restrict__ pe, int pe_mode, long long t, int hw, int V, int sub,
                     float (&u)[C / 16]) {
    constexpr int PER = C / 16;
    const float* row = X + t * C + sub * PER;
#pragma unroll
    for (int g = 0; g < PER / 4; ++g) {
        const f32x4 v = load4(row + 4 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j) u[4 * g + j] = v[j];
    }
    if (pe_mode) {
        const long long prow = pe_mode == 1 ? (t / hw) % V : t % hw;
        const float* pr = pe + prow * C + sub * PER;
#pragma unroll
        for (int g = 0; g < PER / 4; ++g) {
            const f32x4 v = load4(pr + 4 * g);
#pragma unroll
            for (int j = 0; j < 4; ++j) u[4 * g + j] += v[j];
        }
    }
}
LFT_DEV float sum16(float v) {
    v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 1, 64);
    return v;
}
template <int C>
LFT_DEV void ln_stats(const float (&u)[C / 16], float& mean, float& rstd) {
    constexpr int PER = C / 16;
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < PER; ++i) s += u[i];
    mean = sum16(s) * (1.0f / C);
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < PER; ++i) { const float d = u[i] - mean; q += d * d; }
    rstd = 1.0f / sqrtf(sum16(q) * (1.0f / C) + LFT_LN_EPS);
}
template <int C>
__global__ __launch_bounds__(256) void k_ln_fwd(const float* __restrict__ X, const float* __restrict__ pe, int pe_mode,
                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                float* __restrict__ Y, long long N, int hw, int V) {
    constexpr int PER = C / 16;
    const int sub = threadIdx.x & 15;
    const long long t = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const long long tc = min(t, N - 1);
    float u[PER], mean, rstd;
    ln_load<C>(X, pe, pe_mode, tc, hw, V, sub, u);
    ln_stats<C>(u, mean, rstd);
    if (t >= N) return;
#pragma unroll
    for (int g = 0; g < PER / 4; ++g) {
        const f32x4 gm = load4(gamma + sub * PER + 4 * g), bt = load4(beta + sub * PER + 4 * g);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (u[4 * g + j] - mean) * rstd * gm[j] + bt[j];
        store4(Y + t * C + sub * PER + 4 * g, o);
    }
}
template <int C>
__global__ __launch_bounds__(256) void k_ln_bwd(const float* __restrict__ X, const float* __restrict__ pe, int pe_mode,
                                                const float* __restrict__ gamma, const float* dY,
                                                const float* add, float* out,      // out may alias add or dY (same element, same thread)
                                                float* __restrict__ pgb, long long N, int hw, int V) {
    constexpr int PER = C / 16;
    __shared__ float red[16][2 * C];
    const int sub = threadIdx.x & 15, slot = threadIdx.x >> 4;
    float gm[PER], dg[PER], db[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) { gm[i] = gamma[sub * PER + i]; dg[i] = 0.0f; db[i] = 0.0f; }
    // the 16 lanes of a token share t, so the sum16 exchanges always see a full group
    for (long long t = (long long)blockIdx.x * 16 + slot; t < N; t += (long long)gridDim.x * 16) {
        float u[PER], mean, rstd, g[PER], xh[PER], dyv[PER];
        ln_load<C>(X, pe, pe_mode, t, hw, V, sub, u);
        ln_stats<C>(u, mean, rstd);
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int gq = 0; gq < PER / 4; ++gq) {
            const f32x4 d = load4(dY + t * C + sub * PER + 4 * gq);
#pragma unroll
            for (int j = 0; j < 4; ++j) dyv[4 * gq + j] = d[j];
        }
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            xh[i] = (u[i] - mean) * rstd;
            g[i] = dyv[i] * gm[i];
            s1 += g[i]; s2 += g[i] * xh[i];
            dg[i] += dyv[i] * xh[i]; db[i] += dyv[i];
        }
        s1 = sum16(s1) * (1.0f / C); s2 = sum16(s2) * (1.0f / C);
#pragma unroll
        for (int gq = 0; gq < PER / 4; ++gq) {
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = rstd * (g[4 * gq + j] - s1 - xh[4 * gq + j] * s2);
            if (add) {
                const f32x4 a = load4(add + t * C + sub * PER + 4 * gq);
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] += a[j];
            }
            store4(out + t * C + sub * PER + 4 * gq, o);
        }
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) { red[slot][sub * PER + i] = dg[i]; red[slot][C + sub * PER + i] = db[i]; }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += 256) {
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < 16; ++q) s += red[q][i];
        pgb[(size_t)blockIdx.x * 2 * C + i] = s;
    }
}

// ------------------------------------------------------------------------------------------
// Elementwise helpers.
// ------------------------------------------------------------------------------------------
// out = g * act'(y): relu (mode 1): y > 0; leaky relu 0.2 (mode 2): y > 0 ? 1 : 0.2  (y = act(z) has the sign of z)
__global__ void k_act_bwd(const float* g, const float* __restrict__ y, float* out, long long n4, int mode) {   // out may alias g
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const f32x4 gv = load4(g + 4 * i), yv = load4(y + 4 * i);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = yv[j] > 0.0f ? gv[j] : (mode == 1 ? 0.0f : 0.2f * gv[j]);
    store4(out + 4 * i, o);
}
__global__ void k_add3(float* __restrict__ out, const float* __restrict__ a, const float* __restrict__ b, long long n4) {   // out = a + b
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const f32x4 av = load4(a + 4 * i), bv = load4(b + 4 * i);
    store4(out + 4 * i, f32x4{av[0] + bv[0], av[1] + bv[1], av[2] + bv[2], av[3] + bv[3]});
}
__global__ void k_add(float* __restrict__ a, const float* __restrict__ b, long long n4) {       // a += b
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const f32x4 av = load4(a + 4 * i), bv = load4(b + 4 * i);
    store4(a + 4 * i, f32x4{av[0] + bv[0], av[1] + bv[1], av[2] + bv[2], av[3] + bv[3]});
}
// out[i] = sum_img src[img][i], i < n (n = hw * C): gradient of the broadcast position tokens
__global__ void k_sum_images(const float* __restrict__ src, int nimg, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.0f;
    int im = 0;
    for (; im + 8 <= nimg; im += 8) {                                   // eight loads in flight, added in image order (the sum's order is unchanged)
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = src[(long long)(im + k) * n + i];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; im < nimg; ++im) s += src[(long long)im * n + i];
    out[i] = s;
}

// ------------------------------------------------------------------------------------------
// Angular attention (reference LFT.py:230-233): per pixel, sequence = the V views, 8 heads x 8 channels, no mask.
// QK [N][128] (Q | K), Vv / O [N][64].  One workgroup per pixel (b, p); thread = (head, view), VP = padded views.
// Backward is the usual two-pass form: per query (m, 1/l, D = sum_j P dP) and dQ; then per key dK, dV.
// ------------------------------------------------------------------------------------------
LFT_DEV void load8(const float* p, float (&o)[8]) {
    const f32x4 a = load4(p), b = load4(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { o[j] = a[j]; o[4 + j] = b[j]; }
}
LFT_DEV void store8(float* p, const float (&o)[8]) {
    store4(p, f32x4{o[0], o[1], o[2], o[3]});
    store4(p + 4, f32x4{o[4], o[5], o[6], o[7]});
}
LFT_DEV float dot8(const float (&a)[8], const float* b) {
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) s += a[c] * b[c];
    return s;
}
template <int VP> constexpr int kAngHS = VP * 8 + 8;     // floats per head of k_ang_attn's LDS tiles
template <int VP, bool BWD>
__global__ __launch_bounds__(8 * VP) void k_ang_attn(const float* __restrict__ QK, const float* __restrict__ Vv,
                                                     float* __restrict__ O, const float* __restrict__ dO,
                                                     float* __restrict__ dQK, float* __restrict__ dV, int V, int hw) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    // thread = (view i, head hd) with the HEAD fastest: the 8 lanes of a view read its row's 8 head pieces = 256 contiguous
    // bytes (view-fastest, every lane of a wave sat on a different row, 512 KB apart: 64 cache lines per load instruction).
    // LDS tiles [8 heads][HS]: HS = VP * 8 + 8 floats, so that the 8 heads a wave reads together fall on disjoint banks.
    constexpr int HS = kAngHS<VP>;
    float* Ks = sm;                         // [8][VP][8] (+ 8 floats per head)
    float* Vs = Ks + 8 * HS;
    float* Qs = Vs + 8 * HS;                // BWD only
    float* Ds = Qs + 8 * HS;                // BWD only: dO
    float* St = Ds + 8 * HS;                // BWD only: [8][SS] with rows of VP x 3 (m, 1/l, D) + 1 float: the 8 heads a wave reads together sit on 8 banks (at 3 VP floats all on one)
    constexpr int SS = VP * 3 + 1;
    const int hd = threadIdx.x & 7, i = threadIdx.x >> 3;
    const int b = blockIdx.x / hw, pix = blockIdx.x % hw;
    const bool act = i < V;
    const long long row = ((long long)b * V + min(i, V - 1)) * hw + pix;
    const float scale = 0.35355339059327373f;            // 1 / sqrt(8)
    float q[8], tmp[8], dov[8];
    load8(QK + row * 128 + hd * 8, q);
    load8(QK + row * 128 + 64 + hd * 8, tmp);
    store8(Ks + hd * HS + i * 8, tmp);
    load8(Vv + row * 64 + hd * 8, tmp);
    store8(Vs + hd * HS + i * 8, tmp);
    if (BWD) {
        store8(Qs + hd * HS + i * 8, q);
        load8(dO + row * 64 + hd * 8, dov);
        store8(Ds + hd * HS + i * 8, dov);
    }
    __syncthreads();
    // scores once, kept in registers (a second pass that recomputed the dot products was a quarter of the kernel's vector work);
    // the loop over the VP possible keys is unrolled so that the array is indexed by constants, keys >= V are skipped uniformly
    float sc[VP <= 32 ? VP : 1];
    float m = -INFINITY;
    if constexpr (VP <= 32) {
#pragma unroll
        for (int j = 0; j < VP; ++j)
            if (j < V) { sc[j] = dot8(q, Ks + hd * HS + j * 8); m = fmaxf(m, scale * sc[j]); }   // the raw dot product: the expressions below are the two-pass form's, bit for bit
    } else {
        for (int j = 0; j < V; ++j) m = fmaxf(m, scale * dot8(q, Ks + hd * HS + j * 8));
    }
    float l = 0.0f;
    if (!BWD) {
        float o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if constexpr (VP <= 32) {
#pragma unroll
            for (int j = 0; j < VP; ++j)
                if (j < V) {
                    const float pj = expf(scale * sc[j] - m);
                    l += pj;
#pragma unroll
                    for (int c = 0; c < 8; ++c) o[c] += pj * Vs[hd * HS + j * 8 + c];
                }
        } else {
            for (int j = 0; j < V; ++j) {
                const float pj = expf(scale * dot8(q, Ks + hd * HS + j * 8) - m);
                l += pj;
#pragma unroll
                for (int c = 0; c < 8; ++c) o[c] += pj * Vs[hd * HS + j * 8 + c];
            }
        }
        const float inv = 1.0f / l;
#pragma unroll
        for (int c = 0; c < 8; ++c) o[c] *= inv;
        if (act) store8(O + row * 64 + hd * 8, o);
        return;
    }
    // ---- backward, pass A (per query) ----
    float D = 0.0f, av[8] = {0, 0, 0, 0, 0, 0, 0, 0}, bv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto passA = [&](int j, float pj) {
        const float* kj = Ks + hd * HS + j * 8;
        const float dp = dot8(dov, Vs + hd * HS + j * 8);
        l += pj; D += pj * dp;
#pragma unroll
        for (int c = 0; c < 8; ++c) { av[c] += pj * dp * kj[c]; bv[c] += pj * kj[c]; }
    };
    if constexpr (VP <= 32) {
#pragma unroll
        for (int j = 0; j < VP; ++j)
            if (j < V) passA(j, expf(scale * sc[j] - m));
    } else {
        for (int j = 0; j < V; ++j) passA(j, expf(scale * dot8(q, Ks + hd * HS + j * 8) - m));
    }
    const float inv = 1.0f / l;
    D *= inv;
    float dq[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) dq[c] = scale * inv * (av[c] - D * bv[c]);
    if (act) store8(dQK + row * 128 + hd * 8, dq);
    St[hd * SS + i * 3 + 0] = m; St[hd * SS + i * 3 + 1] = inv; St[hd * SS + i * 3 + 2] = D;
    __syncthreads();
    // ---- pass B (per key j = this thread's view) ----
    float kj[8], vj[8], dk[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 8; ++c) { kj[c] = Ks[hd * HS + i * 8 + c]; vj[c] = Vs[hd * HS + i * 8 + c]; }
    for (int qi = 0; qi < V; ++qi) {
        const float* qq = Qs + hd * HS + qi * 8;
        const float* dd = Ds + hd * HS + qi * 8;
        const float pij = expf(scale * dot8(kj, qq) - St[hd * SS + qi * 3]) * St[hd * SS + qi * 3 + 1];
        const float ds = pij * (dot8(vj, dd) - St[hd * SS + qi * 3 + 2]);
#pragma unroll
        for (int c = 0; c < 8; ++c) { dk[c] += ds * qq[c]; dv[c] += pij * dd[c]; }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) dk[c] *= scale;
    if (act) {
        store8(dQK + row * 128 + 64 + hd * 8, dk);
        store8(dV + row * 64 + hd * 8, dv);
    }
}

// ------------------------------------------------------------------------------------------
// Up-sampler tail (reference LFT.py:41-43,80): F = PixelShuffle(lrelu(U)) is never built; Aact = lrelu(U) stays
// in token layout [N][64*s*s] (channel c*s*s + i*s + j <-> HR sub-pixel (i, j), LFT.py:41).  Forward: the mosaic-level
// 3x3 conv 64 -> 1 is the overlap-add GEMM of the inference path (G = M Aact through k_lin with the packed overlap-add
// matrix, then k_assemble_t); backward reads Aact through the index map.  Mosaic HR pixel (Ym, Xm) <-> LR mosaic pixel (Ym/s, Xm/s) =
// (a1*h + y, a2*w + x), sub-pixel (Ym % s, Xm % s).  Zero padding only at the mosaic border.
// ------------------------------------------------------------------------------------------
LFT_DEV long long up_token(int b, int Ym, int Xm, int A, int h, int w, int s, int& sub) {
    const int ly = Ym / s, lx = Xm / s;
    sub = (Ym - ly * s) * s + (Xm - lx * s);
    const int a1 = ly / h, a2 = lx / w;
    return (((long long)b * A * A + a1 * A + a2) * h + (ly - a1 * h)) * w + (lx - a2 * w);
}
// Backward of the tail, mirroring its forward (G = M Aact, out = gather of footprints):
//   dG[t][n]   = dout at the HR pixel that footprint entry n = (I+1)(S+2)+(J+1) of token t lands on (0 outside the mosaic,
//                0 in the padding columns n >= (S+2)^2)                                              -- k_up_gather_bwd
//   dAact      = M^T dG, times lrelu'  (k_lin with the transposed packed matrix and the activation epilogue)
//   dM         = dG^T Aact             (k_wgrad), folded back onto the 64 x 3 x 3 weight by k_upm_fold:
//                M[n(I,J)][c*ss + i*S + j] = w3[c][i-I+1][j-J+1]  =>  dw3[c][ty][tx] = sum_{i,j} dM[n(i-ty+1, j-tx+1)][c*ss + i*S + j]
__global__ __launch_bounds__(256) void k_up_gather_bwd(const float* __restrict__ dout, float* __restrict__ dG, int B, int A, int h, int w,
                                                       int s, int gld) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int V = A * A;
    const long long N = (long long)B * V * h * w;
    if (idx >= N * gld) return;
    const long long t = idx / gld;
    const int n = (int)(idx - t * gld), gp = (s + 2) * (s + 2);
    float v = 0.0f;
    if (n < gp) {
        const int I = n / (s + 2) - 1, J = n % (s + 2) - 1;
        const int x = (int)(t % w), y = (int)((t / w) % h), vv = (int)((t / ((long long)w * h)) % V), b = (int)(t / ((long long)w * h * V));
        const int Y = ((vv / A) * h + y) * s + I, X = ((vv % A) * w + x) * s + J;
        const int HH = A * h * s, WW = A * w * s;
        if (Y >= 0 && Y < HH && X >= 0 && X < WW) v = dout[((long long)b * HH + Y) * WW + X];
    }
    dG[idx] = v;
}
__global__ void k_upm_fold(const float* __restrict__ dM, float* __restrict__ dw3, int s) {       // dM: [32 gt][64 s^2]
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 576) return;
    const int c = idx / 9, ty = (idx % 9) / 3, tx = idx % 3, ss = s * s;
    float acc = 0.0f;
    for (int i = 0; i < s; ++i)
        for (int j = 0; j < s; ++j) {
            const int I = i - (ty - 1), J = j - (tx - 1);                        // always inside [-1, s]
            acc += dM[(size_t)((I + 1) * (s + 2) + (J + 1)) * 64 * ss + c * ss + i * s + j];
        }
    dw3[idx] = acc;
}

// conv_init0 weight gradient (reference LFT.py:24): dW0[c][tap] = sum_t dX0[t][c] * lr[view pixel (y+dy, x+dx)].
// One wave per token range, lane = channel.
__global__ __launch_bounds__(256) void k_conv0_wgrad(const float* __restrict__ dX0, const float* __restrict__ lr,
                                                     float* __restrict__ part, int B, int A, int h, int w, long long toks_per_wave) {
    const int c = threadIdx.x & 63, V = A * A;
    const long long wv = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long N = (long long)B * V * h * w;
    float dw[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) dw[t] = 0.0f;
    const long long t0 = wv * toks_per_wave, t1 = min(t0 + toks_per_wave, N);
    // the token's position (x, y, view, batch) once per wave, then by increments (four 64-bit divisions per token before)
    int x = 0, y = 0, v = 0, b = 0;
    if (t0 < t1) { x = (int)(t0 % w); y = (int)((t0 / w) % h); v = (int)((t0 / ((long long)w * h)) % V); b = (int)(t0 / ((long long)w * h * V)); }
    for (long long t = t0; t < t1; ++t) {
        const float* img = lr + (size_t)b * (A * h) * (A * w) + (size_t)((v / A) * h) * (A * w) + (v % A) * w;
        const float g = dX0[t * 64 + c];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            const float pv = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? img[yy * (A * w) + xx] : 0.0f;
            dw[tap] += g * pv;
        }
        if (++x == w) { x = 0; if (++y == h) { y = 0; if (++v == V) { v = 0; ++b; } } }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) part[wv * 576 + c * 9 + t] = dw[t];
}

// Gradient of the LR input (reference LFT.py:54 and :65: lr feeds the bicubic skip and conv_init0, nothing else), per view:
//   d_lr[y][x] = sum_tap sum_c W0[c][tap] dX0[token(y - dy, x - dx)][c]       conv_init0^T, zero padding at the view border
//              + sum_{oy, ox} Wy[oy][y] Wx[ox][x] dout[oy][ox]               bicubic^T (the skip's taps are clamped to the view)
// Wx[ox][x] is the sum of the cubic coefficients of those taps of output column ox that clamp onto x (source (ox + 0.5)/s - 0.5,
// taps floor - 1 .. floor + 2, as bicubic_at), so a border column collects every clamped tap.  Column ox reaches x only when
// (x - 2) s <= ox < (x + 3) s: 5 s terms per LR pixel and pass.  A gather with a fixed order of additions -- no atomics, every
// element of d_lr written once.  One workgroup per (image, view, 16 x 16 LR tile):
//   1. the dX0 rows of the tile-plus-halo tokens (16 lanes x 16 B per token, coalesced) are folded with W0 into 9 tap partials
//      per token, reduced across the 16 lanes, and staged in LDS (0 outside the view);
//   2. the tile's HR footprint of dout is staged in LDS and contracted separably, columns first, then rows;
//   3. each thread sums its pixel's 9 shifted tap partials and adds the bicubic term.
// dout may be null: the conv term alone (lft_lr_grad_bwd).
constexpr int kLrTile = 16;
template <int S>
__global__ __launch_bounds__(256) void k_lr_grad(const float* __restrict__ dX0, const float* __restrict__ w0, const float* __restrict__ dout,
                                                 float* __restrict__ d_lr, int A, int h, int w) {
    constexpr int T = kLrTile, PH = T + 2, NK = 5 * S, FD = (T + 4) * S;   // tile, partial staging edge, bicubic reach, footprint edge
    __shared__ float pt[9 * PH * PH];        // [tap][PH][PH]: tap partials of tokens (y0 - 1 .., x0 - 1 ..)
    __shared__ float dv[FD * FD];            // dout footprint [nfy][nfx]
    __shared__ float rr[FD * T];             // columns contracted: [nfy][T]
    __shared__ float wt[2 * T * NK];         // bicubic weights: x then y, [T][NK] each
    const int tid = threadIdx.x, V = A * A;
    const int tiles_x = (w + T - 1) / T, tiles = tiles_x * ((h + T - 1) / T);
    const int bid = xcd_tile(blockIdx.x, gridDim.x);            // a view's tiles share halo rows: keep them on one L2
    const int img = bid / tiles, tile = bid - img * tiles;      // img = b * V + view
    const int y0 = (tile / tiles_x) * T, x0 = (tile % tiles_x) * T;
    const int b = img / V, v = img - b * V, a1 = v / A, a2 = v - a1 * A;
    const int HS = h * S, WS = w * S;
    for (int i = tid; i < 9 * PH * PH; i += 256) pt[i] = 0.0f;
    // HR footprint of the tile: output rows / columns that can reach it, clipped to the view
    const int fy0 = max(0, (y0 - 2) * S), fy1 = min(HS, (y0 + T + 2) * S), fx0 = max(0, (x0 - 2) * S), fx1 = min(WS, (x0 + T + 2) * S);
    const int nfy = fy1 - fy0, nfx = fx1 - fx0;
    if (dout) {
        const float* dsrc = dout + (size_t)b * (A * HS) * (A * WS) + (size_t)(a1 * HS + fy0) * (A * WS) + (size_t)a2 * WS + fx0;
        const int nf = nfy * nfx;
        for (int i0 = 0; i0 < nf; i0 += 8 * 256) {              // eight loads in flight per thread before the first LDS write
            float r[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = min(i0 + u * 256 + tid, nf - 1), ry = i / nfx;
                r[u] = dsrc[(size_t)ry * (A * WS) + (i - ry * nfx)];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (i0 + u * 256 + tid < nf) dv[i0 + u * 256 + tid] = r[u];
        }
        for (int i = tid; i < 2 * T * NK; i += 256) {
            const int which = i / (T * NK), j = i - which * T * NK, l = j / NK, k = j - l * NK;
            const int n = which ? h : w, X = (which ? y0 : x0) + l, o = (X - 2) * S + k;
            float acc = 0.0f;
            if (X < n && o >= 0 && o < n * S) {
                const float src = ((float)o + 0.5f) / (float)S - 0.5f, f = floorf(src);
                float c[4];
                cubic_coef(src - f, c);
                const int i0 = (int)f - 1;
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    if (min(max(i0 + a, 0), n - 1) == X) acc += c[a];
            }
            wt[i] = acc;
        }
    }
    __syncthreads();                                            // partials zeroed before the fill below
    {
        const int hy0 = max(y0 - 1, 0), hx0 = max(x0 - 1, 0), nhx = min(x0 + T + 1, w) - hx0;
        const int ntk = (min(y0 + T + 1, h) - hy0) * nhx, q = tid & 15;     // q: this lane's channel quad
        float wq[4][9];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < 9; ++t) wq[j][t] = w0[(4 * q + j) * 9 + t];
        const float* X = dX0 + (size_t)img * h * w * 64 + 4 * q;
        for (int k0 = 0; k0 < ntk; k0 += 64) {                   // 16 tokens per workgroup pass, four passes' loads in flight
            f32x4 g[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = min(k0 + 16 * u + (tid >> 4), ntk - 1), ty = hy0 + k / nhx, tx = hx0 + k % nhx;
                g[u] = load4(X + ((size_t)ty * w + tx) * 64);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float p[9];
#pragma unroll
                for (int t = 0; t < 9; ++t) p[t] = wq[0][t] * g[u][0] + wq[1][t] * g[u][1] + wq[2][t] * g[u][2] + wq[3][t] * g[u][3];
#pragma unroll
                for (int m = 8; m >= 1; m >>= 1)
#pragma unroll
                    for (int t = 0; t < 9; ++t) p[t] += __shfl_xor(p[t], m);
                float mine = p[0];
#pragma unroll
                for (int t = 1; t < 9; ++t) mine = q == t ? p[t] : mine;
                const int k = k0 + 16 * u + (tid >> 4);
                if (k < ntk && q < 9) {
                    const int ty = hy0 + k / nhx, tx = hx0 + k % nhx;
                    pt[q * PH * PH + (ty - y0 + 1) * PH + (tx - x0 + 1)] = mine;
                }
            }
        }
    }
    if (dout) {                                                 // columns: rr[r][l] = sum_k Wx[l][k] dv[r][(x0 + l - 2) S + k - fx0]
        for (int i = tid; i < nfy * T; i += 256) {
            const int r = i / T, l = i - r * T, o0 = (x0 + l - 2) * S - fx0;
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < NK; ++k)
                if (o0 + k >= 0 && o0 + k < nfx) acc += wt[l * NK + k] * dv[r * nfx + o0 + k];
            rr[i] = acc;
        }
    }
    __syncthreads();
    const int ly = tid / T, lx = tid - ly * T, y = y0 + ly, x = x0 + lx;
    if (y >= h || x >= w) return;
    float acc = 0.0f;
#pragma unroll
    for (int t = 0; t < 9; ++t) acc += pt[t * PH * PH + (ly + 2 - t / 3) * PH + (lx + 2 - t % 3)];
    if (dout) {                                                 // rows: sum_k Wy[ly][k] rr[(y - 2) S + k - fy0][lx]
        const int o0 = (y - 2) * S - fy0;
        float bic = 0.0f;
#pragma unroll
        for (int k = 0; k < NK; ++k)
            if (o0 + k >= 0 && o0 + k < nfy) bic += wt[T * NK + ly * NK + k] * rr[(o0 + k) * T + lx];
        acc += bic;
    }
    d_lr[(size_t)b * (A * h) * (A * w) + (size_t)(a1 * h + y) * (A * w) + a2 * w + x] = acc;
}

}  // namespace
