// lft_network.hip -- the network in the C ABI of liblft_hip.so (include/lft_hip.h): the inference path (buffer layouts, weight
// packing plan, stage functions, per-stage test entry points) and the fp32 training step (tape queries, forward, the backward
// variants, gradient buckets, attention maps from the tape; the step itself is lft_train_host.cuh).  Host-side code only enqueues
// work on the caller's stream.  The library's other units: lft_lightfield.hip, lft_objective.hip (lft_amd/_lib.py: UNITS).
//
// Inference and training are ONE unit because hipcc's code for the fp32 inference kernels (k_conv64, k_ang, k_spa1, k_spa2,
// k_up with T = float) depends on whether the training kernels, which instantiate the same fp32 helpers of lft_common.cuh, are
// compiled in the same module: built apart, twelve of them come out with other instructions (tools/kernel_diff.py).
#include "lft_pack_host.cuh"
#include "lft_kernels_infer.cuh"
#include "lft_win_attn.cuh"   // fp32: the LDS-tiled window attention of the training step
#include "lft_train_host.cuh"
#include "lft_attn_maps.cuh" // attention weights from the tape's Q | K (lft_train_attn_maps)

// the library's error buffer and profiler (declared in lft_host.cuh)
char* lft_err_buf() {
    static thread_local char err[kErrLen] = "";
    return err;
}
LftProfiler& lft_prof() {
    static thread_local LftProfiler prof;
    return prof;
}

namespace {

// Fragment counts per stream
constexpr int kFragsConv = 72, kFragsAng = 64, kFragsSpa1 = 240, kFragsSpa1NoQ = 208, kFragsSpa2 = 176;
// 16-bit part B (k_spa_b) runs the 1x1x1 conv folded into the FFN's second Linear: kSpaBFrags fragments (lft_kernels_b.cuh)
inline int frags_spa2(int prec) { return prec == LFT_PREC_F32 ? kFragsSpa2 : kSpaBFrags; }
inline int frags_up(const Dims& d) { return d.nchunk * (4 + 2 * d.gt); }
// Workgroup tiles of NW x 32 tokens in one view image (ViewTile)
inline int view_tiles(const Dims& d, int NW) { return (d.hw + 32 * NW - 1) / (32 * NW); }

struct PackedLayout {
    size_t conv0_w, ln_ang[kLayers], ln_spa[kLayers], ang_pe, petok[kLayers], spa_pe_img;
    size_t w01, s_w01;          // 16-bit only: conv_init.0 composed with conv_init0, fp32 [64][kW01K], and its 12 fragments
    size_t spa_geom;            // 16-bit, lane-major view sizes only: k_spa_b's geometry table (k_spa_b_geom)
    size_t wlw2[kLayers];       // 16-bit only: the 1x1x1 conv composed with feed_forward.4, fp32 [64][256] (k_compose_wlw2)
    size_t s_conv[3], s_ang[kLayers], s_spa1[kLayers], s_spa2[kLayers], s_up, total;
};

PackedLayout packed_layout(const Dims& d, int prec) {
    const size_t esz = prec == LFT_PREC_F32 ? 4 : 2, fragb = 64 * 8 * esz;
    PackedLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = align256(o + bytes); return r; };
    L.conv0_w = take(576 * 4);
    for (int l = 0; l < kLayers; ++l) { L.ln_ang[l] = take(256 * 4); L.ln_spa[l] = take(512 * 4); }
    L.ang_pe = take((size_t)((d.V + 31) / 32) * 2048 * 4);                       // lane-major, per 32-view tile
    for (int l = 0; l < kLayers; ++l) L.petok[l] = take((size_t)view_tiles(d, kNwSpa1) * kNwSpa1 * 4096 * esz);   // lane-major, per 32-token tile
    L.spa_pe_img = take((size_t)d.hw * 64 * esz);
    // The W01 fragments sit directly in front of conv_init.2's stream (fragb is a multiple of 256): k_conv64_lr reads both as one
    const bool lp = prec != LFT_PREC_F32;
    L.w01 = take(lp ? 64 * kW01K * 4 : 0);
    L.s_conv[0] = take(kFragsConv * fragb);
    L.s_w01 = take(lp ? kW01Frags * fragb : 0);
    for (int i = 1; i < 3; ++i) L.s_conv[i] = take(kFragsConv * fragb);
    for (int l = 0; l < kLayers; ++l) {
        L.s_ang[l] = take(kFragsAng * fragb);
        L.s_spa1[l] = take(kFragsSpa1 * fragb);
        L.s_spa2[l] = take(frags_spa2(prec) * fragb);
    }
    L.s_up = take((size_t)frags_up(d) * fragb);
    for (int l = 0; l < kLayers; ++l) L.wlw2[l] = take(lp ? 64 * 256 * 4 : 0);
    // 16-bit with the lane-major hand-off (tok_lane_major): k_spa_b's per-lane geometry, one entry per query tile of a view
    const bool geom = lp && d.hw % (32 * kNwSpa1) == 0 && d.w % 32 == 0;
    L.spa_geom = take(geom ? (size_t)((d.h + kAttTY - 1) / kAttTY) * ((d.w + kAttTX - 1) / kAttTX) * kSpaBGeomTileBytes : 0);
    L.total = o;
    return L;
}

struct WorkLayout {
    size_t x0, feat, xa, xb, tok, q, k, v, o, g, status, total;     // status: the sticky flag word (lft_status_read), last 256 bytes
};
WorkLayout work_layout(const Dims& d, int prec) {
    const size_t esz = prec == LFT_PREC_F32 ? 4 : 2;
    WorkLayout W;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = align256(o + bytes); return r; };
    const size_t n = (size_t)d.ntok;
    W.x0 = take(n * 64 * esz); W.feat = take(n * 64 * esz); W.xa = take(n * 64 * esz); W.xb = take(n * 64 * esz);
    W.tok = take(n * 128 * esz); W.q = take(n * 128 * esz); W.k = take(n * 128 * esz); W.v = take(n * 128 * esz);
    W.o = take(n * 128 * esz);
    W.g = take(n * d.gp * 4);
    W.status = take(256);
    W.total = o;
    return W;
}
// What an inference entry point works with: the shape, both buffer layouts, the stream and the precision.  Made once per call by
// make_fwd, after the entry point's own null-pointer (and layer) checks; the stage functions below take it as `c`.
struct Fwd { Dims d; PackedLayout L; WorkLayout W; hipStream_t st; int prec; };
int make_fwd(int B, int A, int h, int w, int s, int prec, void* stream, Fwd* c) {
    if (int rc = make_dims(B, A, h, w, s, prec, &c->d)) return rc;
    c->L = packed_layout(c->d, prec);            // does not depend on B
    c->W = work_layout(c->d, prec);
    c->st = static_cast<hipStream_t>(stream);
    c->prec = prec;
    return 0;
}

// Dynamic LDS sizes (bytes): the total of the layout each kernel takes its pointers from (ConvLds, Spa1Lds, Spa2Lds, UpLds, AngLds).
template <typename T> size_t lds_conv64(int w) { return ConvLds<T>::total(w); }
// The 16-bit front end: k_conv64_lr adds the staged LR pixels, k_conv64<T, 2> conv_init0's weights; one size serves both
template <typename T> size_t lds_conv64_lr(int w) { return ConvLds<T>::total_lr(w); }
template <typename T, int CH = kSpaChunk> size_t lds_spa1(int w) { return Spa1Lds<T, CH>::total(w); }
template <typename T> size_t lds_spa2() { return Spa2Lds<T>::total; }
template <typename T> size_t lds_up() { return UpLds<T>::total; }
template <typename T> size_t lds_ang() { return AngLds<T, true, 0, 4>::total; }

void conv_ops(std::vector<PackOp>& v, const float* w, int nout) {   // [nout][64][3][3] == [nout][576], k index c*9 + tap
    for (int tap = 0; tap < 9; ++tap)
        for (int ks = 0; ks < 4; ++ks) v.push_back(lin_op(w, 0, nout, 576, 16 * ks, 1, 0, 1.0f, 9, tap));
}

// Lane-major hand-off of the spatial tokens from k_spa1 to part B: every workgroup tile of k_spa1 must be full, and the bf16
// consumer (k_spa_b, 8 x 4 blocks) additionally needs a tile to be 32 columns of ONE image row.
template <typename T> bool tok_lane_major(const Dims& d) {
    return d.hw % (32 * kNwSpa1) == 0 && (sizeof(T) == 4 || d.w % 32 == 0);
}
// k_spa1 launch with the ring chunk size that fits best: 16-fragment chunks if two workgroups then still share a CU
// (<= 80 KiB each) or if they are the only ones fitting at all... else 8-fragment chunks (wide views, fp32).
//
// The spatial path takes a different route per class of view size h x w.  tests/test_gpu_parity.py runs one case per class against
// the oracle and asserts the class itself from tests/spa_classes.py, a restatement of the two functions here and of the LDS sizes
// above (cases are named A<angRes>_s<scale>_B<batch>_<h>x<w>; "tail" = tests/test_gpu_tail.py, lft_tail_fwd):
//   128-token tiles of a view image (front-end convs, k_spa1)
//     one partial tile, starting at token 0              6x6, 8x8, 9x7, 6x5, 6x12 and the view-count cases
//     every tile full, starting at column 0 of a row     32x32, 64x64, 36x64
//     a later tile starting mid-row, partial last tile   13x11 (15 tokens, waves 1..3 empty), 17x19 (a middle tile; 32 32 3 0),
//                                                        35x37 (11 tiles), 31x32 (32 32 32 0), 53x55 .. 58x60
//     full tiles starting mid-row                        16x24;  row-aligned with w < 32: 24x16
//   hand-off k_spa1 -> part B, and last block -> k_up inside lft_forward
//     lane-major in every precision                      32x32, 64x64, 36x64;  partial last row tile of k_spa_b (h % 4 = 2): 62x64
//     lane-major in fp32, row-major in 16 bit            16x24, 24x16 (4x: GT = 2 in k_up)
//     row-major                                          every other case
//     lane-major tail (YLM store, k_up<.., LM> load) against the row-major one, bit for bit: tail 8x32, 32x32 (4x), 62x64; fp32 16x24, 24x16
//   k_spa_b's 4 x 32 query tiles, row-major
//     one column tile, partial                           every case with w < 32;  full with a 3-row last tile: 31x32
//     two column tiles, the second partial               35x37 (5 columns, 3-row last tile), 53x55 .. 58x60
//   k_spa1's ring chunk (launch_spa1 below)
//     16 bit: CH 16 up to w = 55, CH 8 from w = 56       53x55 | 54x56 (row-major), 62x64, 64x64 (lane-major);  CH 16 again from w = 152: not run
//     fp32:   CH 16 up to w = 59, CH 8 from w = 60       57x59 (163 072 B of LDS, with k_conv64 at w = 75 the largest allocation) | 58x60, 62x64, 64x64
//   widest view: fp32 75 columns (k_conv64), 16 bit 347 (k_conv64_lr); k_spa1 would take 155 / 471.  test_init_features_widest_view runs
//   3x75 / 3x347, test_too_wide_view_is_refused one column more (LFT_ERR_SHAPE from allow_lds, nothing launched).
template <typename T, bool PE_ONLY>
int launch_spa1(unsigned nwg, const T* in, const T* ws, const float* ln, const T* petok, T* tok, T* q, T* k, T* v, T* pe_out,
                int nimg, const Fwd& c, unsigned* status) {
    const Dims& d = c.d;
    const size_t l16 = lds_spa1<T, 16>(d.w), l8 = lds_spa1<T, 8>(d.w);
    const size_t share = kMaxLds / kSpaOcc;                               // LDS per workgroup if kSpaOcc of them share a CU
    const bool use8 = (l16 > share && l8 <= share) || l16 > kMaxLds;
    const bool lm = !PE_ONLY && tok_lane_major<T>(d);      // hand the token tile to part B in lane-major tile form
    return dispatch<8, 16>(use8 ? 8 : 16, [&](auto CH) {
        return dispatch<true, false>(lm, [&](auto LM) {
            // 16-bit with the lane-major hand-off: part B (k_spa_b) computes Q from the token tile itself; k_spa1 then skips that projection
            constexpr bool WQ = !(LM && sizeof(T) == 2);
            const size_t lds = CH == 8 ? l8 : l16;
            if (int rc = allow_lds(k_spa1<T, PE_ONLY, CH, LM, WQ>, lds, "k_spa1")) return rc;
            k_spa1<T, PE_ONLY, CH, LM, WQ><<<nwg, 64 * kNwSpa1, lds, c.st>>>(in, ws, ln, petok, tok, q, k, v, pe_out, nimg, d.h, d.w, status);
            return 0;
        });
    });
}

template <typename T>
int pack_impl(const Fwd& c, const float* const* P, void* packed) {
    const Dims& d = c.d;
    const hipStream_t st = c.st;
    const float kAngScale = 0.35355339059327373f * LFT_LOG2E;   // 1/sqrt(8) (head_dim 8), exp2 softmax
    const float kSpaScale = 0.25f * LFT_LOG2E;                   // 1/sqrt(16)
    int rc;
    k_copy_f32<<<3, 256, 0, st>>>(P[0], at<float>(packed, c.L.conv0_w), 576);
    LFT_LAUNCH_OK("k_copy_f32");
    for (int i = 0; i < 3; ++i) {
        std::vector<PackOp> ops;
        conv_ops(ops, P[1 + i], 64);
        if ((rc = run_pack<T>(ops, at<T>(packed, c.L.s_conv[i]), kFragsConv, st))) return rc;
    }
    if constexpr (sizeof(T) == 2) {     // conv_init.0 o conv_init0, composed in fp32, then rounded to ConvLrOp (half, also in bf16 mode: lft_kernels_a.cuh)
        k_compose_w01<<<blocks_for(64 * kW01K, 256), 256, 0, st>>>(P[0], P[1], at<float>(packed, c.L.w01));
        LFT_LAUNCH_OK("k_compose_w01");
        std::vector<PackOp> ops{lin_op(at<float>(packed, c.L.w01), 0, 64, kW01K, 0, kW01K / 16, 0, 1.0f)};
        if ((rc = run_pack<ConvLrOp>(ops, at<ConvLrOp>(packed, c.L.s_w01), kW01Frags, st))) return rc;
    }
    k_pe_tables<T><<<blocks_for(std::max<long long>((long long)((d.V + 31) / 32) * 2048, (long long)d.hw * 64), 256), 256, 0, st>>>(
        at<float>(packed, c.L.ang_pe), at<T>(packed, c.L.spa_pe_img), d.V, d.h, d.w);
    LFT_LAUNCH_OK("k_pe_tables");
    if constexpr (sizeof(T) == 2) {
        if (tok_lane_major<T>(d)) {     // the per-lane geometry of k_spa_b depends on h, w only: built once per view size
            k_spa_b_geom<<<(unsigned)(((d.h + kAttTY - 1) / kAttTY) * ((d.w + kAttTX - 1) / kAttTX)), 256, 0, st>>>(at<unsigned>(packed, c.L.spa_geom), d.h, d.w);
            LFT_LAUNCH_OK("k_spa_b_geom");
        }
    }
    for (int l = 0; l < kLayers; ++l) {
        const float* const* q = P + 4 + 18 * l;
        float* lnS = at<float>(packed, c.L.ln_spa[l]);
        float* lnA = at<float>(packed, c.L.ln_ang[l]);
        const int srcS[4] = {1, 2, 5, 6}, srcA[4] = {10, 11, 14, 15};
        for (int j = 0; j < 4; ++j) {
            k_copy_f32<<<1, 256, 0, st>>>(q[srcS[j]], lnS + 128 * j, 128);
            k_copy_f32<<<1, 256, 0, st>>>(q[srcA[j]], lnA + 64 * j, 64);
        }
        LFT_LAUNCH_OK("k_copy_f32");
        {   // angular stream
            std::vector<PackOp> ops;
            ops.push_back(lin_op(q[12], 0, 64, 64, 0, 4, 1, kAngScale));
            ops.push_back(lin_op(q[12], 64, 64, 64, 0, 4, 1, 1.0f));
            ops.push_back(lin_op(q[12], 128, 64, 64, 0, 4, 1, 1.0f));
            ops.push_back(lin_op(q[13], 0, 64, 64, 0, 4, 1, 1.0f));
            ops.push_back(lin_op(q[16], 0, 128, 64, 0, 4, 1, 1.0f));
            ops.push_back(lin_op(q[17], 0, 64, 128, 0, 8, 1, 1.0f));
            if ((rc = run_pack<T>(ops, at<T>(packed, c.L.s_ang[l]), kFragsAng, st))) return rc;
        }
        {   // spatial part 1: token embedding conv + in_proj
            std::vector<PackOp> ops;
            conv_ops(ops, q[0], 128);
            ops.push_back(lin_op(q[3], 256, 128, 128, 0, 8, 1, 1.0f));          // Wv (consumed first)
            ops.push_back(lin_op(q[3], 128, 128, 128, 0, 8, 1, 1.0f));          // Wk
            ops.push_back(lin_op(q[3], 0, 128, 128, 0, 8, 1, kSpaScale));      // Wq: last -- k_spa1's ring ends before it when part B computes Q itself (kFragsSpa1NoQ)
            if ((rc = run_pack<T>(ops, at<T>(packed, c.L.s_spa1[l]), kFragsSpa1, st))) return rc;
        }
        {   // spatial part 2: out_proj, FFN in 4 chunks, 1x1x1 conv.  out_proj's operand: bf16 -- the attention accumulators
            // inside k_spa_b (acc order); fp32 -- the attention output read back from memory by k_spa2 (natural k)
            std::vector<PackOp> ops;
            // 16-bit (k_spa_b): element (h, j) of the attention fragment is the head's channel label 8 h + j of the V tile in LDS.
            // Row-major K / V: labels are the channels themselves -- natural packing.  Lane-major Q / K / V (tok_lane_major): k_spa1
            // wrote each head's 16 channels in acc order, so label 8 h + j is channel acc(h, j) -- acc-order packing.
            ops.push_back(lin_op(q[4], 0, 128, 128, 0, 8, (sizeof(T) == 2 && tok_lane_major<T>(d)) ? 1 : 0, 1.0f));
            if constexpr (sizeof(T) == 2) {
                // No non-linearity stands between feed_forward.4 (W2) and the 1x1x1 conv (Wl, reference LFT.py:171-174, 187-189):
                // y = Wl (t + W2 hid) = Wl t + (Wl W2) hid.  Wl W2 [64][256] is composed in fp32 and rounded once by k_pack.
                // Stream: Wo[4x8] Wl[2x8] {W1c[2x8] WlW2c[2x4]} x4
                float* wlw2 = at<float>(packed, c.L.wlw2[l]);
                k_compose_wlw2<<<blocks_for(64 * 256, 256), 256, 0, st>>>(q[9], q[8], wlw2);
                LFT_LAUNCH_OK("k_compose_wlw2");
                ops.push_back(lin_op(q[9], 0, 64, 128, 0, 8, 1, 1.0f));
                for (int c = 0; c < 4; ++c) {
                    ops.push_back(lin_op(q[7], 64 * c, 64, 128, 0, 8, 1, 1.0f));
                    ops.push_back(lin_op(wlw2, 0, 64, 256, 64 * c, 4, 1, 1.0f));
                }
            } else {
                for (int c = 0; c < 4; ++c) {
                    ops.push_back(lin_op(q[7], 64 * c, 64, 128, 0, 8, 1, 1.0f));
                    ops.push_back(lin_op(q[8], 0, 128, 256, 64 * c, 4, 1, 1.0f));
                }
                ops.push_back(lin_op(q[9], 0, 64, 128, 0, 8, 1, 1.0f));
            }
            if ((rc = run_pack<T>(ops, at<T>(packed, c.L.s_spa2[l]), frags_spa2(c.prec), st))) return rc;
        }
        // embedded spatial position tokens of this layer (reference LFT.py:180), [h*w][128] in the activation type
        if ((rc = launch_spa1<T, true>((unsigned)view_tiles(d, kNwSpa1), at<T>(packed, c.L.spa_pe_img), at<T>(packed, c.L.s_spa1[l]), nullptr, nullptr,
                                       nullptr, nullptr, nullptr, nullptr, at<T>(packed, c.L.petok[l]), 1, c, nullptr))) return rc;
        LFT_LAUNCH_OK("k_spa1<pe>");
    }
    {   // up-sampler: per 32-row chunk of the 1x1 conv, followed by the matching columns of the overlap-add matrix
        std::vector<PackOp> ops;
        for (int c = 0; c < d.nchunk; ++c) {
            ops.push_back(lin_op(P[76], 32 * c, 32, 64, 0, 4, 1, 1.0f));
            PackOp m = lin_op(P[77], 0, d.gp, 0, 32 * c, 2, 1, 1.0f);
            m.kind = 1; m.s = d.s; m.ntiles = d.gt;
            ops.push_back(m);
        }
        if ((rc = run_pack<T>(ops, at<T>(packed, c.L.s_up), frags_up(d), st))) return rc;
    }
    return 0;
}

// ---------------------------------------------------------------------------- stages
// The front end as it was before the composition, and as fp32 still runs it: conv_init0 to memory, three 64 -> 64 convs.
// conv_init0 to memory (tokens [B,V,h,w,64])
template <typename T>
int launch_conv0(const Fwd& c, const void* packed, const float* lr, T* x0) {
    const Dims& d = c.d;
    k_conv0<T><<<dim3((unsigned)((d.hw + kConv0Tok - 1) / kConv0Tok), (unsigned)(d.B * d.V)), 256, 0, c.st>>>(lr, at<float>(packed, c.L.conv0_w), x0, d.B, d.A, d.h, d.w);
    LFT_LAUNCH_OK("k_conv0");
    return 0;
}
// conv_init.<2 i> over every view image; the caller has allowed `lds` for this RES (before its first launch, so that a view too
// wide is refused with nothing launched)
template <typename T, int RES>
int launch_conv64(const Fwd& c, const void* packed, size_t lds, int i, const T* in, T* out, const T* res = nullptr, ConvLr cl = ConvLr{}) {
    const Dims& d = c.d;
    const int nimg = d.B * d.V;
    k_conv64<T, RES><<<nimg * view_tiles(d, kNwConv), 64 * kNwConv, lds, c.st>>>(in, out, res, at<T>(packed, c.L.s_conv[i]), nimg, d.h, d.w, cl);
    LFT_LAUNCH_OK("k_conv64");
    return 0;
}
template <typename T>
int init_features_x0(const Fwd& c, const void* packed, const float* lr, T* x0, T* ta, T* tb, T* feat) {
    const size_t lds = lds_conv64<T>(c.d.w);
    int rc;
    if ((rc = allow_lds(k_conv64<T, 0>, lds, "k_conv64"))) return rc;
    if ((rc = allow_lds(k_conv64<T, 1>, lds, "k_conv64"))) return rc;
    if ((rc = launch_conv0<T>(c, packed, lr, x0))) return rc;
    if ((rc = launch_conv64<T, 0>(c, packed, lds, 0, x0, ta))) return rc;
    if ((rc = launch_conv64<T, 0>(c, packed, lds, 1, ta, tb))) return rc;
    return launch_conv64<T, 1>(c, packed, lds, 2, tb, feat, x0);
}
// 16-bit: two launches.  conv_init0 is composed into conv_init.0 (k_conv64_lr: LR mosaic -> tb) and recomputed for the
// residual of conv_init.4 (k_conv64<T, 2>); x0 and ta are never written.  Both launches carry the name "k_conv64": the
// benchmark's per-kernel tables are indexed by the names lft_forward_profiled returns.
template <typename T>
int init_features(const Fwd& c, const void* packed, const float* lr, T* x0, T* ta, T* tb, T* feat) {
    if constexpr (sizeof(T) == 4) return init_features_x0<T>(c, packed, lr, x0, ta, tb, feat);
    else {
        const Dims& d = c.d;
        const int nimg = d.B * d.V, nwg = nimg * view_tiles(d, kNwConv);
        const size_t lds = lds_conv64_lr<T>(d.w);
        int rc;
        if (c.L.s_w01 + kW01Frags * 1024 != c.L.s_conv[1]) return fail(LFT_ERR_ARG, "internal: W01 fragments are not in front of conv_init.2's stream");
        if ((rc = allow_lds(k_conv64_lr<T>, lds, "k_conv64"))) return rc;
        if ((rc = allow_lds(k_conv64<T, 2>, lds, "k_conv64"))) return rc;
        k_conv64_lr<T><<<nwg, 64 * kNwConv, lds, c.st>>>(lr, tb, at<T>(packed, c.L.s_w01), d.A, nimg, d.h, d.w);
        LFT_LAUNCH_OK("k_conv64");
        return launch_conv64<T, 2>(c, packed, lds, 2, tb, feat, nullptr, ConvLr{lr, at<float>(packed, c.L.conv0_w), d.A});
    }
}
// Grid of the persistent angular kernels, `per_wg` positions per workgroup: what the positions need, at most what 256 CUs hold by LDS
inline unsigned ang_grid(int npix, int per_wg, size_t lds) { return std::min<unsigned>(blocks_for(npix, per_wg), 256u * (unsigned)std::max<size_t>(1, kMaxLds / lds)); }
template <typename T, int CT, int LL>      // LL: score registers of the last key tile that can hold a view, which covers rows acc_row(i, 0) and acc_row(i, 1) = +4 of register i
int ang_multi(const Fwd& c, const void* packed, int l, const T* in, T* out, unsigned* status) {
    const Dims& d = c.d;
    constexpr bool WLDS = sizeof(T) == 2;                                   // fp32 weights (128 KiB) stay in L2
    constexpr int NG = (sizeof(T) == 2 && CT <= 3) ? 2 : 1;                 // positions per workgroup (they share the LDS weights)
    const size_t lds = AngLds<T, WLDS, NG * CT * 8, NG * CT>::total;
    const int npix = d.B * d.hw;
    int rc;
    const unsigned grid = ang_grid(npix, NG, lds);
    if ((rc = allow_lds(k_ang_multi<T, CT, WLDS, NG, LL>, lds, "k_ang_multi"))) return rc;
    k_ang_multi<T, CT, WLDS, NG, LL><<<grid, 64 * CT * NG, lds, c.st>>>(in, out, at<T>(packed, c.L.s_ang[l]), at<float>(packed, c.L.ln_ang[l]),
                                                                     at<float>(packed, c.L.ang_pe), d.V, d.hw, npix, status);
    LFT_LAUNCH_OK("k_ang");
    return 0;
}
// One kernel instantiation per class of view count, each in the three precisions.  tests/test_gpu_parity.py runs every one of
// them against the oracle: test_ang_block[<case>-<layer>-<prec>] on a few dozen positions, test_ang_block_many_positions[<A>-<prec>]
// on more positions than the grid covers in one sweep (1155 or 2205, odd), where the workgroups loop:
//   V <= 25  (A 1 .. 5)  k_ang<T, 13>              cases A5_s2_B2_6x6, A3_s2_B1_9x7, A2_*, A1_s2_B2_6x7, A4_s2_B1_5x5;  many_positions[1-*], [4-*]
//   V 36, 49 (A 6, 7)    k_ang_multi<T, 2, LL 9>   cases A6_s2_B1_6x5, A7_s2_B1_3x5;                                  many_positions[6-*], [7-*]
//   V 64     (A 8)       k_ang_multi<T, 2, LL 16>  case  A8_s2_B1_5x3;                                                many_positions[8-*]
//   V 81     (A 9)       k_ang_multi<T, 3, LL 9>   case  A9_s4_B1_8x8;                                                many_positions[9-*]
//   V 100    (A 10)      k_ang_multi<T, 4, LL 9>   case  A10_s4_B1_3x5;                                               many_positions[10-*]
//   V 121    (A 11)      k_ang_multi<T, 4, LL 13>  case  A11_s2_B1_4x3;                                               many_positions[11-*]
template <typename T>
int ang_block(const Fwd& c, const void* packed, int l, const T* in, T* out, unsigned* status = nullptr) {
    const Dims& d = c.d;
    // V = A*A (make_dims): above 32 views only 36, 49 | 64 | 81 | 100 | 121 occur, with 4, 17 | 32 | 17 | 4 | 25 rows in the last key tile
    auto multi = [&](auto CT, auto LL) { return ang_multi<T, CT, LL>(c, packed, l, in, out, status); };
    if (d.V > 100) return multi(int_c<4>{}, int_c<13>{});
    if (d.V > 96) return multi(int_c<4>{}, int_c<9>{});
    if (d.V > 64) return multi(int_c<3>{}, int_c<9>{});
    if (d.V == 64) return multi(int_c<2>{}, int_c<16>{});
    if (d.V > 32) return multi(int_c<2>{}, int_c<9>{});
    const int npix = d.B * d.hw;
    const size_t lds = lds_ang<T>();
    int rc;
    const unsigned grid = ang_grid(npix, 4, lds);
    // V <= 25 (5 x 5 and smaller): score rows 25..31 are never a view
    if ((rc = allow_lds(k_ang<T, 13>, lds, "k_ang"))) return rc;
    k_ang<T, 13><<<grid, 256, lds, c.st>>>(in, out, at<T>(packed, c.L.s_ang[l]), at<float>(packed, c.L.ln_ang[l]),
                                         at<float>(packed, c.L.ang_pe), d.V, d.hw, npix, status);
    LFT_LAUNCH_OK("k_ang");
    return 0;
}
// SpaTrans = part A (k_spa1: token embedding, LayerNorm, Q / K / V) + part B (attention and the per-token tail).
template <typename T>
int spa_part_a(const Fwd& c, const void* packed, int l, const T* in, void* ws) {
    const Dims& d = c.d;
    const int nimg = d.B * d.V, nwg = nimg * view_tiles(d, kNwSpa1);
    int rc;
    if ((rc = launch_spa1<T, false>((unsigned)nwg, in, at<T>(packed, c.L.s_spa1[l]), at<float>(packed, c.L.ln_spa[l]), at<T>(packed, c.L.petok[l]),
                                    at<T>(ws, c.W.tok), at<T>(ws, c.W.q), at<T>(ws, c.W.k), at<T>(ws, c.W.v), nullptr, nimg, c, at<unsigned>(ws, c.W.status)))) return rc;
    LFT_LAUNCH_OK("k_spa1");
    return 0;
}
// k_spa_b / k_spa2 variants: launch(SKIP, TOKLM, YLM) as integral constants.  A lane-major output (YLM, the up-sampler's input)
// is only produced by the skip variant from lane-major tokens.
template <typename F> int with_tail_variant(bool skip, bool tok_lm, bool out_lm, F&& launch) {
    if (out_lm) {
        if (!(skip && tok_lm)) return fail(LFT_ERR_ARG, "internal: lane-major output needs the skip variant and lane-major tokens");
        return launch(std::true_type{}, std::true_type{}, std::true_type{});
    }
    return dispatch<true, false>(skip, [&](auto SK) {
        return dispatch<true, false>(tok_lm, [&](auto LM) { return launch(SK, LM, std::false_type{}); });
    });
}
template <typename T>
int spa_part_b(const Fwd& c, const void* packed, int l, const T* skip, T* out, void* ws, bool out_lm = false) {      // out_lm: lane-major output tiles, only for the up-sampler
    const Dims& d = c.d;
    const hipStream_t st = c.st;
    const int nimg = d.B * d.V;
    T *tok = at<T>(ws, c.W.tok), *q = at<T>(ws, c.W.q), *k = at<T>(ws, c.W.k), *v = at<T>(ws, c.W.v), *o = at<T>(ws, c.W.o);
    const float* ln = at<float>(packed, c.L.ln_spa[l]);
    const bool lm = tok_lane_major<T>(d);      // must match launch_spa1's choice
    int rc;
    if constexpr (sizeof(T) == 2) {
        // bf16: windowed attention + out_proj + FFN + 1x1x1 conv in ONE kernel (the attention output stays in registers)
        const unsigned ntile = (unsigned)(nimg * ((d.h + kAttTY - 1) / kAttTY) * ((d.w + kAttTX - 1) / kAttTX));
        if ((rc = with_tail_variant(skip, lm, out_lm, [&](auto SK, auto LM, auto YL) {
                 if (int r = allow_lds(k_spa_b<T, SK, LM, YL>, kSpaBLds, "k_spa_b")) return r;
                 k_spa_b<T, SK, LM, YL><<<ntile, 256, kSpaBLds, st>>>(tok, q, k, v, at<T>(packed, c.L.s_spa2[l]), ln, skip, out, d.h, d.w,
                                                                      at<unsigned>(ws, c.W.status), at<T>(packed, c.L.s_spa1[l]) + (size_t)kFragsSpa1NoQ * 512,
                                                                      at<T>(packed, c.L.petok[l]), at<unsigned>(packed, c.L.spa_geom));
                 return 0;
             }))) return rc;
        LFT_LAUNCH_OK("k_spa_b");
        return 0;
    } else {
        // fp32: the LDS-tiled window attention of the training step (8 x 16 query tile x head pair per workgroup), Q pre-scaled
        const unsigned tiles = (unsigned)(((d.w + kWaTX - 1) / kWaTX) * ((d.h + kWaTY - 1) / kWaTY) * nimg);
        if ((rc = allow_lds(k_win_attn_lds<0, true>, kWaLds, "k_win_attn_lds"))) return rc;
        k_win_attn_lds<0, true><<<dim3(tiles, 4), 256, kWaLds, st>>>(reinterpret_cast<const float*>(q), reinterpret_cast<const float*>(k),
                                                                     reinterpret_cast<const float*>(v), reinterpret_cast<float*>(o),
                                                                     nullptr, nullptr, nullptr, nullptr, nullptr, d.h, d.w, 128);
        LFT_LAUNCH_OK("k_spa_attn");
        const unsigned nb = blocks_for(d.ntok, 32 * kNwSpa2);
        if ((rc = with_tail_variant(skip, lm, out_lm, [&](auto SK, auto LM, auto YL) {
                 if (int r = allow_lds(k_spa2<T, SK, LM, YL>, lds_spa2<T>(), "k_spa2")) return r;
                 k_spa2<T, SK, LM, YL><<<nb, 64 * kNwSpa2, lds_spa2<T>(), st>>>(tok, o, at<T>(packed, c.L.s_spa2[l]), ln, skip, out, d.ntok, at<unsigned>(ws, c.W.status));
                 return 0;
             }))) return rc;
        LFT_LAUNCH_OK("k_spa2");
        return 0;
    }
}
template <typename T>
int spa_block(const Fwd& c, const void* packed, int l, const T* in, const T* skip, T* out, void* ws, bool out_lm = false) {
    if (int rc = spa_part_a<T>(c, packed, l, in, ws)) return rc;
    return spa_part_b<T>(c, packed, l, skip, out, ws, out_lm);
}
template <typename T>
int upsample(const Fwd& c, const void* packed, const T* body, const float* lr, float* out, void* ws, bool in_lm = false) {
    const Dims& d = c.d;
    const hipStream_t st = c.st;
    float* g = at<float>(ws, c.W.g);
    const unsigned nb = blocks_for(d.ntok, 32 * kNwUp);
    int rc = dispatch<1, 2>(d.gt, [&](auto GT) {
        return dispatch<true, false>(in_lm, [&](auto LM) {
            if (int r = allow_lds(k_up<T, GT, LM>, lds_up<T>(), "k_up")) return r;
            k_up<T, GT, LM><<<nb, 64 * kNwUp, lds_up<T>(), st>>>(body, at<T>(packed, c.L.s_up), g, d.ntok, d.nchunk, d.gp);
            return 0;
        });
    });
    if (rc) return rc;
    LFT_LAUNCH_OK("k_up");
    launch_assemble(lr, g, out, d.B, d.A, d.h, d.w, d.s, st, 0, at<unsigned>(ws, c.W.status));
    LFT_LAUNCH_OK("k_assemble");
    return 0;
}

template <typename T>
int forward_impl(const Fwd& c, const void* packed, const float* lr, float* out, void* ws) {
    const Dims& d = c.d;
    T *x0 = at<T>(ws, c.W.x0), *feat = at<T>(ws, c.W.feat), *xa = at<T>(ws, c.W.xa), *xb = at<T>(ws, c.W.xb);
    int rc;
    if ((rc = init_features<T>(c, packed, lr, x0, xa, xb, feat))) return rc;
    const T* cur = feat;
    for (int l = 0; l < kLayers; ++l) {                  // angular first, then spatial (reference LFT.py:249-250)
        if ((rc = ang_block<T>(c, packed, l, cur, xa, at<unsigned>(ws, c.W.status)))) return rc;
        const bool last = l == kLayers - 1;                  // its output only feeds the up-sampler: same 32-token tiling, lane-major tiles
        if ((rc = spa_block<T>(c, packed, l, xa, last ? feat : nullptr, xb, ws, last && tok_lane_major<T>(d)))) return rc;
        cur = xb;
    }
    return upsample<T>(c, packed, xb, lr, out, ws, tok_lane_major<T>(d));
}

// Mean duration of ONE kernel of the forward, launched `reps` times back to back between two HIP events on `stream` (no
// event between launches, unlike lft_forward_profiled).  Inputs are whatever a previous lft_forward left in the
// workspace.  Synchronises the stream.  kernel: "k_conv64", "k_ang", "k_spa1", "k_spa_b" (bf16) / "k_spa2" ... see below.
template <typename T>
int kernel_time_impl(const Fwd& c, const char* name, const void* packed, void* ws, int reps, float* ms_out) {
    const Dims& d = c.d;
    const hipStream_t st = c.st;
    T *x0 = at<T>(ws, c.W.x0), *feat = at<T>(ws, c.W.feat), *xa = at<T>(ws, c.W.xa), *xb = at<T>(ws, c.W.xb);
    const std::string k(name);
    auto once = [&]() -> int {
        if (k == "k_ang") return ang_block<T>(c, packed, 1, xb, xa, at<unsigned>(ws, c.W.status));
        if (k == "k_spa1") return spa_part_a<T>(c, packed, 1, xa, ws);
        if (k == "k_spa_b" || k == "k_spa_attn+k_spa2") return spa_part_b<T>(c, packed, 1, nullptr, xb, ws);
        if (k == "k_conv64") {
            const size_t lds = lds_conv64<T>(d.w);
            if (int rc = allow_lds(k_conv64<T, 0>, lds, "k_conv64")) return rc;
            // input: xb, which every forward writes (the 16-bit front end no longer writes x0); output: x0, which nothing reads
            return launch_conv64<T, 0>(c, packed, lds, 0, xb, x0);
        }
        return fail(LFT_ERR_ARG, "lft_kernel_time: unknown kernel %s", name);
    };
    int rc;
    if ((rc = once())) return rc;                                     // warm (attributes, caches)
    hipEvent_t e0, e1;
    LFT_HIP_OK(hipEventCreate(&e0));
    LFT_HIP_OK(hipEventCreate(&e1));
    LFT_HIP_OK(hipEventRecord(e0, st));
    for (int i = 0; i < reps && !rc; ++i) rc = once();
    LFT_HIP_OK(hipEventRecord(e1, st));
    LFT_HIP_OK(hipEventSynchronize(e1));
    float ms = 0.0f;
    LFT_HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (rc) return rc;
    *ms_out = ms / (float)reps;
    return 0;
}



// The tape fields lft_train_tape_offset knows: top level, and per layer behind "ang<l>." / "spa<l>."
template <typename S> struct TapeField { const char* name; size_t S::*member; };
constexpr TapeField<TrainLayout> kTapeTop[] = {{"x0", &TrainLayout::x0}, {"feat", &TrainLayout::feat}, {"c1", &TrainLayout::c1}, {"c2", &TrainLayout::c2},
                                               {"c3", &TrainLayout::c3}, {"body", &TrainLayout::body}, {"act", &TrainLayout::act}, {"skip", &TrainLayout::skip}};
constexpr TapeField<AngTape> kTapeAng[] = {{"n", &AngTape::n}, {"qk", &AngTape::qk}, {"v", &AngTape::v}, {"o", &AngTape::o},
                                           {"t1", &AngTape::t1}, {"m", &AngTape::m}, {"hdn", &AngTape::hdn}, {"y", &AngTape::y}};
constexpr TapeField<SpaTape> kTapeSpa[] = {{"tok", &SpaTape::tok}, {"n", &SpaTape::n}, {"qk", &SpaTape::qk}, {"v", &SpaTape::v}, {"o", &SpaTape::o},
                                           {"t1", &SpaTape::t1}, {"m", &SpaTape::m}, {"hdn", &SpaTape::hdn}, {"t2", &SpaTape::t2}, {"y", &SpaTape::y},
                                           {"petok", &SpaTape::petok}};
template <typename S, size_t N> bool tape_field(const TapeField<S> (&table)[N], const S& tape, const std::string& name, size_t* out) {
    for (const auto& f : table)
        if (name == f.name) { *out = tape.*f.member; return true; }
    return false;
}

}  // namespace

// ================================================================================ C ABI
extern "C" {

int lft_version(void) { return LFT_ABI_VERSION; }
const char* lft_last_error(void) { return lft_err_buf(); }

int lft_packed_bytes(int A, int h, int w, int s, int prec, size_t* out_bytes) {
    Fwd c;
    if (!out_bytes) return fail(LFT_ERR_ARG, "out_bytes is null");
    if (int rc = make_fwd(1, A, h, w, s, prec, nullptr, &c)) return rc;
    *out_bytes = c.L.total;
    return 0;
}
int lft_workspace_bytes(int B, int A, int h, int w, int s, int prec, size_t* out_bytes) {
    Fwd c;
    if (!out_bytes) return fail(LFT_ERR_ARG, "out_bytes is null");
    if (int rc = make_fwd(B, A, h, w, s, prec, nullptr, &c)) return rc;
    *out_bytes = c.W.total;
    return 0;
}

int lft_pack_weights(const float* const* params, int nparams, void* packed, int A, int h, int w, int s, int prec, void* stream) {
    Fwd c;
    if (!params || !packed) return fail(LFT_ERR_ARG, "null pointer");
    if (nparams != LFT_NUM_PARAMS) return fail(LFT_ERR_ARG, "expected %d parameter tensors, got %d", LFT_NUM_PARAMS, nparams);
    for (int i = 0; i < nparams; ++i)
        if (!params[i]) return fail(LFT_ERR_ARG, "parameter %d is null", i);
    if (int rc = make_fwd(1, A, h, w, s, prec, stream, &c)) return rc;
    return by_prec(prec, [&](auto t) { return pack_impl<decltype(t)>(c, params, packed); });
}

int lft_forward(const void* packed, const float* lr, float* out, void* workspace, int B, int A, int h, int w, int s, int prec, void* stream) {
    Fwd c;
    if (!packed || !lr || !out || !workspace) return fail(LFT_ERR_ARG, "null pointer");
    if (int rc = make_fwd(B, A, h, w, s, prec, stream, &c)) return rc;
    return by_prec(prec, [&](auto t) { return forward_impl<decltype(t)>(c, packed, lr, out, workspace); });
}

int lft_status_reset(void* workspace, int B, int A, int h, int w, int s, int prec, void* stream) {
    Fwd c;
    if (!workspace) return fail(LFT_ERR_ARG, "null pointer");
    if (int rc = make_fwd(B, A, h, w, s, prec, stream, &c)) return rc;
    LFT_HIP_OK(hipMemsetAsync(at<char>(workspace, c.W.status), 0, 256, c.st));
    return 0;
}
int lft_status_read(const void* workspace, int B, int A, int h, int w, int s, int prec, void* stream, unsigned* host_flags) {
    Fwd c;
    if (!workspace) return fail(LFT_ERR_ARG, "null pointer");
    if (int rc = make_fwd(B, A, h, w, s, prec, stream, &c)) return rc;
    unsigned flags = 0;
    LFT_HIP_OK(hipMemcpyAsync(&flags, at<char>(workspace, c.W.status), sizeof(flags), hipMemcpyDeviceToHost, c.st));
    LFT_HIP_OK(hipStreamSynchronize(c.st));
    if (host_flags) *host_flags = flags;
    if (flags == 0) return 0;
    return fail(LFT_STATUS_NONFINITE, "non-finite activations or outputs since the last lft_status_reset (flags 0x%x)%s", flags,
                prec == LFT_PREC_F16 ? ": an activation left the fp16 range (|x| > 65504) or the input holds inf / NaN -- use LFT_PREC_BF16 or LFT_PREC_F32 for these weights"
                                     : ": the input or the weights hold inf / NaN, or an activation overflowed");
}

int lft_forward_profiled(const void* packed, const float* lr, float* out, void* workspace, int B, int A, int h, int w, int s, int prec,
                         void* stream, int max_records, float* ms_out, const char** names_out, int* n_out) {
    if (!ms_out || !names_out || !n_out) return fail(LFT_ERR_ARG, "null pointer");
    return run_profiled(static_cast<hipStream_t>(stream), max_records, ms_out, names_out, n_out,
                        [&] { return lft_forward(packed, lr, out, workspace, B, A, h, w, s, prec, stream); });
}

int lft_kernel_time(const char* kernel, const void* packed, void* workspace, int B, int A, int h, int w, int s, int prec, int reps,
                    void* stream, float* ms_out) {
    Fwd c;
    if (!kernel || !packed || !workspace || !ms_out || reps < 1) return fail(LFT_ERR_ARG, "bad argument");
    if (int rc = make_fwd(B, A, h, w, s, prec, stream, &c)) return rc;
    return by_prec(prec, [&](auto t) { return kernel_time_impl<decltype(t)>(c, kernel, packed, workspace, reps, ms_out); });
}

int lft_bicubic_fwd(const float* lr, float* out, int B, int A, int h, int w, int s, void* stream) {
    Dims d; int rc;
    if (!lr || !out) return fail(LFT_ERR_ARG, "null pointer");
    if ((rc = make_dims(B, A, h, w, s, LFT_PREC_F32, &d))) return rc;
    const dim3 grid((unsigned)((A * w * s + 255) / 256), (unsigned)(A * h * s), (unsigned)B);
    k_bicubic<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(lr, out, B, A, h, w, s);
    LFT_LAUNCH_OK("k_bicubic");
    return 0;
}

// lft_init_features_fwd, and (legacy, test-only: include/lft_hip_test.h) the front end as it ran before the composition
static int init_features_entry(bool legacy, const void* packed, const float* lr, void* act_out, void* workspace, int B, int A, int h, int w, int s,
                               int prec, void* stream) {
    Fwd c;
    if (!packed || !lr || !act_out || !workspace) return fail(LFT_ERR_ARG, "null pointer");
    if (int rc = make_fwd(B, A, h, w, s, prec, stream, &c)) return rc;
    return by_prec(prec, [&](auto t) {
        using T = decltype(t);
        T *x0 = at<T>(workspace, c.W.x0), *xa = at<T>(workspace, c.W.xa), *xb = at<T>(workspace, c.W.xb), *feat = static_cast<T*>(act_out);
        return legacy ? init_features_x0<T>(c, packed, lr, x0, xa, xb, feat) : init_features<T>(c, packed, lr, x0, xa, xb, feat);
    });
}
int lft_init_features_fwd(const void* packed, const float* lr, void* act_out, void* workspace, int B, int A, int h, int w, int s,
                          int prec, void* stream) {
    return init_features_entry(false, packed, lr, act_out, workspace, B, A, h, w, s, prec, stream);
}
int lft_init_features_legacy_fwd(const void* packed, const float* lr, void* act_out, void* workspace, int B, int A, int h, int w, int s,
                                 int prec, void* stream) {
    return init_features_entry(true, packed, lr, act_out, workspace, B, A, h, w, s, prec, stream);
}

int lft_conv0_fwd(const void* packed, const float* lr, void* x0_out, int recomputed, int B, int A, int h, int w, int s, int prec, void* stream) {
    Fwd c;
    if (!packed || !lr || !x0_out) return fail(LFT_ERR_ARG, "null pointer");
    if (int rc = make_fwd(B, A, h, w, s, prec, stream, &c)) return rc;
    if (recomputed && prec == LFT_PREC_F32) return fail(LFT_ERR_ARG, "conv_init0 is recomputed in the 16-bit precisions only");
    return by_prec(prec, [&](auto t) {
        using T = decltype(t);
        const Dims& d = c.d;
        const int nimg = d.B * d.V;
        if constexpr (sizeof(T) == 2) {
            if (recomputed) {
                k_conv0_recomputed<T><<<nimg * view_tiles(d, kNwConv), 64 * kNwConv, 0, c.st>>>(static_cast<T*>(x0_out), nimg, d.h, d.w,
                                                                                                ConvLr{lr, at<float>(packed, c.L.conv0_w), d.A});
                LFT_LAUNCH_OK("k_conv0_recomputed");
                return 0;
            }
        }
        return launch_conv0<T>(c, packed, lr, static_cast<T*>(x0_out));
    });
}

int lft_ang_block_fwd(const void* packed, int layer, const void* act_in, void* act_out, int B, int A, int h, int w, int s, int prec,
                      void* stream) {
    Fwd c;
    if (!packed || !act_in || !act_out) return fail(LFT_ERR_ARG, "null pointer");
    if (layer < 0 || layer >= kLayers) return fail(LFT_ERR_ARG, "layer %d out of range", layer);
    if (int rc = make_fwd(B, A, h, w, s, prec, stream, &c)) return rc;
    return by_prec(prec, [&](auto t) {
        using T = decltype(t);
        return ang_block<T>(c, packed, layer, static_cast<const T*>(act_in), static_cast<T*>(act_out));
    });
}

int lft_spa_block_fwd(const void* packed, int layer, const void* act_in, const void* skip, void* act_out, void* workspace, int B, int A,
                      int h, int w, int s, int prec, void* stream) {
    Fwd c;
    if (!packed || !act_in || !act_out || !workspace) return fail(LFT_ERR_ARG, "null pointer");
    if (layer < 0 || layer >= kLayers) return fail(LFT_ERR_ARG, "layer %d out of range", layer);
    if (int rc = make_fwd(B, A, h, w, s, prec, stream, &c)) return rc;
    return by_prec(prec, [&](auto t) {
        using T = decltype(t);
        return spa_block<T>(c, packed, layer, static_cast<const T*>(act_in), static_cast<const T*>(skip), static_cast<T*>(act_out), workspace);
    });
}

int lft_upsample_fwd(const void* packed, const void* act_in, const float* lr, float* out, void* workspace, int B, int A, int h, int w,
                     int s, int prec, void* stream) {
    Fwd c;
    if (!packed || !act_in || !lr || !out || !workspace) return fail(LFT_ERR_ARG, "null pointer");
    if (int rc = make_fwd(B, A, h, w, s, prec, stream, &c)) return rc;
    return by_prec(prec, [&](auto t) {
        using T = decltype(t);
        return upsample<T>(c, packed, static_cast<const T*>(act_in), lr, out, workspace);
    });
}

// Test-only (include/lft_hip_test.h): the tail of lft_forward -- SpaTrans of layer 3 with the global skip into the workspace's xb,
// then the up-sampler -- with the hand-off between the two chosen by the caller.
int lft_tail_fwd(const void* packed, const void* act_in, const void* skip, const float* lr, float* out, void* workspace,
                 int B, int A, int h, int w, int s, int prec, int handoff, void* stream) {
    Fwd c;
    if (!packed || !act_in || !skip || !lr || !out || !workspace) return fail(LFT_ERR_ARG, "null pointer");
    if (int rc = make_fwd(B, A, h, w, s, prec, stream, &c)) return rc;
    return by_prec(prec, [&](auto t) {
        using T = decltype(t);
        const bool lm = handoff != 0;
        if (lm && !tok_lane_major<T>(c.d))
            return fail(LFT_ERR_SHAPE, "lft_tail_fwd: views of %dx%d have no lane-major hand-off in this precision", c.d.h, c.d.w);
        T* xb = at<T>(workspace, c.W.xb);
        if (int r = spa_block<T>(c, packed, kLayers - 1, static_cast<const T*>(act_in), static_cast<const T*>(skip), xb, workspace, lm)) return r;
        return upsample<T>(c, packed, xb, lr, out, workspace, lm);
    });
}

#if defined(LFT_EXPERIMENT) && !defined(LFT_ISA_MARKS)
// Diagnostic build only (lft_experiment.cuh): copy the stamp buffer to the host (synchronises).
int lft_debug_read_stamps(unsigned long long* host_out, int n) {
    LFT_HIP_OK(hipDeviceSynchronize());
    LFT_HIP_OK(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_lft_stamps), sizeof(unsigned long long) * (size_t)n));
    return 0;
}
int lft_debug_clear_stamps(void) {
    static unsigned long long zeros[4096 * 32];
    LFT_HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(g_lft_stamps), zeros, sizeof(zeros)));
    return 0;
}
#endif

int lft_mfma_selftest(const float* Am, const float* Bm, const float* W2, float* C, float* D, int prec, void* stream) {
    if (!Am || !Bm || !W2 || !C || !D) return fail(LFT_ERR_ARG, "null pointer");
    if (prec != LFT_PREC_F32 && prec != LFT_PREC_BF16 && prec != LFT_PREC_F16) return fail(LFT_ERR_ARG, "bad prec %d", prec);
    by_prec(prec, [&](auto t) { k_selftest<decltype(t)><<<1, 64, 0, static_cast<hipStream_t>(stream)>>>(Am, Bm, W2, C, D); return 0; });
    LFT_LAUNCH_OK("k_selftest");
    return 0;
}


// ================================================================================ training (fp32)
int lft_train_tape_bytes(int B, int A, int h, int w, int s, size_t* out_bytes) {
    Dims d; int rc;
    if (!out_bytes) return fail(LFT_ERR_ARG, "out_bytes is null");
    if ((rc = make_dims(B, A, h, w, s, LFT_PREC_F32, &d))) return rc;
    const TrainLayout T = train_layout(d);
    if (T.rc) return T.rc;                                      // the sizing run of the backward pass failed: no tape size to report
    *out_bytes = T.total * sizeof(float);
    return 0;
}
int lft_train_grad_floats(int s, size_t* out_floats) {
    if (!out_floats) return fail(LFT_ERR_ARG, "out_floats is null");
    if (s != 2 && s != 4) return fail(LFT_ERR_SHAPE, "scale factor must be 2 or 4, got %d", s);
    *out_floats = (size_t)param_info(s).total;
    return 0;
}
int lft_train_tape_offset(const char* name, int B, int A, int h, int w, int s, size_t* out_float_offset) {
    Dims d; int rc;
    if (!name || !out_float_offset) return fail(LFT_ERR_ARG, "null pointer");
    if ((rc = make_dims(B, A, h, w, s, LFT_PREC_F32, &d))) return rc;
    const TrainLayout T = train_layout(d);
    if (T.rc) return T.rc;
    const std::string n(name);
    const bool layered = n.size() > 5 && n[3] >= '0' && n[3] < '0' + kLayers && n[4] == '.';      // "ang<l>.<field>", "spa<l>.<field>"
    const bool found = layered && n.compare(0, 3, "ang") == 0 ? tape_field(kTapeAng, T.ang[n[3] - '0'], n.substr(5), out_float_offset)
                     : layered && n.compare(0, 3, "spa") == 0 ? tape_field(kTapeSpa, T.spa[n[3] - '0'], n.substr(5), out_float_offset)
                                                              : tape_field(kTapeTop, T, n, out_float_offset);
    return found ? 0 : fail(LFT_ERR_ARG, "unknown tape field %s", name);
}
// The checks every training entry point shares, after its own null pointers: the parameter array, the shape, the math mode.
static int train_args(const float* const* params, int nparams, int B, int A, int h, int w, int s, int math, Dims* d) {
    if (nparams != LFT_NUM_PARAMS) return fail(LFT_ERR_ARG, "expected %d parameter tensors, got %d", LFT_NUM_PARAMS, nparams);
    for (int i = 0; i < nparams; ++i) if (!params[i]) return fail(LFT_ERR_ARG, "parameter %d is null", i);
    if (int rc = make_dims(B, A, h, w, s, LFT_PREC_F32, d)) return rc;
    if (math != LFT_MATH_F32 && math != LFT_MATH_BF16X3 && math != LFT_MATH_BF16X6) return fail(LFT_ERR_ARG, "math must be LFT_MATH_F32, LFT_MATH_BF16X3 or LFT_MATH_BF16X6, got %d", math);
    return 0;
}
int lft_train_forward(const float* const* params, int nparams, const float* lr, float* out, void* tape,
                      int B, int A, int h, int w, int s, int math, void* stream) {
    Dims d; int rc;
    if (!params || !lr || !out || !tape) return fail(LFT_ERR_ARG, "null pointer");
    if ((rc = train_args(params, nparams, B, A, h, w, s, math, &d))) return rc;
    return train_forward(params, lr, out, static_cast<float*>(tape), d, math, static_cast<hipStream_t>(stream));
}
int lft_train_backward(const float* const* params, int nparams, const float* lr, void* tape, const float* dout, float* grads,
                       int B, int A, int h, int w, int s, int math, void* stream) {
    Dims d; int rc;
    if (!params || !lr || !tape || !dout || !grads) return fail(LFT_ERR_ARG, "null pointer");
    if ((rc = train_args(params, nparams, B, A, h, w, s, math, &d))) return rc;
    return train_backward(params, lr, static_cast<float*>(tape), dout, grads, d, math, static_cast<hipStream_t>(stream));
}
int lft_train_backward_input(const float* const* params, int nparams, const float* lr, void* tape, const float* dout,
                             float* grads, float* d_lr, int B, int A, int h, int w, int s, int math, void* stream) {
    Dims d; int rc;
    if (!params || !lr || !tape || !dout || !grads || !d_lr) return fail(LFT_ERR_ARG, "null pointer");
    if ((rc = train_args(params, nparams, B, A, h, w, s, math, &d))) return rc;
    BwdRequest rq; rq.d_lr = d_lr;
    return train_backward(params, lr, static_cast<float*>(tape), dout, grads, d, math, static_cast<hipStream_t>(stream), rq);
}
int lft_lr_grad_bwd(const float* w0, const float* dx0, const float* dout, float* d_lr, int B, int A, int h, int w, int s, void* stream) {
    Dims d; int rc;
    if (!w0 || !dx0 || !d_lr) return fail(LFT_ERR_ARG, "null pointer");
    if ((rc = make_dims(B, A, h, w, s, LFT_PREC_F32, &d))) return rc;
    return lr_grad(d, w0, dx0, dout, d_lr, static_cast<hipStream_t>(stream));
}
int lft_train_backward_buckets(const float* const* params, int nparams, const float* lr, void* tape, const float* dout, float* grads,
                               int B, int A, int h, int w, int s, int math, void* stream,
                               lft_bucket_fn on_bucket, void* user) {
    Dims d; int rc;
    if (!params || !lr || !tape || !dout || !grads || !on_bucket) return fail(LFT_ERR_ARG, "null pointer");
    if ((rc = train_args(params, nparams, B, A, h, w, s, math, &d))) return rc;
    BwdRequest rq; rq.on_bucket = on_bucket; rq.user = user;
    return train_backward(params, lr, static_cast<float*>(tape), dout, grads, d, math, static_cast<hipStream_t>(stream), rq);
}
int lft_train_block_backward(const float* const* params, int nparams, const float* lr, void* tape, int block, int layer,
                             const float* d_out, float* d_in, float* grads,
                             int B, int A, int h, int w, int s, int math, void* stream) {
    Dims d; int rc;
    if (!params || !lr || !tape || !d_out || !grads) return fail(LFT_ERR_ARG, "null pointer");
    if (block < LFT_BLOCK_UPSAMPLE || block > LFT_BLOCK_INIT) return fail(LFT_ERR_ARG, "block must be LFT_BLOCK_UPSAMPLE .. LFT_BLOCK_INIT, got %d", block);
    if ((block == LFT_BLOCK_SPA || block == LFT_BLOCK_ANG) && (layer < 0 || layer >= kLayers)) return fail(LFT_ERR_ARG, "layer %d out of range", layer);
    if (block != LFT_BLOCK_INIT && !d_in) return fail(LFT_ERR_ARG, "d_in is null");
    if ((rc = train_args(params, nparams, B, A, h, w, s, math, &d))) return rc;
    const BlockSel sel{block, layer, d_out, d_in};
    BwdRequest rq; rq.sel = &sel;
    return train_backward(params, lr, static_cast<float*>(tape), block == LFT_BLOCK_UPSAMPLE ? d_out : nullptr, grads, d, math,
                          static_cast<hipStream_t>(stream), rq);
}
// Test-only (include/lft_hip_test.h): Prod<math> on one packed fragment, see k_prod_selftest.
int lft_prod_selftest(const float* W, const float* X, float* Y, float* Yl, float* Yr, int math, void* stream) {
    if (!W || !X || !Y || !Yl || !Yr) return fail(LFT_ERR_ARG, "null pointer");
    if (math != LFT_MATH_F32 && math != LFT_MATH_BF16X3 && math != LFT_MATH_BF16X6) return fail(LFT_ERR_ARG, "bad math %d", math);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int mm = math_mode(math);
    float* wp = nullptr;
    LFT_HIP_OK(hipMalloc(&wp, frag_floats(mm) * sizeof(float)));
    std::vector<PackOp> ops{lin_op(W, 0, 32, 16, 0, 1, 0, 1.0f)};
    int rc = mm ? run_pack_split(ops, wp, 1, st, mm) : run_pack<float>(ops, wp, 1, st);
    if (!rc) rc = dispatch<1, 2, 0>(mm, [&](auto MM) { k_prod_selftest<MM><<<1, 64, 0, st>>>(wp, X, Y, Yl, Yr); return 0; });
    const hipError_t e = hipStreamSynchronize(st);                    // the fragment is freed below
    (void)hipFree(wp);
    if (rc) return rc;
    if (e != hipSuccess) return fail((int)e, "k_prod_selftest: %s", hipGetErrorString(e));
    return 0;
}
// ---- attention maps from the tape (lft_attn_maps.cuh) ----
static int attn_maps_args(int block, int heads_mode) {
    if (block != LFT_BLOCK_ANG && block != LFT_BLOCK_SPA) return fail(LFT_ERR_ARG, "block must be LFT_BLOCK_ANG or LFT_BLOCK_SPA, got %d", block);
    if (heads_mode != LFT_MAPS_MEAN && heads_mode != LFT_MAPS_HEADS) return fail(LFT_ERR_ARG, "heads_mode must be LFT_MAPS_MEAN or LFT_MAPS_HEADS, got %d", heads_mode);
    return 0;
}
static size_t attn_maps_count(const Dims& d, int block, int heads_mode) {
    const size_t H = heads_mode == LFT_MAPS_HEADS ? 8 : 1;
    return block == LFT_BLOCK_ANG ? (size_t)d.B * d.hw * H * d.V * d.V : (size_t)d.ntok * H * 25;
}
int lft_attn_maps_floats(int block, int heads_mode, int B, int A, int h, int w, size_t* out_floats) {
    Dims d; int rc;
    if (!out_floats) return fail(LFT_ERR_ARG, "out_floats is null");
    if ((rc = attn_maps_args(block, heads_mode))) return rc;
    if ((rc = make_dims(B, A, h, w, 2, LFT_PREC_F32, &d))) return rc;      // the maps do not depend on the scale factor
    *out_floats = attn_maps_count(d, block, heads_mode);
    return 0;
}
int lft_train_attn_maps(const void* tape, int block, int layer, int heads_mode, float* maps, int B, int A, int h, int w, int s, void* stream) {
    Dims d; int rc;
    if (!tape || !maps) return fail(LFT_ERR_ARG, "null pointer");
    if ((rc = attn_maps_args(block, heads_mode))) return rc;
    if (layer < 0 || layer >= kLayers) return fail(LFT_ERR_ARG, "layer %d out of range", layer);
    if ((rc = make_dims(B, A, h, w, s, LFT_PREC_F32, &d))) return rc;
    const TrainLayout T = train_layout(d);
    if (T.rc) return T.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float* tp = static_cast<const float*>(tape);
    const bool mean = heads_mode == LFT_MAPS_MEAN;
    if (block == LFT_BLOCK_ANG) {
        const size_t lds = ang_maps_lds(d.V);
        const unsigned npix = (unsigned)(d.B * d.hw);
        return dispatch<true, false>(mean, [&](auto MEAN) {
            if (int r = allow_lds(k_ang_maps<MEAN>, lds, "k_ang_maps")) return r;
            k_ang_maps<MEAN><<<npix, kAmThreads, lds, st>>>(tp + T.ang[layer].qk, maps, d.V, d.hw);
            LFT_LAUNCH_OK("k_ang_maps");
            return 0;
        });
    }
    const unsigned tiles = (unsigned)(((d.w + kWaTX - 1) / kWaTX) * ((d.h + kWaTY - 1) / kWaTY) * d.B * d.V);
    return dispatch<true, false>(mean, [&](auto MEAN) {
        k_win_maps<MEAN><<<dim3(tiles, MEAN ? 1 : 4), 256, 0, st>>>(tp + T.spa[layer].qk, maps, d.h, d.w);
        LFT_LAUNCH_OK("k_win_maps");
        return 0;
    });
}
int lft_train_step_profiled(const float* const* params, int nparams, const float* lr, float* out, void* tape, const float* dout, float* grads,
                            int B, int A, int h, int w, int s, int math, void* stream, int max_records, float* ms_out, const char** names_out, int* n_out) {
    Dims d; int rc;
    if (!params || !lr || !out || !tape || !dout || !grads || !ms_out || !names_out || !n_out) return fail(LFT_ERR_ARG, "null pointer");
    if ((rc = train_args(params, nparams, B, A, h, w, s, math, &d))) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return run_profiled(st, max_records, ms_out, names_out, n_out, [&] {     // one stream: every kernel between two events
        int r = train_forward(params, lr, out, static_cast<float*>(tape), d, math, st);
        return r ? r : train_backward(params, lr, static_cast<float*>(tape), dout, grads, d, math, st);
    });
}
int lft_train_grad_bucket(int s, int bucket, size_t* first_float, size_t* n_floats) {
    if (!first_float || !n_floats) return fail(LFT_ERR_ARG, "null pointer");
    if (s != 2 && s != 4) return fail(LFT_ERR_SHAPE, "scale factor must be 2 or 4, got %d", s);
    if (bucket < 0 || bucket >= LFT_GRAD_BUCKETS) return fail(LFT_ERR_ARG, "bucket %d out of range (0..%d)", bucket, LFT_GRAD_BUCKETS - 1);
    grad_bucket_range(s, bucket, first_float, n_floats);
    return 0;
}


}  // extern "C"
