// lft_api.hip -- C ABI of liblft_hip.so (see include/lft_hip.h): buffer layouts, weight packing plan,
// kernel launches.  Host-side code only enqueues work on the caller's stream.
//
// The library is built from this file as TWO translation units, only so that they compile in parallel; both get the same
// compiler flags (COMMON_FLAGS + UNIT_FLAGS of lft_amd/_lib.py, where each flag's reason is written down):
//   LFT_TU == 1   inference, scene tiling, metrics, data preparation, colour, refocus, disparity, debug entry points
//   LFT_TU == 2   the fp32 training step, its losses and optimizer
//   LFT_TU == 0   everything in one unit (tools, resource reports).
// Every kernel and helper is local to its unit (anonymous namespace); the units share only the error buffer.
#include "../../include/lft_hip.h"
#include "../../include/lft_hip_test.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdarg>
#include <cstdio>
#include <cmath>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>

#ifndef LFT_TU
#define LFT_TU 0
#endif

namespace {
#include "lft_kernels_a.cuh"
#include "lft_kernels_b.cuh"
#include "lft_metrics.cuh"
#include "lft_prepare.cuh"    // data preparation (reference Generate_Data_for_*.m)
#include "lft_train.cuh"     // training kernels; the fp32 inference path shares their LDS-tiled window attention
#if LFT_TU != 1
#include "lft_attn_maps.cuh" // attention weights from the tape's Q | K (lft_train_attn_maps)
#include "lft_optim.cuh"     // guarded Adam step: gradient statistics, skip / clip decision, update (lft_adam_step_guarded)
#include "lft_loss.cuh"      // pixel + EPI-gradient loss with L1 / MSE / Charbonnier penalty (lft_lf_loss)
#include "lft_ssim_loss.cuh" // structural term 1 - SSIM and its gradient, fp64 inside (lft_ssim_loss)
#endif
#if LFT_TU != 2
#include "lft_ensemble.cuh"  // dihedral transforms: self-ensemble expand / merge / fused scene integrate, per-sample augmentation
#include "lft_colour.cuh"    // colour path: RGB light field -> Y mosaic; SR Y + up-scaled chroma -> RGB views
#include "lft_refocus.cuh"   // synthetic refocus: focal stack by shift-and-add over the views (lft_refocus)
#include "lft_disparity.cuh" // disparity: plane-sweep cost volume, windowed aggregation, winner-take-all (lft_disparity)
#endif
}  // namespace

#if LFT_TU == 2
extern thread_local char lft_g_err[512];
#else
__attribute__((visibility("hidden"))) thread_local char lft_g_err[512] = "";
#endif
#define g_err lft_g_err

namespace {

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define LFT_HIP_OK(expr)                                                                     \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return fail((int)e_, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)
// Optional per-kernel timing (lft_forward_profiled): an event is recorded on the launch stream after each kernel.
struct Profiler {
    bool on = false;
    hipStream_t st = nullptr;
    std::vector<hipEvent_t> ev;
    std::vector<const char*> names;
};
thread_local Profiler g_prof;
// Launch name with the call's shape appended ("k_lin:128>256", profiled runs only); interned, so the pointer stays valid.
inline const char* prof_name(const char* plain, const char* fmt, ...) {
    if (!g_prof.on) return plain;
    static thread_local std::set<std::string> names;
    char buf[96];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return names.insert(buf).first->c_str();
}
inline void prof_mark(const char* name) {
    if (!g_prof.on) return;
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, g_prof.st);
    g_prof.ev.push_back(e);
    g_prof.names.push_back(name);
}

#define LFT_LAUNCH_OK(name)                                                                  \
    do {                                                                                     \
        hipError_t e_ = hipGetLastError();                                                   \
        if (e_ != hipSuccess) return fail((int)e_, "launch %s: %s", name, hipGetErrorString(e_)); \
        prof_mark(name);                                                                     \
    } while (0)
// run() with an event recorded on st after every kernel it launches, then synchronised: the first max_records launches' names
// and times go to names_out / ms_out, their number to *n_out.  run()'s error comes first, then the synchronisation's.
template <typename Run> int run_profiled(hipStream_t st, int max_records, float* ms_out, const char** names_out, int* n_out, Run&& run) {
    g_prof.on = true; g_prof.st = st; g_prof.ev.clear(); g_prof.names.clear();
    prof_mark("start");
    const int rc = run();
    g_prof.on = false;
    hipError_t e = hipStreamSynchronize(st);
    int n = 0;
    for (size_t i = 1; i < g_prof.ev.size() && n < max_records; ++i, ++n) {
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, g_prof.ev[i - 1], g_prof.ev[i]);
        ms_out[n] = ms;
        names_out[n] = g_prof.names[i];
    }
    for (hipEvent_t ev : g_prof.ev) (void)hipEventDestroy(ev);
    g_prof.ev.clear(); g_prof.names.clear();
    *n_out = n;
    if (rc) return rc;
    if (e != hipSuccess) return fail((int)e, "hipStreamSynchronize: %s", hipGetErrorString(e));
    return 0;
}

constexpr int kLayers = 4;   // reference LFT.py:15

// Compile-time dispatch: f(std::integral_constant<decltype(V), V>{}) for the V of Vs that equals the runtime value v, so that a
// generic lambda can name the kernel variant, e.g. dispatch<true, false>(lm, [&](auto LM) { k<T, LM><<<...>>>(...); return 0; }).
// Vs lists every value a caller passes; any other is an internal error.
template <auto... Vs, typename V, typename F> int dispatch(V v, F&& f) {
    int rc = 0;
    if (((v == Vs && ((rc = f(std::integral_constant<decltype(Vs), Vs>{})), true)) || ...)) return rc;
    return fail(LFT_ERR_ARG, "internal: no kernel variant for %d", (int)v);
}
template <int V> using int_c = std::integral_constant<int, V>;
// f(T{}) with T the element type of precision `prec` (validated by make_dims beforehand).
template <typename F> int by_prec(int prec, F&& f) {
    if (prec == LFT_PREC_F32) return f(float{});
    if (prec == LFT_PREC_BF16) return f(bf16_t{});
    return f(f16_t{});
}
// f(T{}) with T the stored type of a light field of class `lf_class` (validated by the caller beforehand).  F64 = false: the caller
// accepts LFT_LF_UINT8 and LFT_LF_FLOAT32 only, and no double variant of its kernel is built.
template <bool F64 = true, typename F> int by_lf_class(int lf_class, F&& f) {
    if (lf_class == LFT_LF_UINT8) return f(uint8_t{});
    if constexpr (!F64) return f(float{});
    else return lf_class == LFT_LF_FLOAT32 ? f(float{}) : f(double{});
}
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Dims {
    int B, A, V, h, w, hw, s, gp, gt, nchunk;
    long long ntok;
};

int make_dims(int B, int A, int h, int w, int s, int prec, Dims* d) {
    if (prec != LFT_PREC_F32 && prec != LFT_PREC_BF16 && prec != LFT_PREC_F16)
        return fail(LFT_ERR_ARG, "prec must be LFT_PREC_F32, LFT_PREC_BF16 or LFT_PREC_F16, got %d", prec);
    if (B < 1 || A < 1 || h < 1 || w < 1) return fail(LFT_ERR_SHAPE, "B, A, h, w must be positive (B=%d A=%d h=%d w=%d)", B, A, h, w);
    if (s != 2 && s != 4) return fail(LFT_ERR_SHAPE, "scale factor must be 2 or 4, got %d", s);
    if (A * A > 128) return fail(LFT_ERR_UNSUPPORTED, "angRes %d (A*A=%d views > 128) is not implemented in this build", A, A * A);
    if ((long long)B * A * A * h * w > (1LL << 27)) return fail(LFT_ERR_SHAPE, "too many tokens");
    d->B = B; d->A = A; d->V = A * A; d->h = h; d->w = w; d->hw = h * w; d->s = s;
    d->gp = (s + 2) * (s + 2); d->gt = (d->gp + 31) / 32; d->nchunk = 2 * s * s;
    d->ntok = (long long)B * d->V * d->hw;
    return 0;
}

// Fragment counts per stream
constexpr int kFragsConv = 72, kFragsAng = 64, kFragsSpa1 = 240, kFragsSpa1NoQ = 208, kFragsSpa2 = 176;
// 16-bit part B (k_spa_b) runs the 1x1x1 conv folded into the FFN's second Linear: kSpaBFrags fragments (lft_kernels_b.cuh)
inline int frags_spa2(int prec) { return prec == LFT_PREC_F32 ? kFragsSpa2 : kSpaBFrags; }
inline int frags_up(const Dims& d) { return d.nchunk * (4 + 2 * d.gt); }

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
    for (int l = 0; l < kLayers; ++l) L.petok[l] = take((size_t)((d.hw + 32 * kNwSpa1 - 1) / (32 * kNwSpa1)) * kNwSpa1 * 4096 * esz);   // lane-major, per 32-token tile
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

// Dynamic LDS sizes (bytes) and the opt-in above the 64 KiB default (a workgroup may use all 160 KiB of a CU).
template <typename T> size_t lds_conv64(int w) { return WRing<T, kConv64Chunk, kNwConv>::LDS_BYTES + ConvIn<T, kNwConv>::bytes(w) + kNwConv * TileIO<2, T>::BYTES + kConvZeroRow; }
// The 16-bit front end: k_conv64_lr adds the staged LR pixels, k_conv64<T, 2> conv_init0's weights; one size serves both
template <typename T> size_t lds_conv64_lr(int w) { return lds_conv64<T>(w) + std::max<size_t>(LrStage<kNwConv>::bytes(w), kConv0WBytes); }
constexpr size_t kLdsParams = 1024;   // 256 LayerNorm floats
template <typename T, int CH = kSpaChunk> size_t lds_spa1(int w) {      // the tile I/O scratch aliases the conv input tile, which must be large enough for it
    return WRing<T, CH, kNwSpa1>::LDS_BYTES + std::max<size_t>(ConvIn<T, kNwSpa1>::bytes(w), (size_t)kNwSpa1 * TileIO<4, T>::BYTES) + kLdsParams + kConvZeroRow;
}
template <typename T> size_t lds_spa2() { return WRing<T, kSpaChunk, kNwSpa2>::LDS_BYTES + kLdsParams + kNwSpa2 * TileIO<4, T>::BYTES; }
template <typename T> size_t lds_up() { return WRing<T, kUpChunk, kNwUp>::LDS_BYTES + kNwUp * TileIO<2, T>::BYTES; }
template <typename T> size_t lds_ang() { return (size_t)kFragsAng * 1024 * FragInfo<T>::PIECES + kLdsParams + 4 * TileIO<2, T>::BYTES; }
constexpr size_t kMaxLds = 160 * 1024;
template <typename K> int allow_lds(K kernel, size_t bytes, const char* name) {
    if (bytes > kMaxLds) return fail(LFT_ERR_SHAPE, "%s needs %zu B of LDS (> 160 KiB): view width too large for this build", name, bytes);
    if (bytes <= 64 * 1024) return 0;
    // The attribute is sticky per kernel: set it once per (kernel, size) so that steady-state forwards -- and a
    // stream capture of them -- consist of kernel launches only.
    // The attribute belongs to the (device, kernel) pair: a thread that drives two GPUs must set it on each.
    struct Done { int dev; const void* fn; size_t bytes; };
    static thread_local std::vector<Done> done;
    const void* fn = reinterpret_cast<const void*>(kernel);
    int dev = 0;
    LFT_HIP_OK(hipGetDevice(&dev));
    for (const auto& d : done)
        if (d.dev == dev && d.fn == fn && d.bytes >= bytes) return 0;
    LFT_HIP_OK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done.push_back(Done{dev, fn, bytes});
    return 0;
}

template <typename P> P* at(const void* base, size_t off) { return reinterpret_cast<P*>(const_cast<char*>(static_cast<const char*>(base)) + off); }
inline unsigned blocks_for(long long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

// ---------------------------------------------------------------------------- packing plan
PackOp lin_op(const float* src, int row0, int nrows, int ld, int k0, int ksteps, int kmap, float scale, int kmul = 1, int kadd = 0) {
    PackOp p{};
    p.src = src; p.kind = 0; p.row0 = row0; p.nrows = nrows; p.ntiles = (nrows + 31) / 32; p.ld = ld;
    p.kmul = kmul; p.kadd = kadd; p.k0 = k0; p.ksteps = ksteps; p.kmap = kmap; p.scale = scale; p.s = 0; p.frag0 = 0;
    return p;
}
void conv_ops(std::vector<PackOp>& v, const float* w, int nout) {   // [nout][64][3][3] == [nout][576], k index c*9 + tap
    for (int tap = 0; tap < 9; ++tap)
        for (int ks = 0; ks < 4; ++ks) v.push_back(lin_op(w, 0, nout, 576, 16 * ks, 1, 0, 1.0f, 9, tap));
}

// The packing plan, LFT_PACK_MAXOPS operations per launch: launch(a, nf, total) enqueues the kernel `name` for the nf fragments of
// batch a, which follow the `total` fragments of the batches before it.
template <typename Launch>
int pack_batches(std::vector<PackOp>& ops, int expect_frags, const char* name, Launch&& launch) {
    int total = 0;
    size_t i = 0;
    while (i < ops.size()) {
        PackArgs a{};
        int nf = 0;
        while (i < ops.size() && a.nops < LFT_PACK_MAXOPS) {
            a.op[a.nops] = ops[i];
            a.op[a.nops].frag0 = nf;
            nf += ops[i].ntiles * ops[i].ksteps;
            ++a.nops; ++i;
        }
        if (int rc = launch(a, nf, total)) return rc;
        LFT_LAUNCH_OK(name);
        total += nf;
    }
    if (total != expect_frags) return fail(LFT_ERR_ARG, "internal: stream has %d fragments, expected %d", total, expect_frags);
    return 0;
}
template <typename T>
int run_pack(std::vector<PackOp>& ops, T* dst, int expect_frags, hipStream_t st) {
    return pack_batches(ops, expect_frags, "k_pack", [&](const PackArgs& a, int nf, int total) {
        k_pack<T><<<nf, 64, 0, st>>>(a, dst + (size_t)total * 512);
        return 0;
    });
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
        if ((rc = launch_spa1<T, true>((unsigned)((d.hw + 32 * kNwSpa1 - 1) / (32 * kNwSpa1)), at<T>(packed, c.L.spa_pe_img), at<T>(packed, c.L.s_spa1[l]), nullptr, nullptr,
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

void launch_assemble(const float* lr, const float* g, float* out, int B, int A, int h, int w, int s, hipStream_t st, int gld = 0, unsigned* status = nullptr) {
    const dim3 tg((unsigned)((A * w + 7) / 8) * (unsigned)((A * h + 7) / 8) * (unsigned)B);    // 8 x 8 LR mosaic pixels per workgroup; tile order: k_assemble_t
    if (!gld) gld = (s + 2) * (s + 2);
    if (s == 2) k_assemble_t<2><<<tg, 256, 0, st>>>(lr, g, out, B, A, h, w, gld, status);
    else k_assemble_t<4><<<tg, 256, 0, st>>>(lr, g, out, B, A, h, w, gld, status);
}

// ---------------------------------------------------------------------------- stages
// The front end as it was before the composition, and as fp32 still runs it: conv_init0 to memory, three 64 -> 64 convs.
template <typename T>
int init_features_x0(const Fwd& c, const void* packed, const float* lr, T* x0, T* ta, T* tb, T* feat) {
    const Dims& d = c.d;
    const hipStream_t st = c.st;
    const int nimg = d.B * d.V, nwg = nimg * ((d.hw + 32 * kNwConv - 1) / (32 * kNwConv));
    const size_t lds = lds_conv64<T>(d.w);
    int rc;
    if ((rc = allow_lds(k_conv64<T, 0>, lds, "k_conv64"))) return rc;
    if ((rc = allow_lds(k_conv64<T, 1>, lds, "k_conv64"))) return rc;
    k_conv0<T><<<dim3((unsigned)((d.hw + kConv0Tok - 1) / kConv0Tok), (unsigned)nimg), 256, 0, st>>>(lr, at<float>(packed, c.L.conv0_w), x0, d.B, d.A, d.h, d.w);
    LFT_LAUNCH_OK("k_conv0");
    k_conv64<T, 0><<<nwg, 64 * kNwConv, lds, st>>>(x0, ta, nullptr, at<T>(packed, c.L.s_conv[0]), nimg, d.h, d.w, ConvLr{});
    LFT_LAUNCH_OK("k_conv64");
    k_conv64<T, 0><<<nwg, 64 * kNwConv, lds, st>>>(ta, tb, nullptr, at<T>(packed, c.L.s_conv[1]), nimg, d.h, d.w, ConvLr{});
    LFT_LAUNCH_OK("k_conv64");
    k_conv64<T, 1><<<nwg, 64 * kNwConv, lds, st>>>(tb, feat, x0, at<T>(packed, c.L.s_conv[2]), nimg, d.h, d.w, ConvLr{});
    LFT_LAUNCH_OK("k_conv64");
    return 0;
}
// 16-bit: two launches.  conv_init0 is composed into conv_init.0 (k_conv64_lr: LR mosaic -> tb) and recomputed for the
// residual of conv_init.4 (k_conv64<T, 2>); x0 and ta are never written.  Both launches carry the name "k_conv64": the
// benchmark's per-kernel tables are indexed by the names lft_forward_profiled returns.
template <typename T>
int init_features(const Fwd& c, const void* packed, const float* lr, T* x0, T* ta, T* tb, T* feat) {
    if constexpr (sizeof(T) == 4) return init_features_x0<T>(c, packed, lr, x0, ta, tb, feat);
    else {
        const Dims& d = c.d;
        const hipStream_t st = c.st;
        const int nimg = d.B * d.V, nwg = nimg * ((d.hw + 32 * kNwConv - 1) / (32 * kNwConv));
        const size_t lds = lds_conv64_lr<T>(d.w);
        int rc;
        if (c.L.s_w01 + kW01Frags * 1024 != c.L.s_conv[1]) return fail(LFT_ERR_ARG, "internal: W01 fragments are not in front of conv_init.2's stream");
        if ((rc = allow_lds(k_conv64_lr<T>, lds, "k_conv64"))) return rc;
        if ((rc = allow_lds(k_conv64<T, 2>, lds, "k_conv64"))) return rc;
        k_conv64_lr<T><<<nwg, 64 * kNwConv, lds, st>>>(lr, tb, at<T>(packed, c.L.s_w01), d.A, nimg, d.h, d.w);
        LFT_LAUNCH_OK("k_conv64");
        k_conv64<T, 2><<<nwg, 64 * kNwConv, lds, st>>>(tb, feat, nullptr, at<T>(packed, c.L.s_conv[2]), nimg, d.h, d.w,
                                                      ConvLr{lr, at<float>(packed, c.L.conv0_w), d.A});
        LFT_LAUNCH_OK("k_conv64");
        return 0;
    }
}
template <typename T, int CT, int LL>      // LL: score registers of the last key tile that can hold a view, which covers rows acc_row(i, 0) and acc_row(i, 1) = +4 of register i
int ang_multi(const Fwd& c, const void* packed, int l, const T* in, T* out, unsigned* status) {
    const Dims& d = c.d;
    constexpr bool WLDS = sizeof(T) == 2;                                   // fp32 weights (128 KiB) stay in L2
    constexpr int NG = (sizeof(T) == 2 && CT <= 3) ? 2 : 1;                 // positions per workgroup (they share the LDS weights)
    constexpr size_t FB = 1024 * FragInfo<T>::PIECES;
    const size_t lds = (WLDS ? 64 * FB : 0) + 1024 + (size_t)NG * CT * 8 * FB + (size_t)NG * CT * TileIO<2, T>::BYTES;
    const int npix = d.B * d.hw;
    int rc;
    const unsigned grid = std::min<unsigned>(blocks_for(npix, NG), 256u * (unsigned)std::max<size_t>(1, kMaxLds / lds));
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
    const unsigned grid = std::min<unsigned>(blocks_for(npix, 4), 256u * (unsigned)std::max<size_t>(1, kMaxLds / lds));
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
    const int nimg = d.B * d.V, nwg = nimg * ((d.hw + 32 * kNwSpa1 - 1) / (32 * kNwSpa1));
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
            const int nimg = d.B * d.V, nwg = nimg * ((d.hw + 32 * kNwConv - 1) / (32 * kNwConv));
            const size_t lds = lds_conv64<T>(d.w);
            int rc;
            if ((rc = allow_lds(k_conv64<T, 0>, lds, "k_conv64"))) return rc;
            // input: xb, which every forward writes (the 16-bit front end no longer writes x0); output: x0, which nothing reads
            k_conv64<T, 0><<<nwg, 64 * kNwConv, lds, st>>>(xb, x0, nullptr, at<T>(packed, c.L.s_conv[0]), nimg, d.h, d.w, ConvLr{});
            LFT_LAUNCH_OK("k_conv64");
            return 0;
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
#include "lft_train_host.cuh"

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

#if LFT_TU != 2
// ---- the light field [U,V,H,W,C] with five strides (data preparation, colour path); nothing is launched when a check fails ----
// The array itself: pointers, stored class, sizes, strides.  `shape` is the code of a bad size: lft_lf_prepare has always answered
// LFT_ERR_ARG there, the colour path LFT_ERR_SHAPE.
int lf_array_ok(const char* who, int shape, const void* lf, int lf_class, int U, int V, int H, int W, int C, const long long* strides) {
    if (!lf || !strides) return fail(LFT_ERR_ARG, "%s: null pointer", who);
    if (lf_class != LFT_LF_UINT8 && lf_class != LFT_LF_FLOAT32 && lf_class != LFT_LF_FLOAT64)
        return fail(LFT_ERR_ARG, "%s: light-field class must be LFT_LF_UINT8, LFT_LF_FLOAT32 or LFT_LF_FLOAT64, got %d", who, lf_class);
    if (U < 1 || V < 1 || H < 1 || W < 1 || C < 3)
        return fail(shape, "%s: light field [%d,%d,%d,%d,%d] needs positive sizes and at least 3 channels", who, U, V, H, W, C);
    for (int i = 0; i < 5; ++i)
        if (strides[i] < 0) return fail(LFT_ERR_ARG, "%s: stride %d is negative (%lld)", who, i, strides[i]);
    return 0;
}
// Its centre A x A views.  `index`: what the message calls the centre-view index ("the scripts' centre-view index" for
// lft_lf_prepare, which follows the MATLAB scripts).  A separate step because lft_lf_prepare checks its scale factor in between.
int centre_views_ok(const char* who, int shape, const char* index, int U, int V, int A) {
    if (A < 1 || A > U || A > V) return fail(shape, "%s: angRes %d outside the %d x %d views", who, A, U, V);
    if ((U - A) % 2 || (V - A) % 2)
        return fail(shape, "%s: U-A = %d and V-A = %d must be even (%s 0.5*(U-A+2) is not an integer)", who, U - A, V - A, index);
    return 0;
}
// what lft_lf_luma and lft_colour_merge ask of the light field: both of the above, and a grid with one y block per view
int colour_lf_ok(const char* who, const void* lf, int lf_class, int U, int V, int H, int W, int C, const long long* strides, int A) {
    if (int rc = lf_array_ok(who, LFT_ERR_SHAPE, lf, lf_class, U, V, H, W, C, strides)) return rc;
    if (int rc = centre_views_ok(who, LFT_ERR_SHAPE, "the centre-view index", U, V, A)) return rc;
    if (A > 255) return fail(LFT_ERR_SHAPE, "%s: angRes %d needs more than 65535 blocks in the grid's y", who, A);
    return 0;
}
// ---- B light fields [B,A,A,H,W,C] read in place through six strides, one 32 x 32 output tile per workgroup (refocus, disparity) ----
struct WindowedLf {         // the arguments lft_refocus and lft_disparity share, and what windowed_lf_ok derives from them
    const void* lf; int lf_class, B, A, H, W, C; const long long* strides; const void* table; int D, taps;
    long long tiles_x, tiles;           // kRfTile tiles of a view; tiles == 0: an empty shape, no work and no error
};
int too_many_blocks(const char* who, const WindowedLf& l, const char* work) {
    return fail(LFT_ERR_SHAPE, "%s: %d %s of %d slopes over views of %d x %d need more than 2^31 blocks", who, l.B, work, l.D, l.H, l.W);
}
// Every check the two entry points share, in the order they have always made them; nothing is launched when one fails.  The caller's
// own arguments sit in between: `out_class` (called `out_name` in the message), `radius` (lft_disparity only; 0 for lft_refocus),
// `own_null` (one of the caller's other pointers is null).  `work`: what too_many_blocks calls the B batches.
int windowed_lf_ok(const char* who, WindowedLf& l, int out_class, const char* out_name, int radius, bool own_null, const char* work) {
    if (l.lf_class != LFT_LF_UINT8 && l.lf_class != LFT_LF_FLOAT32)
        return fail(LFT_ERR_ARG, "%s: light-field class must be LFT_LF_UINT8 or LFT_LF_FLOAT32, got %d", who, l.lf_class);
    if (out_class != LFT_LF_UINT8 && out_class != LFT_LF_FLOAT32)
        return fail(LFT_ERR_ARG, "%s: %s class must be LFT_LF_UINT8 or LFT_LF_FLOAT32, got %d", who, out_name, out_class);
    if (l.A < 1 || l.A > 4096) return fail(LFT_ERR_ARG, "%s: angRes %d outside 1 .. 4096", who, l.A);      // A*A records indexed in int
    if (l.C < 1 || l.C > 4) return fail(LFT_ERR_ARG, "%s: %d channels (1 .. 4)", who, l.C);
    if (l.taps != 1 && l.taps != 2 && l.taps != 4) return fail(LFT_ERR_ARG, "%s: %d taps (1, 2 or 4)", who, l.taps);
    if (l.D < 1) return fail(LFT_ERR_ARG, "%s: %d slopes", who, l.D);
    if (radius < 0 || radius > kDpMaxR) return fail(LFT_ERR_ARG, "%s: radius %d outside 0 .. %d", who, radius, kDpMaxR);
    if (l.B < 0 || l.H < 0 || l.W < 0) return fail(LFT_ERR_SHAPE, "%s: negative size in B = %d, views of %d x %d", who, l.B, l.H, l.W);
    l.tiles_x = l.tiles = 0;
    if (l.B == 0 || l.H == 0 || l.W == 0) return 0;                 // nothing to read or write
    if (!l.lf || !l.strides || !l.table || own_null) return fail(LFT_ERR_ARG, "%s: null pointer", who);
    for (int i = 0; i < 6; ++i)
        if (l.strides[i] < 0) return fail(LFT_ERR_ARG, "%s: stride %d is negative (%lld)", who, i, l.strides[i]);
    if ((double)(l.H - 1) * (double)l.strides[3] + (double)(l.W - 1) * (double)l.strides[4] + (double)(l.C - 1) * (double)l.strides[5] > 2147483647.0)
        return fail(LFT_ERR_SHAPE, "%s: a view of %d x %d x %d with these strides spans more than 2^31 elements", who, l.H, l.W, l.C);
    l.tiles_x = ((long long)l.W + kRfTile - 1) / kRfTile;
    l.tiles = l.tiles_x * (((long long)l.H + kRfTile - 1) / kRfTile);
    if (l.tiles * l.D * l.B > 0x7fffffffLL) return too_many_blocks(who, l, work);
    return 0;
}
// the members RefocusArgs and SweepArgs have in common
template <typename Args> void fill_windowed(Args& a, const WindowedLf& l) {
    a.lf = l.lf;
    for (int i = 0; i < 3; ++i) a.st[i] = l.strides[i];
    a.sy = (int)l.strides[3]; a.sx = (int)l.strides[4]; a.sc = (int)l.strides[5];
    a.A = l.A; a.H = l.H; a.W = l.W; a.D = l.D; a.tiles_x = (int)l.tiles_x; a.tiles = (int)l.tiles;
    a.table = static_cast<const int*>(l.table);
}
#endif

}  // namespace

// ================================================================================ C ABI
extern "C" {

#if LFT_TU != 2
int lft_version(void) { return LFT_ABI_VERSION; }
const char* lft_last_error(void) { return g_err; }

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
        const float* w0 = at<float>(packed, c.L.conv0_w);
        if constexpr (sizeof(T) == 2) {
            if (recomputed) {
                k_conv0_recomputed<T><<<nimg * ((d.hw + 32 * kNwConv - 1) / (32 * kNwConv)), 64 * kNwConv, 0, c.st>>>(static_cast<T*>(x0_out), nimg, d.h, d.w, ConvLr{lr, w0, d.A});
                LFT_LAUNCH_OK("k_conv0_recomputed");
                return 0;
            }
        }
        k_conv0<T><<<dim3((unsigned)((d.hw + kConv0Tok - 1) / kConv0Tok), (unsigned)nimg), 256, 0, c.st>>>(lr, w0, static_cast<T*>(x0_out), d.B, d.A, d.h, d.w);
        LFT_LAUNCH_OK("k_conv0");
        return 0;
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

static int scene_counts(int h0, int w0, int patch, int stride, int* nu, int* nv) {
    if (h0 < 1 || w0 < 1 || patch < 1 || stride < 1 || stride > patch) return fail(LFT_ERR_SHAPE, "bad scene tiling (h0=%d w0=%d patch=%d stride=%d)", h0, w0, patch, stride);
    const int bdr = (patch - stride) / 2, h = h0 + 2 * bdr, w = w0 + 2 * bdr;
    if (h < patch || w < patch) return fail(LFT_ERR_SHAPE, "view %dx%d is smaller than one patch after extension", h0, w0);
    *nu = (h - patch) / stride + ((h - patch) % stride ? 2 : 1);
    *nv = (w - patch) / stride + ((w - patch) % stride ? 2 : 1);
    return 0;
}
int lft_scene_counts(int h0, int w0, int patch, int stride, int* num_u, int* num_v) {
    if (!num_u || !num_v) return fail(LFT_ERR_ARG, "null pointer");
    return scene_counts(h0, w0, patch, stride, num_u, num_v);
}
int lft_scene_divide(const float* scene, float* patches, int A, int h0, int w0, int patch, int stride, void* stream) {
    int nu, nv, rc;
    if (!scene || !patches || A < 1) return fail(LFT_ERR_ARG, "bad argument");
    if ((rc = scene_counts(h0, w0, patch, stride, &nu, &nv))) return rc;
    const dim3 grid((unsigned)((A * patch + 255) / 256), (unsigned)(A * patch), (unsigned)(nu * nv));
    k_scene_divide<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(scene, patches, A, h0, w0, patch, stride, nv);
    LFT_LAUNCH_OK("k_scene_divide");
    return 0;
}
int lft_scene_integrate(const float* sr_patches, float* sr_scene, int A, int h0, int w0, int patch, int stride, int s, void* stream) {
    int nu, nv, rc;
    if (!sr_patches || !sr_scene || A < 1 || s < 1) return fail(LFT_ERR_ARG, "bad argument");
    if ((rc = scene_counts(h0, w0, patch, stride, &nu, &nv))) return rc;
    const dim3 grid((unsigned)((A * w0 * s + 255) / 256), (unsigned)(A * h0 * s));
    k_scene_integrate<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(sr_patches, sr_scene, A, patch * s, stride * s, h0 * s, w0 * s, nv);
    LFT_LAUNCH_OK("k_scene_integrate");
    return 0;
}

// ---- dihedral transforms (lft_ensemble.cuh) ----
static int dihedral_args(const void* in, const void* out, unsigned mask, int B, int H, int W, int* E, unsigned* blocks) {
    if (!in || !out) return fail(LFT_ERR_ARG, "null pointer");
    if (in == out) return fail(LFT_ERR_ARG, "the transforms do not work in place (in == out)");
    if (mask == 0 || mask > 0xFFu) return fail(LFT_ERR_ARG, "mask 0x%x: one bit per dihedral code 0..7, at least one set", mask);
    if (B < 1 || H < 1 || W < 1) return fail(LFT_ERR_SHAPE, "bad image batch (B=%d H=%d W=%d)", B, H, W);
    *E = __builtin_popcount(mask);
    const unsigned long long n = (unsigned long long)B * (unsigned long long)((H + DH_TILE - 1) / DH_TILE) * (unsigned long long)((W + DH_TILE - 1) / DH_TILE);
    if (n * 8ull > 0x7fffffffull) return fail(LFT_ERR_SHAPE, "batch of %d images of %dx%d needs more than 2^31 blocks", B, H, W);
    *blocks = (unsigned)n;
    return 0;
}
int lft_dihedral_batch(const float* in, float* out, const int* codes, int B, int H, int W, void* stream) {
    int E, rc; unsigned blocks;
    if (!codes) return fail(LFT_ERR_ARG, "null pointer");
    if ((rc = dihedral_args(in, out, 1u, B, H, W, &E, &blocks))) return rc;
    k_dihedral<<<blocks, 256, 0, static_cast<hipStream_t>(stream)>>>(in, out, codes, 1u, 1, H, W);
    LFT_LAUNCH_OK("k_dihedral");
    return 0;
}
int lft_dihedral_expand(const float* in, float* out, unsigned mask, int B, int H, int W, void* stream) {
    int E, rc; unsigned blocks;
    if ((rc = dihedral_args(in, out, mask, B, H, W, &E, &blocks))) return rc;
    k_dihedral<<<blocks * (unsigned)E, 256, 0, static_cast<hipStream_t>(stream)>>>(in, out, nullptr, mask, E, H, W);
    LFT_LAUNCH_OK("k_dihedral");
    return 0;
}
int lft_dihedral_merge(const float* in, float* out, unsigned mask, int B, int H, int W, void* stream) {
    int E, rc; unsigned blocks;
    if ((rc = dihedral_args(in, out, mask, B, H, W, &E, &blocks))) return rc;
    k_dihedral_merge<<<blocks, 256, 0, static_cast<hipStream_t>(stream)>>>(in, out, mask, E, H, W);
    LFT_LAUNCH_OK("k_dihedral_merge");
    return 0;
}
int lft_scene_integrate_ens(const float* sr_variants, float* sr_scene, unsigned mask, int A, int h0, int w0, int patch, int stride, int s,
                            void* stream) {
    int nu, nv, rc;
    if (!sr_variants || !sr_scene) return fail(LFT_ERR_ARG, "null pointer");
    if (sr_variants == sr_scene) return fail(LFT_ERR_ARG, "the merge does not work in place (in == out)");
    if (mask == 0 || mask > 0xFFu) return fail(LFT_ERR_ARG, "mask 0x%x: one bit per dihedral code 0..7, at least one set", mask);
    if (A < 1 || s < 1) return fail(LFT_ERR_SHAPE, "bad scene (A=%d s=%d)", A, s);
    if ((rc = scene_counts(h0, w0, patch, stride, &nu, &nv))) return rc;
    // the variants are A*patch*s square mosaics by construction, so a transposing code needs no further shape check
    const int S = stride * s, ts = (S + DH_TILE - 1) / DH_TILE;
    const unsigned long long n = (unsigned long long)nu * nv * A * A * ts * ts;
    if (n > 0x7fffffffull) return fail(LFT_ERR_SHAPE, "scene needs more than 2^31 blocks");
    k_scene_integrate_ens<<<(unsigned)n, 256, 0, static_cast<hipStream_t>(stream)>>>(sr_variants, sr_scene, mask, __builtin_popcount(mask),
                                                                                    A, patch * s, S, h0 * s, w0 * s, nv);
    LFT_LAUNCH_OK("k_scene_integrate_ens");
    return 0;
}

int lft_mfma_selftest(const float* Am, const float* Bm, const float* W2, float* C, float* D, int prec, void* stream) {
    if (!Am || !Bm || !W2 || !C || !D) return fail(LFT_ERR_ARG, "null pointer");
    if (prec != LFT_PREC_F32 && prec != LFT_PREC_BF16 && prec != LFT_PREC_F16) return fail(LFT_ERR_ARG, "bad prec %d", prec);
    by_prec(prec, [&](auto t) { k_selftest<decltype(t)><<<1, 64, 0, static_cast<hipStream_t>(stream)>>>(Am, Bm, W2, C, D); return 0; });
    LFT_LAUNCH_OK("k_selftest");
    return 0;
}

// ================================================================================ metrics
int lft_view_metrics_scratch_bytes(int B, int A, int h, int w, size_t* out_bytes) {
    if (!out_bytes || B < 1 || A < 1 || h < 1 || w < 1) return fail(LFT_ERR_ARG, "bad argument");
    const size_t ntiles = (size_t)((h + kMetTile - 1) / kMetTile) * ((w + kMetTile - 1) / kMetTile);
    *out_bytes = (size_t)B * A * A * ntiles * 3 * sizeof(double);
    return 0;
}
int lft_view_metrics(const float* label, const float* out, int B, int A, int h, int w, float ssim_range, float* psnr, float* ssim,
                     void* scratch, void* stream) {
    if (!label || !out || !psnr || !ssim || !scratch || B < 1 || A < 1) return fail(LFT_ERR_ARG, "bad argument");
    if (h < 11 || w < 11) return fail(LFT_ERR_SHAPE, "views of %dx%d are smaller than the 11x11 SSIM window", h, w);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int ntiles = ((h + kMetTile - 1) / kMetTile) * ((w + kMetTile - 1) / kMetTile), nviews = B * A * A;
    const double C1 = (0.01 * ssim_range) * (0.01 * ssim_range), C2 = (0.03 * ssim_range) * (0.03 * ssim_range);
    k_view_metrics<<<dim3((unsigned)ntiles, (unsigned)nviews), 256, 0, st>>>(label, out, static_cast<double*>(scratch), A, h, w, C1, C2);
    LFT_LAUNCH_OK("k_view_metrics");
    k_view_metrics_final<<<blocks_for(nviews, 64), 64, 0, st>>>(static_cast<const double*>(scratch), nviews, ntiles, h, w, psnr, ssim);
    LFT_LAUNCH_OK("k_view_metrics_final");
    return 0;
}
int lft_lf_prepare(const void* lf, int lf_class, int U, int V, int H, int W, int C, const long long* strides, int A, int s,
                   const int* crops, int n_crops, int crop_h, int crop_w, const double* weights_h, const int* indices_h, int taps_h,
                   const double* weights_w, const int* indices_w, int taps_w, float* hr, float* lr, void* stream) {
    if (!crops || !weights_h || !indices_h || !weights_w || !indices_w || !hr || !lr) return fail(LFT_ERR_ARG, "lft_lf_prepare: null pointer");
    if (int rc = lf_array_ok("lft_lf_prepare", LFT_ERR_ARG, lf, lf_class, U, V, H, W, C, strides)) return rc;
    if (s != 2 && s != 4) return fail(LFT_ERR_ARG, "lft_lf_prepare: scale factor must be 2 or 4, got %d", s);
    if (int rc = centre_views_ok("lft_lf_prepare", LFT_ERR_ARG, "the scripts' centre-view index", U, V, A)) return rc;
    if (n_crops < 0 || crop_h < 1 || crop_w < 1 || crop_h > H || crop_w > W)
        return fail(LFT_ERR_ARG, "lft_lf_prepare: %d crops of %d x %d in views of %d x %d", n_crops, crop_h, crop_w, H, W);
    for (int i = 0; i < n_crops; ++i) {
        const int y0 = crops[2 * i], x0 = crops[2 * i + 1];
        if (y0 < 0 || x0 < 0 || y0 > H - crop_h || x0 > W - crop_w)
            return fail(LFT_ERR_ARG, "lft_lf_prepare: crop %d at (%d, %d) of %d x %d is outside the %d x %d view", i, y0, x0, crop_h, crop_w, H, W);
    }
    if (taps_h < 1 || taps_w < 1 || taps_h > kPrepMaxTaps || taps_w > kPrepMaxTaps)
        return fail(LFT_ERR_ARG, "lft_lf_prepare: %d / %d taps per output (1 .. %d)", taps_h, taps_w, kPrepMaxTaps);
    hipStream_t st = static_cast<hipStream_t>(stream);
    PrepArgs a{};
    a.lf = lf;
    for (int i = 0; i < 5; ++i) a.st[i] = strides[i];
    a.u0 = (U - A) / 2; a.v0 = (V - A) / 2; a.A = A; a.s = s;
    a.ch = crop_h; a.cw = crop_w; a.oh = (crop_h + s - 1) / s; a.ow = (crop_w + s - 1) / s; a.ph = taps_h; a.pw = taps_w;
    a.wh = weights_h; a.ih = indices_h; a.ww = weights_w; a.iw = indices_w; a.hr = hr; a.lr = lr;
    const int TO = kPrepTileHr / s;
    const unsigned tiles = (unsigned)(((a.oh + TO - 1) / TO) * ((a.ow + TO - 1) / TO));
    for (int n0 = 0; n0 < n_crops; n0 += kPrepCrops) {
        const int nb = std::min(kPrepCrops, n_crops - n0);
        PrepCrops c{};
        for (int i = 0; i < nb; ++i) { c.y0[i] = crops[2 * (n0 + i)]; c.x0[i] = crops[2 * (n0 + i) + 1]; }
        a.n0 = n0;
        const dim3 grid(tiles, (unsigned)(A * A), (unsigned)nb);
        by_lf_class(lf_class, [&](auto t) { k_lf_prepare<decltype(t)><<<grid, 256, 0, st>>>(a, c); return 0; });
        LFT_LAUNCH_OK("k_lf_prepare");
    }
    return 0;
}

// ---- colour path (lft_colour.cuh) ----
int lft_lf_luma(const void* lf, int lf_class, int U, int V, int H, int W, int C, const long long* strides, int A, float* y_out,
                void* stream) {
    if (!y_out) return fail(LFT_ERR_ARG, "lft_lf_luma: null pointer");
    if (int rc = colour_lf_ok("lft_lf_luma", lf, lf_class, U, V, H, W, C, strides, A)) return rc;
    const long long blocks = ((long long)H * W + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(LFT_ERR_SHAPE, "lft_lf_luma: views of %d x %d need more than 2^31 blocks", H, W);
    LumaArgs a{};
    a.lf = lf;
    for (int i = 0; i < 5; ++i) a.st[i] = strides[i];
    a.u0 = (U - A) / 2; a.v0 = (V - A) / 2; a.A = A; a.H = H; a.W = W; a.y = y_out;
    const dim3 grid((unsigned)blocks, (unsigned)(A * A));
    by_lf_class(lf_class, [&](auto t) { k_lf_luma<decltype(t)><<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(a); return 0; });
    LFT_LAUNCH_OK("k_lf_luma");
    return 0;
}

int lft_colour_merge(const void* lf, int lf_class, int U, int V, int H, int W, int C, const long long* strides, int A, int s,
                     const float* sr_y, const double* weights_h, const int* indices_h, int taps_h, const double* weights_w,
                     const int* indices_w, int taps_w, const double* minv, void* out, int out_class, void* stream) {
    if (!weights_h || !indices_h || !weights_w || !indices_w || !minv || !out) return fail(LFT_ERR_ARG, "lft_colour_merge: null pointer");
    if (int rc = colour_lf_ok("lft_colour_merge", lf, lf_class, U, V, H, W, C, strides, A)) return rc;
    if (s != 2 && s != 4) return fail(LFT_ERR_SHAPE, "lft_colour_merge: scale factor must be 2 or 4, got %d", s);
    if (taps_h < 1 || taps_w < 1 || taps_h > kColMaxTaps || taps_w > kColMaxTaps)
        return fail(LFT_ERR_ARG, "lft_colour_merge: %d / %d taps per output (1 .. %d)", taps_h, taps_w, kColMaxTaps);
    if (out_class != LFT_LF_UINT8 && out_class != LFT_LF_FLOAT32)
        return fail(LFT_ERR_ARG, "lft_colour_merge: output class must be LFT_LF_UINT8 or LFT_LF_FLOAT32, got %d", out_class);
    const long long tiles = (((long long)s * H + kColTile - 1) / kColTile) * (((long long)s * W + kColTile - 1) / kColTile);
    if ((long long)s * H > 0x7fffffffLL || (long long)s * W > 0x7fffffffLL || tiles > 0x7fffffffLL)
        return fail(LFT_ERR_SHAPE, "lft_colour_merge: views of %d x %d at %dx need more than 2^31 blocks", H, W, s);
    ColourArgs a{};
    a.lf = lf;
    for (int i = 0; i < 5; ++i) a.st[i] = strides[i];
    a.u0 = (U - A) / 2; a.v0 = (V - A) / 2; a.A = A; a.s = s; a.H = H; a.W = W; a.ph = taps_h; a.pw = taps_w;
    a.sr_y = sr_y; a.wh = weights_h; a.ih = indices_h; a.ww = weights_w; a.iw = indices_w;
    for (int i = 0; i < 9; ++i) a.minv[i] = minv[i];
    a.out = out; a.out_f32 = out_class == LFT_LF_FLOAT32;
    const dim3 grid((unsigned)tiles, (unsigned)(A * A));
    by_lf_class(lf_class, [&](auto t) { k_colour_merge<decltype(t)><<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(a); return 0; });
    LFT_LAUNCH_OK("k_colour_merge");
    return 0;
}

// ---- synthetic refocus (lft_refocus.cuh) ----
int lft_refocus(const void* lf, int lf_class, int B, int A, int H, int W, int C, const long long* strides, const void* table, int D,
                int taps, void* out, int out_class, void* stream) {
    WindowedLf l{lf, lf_class, B, A, H, W, C, strides, table, D, taps, 0, 0};
    if (int rc = windowed_lf_ok("lft_refocus", l, out_class, "output", 0, !out, "stacks")) return rc;
    if (!l.tiles) return 0;                                         // an empty stack
    RefocusArgs a{};
    fill_windowed(a, l);
    a.out = out; a.out_f32 = out_class == LFT_LF_FLOAT32;
    const dim3 grid((unsigned)(l.tiles * D * B));
    by_lf_class<false>(lf_class, [&](auto t) { refocus_kernel<decltype(t)>(C, taps)<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(a); return 0; });
    LFT_LAUNCH_OK("k_refocus");
    return 0;
}

// ---- disparity from a plane sweep (lft_disparity.cuh) ----
// the floats of V [B, D, H, W] (and of m [B, D, H, W, C] behind it): 0 when they do not fit 2^40 bytes
static size_t disparity_floats(int B, int D, int H, int W, int C, int flags, size_t* vol_floats) {
    const double vol = (double)B * D * H * W, all = vol * (flags & LFT_DISPARITY_AIF ? 1 + C : 1);
    if (all * 4.0 > 1099511627776.0) return 0;
    *vol_floats = (size_t)B * D * H * W;
    return *vol_floats * (size_t)(flags & LFT_DISPARITY_AIF ? 1 + C : 1);
}
int lft_disparity_scratch_bytes(int B, int D, int H, int W, int C, int flags, size_t* out_bytes) {
    if (!out_bytes) return fail(LFT_ERR_ARG, "lft_disparity: out_bytes is null");
    if (C < 1 || C > 4) return fail(LFT_ERR_ARG, "lft_disparity: %d channels (1 .. 4)", C);
    if (D < 1) return fail(LFT_ERR_ARG, "lft_disparity: %d slopes", D);
    if (flags & ~LFT_DISPARITY_AIF) return fail(LFT_ERR_ARG, "lft_disparity: unknown flags 0x%x", flags);
    if (B < 0 || H < 0 || W < 0) return fail(LFT_ERR_SHAPE, "lft_disparity: negative size in B = %d, views of %d x %d", B, H, W);
    size_t vol = 0;
    const size_t n = disparity_floats(B, D, H, W, C, flags, &vol);
    if (!n && B && H && W) return fail(LFT_ERR_SHAPE, "lft_disparity: the cost volume of %d x %d x %d x %d needs more than 2^40 bytes", B, D, H, W);
    *out_bytes = n * sizeof(float);
    return 0;
}
int lft_disparity(const void* lf, int lf_class, int B, int A, int H, int W, int C, const long long* strides, const void* table,
                  const float* slopes, int D, int taps, int radius, void* scratch, float* disparity, float* confidence, int* index,
                  float* cost, void* aif, int aif_class, void* stream) {
    WindowedLf l{lf, lf_class, B, A, H, W, C, strides, table, D, taps, 0, 0};
    if (int rc = windowed_lf_ok("lft_disparity", l, aif_class, "all-in-focus", radius, !slopes || !scratch || !disparity || !confidence || !index, "sweeps"))
        return rc;
    if (!l.tiles) return 0;                                         // empty maps
    const long long ptiles_x = ((long long)W + kDpTile - 1) / kDpTile, ptiles = ptiles_x * (((long long)H + kDpTile - 1) / kDpTile);
    if (ptiles * B > 0x7fffffffLL) return too_many_blocks("lft_disparity", l, "sweeps");
    size_t vol = 0;
    if (!disparity_floats(B, D, H, W, C, aif ? LFT_DISPARITY_AIF : 0, &vol))
        return fail(LFT_ERR_SHAPE, "lft_disparity: the cost volume of %d x %d x %d x %d needs more than 2^40 bytes", B, D, H, W);
    if ((uintptr_t)scratch & 3) return fail(LFT_ERR_ARG, "lft_disparity: scratch must be 4-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    SweepArgs s{};
    fill_windowed(s, l);
    s.vol = static_cast<float*>(scratch); s.stack = aif ? s.vol + vol : nullptr;
    const dim3 grid((unsigned)(l.tiles * D * B));
    by_lf_class<false>(lf_class, [&](auto t) { sweep_kernel<decltype(t)>(C, taps)<<<grid, 256, 0, st>>>(s); return 0; });
    LFT_LAUNCH_OK("k_sweep_cost");
    PickArgs p{};
    p.vol = s.vol; p.stack = s.stack; p.slopes = slopes;
    p.H = H; p.W = W; p.D = D; p.C = C; p.r = radius; p.tiles_x = (int)ptiles_x; p.tiles = (int)ptiles;
    p.disparity = disparity; p.confidence = confidence; p.index = index; p.cost = cost; p.aif = aif;
    p.aif_f32 = aif_class == LFT_LF_FLOAT32;
    k_disparity_pick<<<dim3((unsigned)(ptiles * B)), 256, 0, st>>>(p);
    LFT_LAUNCH_OK("k_disparity_pick");
    return 0;
}

#endif  // LFT_TU != 2
#if LFT_TU != 1
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
int lft_l1_loss(const float* sr, const float* hr, long long n, float* dsr, float gscale, float* loss, float* scratch1024, void* stream) {
    if (!sr || !hr || !loss || !scratch1024 || n < 1) return fail(LFT_ERR_ARG, "bad argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = (int)std::min<long long>(1024, (n + 255) / 256);
    k_l1_partial<<<nb, 256, 0, st>>>(sr, hr, dsr, gscale, n, scratch1024);
    LFT_LAUNCH_OK("k_l1_partial");
    k_l1_final<<<1, 64, 0, st>>>(scratch1024, nb, 1.0f / (float)n, loss);
    LFT_LAUNCH_OK("k_l1_final");
    return 0;
}
// ---- light-field loss (lft_loss.cuh) ----
namespace {
// do the n floats at a and the n floats at b share memory / does a gradient image (may be null) share memory with either input
inline bool meets(const float* a, const float* b, long long n) { return (uintptr_t)a < (uintptr_t)(b + n) && (uintptr_t)b < (uintptr_t)(a + n); }
inline bool overlaps(const float* dsr, const float* sr, const float* hr, long long n) { return dsr && (meets(dsr, sr, n) || meets(dsr, hr, n)); }
struct LossShape { long long n; int nblocks[2]; };     // stencil blocks of the scalar and of the 16-byte path
int loss_shape(int B, int A, int H, int W, LossShape* s) {
    if (B < 1 || A < 1 || H < 1 || W < 1) return fail(LFT_ERR_SHAPE, "sizes must be positive, got B %d A %d H %d W %d", B, A, H, W);
    if ((long long)A * A > 128) return fail(LFT_ERR_SHAPE, "A * A = %lld views, at most 128 are supported", (long long)A * A);
    s->n = (long long)B * A * A * H * W;
    for (int v = 0; v < 2; ++v)
        s->nblocks[v] = (int)std::min<long long>(kLossMaxBlocks, (s->n / (v ? 4 : 1) + kLossThreads - 1) / kLossThreads);
    return 0;
}
}  // namespace
int lft_lf_loss_scratch_bytes(int B, int A, int H, int W, size_t* out_bytes) {
    if (!out_bytes) return fail(LFT_ERR_ARG, "null pointer");
    LossShape s;
    if (int rc = loss_shape(B, A, H, W, &s)) return rc;
    *out_bytes = (size_t)s.nblocks[0] * kLossSums * sizeof(double);
    return 0;
}
int lft_lf_loss(const float* sr, const float* hr, int B, int A, int H, int W, int penalty, float eps, float w_pix, float w_epi,
                float* dsr, float gscale, float* loss3, void* scratch, void* stream) {
    if (!sr || !hr || !loss3 || !scratch) return fail(LFT_ERR_ARG, "null pointer");
    if ((((uintptr_t)sr | (uintptr_t)hr | (uintptr_t)dsr | (uintptr_t)loss3) & 3) || ((uintptr_t)scratch & 7))
        return fail(LFT_ERR_ARG, "sr, hr, dsr and loss3 must be 4-byte aligned, scratch 8-byte aligned");
    if (penalty != LFT_LOSS_L1 && penalty != LFT_LOSS_MSE && penalty != LFT_LOSS_CHARBONNIER) return fail(LFT_ERR_ARG, "unknown penalty %d", penalty);
    if (penalty == LFT_LOSS_CHARBONNIER && !(eps > 0.0f)) return fail(LFT_ERR_ARG, "the Charbonnier eps must be positive, got %g", (double)eps);
    if (!(w_pix >= 0.0f) || !(w_epi >= 0.0f)) return fail(LFT_ERR_ARG, "weights must not be negative or NaN, got %g and %g", (double)w_pix, (double)w_epi);
    if (w_pix == 0.0f && w_epi == 0.0f) return fail(LFT_ERR_ARG, "both weights are zero");
    if (std::isnan(gscale)) return fail(LFT_ERR_ARG, "gscale is NaN");
    LossShape s;
    if (int rc = loss_shape(B, A, H, W, &s)) return rc;
    if (overlaps(dsr, sr, hr, s.n)) return fail(LFT_ERR_ARG, "dsr overlaps sr or hr: the stencil reads neighbours, in place would race");
    const double n = (double)s.n;
    const double nt[4] = {n / W * (W - 1), n / H * (H - 1), n / A * (A - 1), n / A * (A - 1)};      // n_x, n_y, n_v, n_u: exact in double
    int T = 0;
    for (double c : nt) T += c > 0.0;
    LossFoldArgs f = {};
    f.inv_n = 1.0 / n; f.inv_T = T ? 1.0 / T : 0.0; f.w_pix = (double)w_pix; f.w_epi = (double)w_epi;
    float ct[4];
    for (int t = 0; t < 4; ++t) {
        f.inv_nt[t] = nt[t] > 0.0 ? 1.0 / nt[t] : 0.0;
        ct[t] = (float)((double)w_epi * f.inv_T * f.inv_nt[t]);
    }
    const LossArgs a = {B, A, H, W, eps * eps, (float)((double)w_pix * f.inv_n), ct[0], ct[1], ct[2], ct[3], gscale};
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(scratch);
    const bool vec = ((long long)A * W) % 4 == 0 && !(((uintptr_t)sr | (uintptr_t)hr | (uintptr_t)dsr) & 15);
    const int nb = s.nblocks[vec];
    const bool grad = dsr != nullptr;
    if (int rc = dispatch<LFT_LOSS_L1, LFT_LOSS_MSE, LFT_LOSS_CHARBONNIER>(penalty, [&](auto PEN) {
            return dispatch<true, false>(vec, [&](auto VEC4) {
                return dispatch<true, false>(grad, [&](auto GRAD) {
                    k_lf_loss<PEN, VEC4 ? 4 : 1, GRAD><<<nb, kLossThreads, 0, st>>>(sr, hr, dsr, a, part);
                    return 0;
                });
            });
        })) return rc;
    LFT_LAUNCH_OK("k_lf_loss");
    k_lf_loss_fold<<<1, kLossThreads, 0, st>>>(part, nb, f, loss3);
    LFT_LAUNCH_OK("k_lf_loss_fold");
    return 0;
}
// ---- structural loss term (lft_ssim_loss.cuh) ----
namespace {
struct SsimShape { long long n, nblocks, views; int tiles_x, ntiles; };
int ssim_shape(int B, int A, int H, int W, SsimShape* s) {
    if (B < 1 || A < 1 || H < 1 || W < 1) return fail(LFT_ERR_SHAPE, "sizes must be positive, got B %d A %d H %d W %d", B, A, H, W);
    if (H < 11 || W < 11) return fail(LFT_ERR_SHAPE, "views of %dx%d are smaller than the 11x11 SSIM window", H, W);
    s->tiles_x = (W + kSsimTile - 1) / kSsimTile;
    const long long ntiles = (long long)s->tiles_x * ((H + kSsimTile - 1) / kSsimTile);
    s->views = (long long)B * A * A;
    s->n = s->views * H * W;
    s->nblocks = s->views * ntiles;
    if (s->nblocks > 0x7fffffffLL) return fail(LFT_ERR_SHAPE, "%lld tiles, more than one launch holds", s->nblocks);
    s->ntiles = (int)ntiles;
    return 0;
}
}  // namespace
int lft_ssim_loss_scratch_bytes(int B, int A, int H, int W, size_t* out_bytes) {
    if (!out_bytes) return fail(LFT_ERR_ARG, "null pointer");
    SsimShape s;
    if (int rc = ssim_shape(B, A, H, W, &s)) return rc;
    *out_bytes = (size_t)s.nblocks * sizeof(double);
    return 0;
}
int lft_ssim_loss(const float* sr, const float* hr, int B, int A, int H, int W, float ssim_range, float w_ssim,
                  float* dsr, float gscale, int accumulate, float* total, float* ssim_out, void* scratch, void* stream) {
    if (!sr || !hr || !total || !ssim_out || !scratch) return fail(LFT_ERR_ARG, "null pointer");
    if ((((uintptr_t)sr | (uintptr_t)hr | (uintptr_t)dsr | (uintptr_t)total | (uintptr_t)ssim_out) & 3) || ((uintptr_t)scratch & 7))
        return fail(LFT_ERR_ARG, "sr, hr, dsr, total and ssim_out must be 4-byte aligned, scratch 8-byte aligned");
    if (!(ssim_range > 0.0f) || !std::isfinite(ssim_range)) return fail(LFT_ERR_ARG, "ssim_range must be positive and finite, got %g", (double)ssim_range);
    if (!(w_ssim > 0.0f) || !std::isfinite(w_ssim)) return fail(LFT_ERR_ARG, "w_ssim must be positive and finite, got %g", (double)w_ssim);
    if (std::isnan(gscale)) return fail(LFT_ERR_ARG, "gscale is NaN");
    if (accumulate != 0 && accumulate != 1) return fail(LFT_ERR_ARG, "accumulate must be 0 or 1, got %d", accumulate);
    SsimShape s;
    if (int rc = ssim_shape(B, A, H, W, &s)) return rc;
    if (overlaps(dsr, sr, hr, s.n)) return fail(LFT_ERR_ARG, "dsr overlaps sr or hr: the windows read neighbours, in place would race");
    const double R = (double)ssim_range, count = (double)s.views * (H - 2 * kSsimR) * (W - 2 * kSsimR);
    SsimArgs a = {};
    a.A = A; a.H = H; a.W = W; a.tiles_x = s.tiles_x; a.ntiles = s.ntiles; a.accumulate = accumulate;
    a.C1 = (0.01 * R) * (0.01 * R); a.C2 = (0.03 * R) * (0.03 * R);                  // as lft_view_metrics forms them
    a.k = -(double)gscale * (double)w_ssim / count;                                   // Q = 1 - S
    const SsimFoldArgs f = {1.0 / count, (double)w_ssim, accumulate};
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(scratch);
    if (dsr) k_ssim_loss<true><<<(unsigned)s.nblocks, kSsimThreads, 0, st>>>(sr, hr, dsr, a, part);
    else k_ssim_loss<false><<<(unsigned)s.nblocks, kSsimThreads, 0, st>>>(sr, hr, dsr, a, part);
    LFT_LAUNCH_OK("k_ssim_loss");
    k_ssim_loss_fold<<<1, kSsimThreads, 0, st>>>(part, s.nblocks, f, total, ssim_out);
    LFT_LAUNCH_OK("k_ssim_loss_fold");
    return 0;
}
int lft_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                  int step, float gscale, float weight_decay, void* stream) {
    if (!p || !g || !m || !v || n < 1 || step < 1 || weight_decay < 0.0f) return fail(LFT_ERR_ARG, "bad argument");
    const float bc1 = (float)(1.0 - std::pow((double)beta1, (double)step)), bc2 = (float)(1.0 - std::pow((double)beta2, (double)step));   // in double, as torch.optim.Adam
    k_adam<<<blocks_for(n, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(p, g, m, v, n, lr, beta1, beta2, eps, bc1, bc2, gscale, weight_decay);
    LFT_LAUNCH_OK("k_adam");
    return 0;
}

// ---- guarded Adam step (lft_optim.cuh) ----
namespace {
// Host memory of the guard blocks lft_guard_init wrote: what lft_adam_step_guarded needs to size its launches and to refuse a
// foreign block or another n without reading device memory.  Bounded: the oldest entry goes when a 257th block is initialised.
struct GuardHost { long long n; int nseg, nblocks; unsigned long long seq; };
constexpr size_t kGuardHostMax = 256;
std::mutex g_guard_mu;
std::map<const void*, GuardHost> g_guards;
unsigned long long g_guard_seq = 0;
// what lft_guard_init remembered of the block at `guard` (to *h, which may be null), or the refusal of a block it never saw
int find_guard(const void* guard, GuardHost* h) {
    std::lock_guard<std::mutex> lock(g_guard_mu);
    auto it = g_guards.find(guard);
    if (it == g_guards.end()) return fail(LFT_ERR_ARG, "guard block %p was not initialised by lft_guard_init", guard);
    if (h) *h = it->second;
    return 0;
}
}  // namespace

int lft_guard_bytes(int nseg, size_t* out_bytes) {
    if (!out_bytes) return fail(LFT_ERR_ARG, "null pointer");
    if (nseg < 1 || nseg > kGuardMaxSeg) return fail(LFT_ERR_ARG, "nseg %d outside 1..%d", nseg, kGuardMaxSeg);
    *out_bytes = sizeof(GuardBlock) + (size_t)(kGuardMaxChunks + nseg) * sizeof(GuardPart);
    return 0;
}
int lft_guard_init(void* guard, const lft_segment* segs, int nseg, long long n, long long steps_applied0, void* stream) {
    if (!guard || !segs) return fail(LFT_ERR_ARG, "null pointer");
    if ((uintptr_t)guard & 15) return fail(LFT_ERR_ARG, "the guard block must be 16-byte aligned");
    if (nseg < 1 || nseg > kGuardMaxSeg) return fail(LFT_ERR_ARG, "nseg %d outside 1..%d", nseg, kGuardMaxSeg);
    if (n < 1) return fail(LFT_ERR_SHAPE, "n must be positive, got %lld", n);
    if (steps_applied0 < 0) return fail(LFT_ERR_ARG, "steps_applied0 must not be negative, got %lld", steps_applied0);
    GuardInitArgs a = {};
    long long off = 0;
    for (int i = 0; i < nseg; ++i) {
        if (segs[i].first != off || segs[i].count < 1 || segs[i].count > n - off)
            return fail(LFT_ERR_SHAPE, "segment %d (first %lld, count %lld) does not continue the tiling of [0, %lld) at %lld", i,
                        segs[i].first, segs[i].count, n, off);
        a.count[i] = segs[i].count;
        if (segs[i].trainable) a.trainable[i >> 5] |= 1u << (i & 31);
        off += segs[i].count;
    }
    if (off != n) return fail(LFT_ERR_SHAPE, "the %d segments cover [0, %lld), not [0, %lld)", nseg, off, n);
    a.n = n; a.steps0 = steps_applied0; a.nseg = nseg;
    a.per = kGuardChunk;                                            // floats per block; larger only to bound the number of partials
    if ((n + a.per - 1) / a.per > kGuardMaxChunks) a.per = ((n + kGuardMaxChunks - 1) / kGuardMaxChunks + 1023) / 1024 * 1024;
    int nblocks = 0;
    for (int i = 0; i < nseg; ++i) nblocks += (int)((a.count[i] + a.per - 1) / a.per);
    if (nblocks > kGuardMaxChunks + nseg) return fail(LFT_ERR_SHAPE, "internal: %d blocks for %d segments", nblocks, nseg);
    k_guard_init<<<1, kGuardMaxSeg, 0, static_cast<hipStream_t>(stream)>>>(static_cast<GuardBlock*>(guard), a);
    LFT_LAUNCH_OK("k_guard_init");
    std::lock_guard<std::mutex> lock(g_guard_mu);
    g_guards[guard] = GuardHost{n, nseg, nblocks, ++g_guard_seq};
    if (g_guards.size() > kGuardHostMax) {
        auto oldest = g_guards.begin();
        for (auto it = g_guards.begin(); it != g_guards.end(); ++it)
            if (it->second.seq < oldest->second.seq) oldest = it;
        g_guards.erase(oldest);
    }
    return 0;
}
int lft_adam_step_guarded(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                          float gscale, float weight_decay, float max_norm, void* guard, void* stream) {
    if (!p || !g || !m || !v || !guard) return fail(LFT_ERR_ARG, "null pointer");
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 3) return fail(LFT_ERR_ARG, "p, g, m, v must be 4-byte aligned");
    if (weight_decay < 0.0f) return fail(LFT_ERR_ARG, "weight decay must not be negative");
    if (std::isnan(max_norm)) return fail(LFT_ERR_ARG, "max_norm is NaN (<= 0 or +inf switches clipping off)");
    GuardHost h;
    if (int rc = find_guard(guard, &h)) return rc;
    if (n != h.n) return fail(LFT_ERR_SHAPE, "n = %lld, but the guard block was initialised for %lld", n, h.n);
    hipStream_t st = static_cast<hipStream_t>(stream);
    GuardBlock* gb = static_cast<GuardBlock*>(guard);
    const int clip = max_norm > 0.0f && !std::isinf(max_norm);
    k_grad_stats<<<h.nblocks, kGuardThreads, 0, st>>>(g, gb);
    LFT_LAUNCH_OK("k_grad_stats");
    k_guard_final<<<1, kGuardThreads, 0, st>>>(gb, gscale, max_norm, clip, beta1, beta2);
    LFT_LAUNCH_OK("k_guard_final");
    k_adam_guarded<<<h.nblocks, kGuardThreads, 0, st>>>(p, g, m, v, gb, lr, beta1, beta2, eps, gscale, weight_decay);
    LFT_LAUNCH_OK("k_adam_guarded");
    return 0;
}
int lft_guard_read(const void* guard, void* stream, lft_guard_report* host) {
    if (!guard || !host) return fail(LFT_ERR_ARG, "null pointer");
    if (int rc = find_guard(guard, nullptr)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    LFT_HIP_OK(hipMemcpyAsync(host, guard, sizeof(lft_guard_report), hipMemcpyDeviceToHost, st));   // the report is the block's first member
    LFT_HIP_OK(hipStreamSynchronize(st));
    return 0;
}
int lft_ema_update(float* ema, const float* p, long long n, float decay, int warmup, long long step, const void* guard, void* stream) {
    if (!ema || !p) return fail(LFT_ERR_ARG, "null pointer");
    if (((uintptr_t)ema | (uintptr_t)p) & 3) return fail(LFT_ERR_ARG, "ema and p must be 4-byte aligned");
    if (n < 1) return fail(LFT_ERR_ARG, "n must be positive, got %lld", n);
    if (meets(ema, p, n)) return fail(LFT_ERR_ARG, "ema and p overlap");
    if (!(decay >= 0.0f && decay < 1.0f)) return fail(LFT_ERR_ARG, "decay %g outside [0, 1)", (double)decay);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!guard) {
        if (step < 1) return fail(LFT_ERR_ARG, "step counts from 1, got %lld", step);
        const long long nchunks = (n + kGuardChunk - 1) / kGuardChunk;
        k_ema_plain<<<(int)std::min<long long>(nchunks, 65536), kGuardThreads, 0, st>>>(ema, p, n, decay, warmup != 0, step);
        LFT_LAUNCH_OK("k_ema_plain");
        return 0;
    }
    GuardHost h;
    if (int rc = find_guard(guard, &h)) return rc;
    if (n != h.n) return fail(LFT_ERR_ARG, "n = %lld, but the guard block was initialised for %lld", n, h.n);
    k_ema_guarded<<<h.nblocks, kGuardThreads, 0, st>>>(ema, p, static_cast<const GuardBlock*>(guard), decay, warmup != 0);
    LFT_LAUNCH_OK("k_ema_guarded");
    return 0;
}

#endif  // LFT_TU != 1
}  // extern "C"
