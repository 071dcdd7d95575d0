// lft_objective.hip -- losses and optimizer steps in the C ABI of liblft_hip.so (include/lft_hip.h): L1, the light-field loss,
// the structural term, the focal-stack term with the adjoint of refocus, Adam, the guarded step and the EMA of the weights.
#include "lft_host.cuh"
#include "../../include/lft_hip_focal.h"
#include "lft_optim.cuh"     // guarded Adam step: gradient statistics, skip / clip decision, update (lft_adam_step_guarded)
#include "lft_loss.cuh"      // pixel + EPI-gradient loss with L1 / MSE / Charbonnier penalty (lft_lf_loss)
#include "lft_ssim_loss.cuh" // structural term 1 - SSIM and its gradient, fp64 inside (lft_ssim_loss)
#include "lft_focal.cuh"     // focal-stack term: refocused residual, its penalty, the adjoint of refocus (lft_focal_loss, lft_refocus_adjoint)

// ================================================================================ C ABI
extern "C" {

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
struct SsimShape { long long n, nblocks, views; SsimWindow win; };
int ssim_shape(int B, int A, int H, int W, float ssim_range, SsimShape* s) {
    if (B < 1 || A < 1 || H < 1 || W < 1) return fail(LFT_ERR_SHAPE, "sizes must be positive, got B %d A %d H %d W %d", B, A, H, W);
    if (int rc = ssim_views_ok(H, W)) return rc;
    s->win = ssim_window(H, W, kSsimTile, ssim_range);
    s->views = (long long)B * A * A;
    s->n = s->views * H * W;
    s->nblocks = s->views * s->win.ntiles;
    if (s->nblocks > 0x7fffffffLL) return fail(LFT_ERR_SHAPE, "%lld tiles, more than one launch holds", s->nblocks);
    return 0;
}
}  // namespace
int lft_ssim_loss_scratch_bytes(int B, int A, int H, int W, size_t* out_bytes) {
    if (!out_bytes) return fail(LFT_ERR_ARG, "null pointer");
    SsimShape s;
    if (int rc = ssim_shape(B, A, H, W, 1.0f, &s)) return rc;
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
    if (int rc = ssim_shape(B, A, H, W, ssim_range, &s)) return rc;
    if (overlaps(dsr, sr, hr, s.n)) return fail(LFT_ERR_ARG, "dsr overlaps sr or hr: the windows read neighbours, in place would race");
    const double count = (double)s.views * (H - 2 * kSsimR) * (W - 2 * kSsimR);
    SsimArgs a = {};
    a.A = A; a.H = H; a.W = W; a.tiles_x = s.win.tiles_x; a.ntiles = (int)s.win.ntiles; a.accumulate = accumulate;
    a.C1 = s.win.C1; a.C2 = s.win.C2;                                                 // ssim_window's, as lft_view_metrics takes them
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
// ---- focal-stack term and the adjoint of refocus (lft_focal.cuh) ----
namespace {
struct FocalShape { long long n_stack, n_mosaic, res_blocks, adj_blocks; int tiles_x, tiles; };
// the rules lft_focal_loss and lft_refocus_adjoint share, under the caller's name
int focal_shape(const char* who, int B, int D, int A, int H, int W, int taps, FocalShape* s) {
    if (taps != 1 && taps != 2 && taps != 4) return fail(LFT_ERR_ARG, "%s: %d taps: 1 (nearest), 2 (linear) and 4 (cubic) are supported", who, taps);
    if (D < 1 || D > LFT_FOCAL_MAX_D) return fail(LFT_ERR_ARG, "%s: %d slopes outside 1 .. %d", who, D, LFT_FOCAL_MAX_D);
    if (B < 1 || A < 1 || H < 1 || W < 1) return fail(LFT_ERR_SHAPE, "%s: sizes must be positive, got B %d A %d H %d W %d", who, B, A, H, W);
    if ((long long)A * A > 128) return fail(LFT_ERR_SHAPE, "%s: A * A = %lld views, at most 128 are supported", who, (long long)A * A);
    if ((long long)A * H * A * W > 0x7fffffffLL) return fail(LFT_ERR_SHAPE, "%s: a mosaic of %d x %d views of %d x %d spans more than 2^31 - 1 elements", who, A, A, H, W);
    s->tiles_x = (W + kFocalTileX - 1) / kFocalTileX;
    s->tiles = s->tiles_x * ((H + kFocalTileY - 1) / kFocalTileY);
    s->n_stack = (long long)B * D * H * W;
    s->n_mosaic = (long long)B * A * A * H * W;
    s->res_blocks = (long long)B * D * s->tiles;
    s->adj_blocks = (long long)B * A * A * s->tiles;
    if (s->res_blocks > 0x7fffffffLL || s->adj_blocks > 0x7fffffffLL)
        return fail(LFT_ERR_SHAPE, "%s: %d images of %d x %d need more than 2^31 - 1 blocks of %d x %d pixels", who, B, H, W, kFocalTileX, kFocalTileY);
    return 0;
}
FocalArgs focal_args(int A, int H, int W, int D, const FocalShape& s, const void* table, int accumulate) {
    FocalArgs a = {};
    a.A = A; a.H = H; a.W = W; a.D = D; a.tiles_x = s.tiles_x; a.tiles = s.tiles;
    a.table = static_cast<const int*>(table); a.accumulate = accumulate;
    return a;
}
int focal_adjoint(const float* G, const FocalArgs& a, const FocalShape& s, int taps, float* out, hipStream_t st) {
    if (int rc = dispatch<1, 2, 4>(taps, [&](auto TAPS) {
            k_focal_adjoint<TAPS><<<(unsigned)s.adj_blocks, kFocalThreads, 0, st>>>(G, a, out);
            return 0;
        })) return rc;
    LFT_LAUNCH_OK("k_focal_adjoint");
    return 0;
}
}  // namespace
int lft_focal_loss_scratch_bytes(int B, int D, int A, int H, int W, size_t* out_bytes) {
    const char* who = "lft_focal_loss_scratch_bytes";
    if (!out_bytes) return fail(LFT_ERR_ARG, "%s: null pointer", who);
    FocalShape s;
    if (int rc = focal_shape(who, B, D, A, H, W, 1, &s)) return rc;
    *out_bytes = align256((size_t)s.res_blocks * sizeof(double)) + (size_t)s.n_stack * sizeof(float);
    return 0;
}
int lft_focal_loss(const float* sr, const float* hr, int B, int A, int H, int W, const void* table, int D, int taps, int penalty,
                   float eps, float w_focal, float* dsr, float gscale, int accumulate, float* total, float* focal_out, float* residual,
                   void* scratch, void* stream) {
    const char* who = "lft_focal_loss";
    FocalShape s;                                                   // sizes first: an empty tensor's pointer may be null
    if (int rc = focal_shape(who, B, D, A, H, W, taps, &s)) return rc;
    if (!sr || !hr || !table || !total || !focal_out || !scratch) return fail(LFT_ERR_ARG, "%s: null pointer", who);
    if ((((uintptr_t)sr | (uintptr_t)hr | (uintptr_t)table | (uintptr_t)dsr | (uintptr_t)total | (uintptr_t)focal_out | (uintptr_t)residual) & 3) ||
        ((uintptr_t)scratch & 7))
        return fail(LFT_ERR_ARG, "%s: sr, hr, table, dsr, total, focal_out and residual must be 4-byte aligned, scratch 8-byte aligned", who);
    if (penalty != LFT_LOSS_L1 && penalty != LFT_LOSS_MSE && penalty != LFT_LOSS_CHARBONNIER) return fail(LFT_ERR_ARG, "%s: unknown penalty %d", who, penalty);
    if (penalty == LFT_LOSS_CHARBONNIER && !(eps > 0.0f)) return fail(LFT_ERR_ARG, "%s: the Charbonnier eps must be positive, got %g", who, (double)eps);
    if (!(w_focal > 0.0f) || !std::isfinite(w_focal)) return fail(LFT_ERR_ARG, "%s: w_focal must be positive and finite, got %g", who, (double)w_focal);
    if (std::isnan(gscale)) return fail(LFT_ERR_ARG, "%s: gscale is NaN", who);
    if (accumulate != 0 && accumulate != 1) return fail(LFT_ERR_ARG, "%s: accumulate must be 0 or 1, got %d", who, accumulate);
    if (overlaps(dsr, sr, hr, s.n_mosaic)) return fail(LFT_ERR_ARG, "%s: dsr overlaps sr or hr", who);
    FocalArgs a = focal_args(A, H, W, D, s, table, accumulate);
    a.eps2 = (double)eps * (double)eps;
    a.c = (double)gscale * (double)w_focal / (double)s.n_stack;
    const FocalFoldArgs f = {1.0 / (double)s.n_stack, (double)w_focal, accumulate};
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(scratch);
    float* G = dsr ? at<float>(scratch, align256((size_t)s.res_blocks * sizeof(double))) : nullptr;
    if (int rc = dispatch<LFT_LOSS_L1, LFT_LOSS_MSE, LFT_LOSS_CHARBONNIER>(penalty, [&](auto PEN) {
            return dispatch<1, 2, 4>(taps, [&](auto TAPS) {
                k_focal_residual<PEN, TAPS><<<(unsigned)s.res_blocks, kFocalThreads, 0, st>>>(sr, hr, a, residual, G, part);
                return 0;
            });
        })) return rc;
    LFT_LAUNCH_OK("k_focal_residual");
    k_focal_fold<<<1, kFocalThreads, 0, st>>>(part, s.res_blocks, f, total, focal_out);
    LFT_LAUNCH_OK("k_focal_fold");
    return dsr ? focal_adjoint(G, a, s, taps, dsr, st) : 0;
}
int lft_refocus_adjoint(const float* stack_grad, int B, int A, int H, int W, const void* table, int D, int taps, float* out,
                        int accumulate, void* stream) {
    const char* who = "lft_refocus_adjoint";
    FocalShape s;
    if (int rc = focal_shape(who, B, D, A, H, W, taps, &s)) return rc;
    if (!stack_grad || !table || !out) return fail(LFT_ERR_ARG, "%s: null pointer", who);
    if (((uintptr_t)stack_grad | (uintptr_t)table | (uintptr_t)out) & 3) return fail(LFT_ERR_ARG, "%s: stack_grad, table and out must be 4-byte aligned", who);
    if (accumulate != 0 && accumulate != 1) return fail(LFT_ERR_ARG, "%s: accumulate must be 0 or 1, got %d", who, accumulate);
    if ((uintptr_t)out < (uintptr_t)(stack_grad + s.n_stack) && (uintptr_t)stack_grad < (uintptr_t)(out + s.n_mosaic))
        return fail(LFT_ERR_ARG, "%s: out overlaps stack_grad", who);
    return focal_adjoint(stack_grad, focal_args(A, H, W, D, s, table, accumulate), s, taps, out, static_cast<hipStream_t>(stream));
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

}  // extern "C"
