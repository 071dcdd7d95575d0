#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// lft_optim.cuh -- the guarded Adam step (lft_adam_step_guarded): gradient statistics, the skip / clip decision and the update,
// three launches on one stream with no host round trip, so that a non-finite gradient or an exploding norm is dealt with on the
// device and the call is graph-capturable (Adam's step counter lives in the guard block, not in a host scalar).
//
//   k_guard_init    writes the guard block: the segment table (one segment per parameter tensor of the flat buffer), the block
//                   map derived from it, the counters, an empty report.
//   k_grad_stats    ONE pass over the flat fp32 gradient buffer: per block the sum of squares (fp64: the square of an fp32 number
//                   is exact in fp64, nothing rounds before it is added) and the number of non-finite elements, which are left
//                   out of the sum.  No floating-point atomics: every block writes one partial.
//   k_guard_final   one workgroup folds the partials in a fixed order (bit-reproducible run to run), per segment and over the
//                   trainable segments, and decides: a non-finite element in a trainable segment -> skip (only steps_skipped
//                   advances); otherwise coef = min(1, max_norm / (norm + 1e-6)) -- torch.nn.utils.clip_grad_norm_'s formula, in
//                   double --, steps_applied += 1 =: t, bc1 = 1 - beta1^t, bc2 = 1 - beta2^t in double as lft_adam_step forms them.
//   k_adam_guarded  k_adam's arithmetic with gi = g * gscale * coef + wd * p over the trainable segments only; on skip p, m and v
//                   keep their bits.
//   k_ema_guarded   (lft_ema_update) ema += a * (p - ema) over the same block map, after the update: a step the guard skipped and a
//   k_ema_plain     frozen segment leave ema alone, and the step number of the warm-up comes from the block.  k_ema_plain is the
//                   form without a guard block: chunks of kGuardChunk floats over [0, n), the step number from the caller.
//
// DIFFERENCE FROM TORCH: clip_grad_norm_ scales .grad in place, so a later reader of .grad sees the clipped gradient.  Here the
// gradient buffer is NEVER written: the coefficient is folded into the update, and g after the call is what the backward pass (and
// the all-reduce) left there.  The report carries the norm and the coefficient for whoever wants the clipped values.
//
// Block map: a block works on at most `per` consecutive floats of ONE segment (per = kGuardChunk, larger only for buffers beyond
// kGuardChunk * kGuardMaxChunks floats, so that the number of partials is bounded by the segment count alone); segment i owns
// blocks bstart[i] .. bstart[i + 1] - 1.  Segments begin at arbitrary float offsets: a block's range is split into a scalar head
// up to the first 16-byte boundary, 16-byte loads / stores, and a scalar tail (guard_walk); sums fold through BlockSum (lft_common.cuh).

constexpr int kGuardMaxSeg = 128;          // seg_norm[128] of lft_guard_report
constexpr int kGuardChunk = 2048;          // floats per block: 256 threads x two 16-byte accesses per array
constexpr int kGuardMaxChunks = 2048;      // n / per never exceeds this; the map has at most kGuardMaxChunks + nseg blocks
constexpr int kGuardThreads = 256;

struct GuardPart { double sumsq; unsigned long long bad; };
struct GuardBlock {
    lft_guard_report rep;                  // first: lft_guard_read copies exactly this
    long long n, per;
    int nseg, nblocks;
    float bc1, bc2;                        // Adam's bias corrections of the step k_guard_final admitted last
    long long first[kGuardMaxSeg], count[kGuardMaxSeg];
    int trainable[kGuardMaxSeg];
    int bstart[kGuardMaxSeg + 1];
    int pad_[3];                           // the partials that follow the block start on a 16-byte boundary
};
static_assert(sizeof(GuardBlock) % 16 == 0, "GuardPart array behind the block must be 16-byte aligned");
static_assert(sizeof(lft_guard_report) == 48 + 4 * kGuardMaxSeg, "lft_guard_report has no padding");

__device__ __host__ inline GuardPart* guard_parts(GuardBlock* gb) { return reinterpret_cast<GuardPart*>(gb + 1); }
__device__ __host__ inline const GuardPart* guard_parts(const GuardBlock* gb) { return reinterpret_cast<const GuardPart*>(gb + 1); }

// Passed BY VALUE as the kernel's argument: the host table is read when the launch is enqueued, no copy from caller memory is
// left in flight when lft_guard_init returns.  first[] is implied by the counts (the table tiles [0, n)).
struct GuardInitArgs {
    long long count[kGuardMaxSeg];
    unsigned trainable[kGuardMaxSeg / 32];
    long long n, per, steps0;
    int nseg;
};

__global__ void k_guard_init(GuardBlock* __restrict__ gb, const GuardInitArgs a) {
    if (blockIdx.x != 0) return;
    for (int i = threadIdx.x; i < kGuardMaxSeg; i += blockDim.x) {
        const bool in = i < a.nseg;
        gb->count[i] = in ? a.count[i] : 0;
        gb->trainable[i] = in ? (int)((a.trainable[i >> 5] >> (i & 31)) & 1u) : 0;
        gb->rep.seg_norm[i] = 0.0f;
    }
    if (threadIdx.x != 0) return;
    long long off = 0;
    int b = 0;
    for (int i = 0; i < kGuardMaxSeg; ++i) {
        gb->first[i] = off;
        gb->bstart[i] = b;
        if (i < a.nseg) {
            off += a.count[i];
            b += (int)((a.count[i] + a.per - 1) / a.per);
        }
    }
    gb->bstart[kGuardMaxSeg] = b;
    gb->n = a.n; gb->per = a.per; gb->nseg = a.nseg; gb->nblocks = b;
    gb->bc1 = 1.0f; gb->bc2 = 1.0f;
    gb->rep.grad_norm = 0.0f; gb->rep.clip_coef = 1.0f;
    gb->rep.skipped_last = 0; gb->rep.bad_segment = -1;
    gb->rep.nonfinite_last = 0;
    gb->rep.steps_applied = a.steps0; gb->rep.steps_skipped = 0; gb->rep.steps_clipped = 0;
}

// Segment and float range [lo, hi) of block b (b < gb->nblocks): the last segment whose first block is <= b.
__device__ inline int guard_range(const GuardBlock* __restrict__ gb, int b, long long* lo, long long* hi) {
    int s0 = 0, s1 = gb->nseg;             // bstart[s0] <= b < bstart[s1]
    while (s1 - s0 > 1) {
        const int mid = (s0 + s1) >> 1;
        if (gb->bstart[mid] <= b) s0 = mid; else s1 = mid;
    }
    const long long first = gb->first[s0], end = first + gb->count[s0];
    *lo = first + (long long)(b - gb->bstart[s0]) * gb->per;
    *hi = *lo + gb->per < end ? *lo + gb->per : end;
    return s0;
}
// Floats of [lo, hi) in front of the first 16-byte boundary of base + lo (base: a float pointer's address).
__device__ inline long long guard_head(uintptr_t base, long long lo, long long hi) {
    const long long head = (long long)((4 - (((base >> 2) + (unsigned long long)lo) & 3)) & 3);
    return head < hi - lo ? head : hi - lo;
}

// One block's walk over [lo, hi) of NRW arrays it updates and one it reads: f(x, r) at every element, x the NRW values there, r the
// value read.  Scalar head to the first 16-byte boundary, 16-byte accesses, scalar tail; all scalar when the alignments differ.
template <int NRW, typename F>
__device__ __forceinline__ void guard_walk(float* const* rw, const float* __restrict__ ro, long long lo, long long hi, int tid, F f) {
    bool same = true;
    for (int j = 0; j < NRW; ++j) same = same && (((uintptr_t)rw[j] >> 2) & 3) == (((uintptr_t)ro >> 2) & 3);
    const long long a = same ? lo + guard_head((uintptr_t)ro, lo, hi) : hi;
    const long long nvec = (hi - a) >> 2, vend = a + 4 * nvec;
    auto one = [&](long long i) {
        float x[NRW + 1];
        for (int j = 0; j < NRW; ++j) x[j] = rw[j][i];
        f(x, ro[i]);
        for (int j = 0; j < NRW; ++j) rw[j][i] = x[j];
    };
    for (long long i = lo + tid; i < a; i += kGuardThreads) one(i);
    for (long long q = tid; q < nvec; q += kGuardThreads) {
        const long long i = a + 4 * q;
        float4 x4[NRW + 1];
        for (int j = 0; j < NRW; ++j) x4[j] = *reinterpret_cast<const float4*>(rw[j] + i);
        const float4 r4 = *reinterpret_cast<const float4*>(ro + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float x[NRW + 1];
            for (int j = 0; j < NRW; ++j) x[j] = reinterpret_cast<const float*>(&x4[j])[e];
            f(x, reinterpret_cast<const float*>(&r4)[e]);
            for (int j = 0; j < NRW; ++j) reinterpret_cast<float*>(&x4[j])[e] = x[j];
        }
        for (int j = 0; j < NRW; ++j) *reinterpret_cast<float4*>(rw[j] + i) = x4[j];
    }
    if (vend + tid < hi) one(vend + tid);
}

__global__ __launch_bounds__(kGuardThreads) void k_grad_stats(const float* __restrict__ g, GuardBlock* __restrict__ gb) {
    __shared__ BlockSum<double, 1, kGuardThreads / 64> s_sum;
    __shared__ BlockSum<unsigned long long, 1, kGuardThreads / 64> s_bad;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= gb->nblocks) return;
    long long lo, hi;
    guard_range(gb, b, &lo, &hi);
    double sum = 0.0;
    unsigned long long bad = 0;
    guard_walk<0>(nullptr, g, lo, hi, tid, [&](float*, float x) {
        if ((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) { ++bad; return; }  // inf or NaN: counted, not summed
        const double d = (double)x;
        sum += d * d;
    });
    s_sum.put(&sum, tid); s_bad.put(&bad, tid);
    __syncthreads();
    if (tid == 0) guard_parts(gb)[b] = GuardPart{s_sum.get(0), s_bad.get(0)};
}

__global__ __launch_bounds__(kGuardThreads) void k_guard_final(GuardBlock* __restrict__ gb, float gscale, float max_norm, int clip,
                                                               float beta1, float beta2) {
    __shared__ double s_sum[kGuardMaxSeg];
    __shared__ unsigned long long s_bad[kGuardMaxSeg];
    if (blockIdx.x != 0) return;
    const int tid = threadIdx.x, lane = tid & 63, nseg = gb->nseg;
    const GuardPart* part = guard_parts(gb);
    for (int s = tid >> 6; s < nseg; s += kGuardThreads / 64) {                     // one wave per segment, lanes stride its partials
        double sum = 0.0;
        unsigned long long bad = 0;
        for (int j = gb->bstart[s] + lane; j < gb->bstart[s + 1]; j += 64) { sum += part[j].sumsq; bad += part[j].bad; }
        sum = wave_sum(sum); bad = wave_sum(bad);
        if (lane == 0) {
            s_sum[s] = sum; s_bad[s] = bad;
            gb->rep.seg_norm[s] = (float)((double)gscale * sqrt(sum));
        }
    }
    __syncthreads();
    if (tid != 0) return;
    double tot = 0.0;
    unsigned long long bad = 0;
    int bad_seg = -1;
    for (int s = 0; s < nseg; ++s) {                                                // a frozen segment's gradient is ignored
        if (!gb->trainable[s]) continue;
        tot += s_sum[s];
        if (s_bad[s] && bad_seg < 0) bad_seg = s;
        bad += s_bad[s];
    }
    const double norm = (double)gscale * sqrt(tot);
    gb->rep.grad_norm = (float)norm;
    gb->rep.nonfinite_last = (long long)bad;
    gb->rep.bad_segment = bad_seg;
    if (bad) {                                                                      // nothing else advances
        gb->rep.skipped_last = 1;
        gb->rep.clip_coef = 0.0f;
        gb->rep.steps_skipped += 1;
        return;
    }
    double coef = 1.0;
    if (clip) {
        coef = (double)max_norm / (norm + 1e-6);
        if (coef > 1.0) coef = 1.0;
    }
    const float cf = (float)coef;
    gb->rep.skipped_last = 0;
    gb->rep.clip_coef = cf;
    if (cf < 1.0f) gb->rep.steps_clipped += 1;
    const long long t = gb->rep.steps_applied + 1;
    gb->rep.steps_applied = t;
    gb->bc1 = (float)(1.0 - pow((double)beta1, (double)t));
    gb->bc2 = (float)(1.0 - pow((double)beta2, (double)t));
}

struct AdamHyper { float lr, b1, b2, eps, bc1, bc2, gscale, coef, wd; };
// Adam at one element (weight_decay: torch.optim.Adam's L2 term), written once: k_adam passes coef = 1, k_adam_guarded the guard's
__device__ inline void adam_one(float& p, float g, float& m, float& v, const AdamHyper& h) {
    const float gi = g * h.gscale * h.coef + h.wd * p;                              // the clip is folded in here; g is not written
    const float mi = h.b1 * m + (1.0f - h.b1) * gi;
    const float vi = h.b2 * v + (1.0f - h.b2) * gi * gi;
    m = mi; v = vi;
    const float denom = sqrtf(vi) / sqrtf(h.bc2) + h.eps;
    p -= (h.lr / h.bc1) * (mi / denom);
}

__global__ __launch_bounds__(kGuardThreads) void k_adam_guarded(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                float* __restrict__ v, const GuardBlock* __restrict__ gb, float lr,
                                                                float b1, float b2, float eps, float gscale, float wd) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= gb->nblocks || gb->rep.skipped_last) return;
    long long lo, hi;
    const int s = guard_range(gb, b, &lo, &hi);
    if (!gb->trainable[s]) return;
    const AdamHyper h = {lr, b1, b2, eps, gb->bc1, gb->bc2, gscale, gb->rep.clip_coef, wd};
    float* const pmv[3] = {p, m, v};
    guard_walk<3>(pmv, g, lo, hi, tid, [&](float* x, float gi) { adam_one(x[0], gi, x[1], x[2], h); });
}

// ---- exponential moving average of the weights (lft_ema_update) ----
// a = (float)(1 - d_t), d_t = warmup ? min(decay, (1 + t) / (10 + t)) : decay, in double (IEEE division and subtraction: the host
// restatement lft_amd.train.ema_decay_at gives the same float).
__device__ inline float ema_alpha(float decay, int warmup, long long t) {
    double d = (double)decay;
    if (warmup) {
        const double w = (1.0 + (double)t) / (10.0 + (double)t);
        if (w < d) d = w;
    }
    return (float)(1.0 - d);
}
__device__ inline void ema_one(float& e, float p, float a) { e += a * (p - e); }
__device__ inline void ema_range(float* __restrict__ ema, const float* __restrict__ p, long long lo, long long hi, float a, int tid) {
    float* const e1[1] = {ema};
    guard_walk<1>(e1, p, lo, hi, tid, [&](float* e, float pi) { ema_one(e[0], pi, a); });
}

__global__ __launch_bounds__(kGuardThreads) void k_ema_guarded(float* __restrict__ ema, const float* __restrict__ p,
                                                               const GuardBlock* __restrict__ gb, float decay, int warmup) {
    const int b = blockIdx.x;
    if (b >= gb->nblocks || gb->rep.skipped_last) return;
    long long lo, hi;
    const int s = guard_range(gb, b, &lo, &hi);
    if (!gb->trainable[s]) return;
    ema_range(ema, p, lo, hi, ema_alpha(decay, warmup, gb->rep.steps_applied), threadIdx.x);
}

__global__ __launch_bounds__(kGuardThreads) void k_ema_plain(float* __restrict__ ema, const float* __restrict__ p, long long n,
                                                             float decay, int warmup, long long step) {
    const float a = ema_alpha(decay, warmup, step);
    const long long nchunks = (n + kGuardChunk - 1) / kGuardChunk;
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const long long lo = c * kGuardChunk, hi = lo + kGuardChunk < n ? lo + kGuardChunk : n;
        ema_range(ema, p, lo, hi, a, threadIdx.x);
    }
}

// Adam (torch.optim.Adam defaults used by the reference, train.py:77-83: betas, eps, weight_decay 0), one flat
// fp32 buffer of all parameters: p -= lr_t * m_hat / (sqrt(v_hat) + eps).  bc1 = 1 - b1^t, bc2 = 1 - b2^t.
__global__ void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                       long long n, float lr, float b1, float b2, float eps, float bc1, float bc2, float gscale, float wd) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    adam_one(p[i], g[i], m[i], v[i], AdamHyper{lr, b1, b2, eps, bc1, bc2, gscale, 1.0f, wd});
}

}  // namespace
