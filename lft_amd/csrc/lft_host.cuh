// lft_host.cuh -- what the host code of every unit of liblft_hip.so starts from: the error buffer and fail(), the launch checks,
// the per-kernel profiler, compile-time dispatch, the shape of a call (Dims) and the small helpers around a launch.  It names no
// kernel: a unit emits the kernels of the headers it includes, and this one comes into all of them.
#pragma once
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
#include "lft_common.cuh"     // bf16_t, f16_t (by_prec)

#define LFT_HIDDEN __attribute__((visibility("hidden")))      // shared by the library's units, seen by no other library
// Optional per-kernel timing (lft_forward_profiled, lft_train_step_profiled): an event is recorded on the launch stream after
// each kernel.
struct LFT_HIDDEN LftProfiler {
    bool on = false;
    hipStream_t st = nullptr;
    std::vector<hipEvent_t> ev;
    std::vector<const char*> names;
};
// One error buffer (per thread, kErrLen bytes) and one profiler for the library: declared here, defined in lft_network.hip.
// Functions, not variables: a unit that only sees the declaration of a thread_local variable reaches it through a weak
// initialisation symbol, which hidden visibility does not leave null.
constexpr size_t kErrLen = 512;
LFT_HIDDEN char* lft_err_buf();
LFT_HIDDEN LftProfiler& lft_prof();

namespace {

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(lft_err_buf(), kErrLen, fmt, ap);
    va_end(ap);
    return code;
}

#define LFT_HIP_OK(expr)                                                                     \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return fail((int)e_, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)
// Launch name with the call's shape appended ("k_lin:128>256", profiled runs only); interned, so the pointer stays valid.
inline const char* prof_name(const char* plain, const char* fmt, ...) {
    if (!lft_prof().on) return plain;
    static thread_local std::set<std::string> names;
    char buf[96];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return names.insert(buf).first->c_str();
}
inline void prof_mark(const char* name) {
    LftProfiler& g_prof = lft_prof();
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
    LftProfiler& g_prof = lft_prof();
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

}  // namespace
