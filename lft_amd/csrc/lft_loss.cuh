// Light-field training loss (lft_lf_loss; the definition is in include/lft_hip.h): a pixel penalty plus the same penalty on the
// gradients of the epipolar-plane images, value and gradient in ONE stencil pass over the mosaic, then one fold.
//
//   k_lf_loss<PEN, VEC, GRAD> : a thread owns VEC pixels of one mosaic row (VEC = 4: 16-byte accesses, row pitch and pointers
//                               permitting; VEC = 1 otherwise).  It forms d = sr - hr there and at the neighbours that exist --
//                               x +- 1 and y +- 1 inside the view, the same pixel of views a2 +- 1 (W columns away) and a1 +- 1 (H rows
//                               away) --, writes dsr and adds rho(d) and rho of the four forward differences that START at its pixels
//                               to five double sums.  GRAD = false (dsr == NULL): only the forward neighbours are read.  The sums are
//                               folded into five doubles per block by BlockSum (lft_common.cuh).
//   k_lf_loss_fold            : one workgroup adds the per-block partials in a fixed order and writes {total, P, E}.
// No atomics: the same bits every run.  Every element offset is formed in 64 bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kLossThreads = 256;
constexpr int kLossMaxBlocks = 2048;            // beyond it the stencil pass strides over the mosaic; bounds the fold
constexpr int kLossSums = 5;                    // rho(d), rho(Dx d), rho(Dy d), rho(Dv d), rho(Du d)

struct LossArgs {
    int B, A, H, W;
    float eps2;                                 // Charbonnier: eps * eps
    float cp, cx, cy, cv, cu;                   // w_pix / n and w_epi / (T n_t): 0 for a difference that does not exist
    float gscale;
};
struct LossFoldArgs {
    double inv_n, inv_nt[4], inv_T, w_pix, w_epi;          // inv_nt[t] = 0 for a difference that does not exist
};

// rho and rho' of the three penalties, in the type of x: fp32 here, fp64 for the focal term (lft_focal.cuh).  The one place they
// are written
__device__ inline float loss_abs(float x) { return fabsf(x); }
__device__ inline double loss_abs(double x) { return fabs(x); }
__device__ inline float loss_sqrt(float x) { return sqrtf(x); }
__device__ inline double loss_sqrt(double x) { return sqrt(x); }
template <int PEN, typename T> __device__ inline T loss_rho(T x, T eps2) {
    if constexpr (PEN == LFT_LOSS_L1) return loss_abs(x);
    else if constexpr (PEN == LFT_LOSS_MSE) return x * x;
    else return loss_sqrt(x * x + eps2);
}
template <int PEN, typename T> __device__ inline T loss_drho(T x, T eps2) {
    if constexpr (PEN == LFT_LOSS_L1) return (T)(x > (T)0) - (T)(x < (T)0);
    else if constexpr (PEN == LFT_LOSS_MSE) return (T)2 * x;
    else return x / loss_sqrt(x * x + eps2);
}
// d = sr - hr of VEC consecutive pixels from element i (VEC = 4: i is a multiple of 4 behind 16-byte aligned pointers)
template <int VEC> __device__ inline void loss_load(const float* __restrict__ sr, const float* __restrict__ hr, long long i, float (&o)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 a = *reinterpret_cast<const float4*>(sr + i), b = *reinterpret_cast<const float4*>(hr + i);
        o[0] = a.x - b.x; o[1] = a.y - b.y; o[2] = a.z - b.z; o[3] = a.w - b.w;
    } else {
        o[0] = sr[i] - hr[i];
    }
}

template <int PEN, int VEC, bool GRAD>
__global__ __launch_bounds__(kLossThreads) void k_lf_loss(const float* __restrict__ sr, const float* __restrict__ hr, float* __restrict__ dsr,
                                                          LossArgs p, double* __restrict__ part) {
    __shared__ BlockSum<double, kLossSums, kLossThreads / 64> red;
    const int H = p.H, W = p.W, A = p.A;
    const long long R = (long long)A * H, C = (long long)A * W;           // rows and columns of one mosaic
    const long long cpr = C / VEC, nchunk = (long long)p.B * R * cpr;     // VEC = 4 only when C is a multiple of 4
    const bool wvec = VEC == 4 && (W & 3) == 0;                           // then a chunk never straddles two views
    double s[kLossSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long q = (long long)blockIdx.x * kLossThreads + threadIdx.x; q < nchunk; q += (long long)gridDim.x * kLossThreads) {
        const long long grow = q / cpr, c0 = (q - grow * cpr) * VEC;      // row over all images, first column
        const long long r = grow % R;
        const int a1 = (int)(r / H), y = (int)(r - (long long)a1 * H);
        const long long i0 = grow * C + c0;
        const bool ym = y > 0, yp = y < H - 1, um = a1 > 0, up = a1 < A - 1;
        float d[VEC], dn[VEC], g[VEC];
        loss_load<VEC>(sr, hr, i0, d);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float rh = loss_rho<PEN>(d[j], p.eps2);
            s[0] += (double)rh;
            if constexpr (GRAD) g[j] = p.cp * loss_drho<PEN>(d[j], p.eps2);
        }
        // rows: y + 1 and view a1 + 1 start a difference here, y - 1 and view a1 - 1 end one here
        if (yp) {
            loss_load<VEC>(sr, hr, i0 + C, dn);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float t = dn[j] - d[j];
                s[2] += (double)loss_rho<PEN>(t, p.eps2);
                if constexpr (GRAD) g[j] -= p.cy * loss_drho<PEN>(t, p.eps2);
            }
        }
        if (up) {
            loss_load<VEC>(sr, hr, i0 + (long long)H * C, dn);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float t = dn[j] - d[j];
                s[4] += (double)loss_rho<PEN>(t, p.eps2);
                if constexpr (GRAD) g[j] -= p.cu * loss_drho<PEN>(t, p.eps2);
            }
        }
        if constexpr (GRAD) {
            if (ym) {
                loss_load<VEC>(sr, hr, i0 - C, dn);
#pragma unroll
                for (int j = 0; j < VEC; ++j) g[j] += p.cy * loss_drho<PEN>(d[j] - dn[j], p.eps2);
            }
            if (um) {
                loss_load<VEC>(sr, hr, i0 - (long long)H * C, dn);
#pragma unroll
                for (int j = 0; j < VEC; ++j) g[j] += p.cu * loss_drho<PEN>(d[j] - dn[j], p.eps2);
            }
        }
        // columns: the same for x +- 1 and views a2 +- 1
        const int a2_0 = (int)(c0 / W), x_0 = (int)(c0 - (long long)a2_0 * W);
        if (wvec) {                                                       // one view for the whole chunk, 16-byte angular loads
            if (a2_0 < A - 1) {
                loss_load<VEC>(sr, hr, i0 + W, dn);
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float t = dn[j] - d[j];
                    s[3] += (double)loss_rho<PEN>(t, p.eps2);
                    if constexpr (GRAD) g[j] -= p.cv * loss_drho<PEN>(t, p.eps2);
                }
            }
            if constexpr (GRAD) {
                if (a2_0 > 0) {
                    loss_load<VEC>(sr, hr, i0 - W, dn);
#pragma unroll
                    for (int j = 0; j < VEC; ++j) g[j] += p.cv * loss_drho<PEN>(d[j] - dn[j], p.eps2);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            int a2 = a2_0, x = x_0 + j;
            if (x >= W) { a2 += x / W; x %= W; }                          // W < 4: a chunk may span several views
            const long long i = i0 + j;
            if (x < W - 1) {
                const float t = (j + 1 < VEC ? d[(j + 1) % VEC] : sr[i + 1] - hr[i + 1]) - d[j];
                s[1] += (double)loss_rho<PEN>(t, p.eps2);
                if constexpr (GRAD) g[j] -= p.cx * loss_drho<PEN>(t, p.eps2);
            }
            if constexpr (GRAD) {
                if (x > 0) g[j] += p.cx * loss_drho<PEN>(d[j] - (j > 0 ? d[(j + VEC - 1) % VEC] : sr[i - 1] - hr[i - 1]), p.eps2);
            }
            if (!wvec) {
                if (a2 < A - 1) {
                    const float t = (sr[i + W] - hr[i + W]) - d[j];
                    s[3] += (double)loss_rho<PEN>(t, p.eps2);
                    if constexpr (GRAD) g[j] -= p.cv * loss_drho<PEN>(t, p.eps2);
                }
                if constexpr (GRAD) {
                    if (a2 > 0) g[j] += p.cv * loss_drho<PEN>(d[j] - (sr[i - W] - hr[i - W]), p.eps2);
                }
            }
        }
        if constexpr (GRAD) {
            if constexpr (VEC == 4) *reinterpret_cast<float4*>(dsr + i0) = make_float4(g[0] * p.gscale, g[1] * p.gscale, g[2] * p.gscale, g[3] * p.gscale);
            else dsr[i0] = g[0] * p.gscale;
        }
    }
    const int tid = threadIdx.x;
    red.put(s, tid);
    __syncthreads();
    if (tid < kLossSums) part[(long long)blockIdx.x * kLossSums + tid] = red.get(tid);
}

__global__ __launch_bounds__(kLossThreads) void k_lf_loss_fold(const double* __restrict__ part, int nb, LossFoldArgs f, float* __restrict__ loss3) {
    __shared__ BlockSum<double, kLossSums, kLossThreads / 64> red;
    if (blockIdx.x != 0) return;
    const int tid = threadIdx.x;
    double s[kLossSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = tid; b < nb; b += kLossThreads)
        for (int k = 0; k < kLossSums; ++k) s[k] += part[(long long)b * kLossSums + k];
    red.put(s, tid);
    __syncthreads();
    if (tid == 0) {
        double t[kLossSums];
        for (int k = 0; k < kLossSums; ++k) t[k] = red.get(k);
        const double P = t[0] * f.inv_n;
        const double E = (t[1] * f.inv_nt[0] + t[2] * f.inv_nt[1] + t[3] * f.inv_nt[2] + t[4] * f.inv_nt[3]) * f.inv_T;
        loss3[0] = (float)(f.w_pix * P + f.w_epi * E);
        loss3[1] = (float)P;
        loss3[2] = (float)E;
    }
}

// L1 loss (reference LFT.py:269-277) and its gradient: loss = mean |sr - hr|; dsr = sign(sr - hr) * gscale.
__global__ __launch_bounds__(256) void k_l1_partial(const float* __restrict__ sr, const float* __restrict__ hr, float* __restrict__ dsr,
                                                    float gscale, long long n, float* __restrict__ part) {
    __shared__ float red[256];
    float s = 0.0f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float d = sr[i] - hr[i];
        s += fabsf(d);
        if (dsr) dsr[i] = d > 0.0f ? gscale : (d < 0.0f ? -gscale : 0.0f);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
__global__ void k_l1_final(const float* __restrict__ part, int nb, float inv_n, float* __restrict__ loss) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        float s = 0.0f;
        for (int i = 0; i < nb; ++i) s += part[i];
        *loss = s * inv_n;
    }
}

}  // namespace
