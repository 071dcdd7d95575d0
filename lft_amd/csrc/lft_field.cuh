// lft_field.cuh -- angular tiling: every view of a U x V light field through an A x A network (lft_field_divide,
// lft_field_integrate).  Declared in include/lft_hip_field.h.
#pragma once
#include "lft_blend.cuh"      // clamp_shear, fold_idx, and the per-window maps of the three scene integrates, which these kernels follow

namespace {

// ------------------------------------------------------------------------------------------
// Field mosaic.  A field mosaic is fp32 [U*h0, V*w0]; view (p, q) occupies rows p*h0 ... and columns q*w0 ...: the scene mosaic with
// two angular sizes.
//
// Windows along one axis of L views, with 1 <= astride <= A <= L.  m(L) = 1 if L = A, else ceil((L-A)/astride) + 1.  The origins are
// o_i = min(i*astride, L-A): strictly increasing, the last one clamped so the last view is covered, consecutive ones at most A apart so
// every view is covered.  mu = m(U) and mv = m(V).  Window w = wu*mv + wv has origin (o_wu, o_wv).  N = nu*nv comes from
// lft_scene_counts.  Batch element b = w*N + n.  A view lies in at most ceil(A/astride) + 1 windows per axis; the +1 comes from the
// clamped last window (A = 2, astride = 2, L = 5 has origins 0, 2, 3, and view 3 is in two windows).
//
// Divide.  [U*h0, V*w0] -> [mu*mv*N, 1, A*patch, A*patch].  Element b is exactly what lft_scene_divide gives for patch n of the A x A
// sub-mosaic of views (o_wu+u, o_wv+v); with a shear (int32 [mu*mv*N], one value per batch element, clamped to +-kmax of
// lft_hip_shear.h) it is exactly what lft_scene_divide_shear gives with k = shear[b].  No sub-mosaic is materialised.
//
// Integrate.  [mu*mv*N, 1, A*pz, A*pz] -> [U*h0*s, V*w0*s], pz = patch*s.  g is the angular table, fp32 [A], strictly positive; win is
// the spatial table: null (the crop) or fp32 [pz] as in lft_hip_blend.h.  The terms of output view (p, q), pixel (Y, X) are visited in
// ascending wu, then wv, then ku, then kv.  A window (wu, wv) takes part when 0 <= u = p - o_wu < A and 0 <= v = q - o_wv < A.
// ga = g[u]*g[v], one rounded product.  With win null there is one term per window: the element lft_scene_integrate would read for that
// window's sub-scene (lft_scene_integrate_shear when sheared), with the weight wt = ga.  With win set there is one term for every
// (ku, kv) that lft_scene_integrate_blend counts as contributing for that window's sub-scene (the same test, the same
// sk_b = s*clamp(shear[b])), with the weight wt = ga*(win[a]*win[b]), each product rounded once.
//     num = num + wt*x,   den = den + wt,   out = num / den
// Every operation is one rounded fp32 operation, contraction is off and the quotient is correctly rounded: a pixel's bits do not
// depend on the launch shape.  Every pixel has at least one term.
//
// Both kernels are gathers, one lane per output element, HBM-bound.  k_field_divide: the window and the patch come from the grid, so
// the origin, the shear and the source row are wave-uniform.  k_field_integrate: g and win go to LDS once per workgroup; a lane loops
// over its candidate windows [wu0, wu1] x [wv0, wv1] -- exactly the windows that take part -- and inside each over the spatial
// candidates of lft_blend.cuh.  NW = 0 is that loop, for any tiling and for every blend.  The crop with at most NW <= 2 windows per
// axis has its NW x NW windows written out, as lft_blend.cuh writes out its candidates: every shear is requested, then every pixel, and
// only then are the terms added in order, so a lane's loads are in flight together.  For the blend the loop stays: writing out the
// windows and a window's 3 x 3 candidates, or the candidates alone, was measured and was slower than the loop (DESIGN.md section 10 has
// the figures): most views lie in one window and most pixels in 2 x 2 patches, and a written-out lane pays for all of them.  Both
// forms add the same terms in the same order and give the same bits.
// ------------------------------------------------------------------------------------------
struct FieldGeom {
    int U, V, A, astride, mu, mv;       // the views, the windows
    int h0, w0, pz, S, nu, nv;          // a view, a patch side, the stride (k_field_integrate: in SR pixels), the patches per axis
    int s, kmax;
};
LFT_DEV int field_origin(int i, int astride, int L, int A) { return min(i * astride, L - A); }

__global__ __launch_bounds__(256) void k_field_divide(const float* __restrict__ field, const int* __restrict__ shear,
                                                      float* __restrict__ patches, const FieldGeom f, int cb) {
    // grid: x = window * cb + block of 256 of the A*patch columns, y = row of the patch mosaic, z = patch index ku*nv + kv; here
    // pz = patch and S = stride, in LR pixels
    const int w = blockIdx.x / cb, X = (blockIdx.x - w * cb) * 256 + threadIdx.x, Y = blockIdx.y, n = blockIdx.z;
    const int patch = f.pz, stride = f.S, P = f.A * patch;
    if (X >= P) return;
    const int wu = w / f.mv, wv = w - wu * f.mv;
    const int ou = field_origin(wu, f.astride, f.U, f.A), ov = field_origin(wv, f.astride, f.V, f.A);
    const size_t b = (size_t)w * (f.nu * f.nv) + n;
    const int k = shear ? clamp_shear(shear[b], f.kmax) : 0, u0 = f.A / 2;
    const int bdr = (patch - stride) / 2, ku = n / f.nv, kv = n - ku * f.nv;
    const int u = Y / patch, y = Y - u * patch, v = X / patch, x = X - v * patch;
    const int ey = ku * stride + y, ex = kv * stride + x;
    float val = 0.0f;                                   // beyond the extended view: zero fill, judged on the unsheared coordinates
    if (ey < f.h0 + 2 * bdr && ex < f.w0 + 2 * bdr)
        val = field[(size_t)((ou + u) * f.h0 + fold_idx(ey - bdr + k * (u - u0), f.h0)) * ((size_t)f.V * f.w0) + (ov + v) * f.w0 +
                    fold_idx(ex - bdr + k * (v - u0), f.w0)];
    patches[(b * P + Y) * P + X] = val;
}

template <int NW>
__global__ __launch_bounds__(256) void k_field_integrate(const float* __restrict__ sub, const int* __restrict__ shear,
                                                         const float* __restrict__ window, const float* __restrict__ angular,
                                                         float* __restrict__ out, const FieldGeom f) {
#pragma clang fp contract(off)
    // grid: k_scene_integrate_blend's -- x over the V*w0 columns of the SR field mosaic, y = its rows; pz, S, h0, w0 are in SR pixels
    extern __shared__ float tab[];                      // g, A entries, then the window table, pz entries
    float* g = tab;
    float* win = tab + f.A;
    for (int i = threadIdx.x; i < f.A; i += 256) g[i] = angular[i];
    if (window)
        for (int i = threadIdx.x; i < f.pz; i += 256) win[i] = window[i];
    __syncthreads();
    const int Xm = blockIdx.x * 256 + threadIdx.x, Ym = blockIdx.y;
    if (Xm >= f.V * f.w0) return;
    const int A = f.A, pz = f.pz, S = f.S, bdr = (pz - S) / 2, u0 = A / 2, N = f.nu * f.nv;
    const int p = Ym / f.h0, Y = Ym - p * f.h0, q = Xm / f.w0, X = Xm - q * f.w0;
    // the windows that take part: o_i >= p - A + 1 from wu0 on, o_i <= p up to wu1
    const int wu0 = p - A + 1 <= 0 ? 0 : min((p - A + f.astride) / f.astride, f.mu - 1), wu1 = p >= f.U - A ? f.mu - 1 : p / f.astride;
    const int wv0 = q - A + 1 <= 0 ? 0 : min((q - A + f.astride) / f.astride, f.mv - 1), wv1 = q >= f.V - A ? f.mv - 1 : q / f.astride;
    // the crop's patch and pixel; the blend's candidates, as in k_scene_integrate_blend
    const int kuc = Y / S, kvc = X / S, ic = Y - kuc * S, jc = X - kvc * S;
    const int ku0 = Y - pz + 1 <= 0 ? 0 : (Y - pz + S) / S, ku1 = min(f.nu - 1, (Y + 2 * bdr) / S);
    const int kv0 = X - pz + 1 <= 0 ? 0 : (X - pz + S) / S, kv1 = min(f.nv - 1, (X + 2 * bdr) / S);
    const size_t P = (size_t)A * pz;
    float num = 0.0f, den = 0.0f;
    if constexpr (NW == 0) {
        for (int wu = wu0; wu <= wu1; ++wu) {
            const int u = p - field_origin(wu, f.astride, f.U, A);
            if (u < 0 || u >= A) continue;
            for (int wv = wv0; wv <= wv1; ++wv) {
                const int v = q - field_origin(wv, f.astride, f.V, A);
                if (v < 0 || v >= A) continue;
                const float ga = g[u] * g[v];
                const size_t base = (size_t)(wu * f.mv + wv) * N;
                if (!window) {
                    const size_t e = base + kuc * f.nv + kvc;
                    const int sk = shear ? f.s * clamp_shear(shear[e], f.kmax) : 0;
                    const int a = bdr + ic - sk * (u - u0), b = bdr + jc - sk * (v - u0);
                    num = num + ga * sub[(e * P + u * pz + a) * P + v * pz + b];
                    den = den + ga;
                    continue;
                }
                for (int ku = ku0; ku <= ku1; ++ku)
                    for (int kv = kv0; kv <= kv1; ++kv) {
                        const size_t e = base + ku * f.nv + kv;
                        const int sk = shear ? f.s * clamp_shear(shear[e], f.kmax) : 0;
                        const int a = Y - ku * S + bdr - sk * (u - u0), b = X - kv * S + bdr - sk * (v - u0);
                        if (a < 0 || a >= pz || b < 0 || b >= pz) continue;
                        const float wt = ga * (win[a] * win[b]);
                        num = num + wt * sub[(e * P + u * pz + a) * P + v * pz + b];
                        den = den + wt;
                    }
            }
        }
    } else {                                            // the crop: one term per window, the NW x NW windows written out
        constexpr int NA = NW * NW;
        int sk[NA];
        bool ok[NA];
        float wt[NA], x[NA];
#pragma unroll
        for (int c = 0; c < NA; ++c) {                  // a window beyond the range reads the last one's shear and contributes nothing
            const int wu = min(wu0 + c / NW, f.mu - 1), wv = min(wv0 + c % NW, f.mv - 1);
            sk[c] = shear ? shear[(size_t)(wu * f.mv + wv) * N + kuc * f.nv + kvc] : 0;
        }
#pragma unroll
        for (int c = 0; c < NA; ++c) {
            const int wu = wu0 + c / NW, wv = wv0 + c % NW;
            const int u = p - field_origin(min(wu, f.mu - 1), f.astride, f.U, A), v = q - field_origin(min(wv, f.mv - 1), f.astride, f.V, A);
            const int k = f.s * clamp_shear(sk[c], f.kmax);
            const int a = bdr + ic - k * (u - u0), b = bdr + jc - k * (v - u0);
            ok[c] = wu <= wu1 && wv <= wv1 && u >= 0 && u < A && v >= 0 && v < A;
            wt[c] = x[c] = 0.0f;
            if (ok[c]) {
                wt[c] = g[u] * g[v];
                x[c] = sub[(((size_t)(wu * f.mv + wv) * N + kuc * f.nv + kvc) * P + u * pz + a) * P + v * pz + b];
            }
        }
#pragma unroll
        for (int c = 0; c < NA; ++c)                    // ascending wu, then wv
            if (ok[c]) {
                num = num + wt[c] * x[c];
                den = den + wt[c];
            }
    }
    out[(size_t)Ym * ((size_t)f.V * f.w0) + Xm] = __fdiv_rn(num, den);
}

}  // namespace
