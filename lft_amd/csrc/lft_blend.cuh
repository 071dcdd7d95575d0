// lft_blend.cuh -- windowed blending of overlapping SR patches into the SR scene (lft_scene_integrate_blend).  Declared in
// include/lft_hip_blend.h.
#pragma once
#include "lft_shear.cuh"      // clamp_shear; the map of k_scene_integrate_shear, which this kernel reads backwards

namespace {

// ------------------------------------------------------------------------------------------
// k_scene_integrate keeps the central stride*s square of every SR patch and drops the rest; the kept squares meet edge to edge.
// Here every SR patch pixel that shows a scene pixel contributes to it, weighted by a separable window over the patch.
//
// All sizes are in SR pixels.  pz = patch*s, S = stride*s, bdr = (pz - S)/2; u0 = A / 2; sk_n = s*clamp(shear[n], +-kmax), or 0
// where shear is null.  Pixel (a, b) of view (u, v) of SR patch n = ku*nv + kv shows scene pixel
//     Y = ku*S + a - bdr + sk_n*(u - u0),   X = kv*S + b - bdr + sk_n*(v - u0)
// which is k_scene_integrate_shear's map, read backwards.  The pixel contributes iff 0 <= Y < h0 and 0 <= X < w0.  That drops the
// reflected margin and everything beyond the extended view, so no zero-filled position ever contributes.
//     num = sum (w[a]*w[b]) * sub[n, u, a, v, b],   den = sum w[a]*w[b],   out = num / den
// The sum runs over the contributing patches in ascending ku, then kv.  Every operation is one rounded fp32 operation (contraction
// is off, as in lft_refocus.cuh) and the division is correctly rounded: a pixel's bits do not depend on the launch shape.
//
// A gather, one lane per SR mosaic element.  The candidates of a lane are ku in [Y/S - m, Y/S + m], m = ceil(pz/S), and the same in
// kv, each tested against the definition.  Of those only ku*S in [Y - pz + 1, Y + 2*bdr] can pass the test (0 <= a < pz with
// |sk_n*(u - u0)| <= bdr): at most NC = ceil(2*pz/S) - 1 per axis, 3 at pz = 2*S, of which 2 x 2 load.  For NC <= 3 the NC x NC
// candidates are written out: every shear is requested, then every contributing pixel, and only then are the terms added in order --
// a lane's loads are in flight together instead of one behind the other (a loop that loads and adds per candidate took 1.37 times as
// long with a shear at pz = 2*S, 0.46 against 0.34 ms for 5x5 views of 1024x1024, and the same time without one).  NC = 0 is
// that loop, for any tiling.  The window goes to LDS once per workgroup; the shear of a candidate is read per lane (the lanes of one
// patch share the address).
// ------------------------------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(256) void k_scene_integrate_blend(const float* __restrict__ sub, const int* __restrict__ shear,
                                                               const float* __restrict__ window, float* __restrict__ out, int A, int pz,
                                                               int stride, int h0, int w0, int nu, int nv, int s, int kmax) {
#pragma clang fp contract(off)
    // grid: k_scene_integrate's -- x over the A*w0 columns of the SR scene mosaic, y = its rows; pz, stride, h0, w0 are in SR pixels
    extern __shared__ float win[];                      // the window table, pz entries
    for (int i = threadIdx.x; i < pz; i += 256) win[i] = window[i];
    __syncthreads();
    const int Xm = blockIdx.x * 256 + threadIdx.x, Ym = blockIdx.y;
    if (Xm >= A * w0) return;
    const int bdr = (pz - stride) / 2, u0 = A / 2;
    const int u = Ym / h0, Y = Ym - u * h0, v = Xm / w0, X = Xm - v * w0;
    const int du = u - u0, dv = v - u0;
    // ku*stride in [Y - pz + 1, Y + 2*bdr], inside the patches there are; a subset of [Y/stride - m, Y/stride + m]
    const int ku0 = Y - pz + 1 <= 0 ? 0 : (Y - pz + stride) / stride, ku1 = min(nu - 1, (Y + 2 * bdr) / stride);
    const int kv0 = X - pz + 1 <= 0 ? 0 : (X - pz + stride) / stride, kv1 = min(nv - 1, (X + 2 * bdr) / stride);
    const size_t P = (size_t)A * pz;
    float num = 0.0f, den = 0.0f;
    if constexpr (NC == 0) {
        for (int ku = ku0; ku <= ku1; ++ku)
            for (int kv = kv0; kv <= kv1; ++kv) {
                const int n = ku * nv + kv;
                const int sk = shear ? s * clamp_shear(shear[n], kmax) : 0;
                const int a = Y - ku * stride + bdr - sk * du, b = X - kv * stride + bdr - sk * dv;
                if (a < 0 || a >= pz || b < 0 || b >= pz) continue;
                const float ww = win[a] * win[b];
                num = num + ww * sub[((size_t)n * P + u * pz + a) * P + v * pz + b];
                den = den + ww;
            }
    } else {
        int sk[NC * NC], a[NC * NC], b[NC * NC];
        bool ok[NC * NC];
        float x[NC * NC];
#pragma unroll
        for (int c = 0; c < NC * NC; ++c) {             // a candidate beyond the range reads the last patch's shear and contributes nothing
            const int ku = min(ku0 + c / NC, nu - 1), kv = min(kv0 + c % NC, nv - 1);
            sk[c] = shear ? shear[ku * nv + kv] : 0;
        }
#pragma unroll
        for (int c = 0; c < NC * NC; ++c) {
            const int ku = ku0 + c / NC, kv = kv0 + c % NC;
            const int k = s * clamp_shear(sk[c], kmax);
            a[c] = Y - ku * stride + bdr - k * du;
            b[c] = X - kv * stride + bdr - k * dv;
            ok[c] = ku <= ku1 && kv <= kv1 && a[c] >= 0 && a[c] < pz && b[c] >= 0 && b[c] < pz;
            x[c] = 0.0f;
            if (ok[c]) x[c] = sub[((size_t)(ku * nv + kv) * P + u * pz + a[c]) * P + v * pz + b[c]];
        }
#pragma unroll
        for (int c = 0; c < NC * NC; ++c)               // ascending ku, then kv
            if (ok[c]) {
                const float ww = win[a[c]] * win[b[c]];
                num = num + ww * x[c];
                den = den + ww;
            }
    }
    out[(size_t)Ym * (A * w0) + Xm] = __fdiv_rn(num, den);
}

}  // namespace
