// lft_occlusion.cuh -- the plane sweep's cost from partial apertures: next to a foreground edge the views on the far side of the
// edge see the foreground at the background's true slope, the variance of all views is large there and a wrong slope wins.  The
// views of one side of the aperture still agree, so the cost below also scores a slope by the variance of up to four subsets of
// the views and lets a subset win where it is much better than the whole aperture.
//
// The inputs, the table, the samples s, the aperture a (fp64 on the host, sum 1) and the centre (cu, cv) are those of
// lft_disparity. Everything below is fp32, one rounded operation per step, with contraction off.
//
// Subsets (host only). Let du = u - cu and dv = v - cv in fp64.
// - "halves": the four subsets du <= 0, du >= 0, dv <= 0, dv >= 0.
// - "quadrants": (<=,<=), (<=,>=), (>=,<=), (>=,>=) in (du, dv).
// - A boolean array [P, A, A] with 1 <= P <= 4.
// - A subset is kept iff at least min_views of its views have a > 0. min_views is an integer >= 2, default 2. One view has
//   variance 0 at every slope and would win everywhere.
// - Dropped subsets never reach the kernel. Subset ids in the outputs are positions in the kept list.
// - If no subset is kept, raise LftError.
// - For a kept subset p: W_p = sum_{p} a in fp64. The row b_p[u,v] = fl32(a/W_p) for members and 0 for the rest.
// - The table [P', A*A] fp32, views in (u, v) order, is the only place these weights are rounded.
//
// Moments.
// - The full aperture is unchanged: m, q, V_full exactly as today, the same FMAs in the same order. m stays refocus's stack bit
//   for bit, and aif is still gathered from it.
// - Per kept subset, over its members in (u, v) order:
//   - m_p = fma(b_p, s, m_p)
//   - q_p = fma(fl(b_p*s), s, q_p)
//   - V_p = sum_c max(q_p - fl(m_p*m_p), 0), with c = 0 first.
//
// Combination.
// - t = min_p V_p and U = fl(beta*t).
// - V = min(V_full, U).
// - choice = 0 if V_full <= U, else the lowest p (1-based) with V_p = t.
// - beta is the margin: finite, >= 1, rounded once to fp32. A subset wins only where it is beta times better than the whole
//   aperture.
//
// After that. Steps 3 to 7 of lft_disparity run word for word on this V, through the existing k_disparity_pick unchanged.
//
// New outputs.
// - subset: uint8 [B, H, W], equal to choice at (k*, y, x).
// - Optionally the whole choice volume, uint8 [B, D, H, W].
// - Read together with index, subset is an occlusion-edge map: 0 where all views agree.
//
// No result may depend on the tile, the launch shape or the arrival order.
//
//   k_sweep_cost_occ  k_sweep_cost's grid and window pipeline with 1 + P' accumulator pairs per element.  The body is written once,
//                     sweep_cost<T, C, TAPS, OCC> in lft_disparity.cuh, and holds what is described here under `if constexpr (OCC)`;
//                     the kernel below is that body with OCC set.  The tile stays 32 x 32 and a lane keeps 4C elements: 2 * 4C * 5 = 160
//                     accumulators at C = 4 and four subsets, which a workgroup of 256 lanes (one wave per SIMD, up to 512
//                     registers each) holds without scratch; what is given up is occupancy, not the window's reuse.  The column
//                     pass first leaves its 4C samples in registers, then walks the subsets: a view's membership is the same for
//                     every lane (b_p[view] != 0, read through a uniform address), so each subset is one scalar branch round an
//                     unrolled loop over statically indexed registers.  After the last view the channel sums go through the
//                     row-pass LDS buffer one moment pair after the other -- the whole aperture first, then the subsets in order,
//                     each between two barriers -- and a lane keeps for its four pixels V_full, the running minimum t and the
//                     subset that set it (strictly smaller replaces: the lowest p wins a tie).  V leaves as fp32, choice as one
//                     byte per pixel and slope.
//   k_occ_gather      one lane per pixel: subset[b, y, x] = choice[b, index[b, y, x], y, x], the index clamped into 0 .. D-1.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lft_disparity.cuh"

namespace {

struct SweepOccArgs {
    SweepArgs s;                     // the plain sweep's arguments; vol takes V = min(V_full, U)
    const float* subsets;            // [P, A*A] b_p, 0 for the views outside the subset
    int P;                           // kept subsets, 1 .. kOccMaxP
    float beta;
    uint8_t* choice;                 // [B, D, H, W] or null
};

struct OccGatherArgs {
    const int* index;                // [B, H, W]
    const uint8_t* choice;           // [B, D, H, W]
    uint8_t* subset;                 // [B, H, W]
    int D;
    size_t plane, n;                 // H * W, B * H * W
};

template <typename T, int C, int TAPS>
__global__ __launch_bounds__(256) void k_sweep_cost_occ(SweepOccArgs oa) { sweep_cost<T, C, TAPS, true>(oa.s, oa.subsets, oa.P, oa.beta, oa.choice); }

__global__ __launch_bounds__(256) void k_occ_gather(OccGatherArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const size_t b = i / a.plane, at = i % a.plane;
    const int k = min(max(a.index[i], 0), a.D - 1);
    a.subset[i] = a.choice[(b * a.D + k) * a.plane + at];
}

// the instantiation for an input type, channel count (1 .. 4) and tap count (1, 2, 4)
template <typename T>
inline void (*sweep_occ_kernel(int C, int taps))(SweepOccArgs) {
    static void (*const k[4][3])(SweepOccArgs) = {{k_sweep_cost_occ<T, 1, 1>, k_sweep_cost_occ<T, 1, 2>, k_sweep_cost_occ<T, 1, 4>},
                                                  {k_sweep_cost_occ<T, 2, 1>, k_sweep_cost_occ<T, 2, 2>, k_sweep_cost_occ<T, 2, 4>},
                                                  {k_sweep_cost_occ<T, 3, 1>, k_sweep_cost_occ<T, 3, 2>, k_sweep_cost_occ<T, 3, 4>},
                                                  {k_sweep_cost_occ<T, 4, 1>, k_sweep_cost_occ<T, 4, 2>, k_sweep_cost_occ<T, 4, 4>}};
    return k[C - 1][taps == 4 ? 2 : taps - 1];
}

}  // namespace
