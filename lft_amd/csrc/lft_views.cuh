// lft_views.cuh -- view synthesis: views at fractional angular positions from the A x A views of a light field and a disparity map.
//
// Inputs:
// - B light fields of A x A views, H x W pixels, C <= 4 channels, read in place through refocus's six element strides.
// - uint8 enters as x/255 (rf_x), float32 as stored.
// - A disparity map Dr, fp32 [B,H,W], given at the angular position reference = (ur,vr).
// - d_range = (lo,hi), lo <= hi, rounded once to fp32. Finite Dr is clamped into it before use; non-finite pixels are skipped.
// - T targets (ut,vt) in view-index units, fp64 on the host.
// - The sign convention is refocus's: a point seen at y in view u is seen at y + d*(u'-u) in view u'.
//
// All coordinate arithmetic is fp32, one rounded operation per step, with the compiler's contraction off as in k_refocus, so a
// numpy float32 restatement reproduces it bit for bit.
//
// 1. Splat. Du = fl32(ut-ur), Dv likewise. Each source pixel (y,x) with clamped d lands at py = fl(y + fl(d*Du)),
//    px = fl(x + fl(d*Dv)) and covers (floor(py)+a, floor(px)+b) for a,b in {0,1}; a=1 is dropped when py is integral, b=1 when px
//    is integral; pixels outside the image are dropped. Dt0[y',x'] is the nearest d among the coverers: the max for
//    near = larger, the min for near = smaller. The result does not depend on arrival order.
//    reach = ceil(max(|lo|,|hi|) * max(|Du|,|Dv|)) + 1; reach > 64 is refused.
// 2. Fill. A hole is a pixel with no coverer. It takes the farther (near = larger: the smaller) of the nearest non-hole Dt0 values
//    to its left and right in the row, each searched up to `fill` pixels (0..64); one side alone gives that one; neither: the same
//    search up and down the column; nothing there either: clamped Dr[y,x], or the far end of d_range if that pixel is non-finite.
//    Only pre-fill values are read. holes = 1 for filled pixels.
// 3. Render. One 16-byte record per (target, view): {du = fl32(u-ut), dv, w, skip}, w >= 0 summing to 1 per target, computed in
//    fp64 on the host and rounded once. For d = Dt[y,x] and each view with w > 0, in (u,v) order: sy = fl(y + fl(d*du)), sx
//    likewise; the view is inside iff 0 <= sy <= H-1 and 0 <= sx <= W-1; iy = floor(sy), f = sy - iy, which is exact.
//    linear: taps iy, iy+1 with weights fl(1-f), f. cubic: taps iy-1 .. iy+2 with Keys' kernel (a = -0.5) at f+1, f, 1-f, 2-f,
//    evaluated in fp32 (in factored forms, vw_keys01 / vw_keys12). Taps are clamped (replicate). Rows are filtered first, then columns, with explicit FMAs as in k_refocus.
//    out = (sum_inside w*s) / (sum_inside w); if no view is inside, the same quotient over all views with w > 0.
//    Output is fp32 or uint8 by refocus's rule: clip, *255, round half to even.
//
// At an integer target whose only view of non-zero weight is that view, the taps are (1,0) / (0,1,0,0) exactly and the output
// equals the input view bit for bit, for fp32 and for uint8.
//
//   k_view_splat   one workgroup per (batch element, 32 x 32 target tile, target), the target fastest and the ids XCD-aware
//                  (xcd_tile): the targets of one tile read the same region of Dr.  The gather form of the splat: the workgroup
//                  reads the reach-expanded source region of Dr and reduces into the tile in LDS with atomicMax on an
//                  order-preserving integer key of d (of -d for near = smaller); 0 is no key.  No global atomics, no init pass,
//                  no dependence on arrival order.  The keys leave to the caller's scratch [B,T,H,W].
//   k_view_render  one workgroup per (batch element, 32 x 8 tile, target), one pixel per lane, a wave two rows of 32 pixels.  A lane
//                  whose key is 0 runs the fill search on the scratch keys (pre-fill values only), writes Dt and holes, then
//                  walks the records of its target: per view of non-zero weight TAPS^2 * C plain loads at the lane's own offset
//                  -- neighbouring lanes at neighbouring addresses except across depth edges --, the row pass, the column pass
//                  and the two pairs of sums in registers.  No LDS, no barrier.
// The steps shared with k_view_render_vis and k_view_fill (lft_visibility.cuh) are device functions here, each written once:
// vw_search (the farther-neighbour search of step 2, which k_disp_fill of lft_refine.cuh runs too), vw_fill (step 2 on the pre-fill
// keys, through vw_search) and vw_sample (one view at (sy, sx): vw_axis twice, the view's base, the TAPS^2 * C gather, rows
// then columns) for all of them; vw_pixel (the workgroup's id and the lane to batch element, target and pixel of a 32 x 8 tile) and
// vw_fill_store (vw_fill, then Dt and holes written) for those two.  k_view_render keeps its own pixel decode, stores and quotient:
// through the helpers it measured slower.  The two render algorithms stay two kernels.
// A pixel's bits do not depend on the tile, on the image beyond its splat sources, fill search and taps, or on the launch shape.
// They do depend on its coordinates: fl(y + fl(d*du)) rounds by the magnitude of y, so a crop away from the origin agrees with the
// whole image to a few 1e-6, not to the bit (tests/test_gpu_views.py::test_tile_independence).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lft_refocus.cuh"

namespace {

constexpr int kVwMaxReach = 64;      // largest splat reach, pixels
constexpr int kVwMaxFill = 64;       // largest fill search, pixels
constexpr int kVwRows = 8;           // rows of a render tile (its width is kRfTile)
constexpr int kVwRec = 4;            // dwords per record (lft_view_record of include/lft_hip_views.h)

struct SplatArgs {
    const float* dr;                 // [B, H, W]
    const float* deltas;             // [T, 2]  (Du, Dv)
    uint32_t* keys;                  // [B, T, H, W]
    float lo, hi;
    int neg, reach;                  // near = smaller: keys of -d
    int H, W, T, tiles_x, tiles;     // tiles of kRfTile x kRfTile
};

struct RenderArgs {
    const void* lf;
    long long st[3];                 // element strides of (b, u, v)
    int sy, sx, sc;                  // element strides of (y, x, c): a view spans less than 2^31 elements
    int A, H, W, D, tiles_x, tiles;  // D: the targets; tiles: of the splat (fill_windowed)
    const int* table;                // [T, A*A] records
    const float* dr;                 // [B, H, W]
    const uint32_t* keys;            // [B, T, H, W]
    float lo, hi;
    int neg, fill;
    int rtiles_x, rtiles;            // tiles of kRfTile x kVwRows
    void* out;                       // [B, T, H, W, C]
    int out_f32;
    float* dt;                       // [B, T, H, W]
    uint8_t* holes;                  // [B, T, H, W]
};

// finite d -> a key that orders as d does, never 0; the zeros share one key
__device__ __forceinline__ uint32_t vw_key(float d) {
    const uint32_t b = __float_as_uint(d == 0.0f ? 0.0f : d);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float vw_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ bool vw_finite(float d) { return fabsf(d) < __builtin_inff(); }

__global__ __launch_bounds__(256) void k_view_splat(SplatArgs a) {
#pragma clang fp contract(off)
    __shared__ uint32_t keys[kRfTile * kRfTile];
    const int tid = threadIdx.x;
    const int bid = xcd_tile(blockIdx.x, gridDim.x);
    const int t = bid % a.T, tile = (bid / a.T) % a.tiles, b = bid / (a.T * a.tiles);
    const int y0 = (tile / a.tiles_x) * kRfTile, x0 = (tile % a.tiles_x) * kRfTile;
    const float du = a.deltas[2 * t], dv = a.deltas[2 * t + 1];
    for (int i = tid; i < kRfTile * kRfTile; i += 256) keys[i] = 0u;
    __syncthreads();

    // the sources that can cover the tile: |fl(d*D)| <= reach - 1, and a coverer lies at floor or floor + 1
    const int ys0 = max(y0 - a.reach, 0), ys1 = min(y0 + kRfTile - 1 + a.reach, a.H - 1);
    const int xs0 = max(x0 - a.reach, 0), xs1 = min(x0 + kRfTile - 1 + a.reach, a.W - 1);
    const int nw = xs1 - xs0 + 1, n = (ys1 - ys0 + 1) * nw;
    const float* dr = a.dr + (size_t)b * a.H * a.W;
    for (int i = tid; i < n; i += 256) {
        const int y = ys0 + i / nw, x = xs0 + i % nw;
        float d = dr[(size_t)y * a.W + x];
        if (!vw_finite(d)) continue;
        d = fminf(fmaxf(d, a.lo), a.hi);
        const float py = (float)y + d * du, px = (float)x + d * dv;
        const float fy = floorf(py), fx = floorf(px);
        // a landing point further off than the caller's reach allows covers nothing here: keep the conversion in range
        if (!(fabsf(fy - (float)y0) < 4096.0f && fabsf(fx - (float)x0) < 4096.0f)) continue;
        const int ty = (int)fy - y0, tx = (int)fx - x0;
        const int na = py != fy ? 2 : 1, nb = px != fx ? 2 : 1;
        const uint32_t k = vw_key(a.neg ? -d : d);
        for (int p = 0; p < na; ++p)
            for (int q = 0; q < nb; ++q) {
                const int yy = ty + p, xx = tx + q;
                if (yy >= 0 && yy < kRfTile && xx >= 0 && xx < kRfTile && y0 + yy < a.H && x0 + xx < a.W) atomicMax(&keys[yy * kRfTile + xx], k);
            }
    }
    __syncthreads();
    uint32_t* o = a.keys + ((size_t)b * a.T + t) * a.H * a.W;
    for (int i = tid; i < kRfTile * kRfTile; i += 256) {
        const int y = y0 + i / kRfTile, x = x0 + i % kRfTile;
        if (y < a.H && x < a.W) o[(size_t)y * a.W + x] = keys[i];
    }
}

// Keys' cubic (a = -0.5) in fp32, in the factored forms that do not cancel: k(t) = 1 - t^2 (2.5 - 1.5 t) at 0 <= t <= 1, and
// k(1 + t) = -0.5 t (1 - t)^2; exactly 1 at 0 and exactly 0 at 1 and 2, and within 19 * 2^-24 of the four weights' true values in sum
// (tests/views_util.py:tol_render)
__device__ __forceinline__ float vw_keys01(float t) {
#pragma clang fp contract(off)
    return 1.0f - (t * t) * (2.5f - 1.5f * t);
}
// k(1 + t) from t and g = fl(1 - t)
__device__ __forceinline__ float vw_keys12(float t, float g) {
#pragma clang fp contract(off)
    return ((-0.5f * t) * g) * g;
}

// taps and weights of one axis at the sample position s of a view of n pixels: element offsets of the clamped taps (stride st)
template <int TAPS>
__device__ __forceinline__ void vw_axis(float s, int n, int st, int (&off)[TAPS], float (&w)[TAPS]) {
#pragma clang fp contract(off)
    const float fl = floorf(s), f = s - fl;
    const int i0 = (int)fminf(fmaxf(fl, -4.0f), (float)n + 4.0f) - (TAPS == 4 ? 1 : 0);      // beyond the clamp every tap is the border pixel
#pragma unroll
    for (int k = 0; k < TAPS; ++k) off[k] = min(max(i0 + k, 0), n - 1) * st;
    if constexpr (TAPS == 2) {
        w[0] = 1.0f - f; w[1] = f;
    } else {
        const float g = 1.0f - f;                                   // k(f + 1), k(f), k(1 - f), k(2 - f)
        w[0] = vw_keys12(f, g); w[1] = vw_keys01(f); w[2] = vw_keys01(g); w[3] = vw_keys12(g, f);
    }
}

// The farther-neighbour search of step 2, shared with k_disp_fill (lft_refine.cuh): key_at(y, x) is the key of a pixel that has a
// value and 0 of one that has none.  The nearest keyed pixel to the left and to the right in the row, each within `fill` pixels;
// if neither side has one, the same up and down the column.  Returns the farther of the two found (the smaller key for either
// `near`), the one found, or 0 for none.
template <typename KeyAt>
__device__ __forceinline__ uint32_t vw_search(KeyAt key_at, int y, int x, int H, int W, int fill) {
    uint32_t k0 = 0u, k1 = 0u;
    for (int s = 1; s <= fill && x - s >= 0 && !k0; ++s) k0 = key_at(y, x - s);
    for (int s = 1; s <= fill && x + s < W && !k1; ++s) k1 = key_at(y, x + s);
    if (!k0 && !k1) {
        for (int s = 1; s <= fill && y - s >= 0 && !k0; ++s) k0 = key_at(y - s, x);
        for (int s = 1; s <= fill && y + s < H && !k1; ++s) k1 = key_at(y + s, x);
    }
    return k0 && k1 ? min(k0, k1) : (k0 | k1);
}

// The fill of one pixel from the pre-fill keys of its target (step 2): Dt[y,x], and whether the pixel was a hole.  The farther of
// two found values has the smaller key for either `near`.  keys points at the target's plane, dr at the batch element's.
__device__ __forceinline__ float vw_fill(const uint32_t* keys, const float* dr, int y, int x, int H, int W, int fill, int neg, float lo, float hi,
                                         bool& hole) {
    uint32_t key = keys[(size_t)y * W + x];
    hole = key == 0u;
    float d;
    if (hole) {
        const uint32_t found = vw_search([&](int yy, int xx) { return keys[(size_t)yy * W + xx]; }, y, x, H, W, fill);
        if (found) {
            key = found;
            d = vw_unkey(key);
            if (neg) d = -d;
        } else {
            const float r = dr[(size_t)y * W + x];
            d = vw_finite(r) ? fminf(fmaxf(r, lo), hi) : (neg ? hi : lo);
        }
    } else {
        d = vw_unkey(key);
        if (neg) d = -d;
    }
    return d == 0.0f ? 0.0f : d;                                     // one zero
}
// Step 2 as k_view_fill and k_view_render_vis (lft_visibility.cuh) run it: vw_fill, then the two stores; dt and holes point at
// the target's plane too.  Returns Dt[y,x].
__device__ __forceinline__ float vw_fill_store(const uint32_t* keys, const float* dr, int y, int x, int H, int W, int fill, int neg, float lo, float hi,
                                               float* dt, uint8_t* holes) {
    bool hole;
    const float d = vw_fill(keys, dr, y, x, H, W, fill, neg, lo, hi, hole);
    dt[(size_t)y * W + x] = d;
    holes[(size_t)y * W + x] = hole ? 1 : 0;
    return d;
}

// This lane's pixel of a kRfTile x kVwRows tile: the workgroup's id, dealt XCD-aware, is (batch element b, tile, target t of n), the
// target fastest.  False for a lane past the image's edge.
__device__ __forceinline__ bool vw_pixel(int n, int rtiles_x, int rtiles, int H, int W, int& b, int& t, int& y, int& x) {
    const int tid = threadIdx.x;
    const int bid = xcd_tile(blockIdx.x, gridDim.x);
    const int tile = (bid / n) % rtiles;
    t = bid % n;
    b = bid / (n * rtiles);
    y = (tile / rtiles_x) * kVwRows + tid / kRfTile;
    x = (tile % rtiles_x) * kRfTile + tid % kRfTile;
    return y < H && x < W;
}

// The sample of step 3: view n of the batch element at lfb, at the position (sy, sx), into s[c].  TAPS^2 * C plain loads; per
// column tap its row pass, then its term of the column pass, every step after a sum's first product one explicit FMA.
template <typename T, int C, int TAPS>
__device__ __forceinline__ void vw_sample(const RenderArgs& a, const T* lfb, int n, float sy, float sx, float (&s)[C]) {
#pragma clang fp contract(off)
    int oy[TAPS], ox[TAPS];
    float wy[TAPS], wx[TAPS];
    vw_axis<TAPS>(sy, a.H, a.sy, oy, wy);
    vw_axis<TAPS>(sx, a.W, a.sx, ox, wx);
    const T* vb = lfb + (n / a.A) * a.st[1] + (n % a.A) * a.st[2];
#pragma unroll
    for (int k = 0; k < TAPS; ++k) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float r = wy[0] * rf_x<T>(vb[oy[0] + ox[k] + c * a.sc]);
#pragma unroll
            for (int j = 1; j < TAPS; ++j) r = __fmaf_rn(wy[j], rf_x<T>(vb[oy[j] + ox[k] + c * a.sc]), r);
            s[c] = k ? __fmaf_rn(wx[k], r, s[c]) : wx[0] * r;
        }
    }
}

template <typename T, int C, int TAPS>
__global__ __launch_bounds__(256) void k_view_render(RenderArgs a) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const int bid = xcd_tile(blockIdx.x, gridDim.x);
    const int t = bid % a.D, tile = (bid / a.D) % a.rtiles, b = bid / (a.D * a.rtiles);
    const int y = (tile / a.rtiles_x) * kVwRows + tid / kRfTile, x = (tile % a.rtiles_x) * kRfTile + tid % kRfTile;
    if (y >= a.H || x >= a.W) return;                                // no barrier below
    const size_t plane = (size_t)a.H * a.W;
    const uint32_t* keys = a.keys + ((size_t)b * a.D + t) * plane;

    bool hole;
    const float d = vw_fill(keys, a.dr + (size_t)b * plane, y, x, a.H, a.W, a.fill, a.neg, a.lo, a.hi, hole);
    const size_t o = ((size_t)b * a.D + t) * plane + (size_t)y * a.W + x;
    a.dt[o] = d;
    a.holes[o] = hole ? 1 : 0;

    // ---- render
    const int nv = a.A * a.A;
    const int* recs = a.table + (size_t)t * nv * kVwRec;
    const T* lfb = static_cast<const T*>(a.lf) + b * a.st[0];
    const float fy = (float)y, fx = (float)x, ymax = (float)(a.H - 1), xmax = (float)(a.W - 1);
    float num_in[C], num_all[C], den_in = 0.0f, den_all = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) { num_in[c] = 0.0f; num_all[c] = 0.0f; }
    for (int n = 0; n < nv; ++n) {
        if (recs[n * kVwRec + 3]) continue;                          // the same for every lane
        const float* rf = reinterpret_cast<const float*>(recs + n * kVwRec);
        const float w = rf[2];
        const float sy = fy + d * rf[0], sx = fx + d * rf[1];
        const bool inside = sy >= 0.0f && sy <= ymax && sx >= 0.0f && sx <= xmax;
        float s[C];
        vw_sample<T, C, TAPS>(a, lfb, n, sy, sx, s);
        den_all = den_all + w;
#pragma unroll
        for (int c = 0; c < C; ++c) num_all[c] = __fmaf_rn(w, s[c], num_all[c]);
        if (inside) {
            den_in = den_in + w;
#pragma unroll
            for (int c = 0; c < C; ++c) num_in[c] = __fmaf_rn(w, s[c], num_in[c]);
        }
    }
    const bool any = den_in > 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float v = any ? num_in[c] / den_in : num_all[c] / den_all;
        if (a.out_f32) static_cast<float*>(a.out)[o * C + c] = v;
        else static_cast<uint8_t*>(a.out)[o * C + c] = rf_byte(v);
    }
}

// the instantiation for an input type, channel count (1 .. 4) and tap count (2, 4)
template <typename T>
inline void (*render_kernel(int C, int taps))(RenderArgs) {
    static void (*const k[4][2])(RenderArgs) = {{k_view_render<T, 1, 2>, k_view_render<T, 1, 4>},
                                                {k_view_render<T, 2, 2>, k_view_render<T, 2, 4>},
                                                {k_view_render<T, 3, 2>, k_view_render<T, 3, 4>},
                                                {k_view_render<T, 4, 2>, k_view_render<T, 4, 4>}};
    return k[C - 1][taps == 4 ? 1 : 0];
}

}  // namespace
