// lft_attn_maps.cuh -- the softmax weights of the two attentions, from the Q | K that lft_train_forward left in the tape
// (include/lft_hip.h: lft_train_attn_maps).  What nn.MultiheadAttention(need_weights=True) hands back in the reference
// (LFT.py:183-187, :230-233); the forward kernels (k_ang_attn, k_win_attn_lds) keep these weights in registers.
// Both kernels only read the tape and accumulate in fp32 with the row maximum subtracted.  The output is 8 (spatial) to V / 4
// (angular) times the Q | K read, so the results of a workgroup go through LDS or a flat element loop: every store instruction
// of a wave covers one contiguous run of the output (measured times and what bounds them: DESIGN.md section 10).
#pragma once
#include "lft_win_attn.cuh"

namespace {

// ------------------------------------------------------------------------------------------
// Angular maps.  One workgroup per pixel (b, y, x); sequence = the V views, 8 heads of 8 channels, scale 1/sqrt(8).
//   QK  : [B, V, hw][128] (Q | K), rows of one pixel are hw rows apart -- k_ang_attn's addressing
//   maps: HEADS [B*hw][8][V][V], MEAN [B*hw][V][V] (average over the heads)
// Phase 1: thread = (view i, head) as in k_ang_attn (head fastest, LDS tiles [8 heads][V * 8 + 8]): row maximum and 1 / sum.
// Phase 2: thread = output ELEMENT (i, j) of all 8 heads, consecutive lanes = consecutive elements of the flat [V * V] block, so
// every store of a wave is 256 contiguous bytes of one head's block; the 8-term dot product is recomputed from LDS (the same
// expression as in phase 1, bit for bit).
// ------------------------------------------------------------------------------------------
constexpr int kAmThreads = 256;
inline size_t ang_maps_lds(int V) { return (size_t)(2 * 8 * (V * 8 + 8) + 8 * (2 * V + 1)) * sizeof(float); }
LFT_DEV int am_div(int a, float inv_b) { return (int)(((float)a + 0.5f) * inv_b); }    // a / b for 0 <= a < 2^17, b <= 2^14: the + 0.5 keeps the quotient clear of an integer
template <bool MEAN>
__global__ __launch_bounds__(kAmThreads) void k_ang_maps(const float* __restrict__ QK, float* __restrict__ maps, int V, int hw) {
    extern __shared__ __attribute__((aligned(16))) float am_sm[];
    const int HS = V * 8 + 8, SS = 2 * V + 1;
    float* Qs = am_sm;                      // [8][HS]
    float* Ks = Qs + 8 * HS;                // [8][HS]
    float* St = Ks + 8 * HS;                // [8][SS]: (m, 1 / l) per (head, query)
    const int b = blockIdx.x / hw, pix = blockIdx.x % hw;
    const float scale2 = 0.35355339059327373f * LFT_LOG2E;            // 1 / sqrt(8), exp2 softmax (one v_exp_f32 per weight)
    // a view's row is 32 pieces of 16 bytes: 16 of Q, 16 of K; piece -> (head, half of the head's 8 channels)
    for (int idx = threadIdx.x; idx < V * 32; idx += kAmThreads) {
        const int i = idx >> 5, piece = idx & 31, c = (piece & 15) * 4;
        const long long row = ((long long)b * V + i) * hw + pix;
        const f32x4 v = load4(QK + row * 128 + piece * 4);
        *reinterpret_cast<f32x4*>((piece < 16 ? Qs : Ks) + (c >> 3) * HS + i * 8 + (c & 7)) = v;
    }
    __syncthreads();
    for (int r = threadIdx.x; r < V * 8; r += kAmThreads) {
        const int hd = r & 7, i = r >> 3;
        float q[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) q[c] = Qs[hd * HS + i * 8 + c];
        float m = -INFINITY, l = 0.0f;
        for (int j = 0; j < V; ++j) m = fmaxf(m, scale2 * dot8(q, Ks + hd * HS + j * 8));
        for (int j = 0; j < V; ++j) l += fast_exp2(scale2 * dot8(q, Ks + hd * HS + j * 8) - m);
        St[hd * SS + 2 * i] = m;
        St[hd * SS + 2 * i + 1] = 1.0f / l;
    }
    __syncthreads();
    const int VV = V * V;
    const float invV = 1.0f / (float)V;
    auto weight = [&](int hd, int i, int j) {
        float q[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) q[c] = Qs[hd * HS + i * 8 + c];
        return fast_exp2(scale2 * dot8(q, Ks + hd * HS + j * 8) - St[hd * SS + 2 * i]) * St[hd * SS + 2 * i + 1];
    };
    float* out = maps + (size_t)blockIdx.x * (MEAN ? 1 : 8) * VV;
    for (int e = threadIdx.x; e < VV; e += kAmThreads) {       // the element's (i, j) once for its 8 heads
        const int i = am_div(e, invV), j = e - i * V;
        float s = 0.0f;
#pragma unroll
        for (int hd = 0; hd < 8; ++hd) {
            const float p = weight(hd, i, j);
            if (MEAN) s += p; else out[(size_t)hd * VV + e] = p;
        }
        if (MEAN) out[e] = 0.125f * s;
    }
}

// ------------------------------------------------------------------------------------------
// Spatial (windowed) maps, compact: per query the 5 x 5 weights on the keys (y + dy - 2, x + dx - 2), exactly 0 where the key is
// outside the view or outside the reference's clamped window (LFT.py:150-160 with its min(h, x + 3) column bound); a query with an
// empty window (h < w, x - 2 >= h) gets 25 zeros -- the forward's convention (k_win_attn_lds), where torch's need_weights path has NaN.
//   QK  : [B*V, h, w][256]: Q = floats 0..127 of a row, K = 128..255
//   maps: HEADS [B*V][8][h][w][25], MEAN [B*V][h][w][25]
// Tiling, K halo staging and the thread -> query map are k_win_attn_lds's (8 x 16 queries x one head PAIR per pass, rows padded to
// 144 B, ds_read_b128 lane groups on runs of 16 queries).  HEADS: one head pair per workgroup (grid.y = 4); MEAN: the workgroup
// walks the four pairs and sums.  The weights then go through LDS (the K tile's memory, free by then) as [head of the pair][tile
// row][16 queries x 25]: a tile row's 400 floats are one contiguous run of the output, written by consecutive lanes.
// ------------------------------------------------------------------------------------------
constexpr int kWmRun = kWaTX * 25;                               // floats of one tile row of one head in the output
static_assert(2 * kWaTY * kWmRun <= kWaTile, "the staged weights must fit the K tile they replace");
LFT_DEV void wm_stage(const float* __restrict__ K, float* lds, long long img0, int y0, int x0, int hp, int h, int w) {
    constexpr int NIT = (kWaSlots * 8 + 255) / 256;
    f32x4 va[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {                               // every piece requested before the first LDS write (wa_stage2)
        const int idx = min((int)threadIdx.x + 256 * i, kWaSlots * 8 - 1);
        const int slot = idx >> 3, piece = idx & 7;
        const int gy = y0 - 2 + slot / kWaHC, gx = x0 - 2 + slot % kWaHC;
        const bool in = gy >= 0 && gy < h && gx >= 0 && gx < w;
        va[i] = load4(K + (size_t)(in ? img0 + gy * w + gx : img0) * 256 + hp * 32 + piece * 4);
    }
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        const int idx = (int)threadIdx.x + 256 * i;
        const int slot = idx >> 3, piece = idx & 7;
        const int gy = y0 - 2 + slot / kWaHC, gx = x0 - 2 + slot % kWaHC;
        const bool in = gy >= 0 && gy < h && gx >= 0 && gx < w;
        if (idx < kWaSlots * 8) *reinterpret_cast<f32x4*>(lds + slot * kWaRow + piece * 4) = in ? va[i] : f32x4{0, 0, 0, 0};
    }
}
template <bool MEAN>
__global__ __launch_bounds__(256) void k_win_maps(const float* __restrict__ QK, float* __restrict__ maps, int h, int w) {
    __shared__ __attribute__((aligned(16))) float tK[kWaTile];
    const int tiles_x = (w + kWaTX - 1) / kWaTX, tiles_y = (h + kWaTY - 1) / kWaTY;
    const int bid = xcd_tile(blockIdx.x, gridDim.x);
    const int tx = bid % tiles_x, ty = (bid / tiles_x) % tiles_y, im = bid / (tiles_x * tiles_y);
    const int y0 = ty * kWaTY, x0 = tx * kWaTX;
    const long long img0 = (long long)im * h * w;
    const int hl = threadIdx.x >> 7, qi = (threadIdx.x & 96) + ldsb128_pos(threadIdx.x & 31), qy = qi >> 4, qx = qi & 15;
    const int y = y0 + qy, x = x0 + qx;
    const long long tok = img0 + min(y, h - 1) * w + min(x, w - 1);
    const int wy0 = max(0, y - 2), wy1 = min(h, y + 3), wx0 = max(0, x - 2), wx1 = min(min(h, x + 3), w);   // LFT.py:150-160 (sic)
    const float scale2 = 0.25f * LFT_LOG2E;                            // 1 / sqrt(16), exp2 softmax
    const float* bK = tK + (qy * kWaHC + qx) * kWaRow + hl * 16;
    float p[25];
#pragma unroll
    for (int t = 0; t < 25; ++t) p[t] = 0.0f;
    const int hp0 = MEAN ? 0 : blockIdx.y, hp1 = MEAN ? 4 : blockIdx.y + 1;
    for (int hp = hp0; hp < hp1; ++hp) {
        float q[16], kv[16], sc[25];
        ld16(QK + (size_t)tok * 256 + hp * 32 + hl * 16, q);
        if (hp != hp0) __syncthreads();                                // the previous pair's reads of the tile are done
        wm_stage(QK + 128, tK, img0, y0, x0, hp, h, w);
        __syncthreads();
        float m = -INFINITY;
#pragma unroll
        for (int t = 0; t < 25; ++t) {
            const int ky = y - 2 + t / 5, kx = x - 2 + t % 5;
            const bool ok = ky >= wy0 && ky < wy1 && kx >= wx0 && kx < wx1;
            lds16(bK + ((t / 5) * kWaHC + t % 5) * kWaRow, kv);
            sc[t] = ok ? scale2 * dot16(q, kv) : -INFINITY;
            m = fmaxf(m, sc[t]);
        }
        if (m == -INFINITY) m = 0.0f;                                  // empty window: all weights 0
        float l = 0.0f;
#pragma unroll
        for (int t = 0; t < 25; ++t) { sc[t] = fast_exp2(sc[t] - m); l += sc[t]; }     // exp2(-inf) = 0: exactly 0 outside the window
        const float inv = l > 0.0f ? 1.0f / l : 0.0f;
#pragma unroll
        for (int t = 0; t < 25; ++t) p[t] += sc[t] * inv;
    }
    __syncthreads();                                                   // all reads of the K tile are done: it becomes the output stage
    float* stg = tK + (hl * kWaTY + qy) * kWmRun + qx * 25;            // 25 floats per query: odd stride, lanes on distinct banks
#pragma unroll
    for (int t = 0; t < 25; ++t) stg[t] = p[t];
    __syncthreads();
    const int run = min(kWaTX, w - x0) * 25;                           // floats of a tile row that are inside the view
    const size_t rowf = (size_t)w * 25;
    if (MEAN) {
        for (int idx = threadIdx.x; idx < kWaTY * kWmRun; idx += 256) {
            const int ry = idx / kWmRun, k = idx % kWmRun;
            if (y0 + ry < h && k < run)
                maps[((size_t)im * h + y0 + ry) * rowf + (size_t)x0 * 25 + k] = 0.125f * (tK[idx] + tK[kWaTY * kWmRun + idx]);
        }
    } else {
        for (int idx = threadIdx.x; idx < 2 * kWaTY * kWmRun; idx += 256) {
            const int hh = idx / (kWaTY * kWmRun), ry = (idx / kWmRun) % kWaTY, k = idx % kWmRun;
            if (y0 + ry < h && k < run)
                maps[(((size_t)im * 8 + blockIdx.y * 2 + hh) * h + y0 + ry) * rowf + (size_t)x0 * 25 + k] = tK[idx];
        }
    }
}

}  // namespace
