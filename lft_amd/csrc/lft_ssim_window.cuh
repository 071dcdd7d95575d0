// lft_ssim_window.cuh -- the 11x11 Gaussian window of scikit-image's SSIM (sigma 1.5, sample covariance) in fp64, written once for
// k_view_metrics (26-wide input tile, 16 centres) and k_ssim_loss (36-wide, 26 centres); the geometries are template parameters.
#pragma once
#include "lft_host.cuh"         // fail(); the HIP runtime

namespace {

constexpr int kSsimR = 5, kSsimTaps = 2 * kSsimR + 1;

// exp(-k^2 / (2 sigma^2)) of tap k = -kSsimR .. kSsimR, and the weights g from the 11 of them (raw(i), i = k + kSsimR: computed in
// place or staged by the caller): summed in index order, then divided
__device__ __forceinline__ double ssim_gauss_raw(int k) { return exp(-0.5 * k * k / (1.5 * 1.5)); }
template <typename Raw> __device__ __forceinline__ void ssim_gauss(double (&g)[kSsimTaps], Raw raw) {
    double s = 0.0;
    for (int i = 0; i < kSsimTaps; ++i) { g[i] = raw(i); s += g[i]; }
    for (int i = 0; i < kSsimTaps; ++i) g[i] /= s;
}

// The five moment maps along the rows: hz[{x, y, xx, yy, xy}][r][c] = sum_k g[k] * moment(tx[r][c + k], ty[r][c + k])
template <int ROWS, int CENTRES, int PITCH, int THREADS>
__device__ __forceinline__ void ssim_moment_rows(const float (*tx)[PITCH], const float (*ty)[PITCH], double (*hz)[ROWS][CENTRES],
                                                 const double (&g)[kSsimTaps], int tid) {
    for (int i = tid; i < ROWS * CENTRES; i += THREADS) {
        const int r = i / CENTRES, c = i % CENTRES;
        double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
        for (int k = 0; k < kSsimTaps; ++k) {
            const double x = tx[r][c + k], y = ty[r][c + k];
            sx += g[k] * x; sy += g[k] * y; sxx += g[k] * x * x; syy += g[k] * y * y; sxy += g[k] * x * y;
        }
        hz[0][r][c] = sx; hz[1][r][c] = sy; hz[2][r][c] = sxx; hz[3][r][c] = syy; hz[4][r][c] = sxy;
    }
}

// The moments at the centre whose window starts at row r of column c of hz, and S = (A1 * A2) / (B1 * B2) there.
struct SsimAt { double mx, my, A1, A2, B1, B2, S; };
constexpr double kSsimCov = 121.0 / 120.0;      // sample covariance of the 11 x 11 window, as scikit-image normalises it
template <int ROWS, int CENTRES>
__device__ __forceinline__ SsimAt ssim_at(const double (*hz)[ROWS][CENTRES], int r, int c, const double (&g)[kSsimTaps], double C1, double C2) {
    double m[5] = {0, 0, 0, 0, 0};
    for (int k = 0; k < kSsimTaps; ++k)
        for (int q = 0; q < 5; ++q) m[q] += g[k] * hz[q][r + k][c];
    SsimAt s = {m[0], m[1]};
    const double vx = kSsimCov * (m[2] - s.mx * s.mx), vy = kSsimCov * (m[3] - s.my * s.my), vxy = kSsimCov * (m[4] - s.mx * s.my);
    s.A1 = 2 * s.mx * s.my + C1; s.A2 = 2 * vxy + C2; s.B1 = s.mx * s.mx + s.my * s.my + C1; s.B2 = vx + vy + C2;
    s.S = (s.A1 * s.A2) / (s.B1 * s.B2);
    return s;
}

// Host, for lft_view_metrics and lft_ssim_loss: C1, C2 and the tiles of `tile` centres per side; the refusal of smaller views
struct SsimWindow { double C1, C2; int tiles_x; long long ntiles; };
inline SsimWindow ssim_window(int h, int w, int tile, float range) {
    const int tx = (w + tile - 1) / tile;
    return {(0.01 * range) * (0.01 * range), (0.03 * range) * (0.03 * range), tx, (long long)tx * ((h + tile - 1) / tile)};
}
inline int ssim_views_ok(int h, int w) {
    return h < kSsimTaps || w < kSsimTaps ? fail(LFT_ERR_SHAPE, "views of %dx%d are smaller than the 11x11 SSIM window", h, w) : 0;
}

}  // namespace
