// lft_lightfield.hip -- what handles light fields around the network, in the C ABI of liblft_hip.so (include/lft_hip.h): scene
// tiling, dihedral transforms and self-ensemble, view metrics, data preparation, the colour path, refocus, disparity, view
// synthesis (declared in include/lft_hip_views.h), semi-global aggregation (declared in include/lft_hip_sgm.h), the sweep's
// occlusion-aware cost (declared in include/lft_hip_occlusion.h), the all-in-focus image from the winning partial aperture
// (declared in include/lft_hip_aif.h), scene tiling with a per-patch integer shear (declared in include/lft_hip_shear.h),
// windowed blending of overlapping SR patches (declared in include/lft_hip_blend.h), angular tiling of a U x V field (declared in
// include/lft_hip_field.h) and the refinement of a selected disparity map (declared in include/lft_hip_refine.h).
#include "lft_host.cuh"
#include "../../include/lft_hip_views.h"
#include "../../include/lft_hip_sgm.h"
#include "../../include/lft_hip_visibility.h"
#include "../../include/lft_hip_occlusion.h"
#include "../../include/lft_hip_aif.h"
#include "../../include/lft_hip_shear.h"
#include "../../include/lft_hip_blend.h"
#include "../../include/lft_hip_field.h"
#include "../../include/lft_hip_refine.h"
#include "lft_scene.cuh"     // scene tiling: divide into patch mosaics, integrate
#include "lft_shear.cuh"     // scene tiling with a per-patch integer shear, the vote that chooses it (lft_scene_divide_shear, lft_shear_vote)
#include "lft_blend.cuh"     // windowed blending of overlapping SR patches into the SR scene (lft_scene_integrate_blend)
#include "lft_field.cuh"     // angular tiling: A x A windows over a U x V field, cut and put together (lft_field_divide, lft_field_integrate)
#include "lft_metrics.cuh"
#include "lft_prepare.cuh"    // data preparation (reference Generate_Data_for_*.m)
#include "lft_ensemble.cuh"  // dihedral transforms: self-ensemble expand / merge / fused scene integrate, per-sample augmentation
#include "lft_colour.cuh"    // colour path: RGB light field -> Y mosaic; SR Y + up-scaled chroma -> RGB views
#include "lft_refocus.cuh"   // synthetic refocus: focal stack by shift-and-add over the views (lft_refocus)
#include "lft_disparity.cuh" // disparity: plane-sweep cost volume, windowed aggregation, winner-take-all (lft_disparity)
#include "lft_views.cuh"     // view synthesis: splat the disparity to the target, fill, gather the views (lft_view_render)
#include "lft_visibility.cuh" // view synthesis with a per-view visibility test, the warp of a map to other positions (lft_view_render_visible)
#include "lft_sgm.cuh"       // semi-global aggregation of a cost volume: the path scans, the sum and the selection (lft_sgm)
#include "lft_occlusion.cuh" // the sweep's cost from partial apertures: min over the whole aperture and up to four subsets (lft_disparity_occ)
#include "lft_aif.cuh"       // the all-in-focus image from the winning partial aperture: one gather pass over the views (lft_aif_at)
#include "lft_refine.cuh"    // refinement of a selected map: cross-view check, farther-neighbour fill, guided weighted median (lft_disp_*)

namespace {

// ---- the light field [U,V,H,W,C] with five strides (data preparation, colour path); nothing is launched when a check fails ----
// The array itself: pointers, stored class, sizes, strides.  `shape` is the code of a bad size: lft_lf_prepare has always answered
// LFT_ERR_ARG there, the colour path LFT_ERR_SHAPE.
int lf_array_ok(const char* who, int shape, const void* lf, int lf_class, int U, int V, int H, int W, int C, const long long* strides) {
    if (!lf || !strides) return fail(LFT_ERR_ARG, "%s: null pointer", who);
    if (lf_class != LFT_LF_UINT8 && lf_class != LFT_LF_FLOAT32 && lf_class != LFT_LF_FLOAT64)
        return fail(LFT_ERR_ARG, "%s: light-field class must be LFT_LF_UINT8, LFT_LF_FLOAT32 or LFT_LF_FLOAT64, got %d", who, lf_class);
    if (U < 1 || V < 1 || H < 1 || W < 1 || C < 3)
        return fail(shape, "%s: light field [%d,%d,%d,%d,%d] needs positive sizes and at least 3 channels", who, U, V, H, W, C);
    for (int i = 0; i < 5; ++i)
        if (strides[i] < 0) return fail(LFT_ERR_ARG, "%s: stride %d is negative (%lld)", who, i, strides[i]);
    return 0;
}
// Its centre A x A views.  `index`: what the message calls the centre-view index ("the scripts' centre-view index" for
// lft_lf_prepare, which follows the MATLAB scripts).  A separate step because lft_lf_prepare checks its scale factor in between.
int centre_views_ok(const char* who, int shape, const char* index, int U, int V, int A) {
    if (A < 1 || A > U || A > V) return fail(shape, "%s: angRes %d outside the %d x %d views", who, A, U, V);
    if ((U - A) % 2 || (V - A) % 2)
        return fail(shape, "%s: U-A = %d and V-A = %d must be even (%s 0.5*(U-A+2) is not an integer)", who, U - A, V - A, index);
    return 0;
}
// what lft_lf_luma and lft_colour_merge ask of the light field: both of the above, and a grid with one y block per view
int colour_lf_ok(const char* who, const void* lf, int lf_class, int U, int V, int H, int W, int C, const long long* strides, int A) {
    if (int rc = lf_array_ok(who, LFT_ERR_SHAPE, lf, lf_class, U, V, H, W, C, strides)) return rc;
    if (int rc = centre_views_ok(who, LFT_ERR_SHAPE, "the centre-view index", U, V, A)) return rc;
    if (A > 255) return fail(LFT_ERR_SHAPE, "%s: angRes %d needs more than 65535 blocks in the grid's y", who, A);
    return 0;
}
template <typename Args> void fill_centre_views(Args& a, const void* lf, const long long* strides, int U, int V, int A) {   // Prep-, Luma-, ColourArgs
    for (int i = 0; i < 5; ++i) a.st[i] = strides[i];
    a.lf = lf; a.u0 = (U - A) / 2; a.v0 = (V - A) / 2; a.A = A;
}
int taps_ok(const char* who, int taps_h, int taps_w, int limit) {       // the taps per output of the caller's two tables
    return taps_h < 1 || taps_w < 1 || taps_h > limit || taps_w > limit ? fail(LFT_ERR_ARG, "%s: %d / %d taps per output (1 .. %d)", who, taps_h, taps_w, limit) : 0;
}
// ---- B light fields [B,A,A,H,W,C] read in place through six strides, one 32 x 32 output tile per workgroup (refocus, disparity,
// view synthesis with its targets in the place of the slopes) ----
struct WindowedLf {         // the arguments lft_refocus, lft_disparity and lft_view_render share, and what windowed_lf_ok derives from them
    const void* lf; int lf_class, B, A, H, W, C; const long long* strides; const void* table; int D, taps;
    long long tiles_x, tiles;           // kRfTile tiles of a view; tiles == 0: an empty shape, no work and no error
};
int too_many_blocks(const char* who, const WindowedLf& l, const char* work) {
    return fail(LFT_ERR_SHAPE, "%s: %d %s of %d slopes over views of %d x %d need more than 2^31 blocks", who, l.B, work, l.D, l.H, l.W);
}
// Every check the two entry points share, in the order they have always made them; nothing is launched when one fails.  The caller's
// own arguments sit in between: `out_class` (called `out_name` in the message), `radius` (lft_disparity only; 0 for lft_refocus),
// `own_null` (one of the caller's other pointers is null).  `work`: what too_many_blocks calls the B batches.
int windowed_lf_ok(const char* who, WindowedLf& l, int out_class, const char* out_name, int radius, bool own_null, const char* work) {
    if (l.lf_class != LFT_LF_UINT8 && l.lf_class != LFT_LF_FLOAT32)
        return fail(LFT_ERR_ARG, "%s: light-field class must be LFT_LF_UINT8 or LFT_LF_FLOAT32, got %d", who, l.lf_class);
    if (out_class != LFT_LF_UINT8 && out_class != LFT_LF_FLOAT32)
        return fail(LFT_ERR_ARG, "%s: %s class must be LFT_LF_UINT8 or LFT_LF_FLOAT32, got %d", who, out_name, out_class);
    if (l.A < 1 || l.A > 4096) return fail(LFT_ERR_ARG, "%s: angRes %d outside 1 .. 4096", who, l.A);      // A*A records indexed in int
    if (l.C < 1 || l.C > 4) return fail(LFT_ERR_ARG, "%s: %d channels (1 .. 4)", who, l.C);
    if (l.taps != 1 && l.taps != 2 && l.taps != 4) return fail(LFT_ERR_ARG, "%s: %d taps (1, 2 or 4)", who, l.taps);
    if (l.D < 1) return fail(LFT_ERR_ARG, "%s: %d slopes", who, l.D);
    if (radius < 0 || radius > kDpMaxR) return fail(LFT_ERR_ARG, "%s: radius %d outside 0 .. %d", who, radius, kDpMaxR);
    if (l.B < 0 || l.H < 0 || l.W < 0) return fail(LFT_ERR_SHAPE, "%s: negative size in B = %d, views of %d x %d", who, l.B, l.H, l.W);
    l.tiles_x = l.tiles = 0;
    if (l.B == 0 || l.H == 0 || l.W == 0) return 0;                 // nothing to read or write
    if (!l.lf || !l.strides || !l.table || own_null) return fail(LFT_ERR_ARG, "%s: null pointer", who);
    for (int i = 0; i < 6; ++i)
        if (l.strides[i] < 0) return fail(LFT_ERR_ARG, "%s: stride %d is negative (%lld)", who, i, l.strides[i]);
    if ((double)(l.H - 1) * (double)l.strides[3] + (double)(l.W - 1) * (double)l.strides[4] + (double)(l.C - 1) * (double)l.strides[5] > 2147483647.0)
        return fail(LFT_ERR_SHAPE, "%s: a view of %d x %d x %d with these strides spans more than 2^31 elements", who, l.H, l.W, l.C);
    l.tiles_x = ((long long)l.W + kRfTile - 1) / kRfTile;
    l.tiles = l.tiles_x * (((long long)l.H + kRfTile - 1) / kRfTile);
    if (l.tiles * l.D * l.B > 0x7fffffffLL) return too_many_blocks(who, l, work);
    return 0;
}
// the members RefocusArgs and SweepArgs have in common
template <typename Args> void fill_windowed(Args& a, const WindowedLf& l) {
    a.lf = l.lf;
    for (int i = 0; i < 3; ++i) a.st[i] = l.strides[i];
    a.sy = (int)l.strides[3]; a.sx = (int)l.strides[4]; a.sc = (int)l.strides[5];
    a.A = l.A; a.H = l.H; a.W = l.W; a.D = l.D; a.tiles_x = (int)l.tiles_x; a.tiles = (int)l.tiles;
    a.table = static_cast<const int*>(l.table);
}

}  // namespace

// ================================================================================ C ABI
extern "C" {

static int scene_counts(int h0, int w0, int patch, int stride, int* nu, int* nv) {
    if (h0 < 1 || w0 < 1 || patch < 1 || stride < 1 || stride > patch) return fail(LFT_ERR_SHAPE, "bad scene tiling (h0=%d w0=%d patch=%d stride=%d)", h0, w0, patch, stride);
    const int bdr = (patch - stride) / 2, h = h0 + 2 * bdr, w = w0 + 2 * bdr;
    if (h < patch || w < patch) return fail(LFT_ERR_SHAPE, "view %dx%d is smaller than one patch after extension", h0, w0);
    *nu = (h - patch) / stride + ((h - patch) % stride ? 2 : 1);
    *nv = (w - patch) / stride + ((w - patch) % stride ? 2 : 1);
    return 0;
}
int lft_scene_counts(int h0, int w0, int patch, int stride, int* num_u, int* num_v) {
    if (!num_u || !num_v) return fail(LFT_ERR_ARG, "null pointer");
    return scene_counts(h0, w0, patch, stride, num_u, num_v);
}
int lft_scene_divide(const float* scene, float* patches, int A, int h0, int w0, int patch, int stride, void* stream) {
    int nu, nv, rc;
    if (!scene || !patches || A < 1) return fail(LFT_ERR_ARG, "bad argument");
    if ((rc = scene_counts(h0, w0, patch, stride, &nu, &nv))) return rc;
    const dim3 grid((unsigned)((A * patch + 255) / 256), (unsigned)(A * patch), (unsigned)(nu * nv));
    k_scene_divide<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(scene, patches, A, h0, w0, patch, stride, nv);
    LFT_LAUNCH_OK("k_scene_divide");
    return 0;
}
int lft_scene_integrate(const float* sr_patches, float* sr_scene, int A, int h0, int w0, int patch, int stride, int s, void* stream) {
    int nu, nv, rc;
    if (!sr_patches || !sr_scene || A < 1 || s < 1) return fail(LFT_ERR_ARG, "bad argument");
    if ((rc = scene_counts(h0, w0, patch, stride, &nu, &nv))) return rc;
    const dim3 grid((unsigned)((A * w0 * s + 255) / 256), (unsigned)(A * h0 * s));
    k_scene_integrate<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(sr_patches, sr_scene, A, patch * s, stride * s, h0 * s, w0 * s, nv);
    LFT_LAUNCH_OK("k_scene_integrate");
    return 0;
}

// ---- dihedral transforms (lft_ensemble.cuh) ----
static int dihedral_args(const void* in, const void* out, unsigned mask, int B, int H, int W, int* E, unsigned* blocks) {
    if (!in || !out) return fail(LFT_ERR_ARG, "null pointer");
    if (in == out) return fail(LFT_ERR_ARG, "the transforms do not work in place (in == out)");
    if (mask == 0 || mask > 0xFFu) return fail(LFT_ERR_ARG, "mask 0x%x: one bit per dihedral code 0..7, at least one set", mask);
    if (B < 1 || H < 1 || W < 1) return fail(LFT_ERR_SHAPE, "bad image batch (B=%d H=%d W=%d)", B, H, W);
    *E = __builtin_popcount(mask);
    const unsigned long long n = (unsigned long long)B * (unsigned long long)((H + DH_TILE - 1) / DH_TILE) * (unsigned long long)((W + DH_TILE - 1) / DH_TILE);
    if (n * 8ull > 0x7fffffffull) return fail(LFT_ERR_SHAPE, "batch of %d images of %dx%d needs more than 2^31 blocks", B, H, W);
    *blocks = (unsigned)n;
    return 0;
}
int lft_dihedral_batch(const float* in, float* out, const int* codes, int B, int H, int W, void* stream) {
    int E, rc; unsigned blocks;
    if (!codes) return fail(LFT_ERR_ARG, "null pointer");
    if ((rc = dihedral_args(in, out, 1u, B, H, W, &E, &blocks))) return rc;
    k_dihedral<<<blocks, 256, 0, static_cast<hipStream_t>(stream)>>>(in, out, codes, 1u, 1, H, W);
    LFT_LAUNCH_OK("k_dihedral");
    return 0;
}
int lft_dihedral_expand(const float* in, float* out, unsigned mask, int B, int H, int W, void* stream) {
    int E, rc; unsigned blocks;
    if ((rc = dihedral_args(in, out, mask, B, H, W, &E, &blocks))) return rc;
    k_dihedral<<<blocks * (unsigned)E, 256, 0, static_cast<hipStream_t>(stream)>>>(in, out, nullptr, mask, E, H, W);
    LFT_LAUNCH_OK("k_dihedral");
    return 0;
}
int lft_dihedral_merge(const float* in, float* out, unsigned mask, int B, int H, int W, void* stream) {
    int E, rc; unsigned blocks;
    if ((rc = dihedral_args(in, out, mask, B, H, W, &E, &blocks))) return rc;
    k_dihedral_merge<<<blocks, 256, 0, static_cast<hipStream_t>(stream)>>>(in, out, mask, E, H, W);
    LFT_LAUNCH_OK("k_dihedral_merge");
    return 0;
}
int lft_scene_integrate_ens(const float* sr_variants, float* sr_scene, unsigned mask, int A, int h0, int w0, int patch, int stride, int s,
                            void* stream) {
    int nu, nv, rc;
    if (!sr_variants || !sr_scene) return fail(LFT_ERR_ARG, "null pointer");
    if (sr_variants == sr_scene) return fail(LFT_ERR_ARG, "the merge does not work in place (in == out)");
    if (mask == 0 || mask > 0xFFu) return fail(LFT_ERR_ARG, "mask 0x%x: one bit per dihedral code 0..7, at least one set", mask);
    if (A < 1 || s < 1) return fail(LFT_ERR_SHAPE, "bad scene (A=%d s=%d)", A, s);
    if ((rc = scene_counts(h0, w0, patch, stride, &nu, &nv))) return rc;
    // the variants are A*patch*s square mosaics by construction, so a transposing code needs no further shape check
    const int S = stride * s, ts = (S + DH_TILE - 1) / DH_TILE;
    const unsigned long long n = (unsigned long long)nu * nv * A * A * ts * ts;
    if (n > 0x7fffffffull) return fail(LFT_ERR_SHAPE, "scene needs more than 2^31 blocks");
    k_scene_integrate_ens<<<(unsigned)n, 256, 0, static_cast<hipStream_t>(stream)>>>(sr_variants, sr_scene, mask, __builtin_popcount(mask),
                                                                                    A, patch * s, S, h0 * s, w0 * s, nv);
    LFT_LAUNCH_OK("k_scene_integrate_ens");
    return 0;
}

// ================================================================================ metrics
int lft_view_metrics_scratch_bytes(int B, int A, int h, int w, size_t* out_bytes) {
    if (!out_bytes || B < 1 || A < 1 || h < 1 || w < 1) return fail(LFT_ERR_ARG, "bad argument");
    *out_bytes = (size_t)B * A * A * (size_t)ssim_window(h, w, kMetTile, 1.0f).ntiles * 3 * sizeof(double);
    return 0;
}
int lft_view_metrics(const float* label, const float* out, int B, int A, int h, int w, float ssim_range, float* psnr, float* ssim,
                     void* scratch, void* stream) {
    if (!label || !out || !psnr || !ssim || !scratch || B < 1 || A < 1) return fail(LFT_ERR_ARG, "bad argument");
    if (int rc = ssim_views_ok(h, w)) return rc;
    const SsimWindow win = ssim_window(h, w, kMetTile, ssim_range);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int ntiles = (int)win.ntiles, nviews = B * A * A;
    k_view_metrics<<<dim3((unsigned)ntiles, (unsigned)nviews), 256, 0, st>>>(label, out, static_cast<double*>(scratch), A, h, w, win.C1, win.C2);
    LFT_LAUNCH_OK("k_view_metrics");
    k_view_metrics_final<<<blocks_for(nviews, 64), 64, 0, st>>>(static_cast<const double*>(scratch), nviews, ntiles, h, w, psnr, ssim);
    LFT_LAUNCH_OK("k_view_metrics_final");
    return 0;
}
int lft_lf_prepare(const void* lf, int lf_class, int U, int V, int H, int W, int C, const long long* strides, int A, int s,
                   const int* crops, int n_crops, int crop_h, int crop_w, const double* weights_h, const int* indices_h, int taps_h,
                   const double* weights_w, const int* indices_w, int taps_w, float* hr, float* lr, void* stream) {
    if (!crops || !weights_h || !indices_h || !weights_w || !indices_w || !hr || !lr) return fail(LFT_ERR_ARG, "lft_lf_prepare: null pointer");
    if (int rc = lf_array_ok("lft_lf_prepare", LFT_ERR_ARG, lf, lf_class, U, V, H, W, C, strides)) return rc;
    if (s != 2 && s != 4) return fail(LFT_ERR_ARG, "lft_lf_prepare: scale factor must be 2 or 4, got %d", s);
    if (int rc = centre_views_ok("lft_lf_prepare", LFT_ERR_ARG, "the scripts' centre-view index", U, V, A)) return rc;
    if (n_crops < 0 || crop_h < 1 || crop_w < 1 || crop_h > H || crop_w > W)
        return fail(LFT_ERR_ARG, "lft_lf_prepare: %d crops of %d x %d in views of %d x %d", n_crops, crop_h, crop_w, H, W);
    for (int i = 0; i < n_crops; ++i) {
        const int y0 = crops[2 * i], x0 = crops[2 * i + 1];
        if (y0 < 0 || x0 < 0 || y0 > H - crop_h || x0 > W - crop_w)
            return fail(LFT_ERR_ARG, "lft_lf_prepare: crop %d at (%d, %d) of %d x %d is outside the %d x %d view", i, y0, x0, crop_h, crop_w, H, W);
    }
    if (int rc = taps_ok("lft_lf_prepare", taps_h, taps_w, kPrepMaxTaps)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    PrepArgs a{};
    fill_centre_views(a, lf, strides, U, V, A);
    a.s = s; a.ch = crop_h; a.cw = crop_w; a.oh = (crop_h + s - 1) / s; a.ow = (crop_w + s - 1) / s; a.ph = taps_h; a.pw = taps_w;
    a.wh = weights_h; a.ih = indices_h; a.ww = weights_w; a.iw = indices_w; a.hr = hr; a.lr = lr;
    const int TO = kPrepTileHr / s;
    const unsigned tiles = (unsigned)(((a.oh + TO - 1) / TO) * ((a.ow + TO - 1) / TO));
    for (int n0 = 0; n0 < n_crops; n0 += kPrepCrops) {
        const int nb = std::min(kPrepCrops, n_crops - n0);
        PrepCrops c{};
        for (int i = 0; i < nb; ++i) { c.y0[i] = crops[2 * (n0 + i)]; c.x0[i] = crops[2 * (n0 + i) + 1]; }
        a.n0 = n0;
        const dim3 grid(tiles, (unsigned)(A * A), (unsigned)nb);
        by_lf_class(lf_class, [&](auto t) { k_lf_prepare<decltype(t)><<<grid, 256, 0, st>>>(a, c); return 0; });
        LFT_LAUNCH_OK("k_lf_prepare");
    }
    return 0;
}

// ---- colour path (lft_colour.cuh) ----
int lft_lf_luma(const void* lf, int lf_class, int U, int V, int H, int W, int C, const long long* strides, int A, float* y_out,
                void* stream) {
    if (!y_out) return fail(LFT_ERR_ARG, "lft_lf_luma: null pointer");
    if (int rc = colour_lf_ok("lft_lf_luma", lf, lf_class, U, V, H, W, C, strides, A)) return rc;
    const long long blocks = ((long long)H * W + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(LFT_ERR_SHAPE, "lft_lf_luma: views of %d x %d need more than 2^31 blocks", H, W);
    LumaArgs a{};
    fill_centre_views(a, lf, strides, U, V, A);
    a.H = H; a.W = W; a.y = y_out;
    const dim3 grid((unsigned)blocks, (unsigned)(A * A));
    by_lf_class(lf_class, [&](auto t) { k_lf_luma<decltype(t)><<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(a); return 0; });
    LFT_LAUNCH_OK("k_lf_luma");
    return 0;
}

int lft_colour_merge(const void* lf, int lf_class, int U, int V, int H, int W, int C, const long long* strides, int A, int s,
                     const float* sr_y, const double* weights_h, const int* indices_h, int taps_h, const double* weights_w,
                     const int* indices_w, int taps_w, const double* minv, void* out, int out_class, void* stream) {
    if (!weights_h || !indices_h || !weights_w || !indices_w || !minv || !out) return fail(LFT_ERR_ARG, "lft_colour_merge: null pointer");
    if (int rc = colour_lf_ok("lft_colour_merge", lf, lf_class, U, V, H, W, C, strides, A)) return rc;
    if (s != 2 && s != 4) return fail(LFT_ERR_SHAPE, "lft_colour_merge: scale factor must be 2 or 4, got %d", s);
    if (int rc = taps_ok("lft_colour_merge", taps_h, taps_w, kColMaxTaps)) return rc;
    if (out_class != LFT_LF_UINT8 && out_class != LFT_LF_FLOAT32)
        return fail(LFT_ERR_ARG, "lft_colour_merge: output class must be LFT_LF_UINT8 or LFT_LF_FLOAT32, got %d", out_class);
    const long long tiles = (((long long)s * H + kColTile - 1) / kColTile) * (((long long)s * W + kColTile - 1) / kColTile);
    if ((long long)s * H > 0x7fffffffLL || (long long)s * W > 0x7fffffffLL || tiles > 0x7fffffffLL)
        return fail(LFT_ERR_SHAPE, "lft_colour_merge: views of %d x %d at %dx need more than 2^31 blocks", H, W, s);
    ColourArgs a{};
    fill_centre_views(a, lf, strides, U, V, A);
    a.s = s; a.H = H; a.W = W; a.ph = taps_h; a.pw = taps_w;
    a.sr_y = sr_y; a.wh = weights_h; a.ih = indices_h; a.ww = weights_w; a.iw = indices_w;
    for (int i = 0; i < 9; ++i) a.minv[i] = minv[i];
    a.out = out; a.out_f32 = out_class == LFT_LF_FLOAT32;
    const dim3 grid((unsigned)tiles, (unsigned)(A * A));
    by_lf_class(lf_class, [&](auto t) { k_colour_merge<decltype(t)><<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(a); return 0; });
    LFT_LAUNCH_OK("k_colour_merge");
    return 0;
}

// ---- synthetic refocus (lft_refocus.cuh) ----
int lft_refocus(const void* lf, int lf_class, int B, int A, int H, int W, int C, const long long* strides, const void* table, int D,
                int taps, void* out, int out_class, void* stream) {
    WindowedLf l{lf, lf_class, B, A, H, W, C, strides, table, D, taps, 0, 0};
    if (int rc = windowed_lf_ok("lft_refocus", l, out_class, "output", 0, !out, "stacks")) return rc;
    if (!l.tiles) return 0;                                         // an empty stack
    RefocusArgs a{};
    fill_windowed(a, l);
    a.out = out; a.out_f32 = out_class == LFT_LF_FLOAT32;
    const dim3 grid((unsigned)(l.tiles * D * B));
    by_lf_class<false>(lf_class, [&](auto t) { refocus_kernel<decltype(t)>(C, taps)<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(a); return 0; });
    LFT_LAUNCH_OK("k_refocus");
    return 0;
}

// ---- disparity from a plane sweep (lft_disparity.cuh) ----
// the floats of V [B, D, H, W] (and of m [B, D, H, W, C] behind it): 0 when they do not fit 2^40 bytes
static size_t disparity_floats(int B, int D, int H, int W, int C, int flags, size_t* vol_floats) {
    const double vol = (double)B * D * H * W, all = vol * (flags & LFT_DISPARITY_AIF ? 1 + C : 1);
    if (all * 4.0 > 1099511627776.0) return 0;
    *vol_floats = (size_t)B * D * H * W;
    return *vol_floats * (size_t)(flags & LFT_DISPARITY_AIF ? 1 + C : 1);
}
// The body of the two scratch-size queries.  `who` starts every message; with_choice: the bytes of the choice volume [B, D, H, W]
// behind the floats, rounded up to whole dwords.
static int disparity_scratch_bytes(const char* who, bool with_choice, int B, int D, int H, int W, int C, int flags, size_t* out_bytes) {
    if (!out_bytes) return fail(LFT_ERR_ARG, "%s: out_bytes is null", who);
    if (C < 1 || C > 4) return fail(LFT_ERR_ARG, "%s: %d channels (1 .. 4)", who, C);
    if (D < 1) return fail(LFT_ERR_ARG, "%s: %d slopes", who, D);
    if (flags & ~LFT_DISPARITY_AIF) return fail(LFT_ERR_ARG, "%s: unknown flags 0x%x", who, flags);
    if (B < 0 || H < 0 || W < 0) return fail(LFT_ERR_SHAPE, "%s: negative size in B = %d, views of %d x %d", who, B, H, W);
    size_t vol = 0;
    const size_t n = disparity_floats(B, D, H, W, C, flags, &vol);
    if (!n && B && H && W) return fail(LFT_ERR_SHAPE, "%s: the cost volume of %d x %d x %d x %d needs more than 2^40 bytes", who, B, D, H, W);
    *out_bytes = n * sizeof(float) + (with_choice && n ? (vol + 3) / 4 * 4 : 0);
    return 0;
}
int lft_disparity_scratch_bytes(int B, int D, int H, int W, int C, int flags, size_t* out_bytes) {
    return disparity_scratch_bytes("lft_disparity", false, B, D, H, W, C, flags, out_bytes);
}
// k_occ_gather over the B * H * W pixels, one per lane of `blocks` workgroups (lft_occlusion.cuh)
static int enqueue_occ_gather(const int* index, const unsigned char* choice, unsigned char* subset, int B, int D, int H, int W, long long blocks, hipStream_t st) {
    const OccGatherArgs g{index, choice, subset, D, (size_t)H * W, (size_t)B * H * W};
    k_occ_gather<<<dim3((unsigned)blocks), 256, 0, st>>>(g);
    LFT_LAUNCH_OK("k_occ_gather");
    return 0;
}
// What lft_disparity_occ adds to lft_disparity's arguments (lft_occlusion.cuh; declared in include/lft_hip_occlusion.h).
struct OccAdds { const float* subsets; int P; float beta; unsigned char* subset; unsigned char* choice; };
// The body of lft_disparity (occ == nullptr) and lft_disparity_occ: the checks in the order each has always made them, the sweep
// of its kind, k_disparity_pick, and k_occ_gather when `subset` is asked for.  `who` starts every message.
static int sweep_and_pick(const char* who, const OccAdds* occ, const void* lf, int lf_class, int B, int A, int H, int W, int C, const long long* strides,
                          const void* table, const float* slopes, int D, int taps, int radius, void* scratch, float* disparity, float* confidence,
                          int* index, float* cost, void* aif, int aif_class, void* stream) {
    WindowedLf l{lf, lf_class, B, A, H, W, C, strides, table, D, taps, 0, 0};
    const bool own_null = (occ && !occ->subsets) || !slopes || !scratch || !disparity || !confidence || !index;
    if (int rc = windowed_lf_ok(who, l, aif_class, "all-in-focus", radius, own_null, "sweeps")) return rc;
    if (occ && (occ->P < 1 || occ->P > LFT_OCC_MAX_SUBSETS)) return fail(LFT_ERR_ARG, "%s: %d subsets outside 1 .. %d", who, occ->P, LFT_OCC_MAX_SUBSETS);
    if (occ && (!std::isfinite(occ->beta) || occ->beta < 1.0f)) return fail(LFT_ERR_ARG, "%s: margin %g must be finite and >= 1", who, occ->beta);
    if (!l.tiles) return 0;                                         // empty maps
    const long long ptiles_x = ((long long)W + kDpTile - 1) / kDpTile, ptiles = ptiles_x * (((long long)H + kDpTile - 1) / kDpTile);
    const long long gblocks = ((long long)B * H * W + 255) / 256;   // of k_occ_gather
    if (ptiles * B > 0x7fffffffLL || (occ && gblocks > 0x7fffffffLL)) return too_many_blocks(who, l, "sweeps");
    size_t vol = 0;
    const size_t floats = disparity_floats(B, D, H, W, C, aif ? LFT_DISPARITY_AIF : 0, &vol);
    if (!floats) return fail(LFT_ERR_SHAPE, "%s: the cost volume of %d x %d x %d x %d needs more than 2^40 bytes", who, B, D, H, W);
    if ((uintptr_t)scratch & 3) return fail(LFT_ERR_ARG, "%s: scratch must be 4-byte aligned", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    SweepOccArgs s{};
    fill_windowed(s.s, l);
    s.s.vol = static_cast<float*>(scratch); s.s.stack = aif ? s.s.vol + vol : nullptr;
    const dim3 grid((unsigned)(l.tiles * D * B));
    if (occ) {
        s.subsets = occ->subsets; s.P = occ->P; s.beta = occ->beta;
        s.choice = occ->choice ? occ->choice : occ->subset ? reinterpret_cast<uint8_t*>(s.s.vol + floats) : nullptr;
        by_lf_class<false>(lf_class, [&](auto t) { sweep_occ_kernel<decltype(t)>(C, taps)<<<grid, 256, 0, st>>>(s); return 0; });
        LFT_LAUNCH_OK("k_sweep_cost_occ");
    } else {
        by_lf_class<false>(lf_class, [&](auto t) { sweep_kernel<decltype(t)>(C, taps)<<<grid, 256, 0, st>>>(s.s); return 0; });
        LFT_LAUNCH_OK("k_sweep_cost");
    }
    PickArgs p{};
    p.vol = s.s.vol; p.stack = s.s.stack; p.slopes = slopes;
    p.H = H; p.W = W; p.D = D; p.C = C; p.r = radius; p.tiles_x = (int)ptiles_x; p.tiles = (int)ptiles;
    p.disparity = disparity; p.confidence = confidence; p.index = index; p.cost = cost; p.aif = aif;
    p.aif_f32 = aif_class == LFT_LF_FLOAT32;
    k_disparity_pick<<<dim3((unsigned)(ptiles * B)), 256, 0, st>>>(p);
    LFT_LAUNCH_OK("k_disparity_pick");
    return occ && occ->subset ? enqueue_occ_gather(index, s.choice, occ->subset, B, D, H, W, gblocks, st) : 0;
}
int lft_disparity(const void* lf, int lf_class, int B, int A, int H, int W, int C, const long long* strides, const void* table,
                  const float* slopes, int D, int taps, int radius, void* scratch, float* disparity, float* confidence, int* index,
                  float* cost, void* aif, int aif_class, void* stream) {
    return sweep_and_pick("lft_disparity", nullptr, lf, lf_class, B, A, H, W, C, strides, table, slopes, D, taps, radius, scratch, disparity, confidence, index,
                          cost, aif, aif_class, stream);
}

// ---- view synthesis (lft_views.cuh; declared in include/lft_hip_views.h) ----
// The pre-fill map [B, N, H, W] of keys, one dword each, must fit 2^40 bytes.  `who` starts the message.
static int prefill_map_ok(const char* who, int B, int N, int H, int W) {
    if ((double)B * N * H * W * 4.0 > 1099511627776.0)
        return fail(LFT_ERR_SHAPE, "%s: the pre-fill map of %d x %d x %d x %d needs more than 2^40 bytes", who, B, N, H, W);
    return 0;
}
// The body of the two scratch-size queries: the bytes of the pre-fill map.  The messages call the N planes `what`, of `planes`.
static int prefill_map_bytes(const char* who, const char* what, const char* planes, int B, int N, int H, int W, size_t* out_bytes) {
    if (!out_bytes) return fail(LFT_ERR_ARG, "%s: out_bytes is null", who);
    if (N < 1) return fail(LFT_ERR_ARG, "%s: %d %s", who, N, what);
    if (B < 0 || H < 0 || W < 0) return fail(LFT_ERR_SHAPE, "%s: negative size in B = %d, %s of %d x %d", who, B, planes, H, W);
    if (int rc = prefill_map_ok(who, B, N, H, W)) return rc;
    *out_bytes = (size_t)B * N * H * W * sizeof(uint32_t);
    return 0;
}
int lft_view_render_scratch_bytes(int B, int T, int H, int W, size_t* out_bytes) {
    return prefill_map_bytes("lft_view_render", "targets", "views", B, T, H, W, out_bytes);
}
// What lft_view_render and lft_view_render_visible check after windowed_lf_ok, in lft_view_render's order, and the launch shape
// they share.  `who` starts every message.  rtiles == 0: an empty shape, no work and no error.
struct ViewLaunch { int reach; long long rtiles_x, rtiles; };
static int view_values_ok(const char* who, int H, int W, float max_delta, float lo, float hi, int near, int fill, ViewLaunch& v) {
    if (fill < 0 || fill > kVwMaxFill) return fail(LFT_ERR_ARG, "%s: fill %d outside 0 .. %d", who, fill, kVwMaxFill);
    if (!std::isfinite(lo) || !std::isfinite(hi) || lo > hi) return fail(LFT_ERR_ARG, "%s: d_range (%g, %g) must be finite with lo <= hi", who, lo, hi);
    if (near != LFT_VIEW_NEAR_LARGER && near != LFT_VIEW_NEAR_SMALLER) return fail(LFT_ERR_ARG, "%s: near must be LFT_VIEW_NEAR_LARGER or LFT_VIEW_NEAR_SMALLER, got %d", who, near);
    if (!std::isfinite(max_delta) || max_delta < 0.0f) return fail(LFT_ERR_ARG, "%s: max_delta %g must be finite and >= 0", who, max_delta);
    // exact in double; an integer bound of the exact product also bounds its fp32 rounding
    const double reach = std::ceil(std::max(std::fabs((double)lo), std::fabs((double)hi)) * (double)max_delta) + 1.0;
    if (reach > (double)kVwMaxReach) return fail(LFT_ERR_SHAPE, "%s: reach %.0f pixels (d_range times the largest target offset) above %d", who, reach, kVwMaxReach);
    if (H > (1 << 24) || W > (1 << 24)) return fail(LFT_ERR_SHAPE, "%s: views of %d x %d: pixel coordinates are fp32, at most 2^24", who, H, W);
    v.reach = (int)reach;
    return 0;
}
static int view_render_ok(const char* who, WindowedLf& l, int views_class, bool own_null, float max_delta, float lo, float hi, int near, int fill,
                          float tau, const void* scratch, ViewLaunch& v) {
    v = ViewLaunch{0, 0, 0};
    if (int rc = windowed_lf_ok(who, l, views_class, "output", 0, own_null, "renders")) return rc;
    if (l.taps != 2 && l.taps != 4) return fail(LFT_ERR_ARG, "%s: %d taps (2 or 4: nearest is not offered)", who, l.taps);
    if (int rc = view_values_ok(who, l.H, l.W, max_delta, lo, hi, near, fill, v)) return rc;
    if (!std::isfinite(tau) || tau < 0.0f) return fail(LFT_ERR_ARG, "%s: tau %g must be finite and >= 0", who, tau);
    if (!l.tiles) return 0;                                         // nothing to render
    const long long rtiles = l.tiles_x * (((long long)l.H + kVwRows - 1) / kVwRows);
    if (rtiles * l.D * l.B > 0x7fffffffLL) return too_many_blocks(who, l, "renders");
    if (int rc = prefill_map_ok(who, l.B, l.D, l.H, l.W)) return rc;
    if ((uintptr_t)scratch & 3) return fail(LFT_ERR_ARG, "%s: scratch must be 4-byte aligned", who);
    v.rtiles_x = l.tiles_x; v.rtiles = rtiles;
    return 0;
}
static SplatArgs splat_args(const float* disparity, const float* deltas, void* scratch, float lo, float hi, int near, int reach, int H, int W, int T,
                            long long tiles_x, long long tiles) {
    SplatArgs s{};
    s.dr = disparity; s.deltas = deltas; s.keys = static_cast<uint32_t*>(scratch); s.lo = lo; s.hi = hi;
    s.neg = near == LFT_VIEW_NEAR_SMALLER; s.reach = reach;
    s.H = H; s.W = W; s.T = T; s.tiles_x = (int)tiles_x; s.tiles = (int)tiles;
    return s;
}
// step 1 of the three entry points: k_view_splat over (batch element, kRfTile tile, target)
static int enqueue_splat(const SplatArgs& s, int B, hipStream_t st) {
    k_view_splat<<<dim3((unsigned)((long long)s.tiles * s.T * B)), 256, 0, st>>>(s);
    LFT_LAUNCH_OK("k_view_splat");
    return 0;
}
static RenderArgs render_args(const WindowedLf& l, const SplatArgs& s, const ViewLaunch& v, int fill, void* views, int views_class, float* target_disparity,
                              unsigned char* holes) {
    RenderArgs r{};
    fill_windowed(r, l);
    r.dr = s.dr; r.keys = s.keys; r.lo = s.lo; r.hi = s.hi; r.neg = s.neg; r.fill = fill;
    r.rtiles_x = (int)v.rtiles_x; r.rtiles = (int)v.rtiles;
    r.out = views; r.out_f32 = views_class == LFT_LF_FLOAT32; r.dt = target_disparity; r.holes = holes;
    return r;
}
int lft_view_render(const void* lf, int lf_class, int B, int A, int H, int W, int C, const long long* strides, const float* disparity,
                    const float* deltas, float max_delta, const void* records, int T, int taps, float lo, float hi, int near, int fill,
                    void* scratch, void* views, int views_class, float* target_disparity, unsigned char* holes, void* stream) {
    WindowedLf l{lf, lf_class, B, A, H, W, C, strides, records, T, taps, 0, 0};
    ViewLaunch v;
    if (int rc = view_render_ok("lft_view_render", l, views_class, !disparity || !deltas || !scratch || !views || !target_disparity || !holes, max_delta, lo, hi,
                                near, fill, 0.0f, scratch, v))
        return rc;
    if (!v.rtiles) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const SplatArgs s = splat_args(disparity, deltas, scratch, lo, hi, near, v.reach, H, W, T, l.tiles_x, l.tiles);
    if (int rc = enqueue_splat(s, B, st)) return rc;
    const RenderArgs r = render_args(l, s, v, fill, views, views_class, target_disparity, holes);
    const dim3 grid((unsigned)(v.rtiles * T * B));
    by_lf_class<false>(lf_class, [&](auto t) { render_kernel<decltype(t)>(C, taps)<<<grid, 256, 0, st>>>(r); return 0; });
    LFT_LAUNCH_OK("k_view_render");
    return 0;
}

// ---- view synthesis with the per-view visibility test (lft_visibility.cuh; declared in include/lft_hip_visibility.h) ----
static_assert(kVsMask == LFT_VIS_MASK_VIEWS, "the header states the views whose visible bit stays in registers");
int lft_view_visible_scratch_bytes(int B, int N, int H, int W, size_t* out_bytes) {
    return prefill_map_bytes("lft_view_visible_scratch_bytes", "positions", "maps", B, N, H, W, out_bytes);
}
int lft_view_warp_disparity(const float* disparity, int B, int H, int W, const float* deltas, float max_delta, int N, float lo, float hi,
                            int near, int fill, void* scratch, float* maps, unsigned char* holes, void* stream) {
    const char* who = "lft_view_warp_disparity";
    if (N < 1) return fail(LFT_ERR_ARG, "%s: %d positions", who, N);
    if (B < 0 || H < 0 || W < 0) return fail(LFT_ERR_SHAPE, "%s: negative size in B = %d, maps of %d x %d", who, B, H, W);
    ViewLaunch v{0, 0, 0};
    if (int rc = view_values_ok(who, H, W, max_delta, lo, hi, near, fill, v)) return rc;
    if (B == 0 || H == 0 || W == 0) return 0;                       // nothing to read or write
    if (!disparity || !deltas || !scratch || !maps || !holes) return fail(LFT_ERR_ARG, "%s: null pointer", who);
    const long long tiles_x = ((long long)W + kRfTile - 1) / kRfTile, tiles = tiles_x * (((long long)H + kRfTile - 1) / kRfTile);
    const long long rtiles = tiles_x * (((long long)H + kVwRows - 1) / kVwRows);
    if (rtiles * N * B > 0x7fffffffLL) return fail(LFT_ERR_SHAPE, "%s: %d warps to %d positions over maps of %d x %d need more than 2^31 blocks", who, B, N, H, W);
    if (int rc = prefill_map_ok(who, B, N, H, W)) return rc;
    if ((uintptr_t)scratch & 3) return fail(LFT_ERR_ARG, "%s: scratch must be 4-byte aligned", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const SplatArgs s = splat_args(disparity, deltas, scratch, lo, hi, near, v.reach, H, W, N, tiles_x, tiles);
    if (int rc = enqueue_splat(s, B, st)) return rc;
    FillArgs f{};
    f.keys = s.keys; f.dr = disparity; f.lo = lo; f.hi = hi; f.neg = s.neg; f.fill = fill;
    f.H = H; f.W = W; f.N = N; f.rtiles_x = (int)tiles_x; f.rtiles = (int)rtiles;
    f.maps = maps; f.holes = holes;
    k_view_fill<<<dim3((unsigned)(rtiles * N * B)), 256, 0, st>>>(f);
    LFT_LAUNCH_OK("k_view_fill");
    return 0;
}
int lft_view_render_visible(const void* lf, int lf_class, int B, int A, int H, int W, int C, const long long* strides, const float* disparity,
                            const float* view_disparity, float tau, const float* deltas, float max_delta, const void* records, int T, int taps,
                            float lo, float hi, int near, int fill, void* scratch, void* views, int views_class, float* target_disparity,
                            unsigned char* holes, unsigned char* visible, void* stream) {
    WindowedLf l{lf, lf_class, B, A, H, W, C, strides, records, T, taps, 0, 0};
    ViewLaunch v;
    if (int rc = view_render_ok("lft_view_render_visible", l, views_class,
                                !disparity || !view_disparity || !deltas || !scratch || !views || !target_disparity || !holes || !visible, max_delta, lo, hi,
                                near, fill, tau, scratch, v))
        return rc;
    if (!v.rtiles) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const SplatArgs s = splat_args(disparity, deltas, scratch, lo, hi, near, v.reach, H, W, T, l.tiles_x, l.tiles);
    if (int rc = enqueue_splat(s, B, st)) return rc;
    VisArgs r{};
    r.r = render_args(l, s, v, fill, views, views_class, target_disparity, holes);
    r.dv = view_disparity; r.tau = tau; r.visible = visible;
    const dim3 grid((unsigned)(v.rtiles * T * B));
    by_lf_class<false>(lf_class, [&](auto t) { render_vis_kernel<decltype(t)>(C, taps)<<<grid, 256, 0, st>>>(r); return 0; });
    LFT_LAUNCH_OK("k_view_render_vis");
    return 0;
}

// ---- semi-global aggregation (lft_sgm.cuh; declared in include/lft_hip_sgm.h) ----
static_assert(kSgMaxD == LFT_SGM_MAX_D && kSgMaxD <= 4 * 64 && kSgMaxD <= kSgSegs * 64,
              "a row's wave holds four slopes per lane, a line's wave a segment of at most 64");
// What the size query and the call both judge; *vol: the floats of one volume [B, D, H, W], 0 for an empty shape.
static int sgm_shape_ok(int B, int D, int H, int W, int paths, size_t* vol) {
    if (paths != 4 && paths != 8) return fail(LFT_ERR_ARG, "lft_sgm: %d paths (4 or 8)", paths);
    if (D < 1 || D > LFT_SGM_MAX_D) return fail(LFT_ERR_ARG, "lft_sgm: %d slopes outside 1 .. %d", D, LFT_SGM_MAX_D);
    if (B < 0 || H < 0 || W < 0) return fail(LFT_ERR_SHAPE, "lft_sgm: negative size in B = %d, maps of %d x %d", B, H, W);
    if ((double)H * W > 2147483647.0) return fail(LFT_ERR_SHAPE, "lft_sgm: maps of %d x %d have more than 2^31 pixels", H, W);
    if ((double)paths * B * D * H * W * 4.0 > 1099511627776.0)
        return fail(LFT_ERR_SHAPE, "lft_sgm: %d path volumes of %d x %d x %d x %d need more than 2^40 bytes", paths, B, D, H, W);
    *vol = (size_t)B * D * H * W;
    return 0;
}
int lft_sgm_scratch_bytes(int B, int D, int H, int W, int paths, size_t* out_bytes) {
    if (!out_bytes) return fail(LFT_ERR_ARG, "lft_sgm: out_bytes is null");
    size_t vol = 0;
    if (int rc = sgm_shape_ok(B, D, H, W, paths, &vol)) return rc;
    *out_bytes = (size_t)paths * vol * sizeof(float);
    return 0;
}
int lft_sgm(const float* cost, int B, int D, int H, int W, int C, const float* slopes, int paths, float p1, float p2,
            const float* guide, float gain, const float* stack, void* scratch, float* disparity, float* confidence, int* index,
            float* aggregated, void* aif, int aif_class, void* stream) {
    size_t vol = 0;
    if (int rc = sgm_shape_ok(B, D, H, W, paths, &vol)) return rc;
    if (C < 1 || C > 4) return fail(LFT_ERR_ARG, "lft_sgm: %d channels (1 .. 4)", C);
    if (!std::isfinite(p1) || !std::isfinite(p2) || !std::isfinite(gain) || p1 < 0.0f || p2 < 0.0f || gain < 0.0f)
        return fail(LFT_ERR_ARG, "lft_sgm: p1 %g, p2 %g and gain %g must be finite and >= 0", p1, p2, gain);
    if (p2 < p1) return fail(LFT_ERR_ARG, "lft_sgm: p2 %g below p1 %g", p2, p1);
    if (gain > 0.0f && !guide) return fail(LFT_ERR_ARG, "lft_sgm: gain %g without a guide", gain);
    if (aif && !stack) return fail(LFT_ERR_ARG, "lft_sgm: all-in-focus output without a stack");
    if (aif_class != LFT_LF_UINT8 && aif_class != LFT_LF_FLOAT32)
        return fail(LFT_ERR_ARG, "lft_sgm: all-in-focus class must be LFT_LF_UINT8 or LFT_LF_FLOAT32, got %d", aif_class);
    if (!vol) return 0;                                             // empty maps
    if (!cost || !slopes || !scratch || !disparity || !confidence || !index) return fail(LFT_ERR_ARG, "lft_sgm: null pointer");
    if ((uintptr_t)scratch & 3) return fail(LFT_ERR_ARG, "lft_sgm: scratch must be 4-byte aligned");
    SgmScanArgs s{};
    s.cost = cost; s.guide = guide; s.paths = static_cast<float*>(scratch);
    s.B = B; s.D = D; s.H = H; s.W = W; s.R = paths; s.kc = (D + kSgSegs - 1) / kSgSegs;
    s.p1 = p1; s.p2 = p2; s.gain = gain;
    long long at = 0;
    for (int i = 0; i < paths; ++i) {                               // the grid's order: r2 .. r7 (r2, r3 of four paths), then r0, r1
        s.start[i] = (int)at;
        const bool rows = i >= paths - 2, diagonal = !rows && i >= 2;
        at += rows ? ((long long)H + kSgRows - 1) / kSgRows : ((long long)W + (diagonal ? H - 1 : 0) + kSgLines - 1) / kSgLines;
    }
    s.start[paths] = (int)at;
    const long long per = ((long long)H * W + 255) / 256;
    if (at * B > 0x7fffffffLL || per * B > 0x7fffffffLL)
        return fail(LFT_ERR_SHAPE, "lft_sgm: %d maps of %d x %d need more than 2^31 blocks", B, H, W);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(at * B));
    // the registers a lane keeps for its segment of the slopes, and the rows it loads ahead
    auto scan = [&](auto kc, auto pf) {
        if (guide) k_sgm_scan<decltype(kc)::value, decltype(pf)::value, true><<<grid, 256, 0, st>>>(s);
        else k_sgm_scan<decltype(kc)::value, decltype(pf)::value, false><<<grid, 256, 0, st>>>(s);
    };
    if (s.kc <= 4) scan(int_c<4>{}, int_c<4>{});
    else if (s.kc <= 8) scan(int_c<8>{}, int_c<4>{});
    else if (s.kc <= 12) scan(int_c<12>{}, int_c<4>{});
    else if (s.kc <= 16) scan(int_c<16>{}, int_c<4>{});
    else if (s.kc <= 32) scan(int_c<32>{}, int_c<2>{});
    else scan(int_c<64>{}, int_c<2>{});
    LFT_LAUNCH_OK("k_sgm_scan");
    SgmPickArgs p{};
    p.paths = s.paths; p.stack = stack; p.slopes = slopes;
    p.H = H; p.W = W; p.D = D; p.C = C; p.R = paths; p.per = (int)per; p.vol = vol;
    p.disparity = disparity; p.confidence = confidence; p.index = index; p.aggregated = aggregated; p.aif = aif;
    p.aif_f32 = aif_class == LFT_LF_FLOAT32;
    k_sgm_pick<<<dim3((unsigned)(per * B)), 256, 0, st>>>(p);
    LFT_LAUNCH_OK("k_sgm_pick");
    return 0;
}

// ---- the sweep's occlusion-aware cost (lft_occlusion.cuh; declared in include/lft_hip_occlusion.h) ----
static_assert(kOccMaxP == LFT_OCC_MAX_SUBSETS, "the header states how many subsets the kernel keeps accumulators for");
int lft_disparity_occ_scratch_bytes(int B, int D, int H, int W, int C, int flags, size_t* out_bytes) {
    return disparity_scratch_bytes("lft_disparity_occ", true, B, D, H, W, C, flags, out_bytes);
}
int lft_disparity_occ(const void* lf, int lf_class, int B, int A, int H, int W, int C, const long long* strides, const void* table,
                      const float* subsets, int P, float beta, const float* slopes, int D, int taps, int radius, void* scratch,
                      float* disparity, float* confidence, int* index, unsigned char* subset, unsigned char* choice, float* cost,
                      void* aif, int aif_class, void* stream) {
    const OccAdds occ{subsets, P, beta, subset, choice};
    return sweep_and_pick("lft_disparity_occ", &occ, lf, lf_class, B, A, H, W, C, strides, table, slopes, D, taps, radius, scratch, disparity, confidence, index,
                          cost, aif, aif_class, stream);
}
int lft_occ_gather(const int* index, const unsigned char* choice, int B, int D, int H, int W, unsigned char* subset, void* stream) {
    const char* who = "lft_occ_gather";
    if (D < 1) return fail(LFT_ERR_ARG, "%s: %d slopes", who, D);
    if (B < 0 || H < 0 || W < 0) return fail(LFT_ERR_SHAPE, "%s: negative size in B = %d, maps of %d x %d", who, B, H, W);
    if (B == 0 || H == 0 || W == 0) return 0;                       // nothing to read or write
    const double blocks = std::ceil((double)B * H * W / 256.0);
    if (blocks > 2147483647.0) return fail(LFT_ERR_SHAPE, "%s: %d maps of %d x %d need more than 2^31 blocks", who, B, H, W);
    if (!index || !choice || !subset) return fail(LFT_ERR_ARG, "%s: null pointer", who);
    return enqueue_occ_gather(index, choice, subset, B, D, H, W, (long long)blocks, static_cast<hipStream_t>(stream));
}

// ---- the all-in-focus image from the winning partial aperture (lft_aif.cuh; declared in include/lft_hip_aif.h) ----
int lft_aif_at(const void* lf, int lf_class, int B, int A, int H, int W, int C, const long long* strides, const void* table, int D,
               const float* subsets, int P, const int* index, const unsigned char* subset, int taps, void* aif, int aif_class, void* stream) {
    const char* who = "lft_aif_at";
    WindowedLf l{lf, lf_class, B, A, H, W, C, strides, table, D, taps, 0, 0};
    if (int rc = windowed_lf_ok(who, l, aif_class, "output", 0, false, "stacks")) return rc;          // lft_refocus's rules and words
    if (P < 0 || P > LFT_OCC_MAX_SUBSETS) return fail(LFT_ERR_ARG, "%s: %d subsets outside 0 .. %d", who, P, LFT_OCC_MAX_SUBSETS);
    if (!subsets != !P) return fail(LFT_ERR_ARG, "%s: the subsets table must be null exactly when P = 0, got %s with P = %d", who, subsets ? "a table" : "null", P);
    if (!l.tiles) return 0;                                         // an empty image
    if (!index || !aif) return fail(LFT_ERR_ARG, "%s: null pointer", who);
    const long long rtiles = l.tiles_x * (((long long)H + kVwRows - 1) / kVwRows);
    if (rtiles * B > 0x7fffffffLL) return fail(LFT_ERR_SHAPE, "%s: %d images of %d x %d need more than 2^31 blocks", who, B, H, W);
    AifArgs a{};
    fill_windowed(a, l);
    a.subsets = subsets; a.P = P; a.index = index; a.subset = subset;
    a.rtiles_x = (int)l.tiles_x; a.rtiles = (int)rtiles;
    a.out = aif; a.out_f32 = aif_class == LFT_LF_FLOAT32;
    const dim3 grid((unsigned)(rtiles * B));
    by_lf_class<false>(lf_class, [&](auto t) { aif_kernel<decltype(t)>(C, taps)<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(a); return 0; });
    LFT_LAUNCH_OK("k_aif_at");
    return 0;
}

// ---- scene tiling with a per-patch integer shear (lft_shear.cuh; declared in include/lft_hip_shear.h) ----
static_assert(kShearMax == LFT_SHEAR_MAX, "the header states the largest shear the vote keeps a count for");
// What the two tiling calls judge after their pointers: lft_scene_divide's tiling with its words, then what the shear adds.
// *kmax: the largest |k| whose cut stays inside the patch's border.
static int shear_tiling_ok(const char* who, int A, int h0, int w0, int patch, int stride, int* nu, int* nv, int* kmax) {
    if (int rc = scene_counts(h0, w0, patch, stride, nu, nv)) return rc;
    if ((patch - stride) % 2) return fail(LFT_ERR_SHAPE, "%s: patch - stride = %d is odd: the border must be the same on both sides", who, patch - stride);
    const int bdr = (patch - stride) / 2, u0 = A / 2, R = std::max(u0, A - 1 - u0);
    *kmax = R == 0 ? LFT_SHEAR_MAX : std::min(LFT_SHEAR_MAX, bdr / R);
    return 0;
}
int lft_scene_divide_shear(const float* scene, const int* shear, float* patches, int A, int h0, int w0, int patch, int stride, void* stream) {
    const char* who = "lft_scene_divide_shear";
    int nu, nv, kmax;
    if (!scene || !shear || !patches) return fail(LFT_ERR_ARG, "%s: null pointer", who);
    if (A < 1) return fail(LFT_ERR_ARG, "%s: angRes %d", who, A);
    if (int rc = shear_tiling_ok(who, A, h0, w0, patch, stride, &nu, &nv, &kmax)) return rc;
    // this launch: one block row per row of a patch mosaic, one block plane per patch; the scene mosaic is indexed in int
    if ((long long)A * patch > 65535 || (long long)nu * nv > 65535)
        return fail(LFT_ERR_SHAPE, "%s: patch mosaics of %lld rows and %d x %d patches need more than 65535 blocks in the grid's y or z", who, (long long)A * patch, nu, nv);
    if ((long long)A * h0 > 0x7fffffffLL || (long long)A * w0 > 0x7fffffffLL) return fail(LFT_ERR_SHAPE, "%s: a scene mosaic of %d x %d views of %d x %d has more than 2^31 rows or columns", who, A, A, h0, w0);
    const dim3 grid((unsigned)((A * patch + 255) / 256), (unsigned)(A * patch), (unsigned)(nu * nv));
    k_scene_divide_shear<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(scene, shear, patches, A, h0, w0, patch, stride, nv, kmax);
    LFT_LAUNCH_OK("k_scene_divide_shear");
    return 0;
}
int lft_scene_integrate_shear(const float* sr_patches, const int* shear, float* sr_scene, int A, int h0, int w0, int patch, int stride, int s, void* stream) {
    const char* who = "lft_scene_integrate_shear";
    int nu, nv, kmax;
    if (!sr_patches || !shear || !sr_scene) return fail(LFT_ERR_ARG, "%s: null pointer", who);
    if (A < 1 || s < 1) return fail(LFT_ERR_ARG, "%s: angRes %d, scale factor %d", who, A, s);
    if (int rc = shear_tiling_ok(who, A, h0, w0, patch, stride, &nu, &nv, &kmax)) return rc;
    // this launch: one block row per row of the SR scene mosaic; its columns, the patch index and a patch mosaic's side are ints
    if ((long long)A * h0 * s > 65535) return fail(LFT_ERR_SHAPE, "%s: an SR scene mosaic of %lld rows needs more than 65535 blocks in the grid's y", who, (long long)A * h0 * s);
    if ((long long)A * w0 * s > 0x7fffffffLL || (long long)nu * nv > 0x7fffffffLL)
        return fail(LFT_ERR_SHAPE, "%s: an SR scene mosaic of %lld columns in %d x %d patches is indexed beyond 2^31", who, (long long)A * w0 * s, nu, nv);
    if ((long long)patch * s * A > 0x7fffffffLL) return fail(LFT_ERR_SHAPE, "%s: SR patch mosaics of %lld pixels a side", who, (long long)patch * s * A);
    const dim3 grid((unsigned)((A * w0 * s + 255) / 256), (unsigned)(A * h0 * s));
    k_scene_integrate_shear<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(sr_patches, shear, sr_scene, A, patch * s, stride * s, h0 * s, w0 * s, nv, s, kmax);
    LFT_LAUNCH_OK("k_scene_integrate_shear");
    return 0;
}
int lft_shear_vote(const int* index, const float* confidence, const int* slopes, int B, int H, int W, int D, int margin, float min_confidence, int* counts,
                   int* shear, void* stream) {
    const char* who = "lft_shear_vote";
    if (!index || !confidence || !slopes || !counts || !shear) return fail(LFT_ERR_ARG, "%s: null pointer", who);
    if (B < 0 || H < 1 || W < 1) return fail(LFT_ERR_SHAPE, "%s: B = %d, maps of %d x %d", who, B, H, W);
    if (D < 1 || D > 2 * LFT_SHEAR_MAX + 1) return fail(LFT_ERR_SHAPE, "%s: %d slopes outside 1 .. %d", who, D, 2 * LFT_SHEAR_MAX + 1);
    if (margin < 0 || 2LL * margin >= std::min(H, W)) return fail(LFT_ERR_SHAPE, "%s: margin %d leaves nothing of maps of %d x %d", who, margin, H, W);
    if (!std::isfinite(min_confidence)) return fail(LFT_ERR_ARG, "%s: min_confidence %g must be finite", who, min_confidence);
    if (B == 0) return 0;                                           // nothing to vote on
    const VoteArgs a{index, confidence, slopes, H, W, D, margin, min_confidence, counts, shear};
    k_shear_vote<<<dim3((unsigned)B), 256, 0, static_cast<hipStream_t>(stream)>>>(a);
    LFT_LAUNCH_OK("k_shear_vote");
    return 0;
}

// ---- windowed blending of overlapping SR patches (lft_blend.cuh; declared in include/lft_hip_blend.h) ----
int lft_scene_integrate_blend(const float* sr_patches, const int* shear, const float* window, float* sr_scene, int A, int h0, int w0, int patch, int stride,
                              int s, void* stream) {
    const char* who = "lft_scene_integrate_blend";
    int nu, nv, kmax;
    if (!sr_patches || !window || !sr_scene) return fail(LFT_ERR_ARG, "%s: null pointer", who);      // shear may be null: no shear
    if (A < 1) return fail(LFT_ERR_ARG, "%s: angRes %d", who, A);
    if (s != 2 && s != 4) return fail(LFT_ERR_ARG, "%s: scale factor %d (2 or 4)", who, s);
    if (int rc = shear_tiling_ok(who, A, h0, w0, patch, stride, &nu, &nv, &kmax)) return rc;
    // this launch: k_scene_integrate_shear's grid and its limits, and the window table in LDS
    if ((long long)patch * s > LFT_BLEND_MAX_PZ) return fail(LFT_ERR_SHAPE, "%s: a window of %lld entries (at most %d)", who, (long long)patch * s, LFT_BLEND_MAX_PZ);
    if ((long long)A * h0 * s > 65535) return fail(LFT_ERR_SHAPE, "%s: an SR scene mosaic of %lld rows needs more than 65535 blocks in the grid's y", who, (long long)A * h0 * s);
    if ((long long)A * w0 * s > 0x7fffffffLL || (long long)nu * nv > 0x7fffffffLL)
        return fail(LFT_ERR_SHAPE, "%s: an SR scene mosaic of %lld columns in %d x %d patches is indexed beyond 2^31", who, (long long)A * w0 * s, nu, nv);
    if ((long long)patch * s * A > 0x7fffffffLL) return fail(LFT_ERR_SHAPE, "%s: SR patch mosaics of %lld pixels a side", who, (long long)patch * s * A);
    const dim3 grid((unsigned)((A * w0 * s + 255) / 256), (unsigned)(A * h0 * s));
    // the candidates per axis, ceil(2*pz/S) - 1: up to 3 the kernel has them written out, beyond that it loops
    const int nc = (2 * patch + stride - 1) / stride - 1;
    const auto kernel = nc == 1 ? k_scene_integrate_blend<1> : nc == 2 ? k_scene_integrate_blend<2> : nc == 3 ? k_scene_integrate_blend<3> : k_scene_integrate_blend<0>;
    kernel<<<grid, 256, (size_t)patch * s * sizeof(float), static_cast<hipStream_t>(stream)>>>(sr_patches, shear, window, sr_scene, A, patch * s, stride * s, h0 * s,
                                                                                           w0 * s, nu, nv, s, kmax);
    LFT_LAUNCH_OK("k_scene_integrate_blend");
    return 0;
}

// ---- angular tiling of a U x V field (lft_field.cuh; declared in include/lft_hip_field.h) ----
// The windows of both axes: *mu, *mv.
static int field_windows_ok(const char* who, int U, int V, int A, int astride, int* mu, int* mv) {
    if (A < 1) return fail(LFT_ERR_ARG, "%s: angRes %d", who, A);
    if (U < A || V < A || U > LFT_FIELD_MAX_VIEWS || V > LFT_FIELD_MAX_VIEWS)
        return fail(LFT_ERR_SHAPE, "%s: a field of %d x %d views (each axis %d .. %d for angRes %d)", who, U, V, A, LFT_FIELD_MAX_VIEWS, A);
    if (astride < 1 || astride > A) return fail(LFT_ERR_SHAPE, "%s: angular stride %d outside 1 .. angRes %d", who, astride, A);
    *mu = U == A ? 1 : (U - A + astride - 1) / astride + 1;
    *mv = V == A ? 1 : (V - A + astride - 1) / astride + 1;
    return 0;
}
// the most windows one view lies in along an axis of L views in m windows
static int field_multiplicity(int L, int A, int astride, int m) {
    int most = 0;
    for (int p = 0; p < L; ++p) {
        int c = 0;
        for (int i = 0; i < m; ++i) {
            const int o = std::min(i * astride, L - A);
            c += p >= o && p < o + A;
        }
        most = std::max(most, c);
    }
    return most;
}
int lft_field_counts(int U, int V, int A, int astride, int* mu, int* mv) {
    const char* who = "lft_field_counts";
    if (!mu || !mv) return fail(LFT_ERR_ARG, "%s: null pointer", who);
    return field_windows_ok(who, U, V, A, astride, mu, mv);
}
int lft_field_divide(const float* field, const int* shear, float* patches, int U, int V, int A, int astride, int h0, int w0, int patch, int stride, void* stream) {
    const char* who = "lft_field_divide";
    int mu, mv, nu, nv, kmax = 0;
    if (!field || !patches) return fail(LFT_ERR_ARG, "%s: null pointer", who);                          // shear may be null: the plain cut
    if (int rc = field_windows_ok(who, U, V, A, astride, &mu, &mv)) return rc;
    if (int rc = shear ? shear_tiling_ok(who, A, h0, w0, patch, stride, &nu, &nv, &kmax) : scene_counts(h0, w0, patch, stride, &nu, &nv)) return rc;
    // this launch: one block row per row of a patch mosaic, one block plane per patch, the windows along x; the mosaics are indexed in int
    const long long cb = ((long long)A * patch + 255) / 256;
    if ((long long)A * patch > 65535 || (long long)nu * nv > 65535)
        return fail(LFT_ERR_SHAPE, "%s: patch mosaics of %lld rows and %d x %d patches need more than 65535 blocks in the grid's y or z", who, (long long)A * patch, nu, nv);
    if ((long long)U * h0 > 0x7fffffffLL || (long long)V * w0 > 0x7fffffffLL || (long long)mu * mv * nu * nv > 0x7fffffffLL)
        return fail(LFT_ERR_SHAPE, "%s: a field mosaic of %d x %d views of %d x %d in %d x %d windows of %d x %d patches is indexed beyond 2^31", who, U, V, h0, w0, mu, mv,
                    nu, nv);
    if (cb * mu * mv > 0x7fffffffLL) return fail(LFT_ERR_SHAPE, "%s: %d x %d windows of %lld column blocks need more than 2^31 blocks in the grid's x", who, mu, mv, cb);
    const FieldGeom f{U, V, A, astride, mu, mv, h0, w0, patch, stride, nu, nv, 1, kmax};
    const dim3 grid((unsigned)(cb * mu * mv), (unsigned)(A * patch), (unsigned)(nu * nv));
    k_field_divide<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(field, shear, patches, f, (int)cb);
    LFT_LAUNCH_OK("k_field_divide");
    return 0;
}
int lft_field_integrate(const float* sr_patches, const int* shear, const float* window, const float* angular, float* sr_field, int U, int V, int A, int astride,
                        int h0, int w0, int patch, int stride, int s, void* stream) {
    const char* who = "lft_field_integrate";
    int mu, mv, nu, nv, kmax = 0;
    if (!sr_patches || !angular || !sr_field) return fail(LFT_ERR_ARG, "%s: null pointer", who);         // shear may be null: no shear; window: the crop
    if (A < 1) return fail(LFT_ERR_ARG, "%s: angRes %d", who, A);
    if (s != 2 && s != 4) return fail(LFT_ERR_ARG, "%s: scale factor %d (2 or 4)", who, s);
    if (int rc = field_windows_ok(who, U, V, A, astride, &mu, &mv)) return rc;
    if (int rc = shear || window ? shear_tiling_ok(who, A, h0, w0, patch, stride, &nu, &nv, &kmax) : scene_counts(h0, w0, patch, stride, &nu, &nv)) return rc;
    // this launch: k_scene_integrate_blend's grid and its limits, and the two tables in LDS
    if ((long long)patch * s > LFT_BLEND_MAX_PZ) return fail(LFT_ERR_SHAPE, "%s: a window of %lld entries (at most %d)", who, (long long)patch * s, LFT_BLEND_MAX_PZ);
    if ((long long)U * h0 * s > 65535) return fail(LFT_ERR_SHAPE, "%s: an SR field mosaic of %lld rows needs more than 65535 blocks in the grid's y", who, (long long)U * h0 * s);
    if ((long long)V * w0 * s > 0x7fffffffLL || (long long)mu * mv * nu * nv > 0x7fffffffLL)
        return fail(LFT_ERR_SHAPE, "%s: an SR field mosaic of %lld columns in %d x %d windows of %d x %d patches is indexed beyond 2^31", who, (long long)V * w0 * s, mu,
                    mv, nu, nv);
    if ((long long)patch * s * A > 0x7fffffffLL) return fail(LFT_ERR_SHAPE, "%s: SR patch mosaics of %lld pixels a side", who, (long long)patch * s * A);
    const FieldGeom f{U, V, A, astride, mu, mv, h0 * s, w0 * s, patch * s, stride * s, nu, nv, s, kmax};
    const dim3 grid((unsigned)((V * w0 * s + 255) / 256), (unsigned)(U * h0 * s));
    // the crop with at most 2 windows a view lies in per axis has them written out; everything else, every blend included, loops
    const int mult = std::max(field_multiplicity(U, A, astride, mu), field_multiplicity(V, A, astride, mv));
    const auto kernel = window || mult > 2 ? k_field_integrate<0> : mult == 1 ? k_field_integrate<1> : k_field_integrate<2>;
    kernel<<<grid, 256, ((size_t)A + (window ? (size_t)patch * s : 0)) * sizeof(float), static_cast<hipStream_t>(stream)>>>(sr_patches, shear, window, angular, sr_field, f);
    LFT_LAUNCH_OK("k_field_integrate");
    return 0;
}

// ---- refinement of a selected disparity map (lft_refine.cuh; declared in include/lft_hip_refine.h) ----
static_assert(kRnMaxViews == LFT_REFINE_MAX_VIEWS && kRnMaxRadius == LFT_REFINE_MAX_RADIUS && kRnMaxFill == LFT_REFINE_MAX_FILL && kRnTable == LFT_REFINE_TABLE,
              "the header states the limits the kernels are built for");
// What the three calls judge of their maps after their own arguments: 0 with *empty set for a shape without work.
static int refine_maps_ok(const char* who, int B, int H, int W, bool* empty) {
    if (B < 0 || H < 0 || W < 0) return fail(LFT_ERR_SHAPE, "%s: negative size in B = %d, maps of %d x %d", who, B, H, W);
    *empty = B == 0 || H == 0 || W == 0;
    if (*empty) return 0;                                           // nothing to read or write
    if (H > (1 << 24) || W > (1 << 24)) return fail(LFT_ERR_SHAPE, "%s: maps of %d x %d: pixel coordinates are fp32, at most 2^24", who, H, W);
    if ((double)H * W > 2147483647.0) return fail(LFT_ERR_SHAPE, "%s: maps of %d x %d have more than 2^31 pixels", who, H, W);
    return 0;
}
static int refine_near_ok(const char* who, int near) {
    if (near != LFT_VIEW_NEAR_LARGER && near != LFT_VIEW_NEAR_SMALLER) return fail(LFT_ERR_ARG, "%s: near must be LFT_VIEW_NEAR_LARGER or LFT_VIEW_NEAR_SMALLER, got %d", who, near);
    return 0;
}
static int refine_blocks_ok(const char* who, long long blocks, int B, int H, int W) {
    if (blocks > 0x7fffffffLL) return fail(LFT_ERR_SHAPE, "%s: %d maps of %d x %d need more than 2^31 blocks", who, B, H, W);
    return 0;
}
int lft_disp_check(const float* disparity, const float* view_disparity, const float* deltas, int B, int N, int H, int W, float tau, int near, int min_agree,
                   int max_conflict, unsigned char* valid, unsigned char* agree, unsigned char* conflict, void* stream) {
    const char* who = "lft_disp_check";
    bool empty;
    if (N < 1 || N > LFT_REFINE_MAX_VIEWS) return fail(LFT_ERR_ARG, "%s: %d views outside 1 .. %d", who, N, LFT_REFINE_MAX_VIEWS);
    if (!std::isfinite(tau) || tau < 0.0f) return fail(LFT_ERR_ARG, "%s: tau %g must be finite and >= 0", who, tau);
    if (int rc = refine_near_ok(who, near)) return rc;
    if (min_agree < 0 || max_conflict < 0) return fail(LFT_ERR_ARG, "%s: min_agree %d and max_conflict %d must be >= 0", who, min_agree, max_conflict);
    if (int rc = refine_maps_ok(who, B, H, W, &empty)) return rc;
    if (empty) return 0;
    if (!disparity || !view_disparity || !deltas || !valid || !agree || !conflict) return fail(LFT_ERR_ARG, "%s: null pointer", who);
    const long long per = ((long long)H * W + 255) / 256;
    if (int rc = refine_blocks_ok(who, per * B, B, H, W)) return rc;
    const CheckArgs a{disparity, view_disparity, deltas, tau, near == LFT_VIEW_NEAR_SMALLER, min_agree, max_conflict, H, W, N, (int)per, valid, agree, conflict};
    k_disp_check<<<dim3((unsigned)(per * B)), 256, 0, static_cast<hipStream_t>(stream)>>>(a);
    LFT_LAUNCH_OK("k_disp_check");
    return 0;
}
int lft_disp_fill(const float* disparity, const unsigned char* valid, int B, int H, int W, int reach, int near, float* out, unsigned char* holes, void* stream) {
    const char* who = "lft_disp_fill";
    bool empty;
    if (reach < 0 || reach > LFT_REFINE_MAX_FILL) return fail(LFT_ERR_ARG, "%s: reach %d outside 0 .. %d", who, reach, LFT_REFINE_MAX_FILL);
    if (int rc = refine_near_ok(who, near)) return rc;
    if (int rc = refine_maps_ok(who, B, H, W, &empty)) return rc;
    if (empty) return 0;
    if (!disparity || !out || !holes) return fail(LFT_ERR_ARG, "%s: null pointer", who);     // valid may be null: all valid
    if (out == disparity) return fail(LFT_ERR_ARG, "%s: the fill does not work in place (out == disparity)", who);
    const long long tiles_x = ((long long)W + kRfTile - 1) / kRfTile, rtiles = tiles_x * (((long long)H + kVwRows - 1) / kVwRows);
    if (int rc = refine_blocks_ok(who, rtiles * B, B, H, W)) return rc;
    const DispFillArgs a{disparity, valid, reach, near == LFT_VIEW_NEAR_SMALLER, H, W, (int)tiles_x, (int)rtiles, out, holes};
    k_disp_fill<<<dim3((unsigned)(rtiles * B)), 256, 0, static_cast<hipStream_t>(stream)>>>(a);
    LFT_LAUNCH_OK("k_disp_fill");
    return 0;
}
int lft_disp_wmedian(const float* disparity, const unsigned char* valid, const unsigned char* guide, const unsigned short* table, int B, int H, int W, int C,
                     int radius, float* out, unsigned char* flags, void* stream) {
    const char* who = "lft_disp_wmedian";
    bool empty;
    if (C < 1 || C > 4) return fail(LFT_ERR_ARG, "%s: %d guide channels (1 .. 4)", who, C);
    if (radius < 0 || radius > LFT_REFINE_MAX_RADIUS) return fail(LFT_ERR_ARG, "%s: radius %d outside 0 .. %d", who, radius, LFT_REFINE_MAX_RADIUS);
    if (int rc = refine_maps_ok(who, B, H, W, &empty)) return rc;
    if (empty) return 0;
    if (!disparity || !guide || !table || !out || !flags) return fail(LFT_ERR_ARG, "%s: null pointer", who);     // valid may be null: all valid
    if (out == disparity) return fail(LFT_ERR_ARG, "%s: the median does not work in place (out == disparity)", who);
    const long long tiles_x = ((long long)W + kRnTileW - 1) / kRnTileW, tiles = tiles_x * (((long long)H + kRnTileH - 1) / kRnTileH);
    if (int rc = refine_blocks_ok(who, tiles * B, B, H, W)) return rc;
    const MedianArgs a{disparity, valid, guide, table, H, W, C, (int)tiles_x, (int)tiles, out, flags};
    static void (*const kernel[kRnMaxRadius + 1])(MedianArgs) = {k_disp_wmedian<0>, k_disp_wmedian<1>, k_disp_wmedian<2>, k_disp_wmedian<3>,
                                                                 k_disp_wmedian<4>, k_disp_wmedian<5>, k_disp_wmedian<6>, k_disp_wmedian<7>};
    kernel[radius]<<<dim3((unsigned)(tiles * B)), 256, 0, static_cast<hipStream_t>(stream)>>>(a);
    LFT_LAUNCH_OK("k_disp_wmedian");
    return 0;
}

}  // extern "C"
