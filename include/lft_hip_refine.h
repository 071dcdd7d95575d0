/* lft_hip_refine.h -- refinement of a selected disparity map: the cross-view consistency check, the farther-neighbour fill and
 * the guided weighted median, entry points of liblft_hip.so.
 * Added beside ABI 5; lft_version unchanged.  The conventions are those of lft_hip.h (plain pointers, DEVICE unless noted, enqueue
 * only, 0 / LFT_ERR_* / hipError_t, lft_last_error); a library that lacks these symbols is an older build of the same ABI.
 *
 * Common rules.  `near` is LFT_VIEW_NEAR_LARGER or LFT_VIEW_NEAR_SMALLER of lft_hip_views.h.  All floating-point comparisons are
 * fp32.  Coordinates are fp32, one rounded operation per step, contraction off.  No result depends on tile, launch shape or
 * arrival order.  Each call only enqueues on `stream` (one launch, graph-capturable), allocates nothing, needs no scratch and never
 * synchronises.  Every refusal is made on the host before anything is launched, with a message that starts with the function's
 * name.  B, H or W == 0: no work, return 0.
 *
 * 1. lft_disp_check (k_disp_check): cross-view consistency.
 * Dr: fp32 [B,H,W], the map at the reference position.  Dv: fp32 [B,N,H,W], the maps of N other positions,
 * 1 <= N <= LFT_REFINE_MAX_VIEWS.  deltas: N pairs (Du, Dv) = position - reference, fp32, the pairs of lft_view_warp_disparity.
 * tau >= 0, finite, rounded once to fp32.  min_agree >= 0 and max_conflict >= 0.
 * Per pixel (y,x) with d = Dr[y,x], over the views in order n = 0..N-1:
 * - py = fl(y + fl(d*Du)), and px likewise.
 * - Footprint: (floor(py)+a, floor(px)+b) for a, b in {0,1}.  a = 1 is dropped when py is integral, b = 1 when px is integral.
 *   Positions outside the image are dropped, not clamped; that is decided in fp32 before any conversion to int, so a huge or
 *   non-finite py is simply outside.
 * - Let Q be the finite values Dv[n, ., .] on the footprint.  View n falls in the first class that applies:
 *   agree: some q in Q has fl(d - tau) <= q <= fl(d + tau).
 *   occluded: some q in Q is nearer than the band: q > fl(d + tau) for near = larger, q < fl(d - tau) for near = smaller.
 *   conflict: Q is non-empty, so every q is farther than the band: the view looks through the surface the map claims.
 *   unseen: Q is empty.
 * Outputs, all uint8 [B,H,W]: agree, the count of agreeing views; conflict, the count of conflicting views;
 * valid = finite(d) && agree >= min_agree && conflict <= max_conflict.  A non-finite d gives 0, 0, 0.
 * Every step is a comparison, so a numpy float32 restatement gives the same bytes.
 *
 * 2. lft_disp_fill (k_disp_fill): farther-neighbour fill.
 * D: fp32 [B,H,W].  valid: uint8 [B,H,W], or NULL for all valid.  reach: 0..LFT_REFINE_MAX_FILL.
 * - A pixel is good iff valid != 0 and D is finite there.  A good pixel passes through bit for bit, with holes = 0.
 * - Any other pixel takes the farther (near = larger: the smaller) of the nearest good values to its left and to its right in the
 *   row, each side searched up to `reach` pixels.  If only one side has a good value, the pixel takes that one.  If neither side
 *   has one, the same search runs up and down the column.  A pixel that got a value has holes = 1.
 * - If nothing is found, out has the bits of D and holes = 2.
 * - Only input values are read: a filled pixel never feeds another.  out must not be D.
 * This is step 2 of lft_view_render with a mask in the place of "no coverer"; the search is the one function both kernels call.
 *
 * 3. lft_disp_wmedian (k_disp_wmedian): guided weighted median.
 * D: fp32 [B,H,W].  valid: uint8 or NULL.  guide: uint8 [B,H,W,C], 1 <= C <= 4.  table: uint16 [LFT_REFINE_TABLE].
 * radius r: 0..LFT_REFINE_MAX_RADIUS.  Per pixel p:
 * - The window is every q = p + (dy,dx) with |dy|, |dx| <= r that lies inside the image; positions outside are dropped.
 * - q is a sample iff it is good, in the sense of 2.  Its weight is the integer w_q = table[min(1023, sum_c |g_c(p) - g_c(q)|)].
 * - T = sum w_q over the samples; it is at most 225*65535, so 2T fits 32 bits.
 * - T = 0: out has the bits of D[p] and flag = 2.
 * - Otherwise out = min{ v : 2 * sum_{q: D[q] <= v} w_q >= T } over the sample values v, the lower weighted median, and flag = 0 if
 *   p was good, else flag = 1.
 * The sums are integers, so the definition has no order to fix and is exact.  The result is the value of a sample.  Values are
 * compared as numbers: where -0 and +0 both occur, either may come back.  out must not be D.
 *
 * Refused -- LFT_ERR_ARG: N outside 1 .. LFT_REFINE_MAX_VIEWS, a tau that is negative or not finite, a `near` that is neither
 * constant, negative counts, reach, radius or C out of range, a null pointer with a non-empty shape (valid may be null where
 * stated), out == D.  LFT_ERR_SHAPE: a negative size, H or W above 2^24 (pixel coordinates are fp32), maps an int cannot index or
 * that need more than 2^31 blocks. */
#ifndef LFT_HIP_REFINE_H
#define LFT_HIP_REFINE_H

#ifdef __cplusplus
extern "C" {
#endif

#define LFT_REFINE_MAX_VIEWS 128
#define LFT_REFINE_MAX_RADIUS 7
#define LFT_REFINE_MAX_FILL 64
#define LFT_REFINE_TABLE 1024

int lft_disp_check(const float* disparity, const float* view_disparity, const float* deltas, int B, int N, int H, int W, float tau, int near, int min_agree, int max_conflict, unsigned char* valid, unsigned char* agree, unsigned char* conflict, void* stream);
int lft_disp_fill(const float* disparity, const unsigned char* valid, int B, int H, int W, int reach, int near, float* out, unsigned char* holes, void* stream);
int lft_disp_wmedian(const float* disparity, const unsigned char* valid, const unsigned char* guide, const unsigned short* table, int B, int H, int W, int C, int radius, float* out, unsigned char* flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif
