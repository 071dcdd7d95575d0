/* lft_hip_test.h -- test-only entry points of liblft_hip.so (NOT part of the product ABI of lft_hip.h; no reference counterpart).
 * The library exports them for tests/ only: the MFMA fragment-layout self test the parity suite starts with, the product-policy
 * self test of the training GEMMs, the two stages the composed 16-bit front end is compared against, and the tail of the forward
 * (last SpaTrans + up-sampler) with either hand-off between the two. */
#ifndef LFT_HIP_TEST_H
#define LFT_HIP_TEST_H
#ifdef __cplusplus
extern "C" {
#endif

/* MFMA fragment-layout self test: C = Am[32x16] * Bm[16x32], D = W2[32x32] * C.  All fp32 device buffers. */
int lft_mfma_selftest(const float* Am, const float* Bm, const float* W2, float* C, float* D, int prec, void* stream);

/* Product-policy self test of the training GEMMs (math = LFT_MATH_*): W [32][16] is packed as one weight fragment, X is [32 tokens][16];
 * Y [32 tokens][32] = X W^T, Yl / Yr = the same product with X's rows moved by one token (row t takes row t - 1 / t + 1, a zero row at
 * the edge).  All fp32 device buffers; returns after the stream has drained. */
int lft_prod_selftest(const float* W, const float* X, float* Y, float* Yl, float* Yr, int math, void* stream);

/* lft_init_features_fwd as it ran before conv_init0 was composed into conv_init.0 (and as fp32 still runs it): conv_init0 written
 * to the workspace, then the three 64 -> 64 convolutions.  Same arguments as lft_init_features_fwd. */
int lft_init_features_legacy_fwd(const void* packed, const float* lr, void* act_out, void* workspace, int B, int A, int h, int w, int s,
                                 int prec, void* stream);

/* conv_init0 alone, tokens [B*A*A*h*w][64] in the activation type: recomputed == 0 -- the stand-alone kernel; recomputed != 0 (16-bit
 * only) -- the residual tile the last convolution of the front end computes from the LR pixels.  The two must be bit-identical. */
int lft_conv0_fwd(const void* packed, const float* lr, void* x0_out, int recomputed, int B, int A, int h, int w, int s, int prec, void* stream);

/* SpaTrans of layer 3 with the global skip, then the up-sampler, as lft_forward chains them (act_in / skip: tokens in the activation
 * type, out: the fp32 HR mosaic).  handoff != 0: the block writes lane-major tiles and k_up reads them (requires the lane-major
 * property of the view size in this precision, else LFT_ERR_SHAPE and nothing is launched).  handoff == 0: row-major. */
int lft_tail_fwd(const void* packed, const void* act_in, const void* skip, const float* lr, float* out, void* workspace,
                 int B, int A, int h, int w, int s, int prec, int handoff, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LFT_HIP_TEST_H */
