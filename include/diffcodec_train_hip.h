/* C ABI of the backward of the fp32 extractor convolution (csrc/conv_f32_grad.hip), compiled into libdiffcodec_hip.so next to the
 * entry points of the four other headers and bound by diffcodec_amd.lib.TRAIN_SIGNATURES.  diffcodec_amd.train wraps them in an
 * autograd function.
 *
 * The operator is dc_conv3x3_nchw_f32 (include/diffcodec_hip.h): z = conv3x3(x, w, padding 1, stride 1 | 2 | 4) + bias and
 * y = silu ? SiLU(z) : z, everything fp32, NCHW activations and OIHW weights.  Its backward is three launches:
 *   gz = gy * silu'(z)                                  dc_silu_grad_f32      (only with SiLU)
 *   dx = the data gradient of gz                        dc_conv3x3_f32_dgrad
 *   dw, db = the weight and bias gradients of gz        dc_conv3x3_f32_wgrad
 *
 * Every launcher only enqueues kernels on `stream` (a hipStream_t; null = the default stream; no memset or copy nodes) and touches
 * no memory but the caller's tensors, so a chain of them is capturable into a graph.  Exact fp32, fixed summation order, no float
 * atomics, every output element written exactly once (nothing needs zeroing): bitwise reproducible.  The weight is read in its
 * checkpoint layout on every call: nothing is packed or cached on the host.  Return 0, -1 for an invalid argument (nothing is
 * launched), -2 when the launch fails.
 *
 * Sizes every entry accepts: N, Cin, Cout in 1..65535, H and W in 1..16384 with H * W <= 2^28, stride 1 | 2 | 4. */
#ifndef DIFFCODEC_TRAIN_HIP_H
#define DIFFCODEC_TRAIN_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* gz[i] = gy[i] * silu'(z[i]), silu'(z) = s + z s (1 - s) with s = sigmoid(z) evaluated as the forward's SiLU evaluates it.
 * z, gy, gz: n contiguous floats; gz may be gy. */
int dc_silu_grad_f32(const float* z, const float* gy, float* gz, long long n, void* stream);

/* Data gradient.  gz: contiguous [N][Cout][Ho][Wo], Ho = (H - 1) / stride + 1 (Wo alike); w: OIHW [Cout][Cin][3][3];
 * dx: contiguous [N][Cin][H][W], every element written (pixels no output reads get 0).  A gather per dx element over the taps of
 * its stride phase; an image's dx does not depend on its position in the batch. */
int dc_conv3x3_f32_dgrad(const float* gz, const float* w, float* dx, int N, int Cin, int H, int W, int Cout, int stride, void* stream);

/* Bytes of dc_conv3x3_f32_wgrad's workspace (any contents, 16-byte aligned); -1 for a refused shape.  Exactly what the launch
 * touches: the split-K partials of dw, then one bias partial per image.  Strictly increasing in N and at most N times the size
 * for one image. */
long long dc_conv3x3_f32_wgrad_ws_bytes(int N, int Cin, int H, int W, int Cout, int stride);

/* Weight and bias gradient.  x: [N][Cin][H][W] with dense CHW planes and `x_batch_stride` floats between images (>= Cin * H * W:
 * a channel-slice view); gz as above; dw: OIHW [Cout][Cin][3][3]; db: [Cout] or null.  The reduction over the N * Ho * Wo pixels
 * is split over a partition that depends on the shape alone; every part writes its partial into ws and a finish launch adds the
 * partials in part order. */
int dc_conv3x3_f32_wgrad(const float* x, long long x_batch_stride, const float* gz, float* dw, float* db, void* ws, int N, int Cin,
                         int H, int W, int Cout, int stride, void* stream);

/* The instance dc_conv3x3_f32_dgrad (kind DC_F32GRAD_DGRAD) or dc_conv3x3_f32_wgrad (kind DC_F32GRAD_WGRAD) launches for a shape,
 * without launching: the launchers decide with the same function.  Returns 0, or -1 for what the launch refuses, and fills
 * info[DC_F32GRAD_ROUTE_INFO_INTS]:
 *   info[0] form: DC_F32GRAD_MFMA (v_mfma_f32_32x32x2_f32) | DC_F32GRAD_VALU (the generic form)
 *   info[1] the STRIDE template argument of the MFMA form (1 | 2); the generic form takes the stride at run time: 0
 *   info[2] channels per workgroup: dgrad MFMA 64 | 32 input channels, wgrad MFMA 64 (x 64 input channels); generic form: 0
 *   info[3], info[4] columns x rows of the pixel tile (dgrad: 128 pixels of dx's phase grid; wgrad: one K step's 32 output pixels,
 *            the generic wgrad one whole output row)
 *   info[5], info[6], info[7] wgrad only: image groups, K parts per image group, K steps per part (parts = info[5] * info[6]). */
#define DC_F32GRAD_ROUTE_INFO_INTS 8
#define DC_F32GRAD_DGRAD 0
#define DC_F32GRAD_WGRAD 1
#define DC_F32GRAD_MFMA 1
#define DC_F32GRAD_VALU 2
int dc_conv3x3_f32_grad_route(int kind, int N, int Cin, int H, int W, int Cout, int stride, int* info);

#ifdef __cplusplus
}
#endif
#endif
