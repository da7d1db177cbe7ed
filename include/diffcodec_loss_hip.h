/* C ABI of the training losses (csrc/lpips_grad.hip, csrc/edge_loss.hip), compiled into libdiffcodec_hip.so next to the entry
 * points of include/diffcodec_hip.h and include/diffcodec_flow_hip.h and bound by diffcodec_amd.lib.LOSS_SIGNATURES:
 * the NormFix LPIPS (AlexNet) value with its post-ReLU maps kept, its backward to the images, and the Sobel edge loss with its
 * backward.  diffcodec_amd.losses wraps them in autograd functions.
 *
 * Every launcher only enqueues kernels on `stream` (a hipStream_t; null = the default stream; no memset or copy nodes) and touches
 * no memory but the caller's tensors, so a chain of them is capturable into a graph.  Exact fp32, fixed summation order, no float
 * atomics, every output element written exactly once (nothing needs zeroing): bitwise reproducible and independent of the pair's
 * position in the batch.  Return 0, -1 for an invalid argument (nothing is launched), -2 when the launch fails.
 *
 * Layers are numbered 0..4 (relu1..relu5: 64, 192, 384, 256, 256 channels).  `sides`: bit 0 = the first operand wants a gradient,
 * bit 1 = the second; the backward works on M = N * popcount(sides) images, the first operand's first. */
#ifndef DIFFCODEC_LOSS_HIP_H
#define DIFFCODEC_LOSS_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of the packed data-gradient weights: for conv2..conv5 in that order the matrix [(co, ky, kx)][Cin] with the taps mirrored,
 * element [(co * k + ky) * k + kx][ci] = w[co][ci][k - 1 - ky][k - 1 - kx] (diffcodec_amd.losses.pack_lpips_dgrad_weights). */
int dc_lpips_dgrad_weight_floats(void);
/* Bytes of the caller-owned buffer that holds the maps of one dc_lpips_alex_keep call (-1 for a refused size). */
long long dc_lpips_keep_ws_bytes(int N, int H, int W);
/* Bytes of the backward's scratch (any contents, 256-byte aligned); -1 for a refused size or sides outside 1..3. */
long long dc_lpips_train_ws_bytes(int N, int H, int W, int sides);

/* dc_lpips_alex(normfix = 1) on fp32 operands whose five post-ReLU maps of the 2N images stay in `keep` for the backward: the
 * forward convolutions run once.  x, y, strides, normalize, weights, out ([6][N] fp64: five layer terms, then the value) as
 * dc_lpips_alex; the value bits equal dc_lpips_alex's. */
int dc_lpips_alex_keep(const float* x, const float* y, const long long* strides, int N, int H, int W, int normalize,
                       const float* weights, void* keep, double* out, void* stream);
/* The whole backward: from the kept maps and g [5][N] (fp32: the upstream gradient of layer term l of pair n, the value's gradient
 * already added to each layer) to dx and / or dy, contiguous fp32 [N][3][H][W] (the one `sides` does not name may be null).
 * normalize contributes its factor 2, the scaling layer 1 / scale_c.  weights: the forward vector (lin weights and conv1);
 * dweights: dc_lpips_dgrad_weight_floats() floats; ws: dc_lpips_train_ws_bytes bytes. */
int dc_lpips_alex_backward(const void* keep, const float* g, int N, int H, int W, int normalize, int sides, const float* weights,
                           const float* dweights, void* ws, float* dx, float* dy, void* stream);

/* Gradient of layer `layer`'s distance term w.r.t. its post-ReLU maps.  f: [2N][C][HW] (image n against image N + n); g: [N];
 * out: [M][C][HW].  With n = sqrt(sum_c (x_c^2 + 1e-8)), u = x / n, d = u_self - u_other and t_c = 2 g w_c d_c / HW:
 * out_c = (t_c - u_c sum_k u_k t_k) / n where the map is positive, 0 where it is not (the ReLU below). */
int dc_lpips_tail_grad(int layer, const float* f, int N, int HW, int sides, const float* weights, const float* g, float* out,
                       void* stream);
/* Data gradient of conv2..conv5 (layer 1..4) on v_mfma_f32_32x32x2_f32.  gin: [M][Cout][H][W], the gradient at the convolution's
 * output; y: [M][Cin][H][W] = (add ? add : 0) + dgrad, set to 0 where map <= 0 when map is given (add, map: null or [M][Cin][H][W];
 * y may be add itself, not gin).  H, W <= 4096. */
int dc_lpips_conv_dgrad(int layer, const float* gin, int M, int H, int W, const float* dweights, const float* add, const float* map,
                        float* y, void* stream);
/* Gradient of max_pool2d(3, stride 2) in gather form.  gp: [planes][(H - 3) / 2 + 1][(W - 3) / 2 + 1]; map: the pooled map
 * [planes][H][W], whose windows' argmax is recomputed (the first maximum in raster order wins); y = (add ? add : 0) + the
 * gradients of the windows that chose the element, in window raster order, and 0 where map <= 0.  H, W >= 3. */
int dc_lpips_pool_grad(const float* gp, const float* map, const float* add, int planes, int H, int W, float* y, void* stream);
/* Data gradient of conv1 (64 -> 3, 11x11, stride 4, pad 2) and of the input transform.  gin: [M][64][Ho][Wo]; the first nx images
 * go to dx, the others to dy (contiguous fp32 [.][3][H][W]); rows and columns no window reaches get 0. */
int dc_lpips_conv1_dgrad(const float* gin, int M, int nx, int H, int W, int normalize, const float* weights, float* dx, float* dy,
                         void* stream);

/* Sobel edge loss: with v = (x + 1) / 2, gx / gy = the per-channel Sobel x / y correlations with zero padding 1 and
 * e = sqrt(gx^2 + gy^2 + 1e-6): |e(pred) - e(target)| per element.  pred, target: fp32 [N][C][H][W] through the element strides
 * strides = (n, c, h, w) of pred, then of target (host array).  reduction 0: out_map contiguous fp32 [N][C][H][W] (ws, out
 * unused, may be null); 1: the mean, 2: the sum, as one fp64 in out[0] (per-workgroup fp64 partials in ws, summed in a fixed
 * order by a second launch).  dc_sobel_edge_ws_bytes: bytes of ws; -1 for a refused shape. */
long long dc_sobel_edge_ws_bytes(int N, int C, int H, int W);
int dc_sobel_edge_loss(const float* pred, const float* target, const long long* strides, int N, int C, int H, int W, int reduction,
                       void* ws, float* out_map, double* out, void* stream);
/* Its gradient w.r.t. pred (side 0) or target (side 1) in one gather launch: grad contiguous fp32 [N][C][H][W].  The upstream
 * gradient of element q is (per_element ? gout[q] : gout[0]) * scale (gout on the device); sign(0) = 0. */
int dc_sobel_edge_grad(const float* pred, const float* target, const long long* strides, int N, int C, int H, int W, int side,
                       const float* gout, int per_element, float scale, float* grad, void* stream);

#ifdef __cplusplus
}
#endif
#endif
