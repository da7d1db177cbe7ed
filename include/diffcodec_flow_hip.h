/* C ABI of the flow-propagation stages (csrc/cmp.hip), compiled into libdiffcodec_hip.so next to include/diffcodec_hip.h's entry
 * points and bound by diffcodec_amd.lib.FLOW_SIGNATURES.  The Conditional Motion Propagation network turns the sparse guide
 * vectors of the codec's side information and an anchor frame into dense flow; diffcodec_amd.flow_propagation.HipCMP chains
 * these launchers into the whole network.
 *
 * Every launcher only enqueues on `stream` (a hipStream_t; null = the default stream) and touches no memory but the caller's
 * tensors, so a chain of them is capturable into a graph on one stream.  Exact fp32, fixed summation order, no float atomics:
 * bitwise reproducible and independent of the batch size.  Return 0, -1 for an invalid argument (nothing is launched), -2 when
 * the launch fails. */
#ifndef DIFFCODEC_FLOW_HIP_H
#define DIFFCODEC_FLOW_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* 2D convolution + folded eval BatchNorm (+ residual) (+ ReLU) on v_mfma_f32_32x32x2_f32.
 * x: the operand [N][Cin][H][W] read through the element strides xstrides = (n, c, h, w) (host array); fp32, or with x_u8 = 1
 * uint8 with Cin = 3 (a frame, usually NHWC and possibly a cropped view), taken as (v - mean_c) / div_c with mean_div = host
 * array (mean_0..2, div_0..2); the zero padding is applied after that normalisation.  mean_div may be null when x_u8 = 0.
 * k in {1, 3, 5, 7}; stride in {1, 2}; dilation in {1, 2, 4}; padding = dilation * (k - 1) / 2 on each side, so
 * Ho = (H + 2 pad - dilation (k - 1) - 1) / stride + 1 and likewise Wo.
 * packed (device, fp32, 16-byte aligned): the K-major matrix [rows][CoP] with element [(ci * k + kh) * k + kw][co], rows =
 * Cin k k rounded up to 32 (zero rows), CoP = Cout rounded up to 32 (zero columns); then s [CoP]; then t [CoP], with
 * y = s * conv + t (s = gamma / sqrt(var + eps), t = beta - mean s + bias s; s = 1, t = bias for a plain convolution).
 * residual: null, or contiguous fp32 [N][Cout][Ho][Wo] added before the ReLU.  relu = 0 leaves the sum.
 * y: fp32 [N][Ctot][Ho][Wo], of which channels c_off .. c_off + Cout are written and the others left alone. */
int dc_cmp_conv(const void* x, int x_u8, const long long* xstrides, const float* mean_div, int N, int Cin, int H, int W, int k,
                int stride, int dilation, const float* packed, int Cout, const float* residual, int relu, float* y, int Ctot,
                int c_off, void* stream);
/* Max-pool of a contiguous fp32 [NC][H][W] map with a k x k window (k <= 8), the given stride and padding (2 pad <= k); the padded
 * positions never enter the max (PyTorch's rule) and NaN propagates.  y [NC][(H + 2 pad - k) / stride + 1][likewise]; a size
 * that would leave an empty map is refused. */
int dc_cmp_maxpool(const float* x, int NC, int H, int W, int k, int stride, int pad, float* y, void* stream);
/* Average-pool 2 x 2 / 2 of a contiguous fp32 [N][C][H][W] map, written to channels c_off .. c_off + C of
 * y [N][Ctot][H / 2][W / 2] (floor). */
int dc_cmp_avgpool(const float* x, int N, int C, int H, int W, float* y, int Ctot, int c_off, void* stream);
/* Bilinear upsample with align_corners = True of a contiguous fp32 [N][C][H][W] map to Ho x Wo, written to channels
 * c_off .. c_off + C of y [N][Ctot][Ho][Wo].  A source of size 1 along an axis gives a constant along it. */
int dc_cmp_upsample(const float* x, int N, int C, int H, int W, int Ho, int Wo, float* y, int Ctot, int c_off, void* stream);
/* Logits [N][2 nbins][h][w] -> flow [N][2][h][w]: per pixel a softmax over the first nbins channels (x) and one over the last
 * nbins (y), each followed by the expectation over the bin centres (i + 1/2) * 2 fmax / nbins - fmax.  Max-subtracted: logits
 * of +-1e3 neither overflow nor give NaN. */
int dc_cmp_convert_flow(const float* logits, int N, int nbins, int h, int w, float fmax, float* flow, void* stream);
/* The reference's 'grid' guide sampling in gather form: flow [N][2][H][W] -> sparse [N][4][H][W]; channels 0-1 hold the flow at
 * the points (y0 + a stride, x0 + b stride), y0 = (H - H / stride * stride) / 2 and likewise x0, and zero elsewhere; channels
 * 2-3 hold the mask (1 at those points). */
int dc_cmp_sparse_grid(const float* flow, int N, int H, int W, int stride, float* sparse, void* stream);

/* The 1x1 head fused with the expectation: x contiguous fp32 [N][Cin][h][w] -> flow [N][2][h][w] in one launch (the head's
 * convolution with bias, then dc_cmp_convert_flow's arithmetic on the accumulators; the sums of a pixel are split over two lanes
 * and added in a fixed order).  packed: dc_cmp_conv's layout for (Cin, Cout = 2 nbins, k = 1); 2 nbins <= 224.  logits: null, or
 * [N][2 nbins][h][w] to receive the logits as well (bit for bit dc_cmp_conv's). */
int dc_cmp_head(const float* x, int N, int Cin, int h, int w, const float* packed, int nbins, float fmax, float* logits, float* flow,
                void* stream);

/* The whole network.  arch: 0 = resnet50 + shallownet8x + MotionDecoderSkipLayer (74 convolutions, logits at H/2), 1 = resnet50 +
 * shallownet8x + MotionDecoderPlain with decoder_combo [1, 2, 4] (63 convolutions, logits at H/8); img_enc_dim 256, sparse_enc_dim
 * 16, output_dim 2 nbins.  image / image_u8 / image_strides: dc_cmp_conv's operand forms with the configs' data_mean / data_div;
 * sparse: contiguous fp32 [N][4][H][W].  weights (device, fp32, 16-byte aligned, dc_cmp_weight_floats(arch, nbins) elements): every
 * convolution's `packed` block back to back in forward order: stem; per bottleneck [downsample,] conv1, conv2, conv3; conv5; the two
 * sparse-encoder convolutions; decoder1, decoder2, decoder4 (, decoder8); SkipLayer only: fusion8, skipconv4, fusion4, skipconv2,
 * fusion2; the head.  ws (device, 256-byte aligned): dc_cmp_ws_bytes(arch, N, H, W) bytes, any contents, owned by the caller.
 * dc_cmp_ws_bytes returns -1 for a refused size: one where the reference's own torch.cat fails (the encoders disagree at 1/8,
 * e.g. H = 68), where a decoder max-pool would be empty (1/8 map below 8 for arch 0, below 4 for arch 1) or that is out of range;
 * the launchers return -1 for the same sizes.  dc_cmp_weight_floats returns -1 for an unknown arch or 2 nbins > 224. */
int dc_cmp_weight_floats(int arch, int nbins);
long long dc_cmp_ws_bytes(int arch, int N, int H, int W);
/* CMP.forward (+ Fuser.convert_flow): logits [N][2 nbins][h][w] and / or flow [N][2][h][w] at the network's resolution; either may
 * be null (not both), and the logits are stored only when asked for. */
int dc_cmp_forward(int arch, const void* image, int image_u8, const long long* image_strides, const float* sparse, int N, int H, int W,
                   int nbins, float fmax, const float* weights, void* ws, float* logits, float* flow, void* stream);
/* CMP.eval without its loss: the flow upsampled (align_corners = True) to flow_up [N][2][H][W]. */
int dc_cmp_flow(int arch, const void* image, int image_u8, const long long* image_strides, const float* sparse, int N, int H, int W,
                int nbins, float fmax, const float* weights, void* ws, float* flow_up, void* stream);
/* The same with every named intermediate written to the caller's contiguous fp32 tensors.  maps = host array of device pointers:
 * arch 0: sparse_enc [N][16][h8][w8], img_enc [N][256][h8][w8], the stem map [N][64][h2][w2], layer1 [N][256][h4][w4], then the
 * fused maps f8 [N][256][h8][w8], f4 [N][128][h4][w4], f2 [N][64][h2][w2] (7 pointers); arch 1: the first four, then the
 * concatenated decoder map [N][384][h8][w8] (5 pointers).  logits, flow, flow_up as above, all required. */
int dc_cmp_endpoints(int arch, const void* image, int image_u8, const long long* image_strides, const float* sparse, int N, int H, int W,
                     int nbins, float fmax, const float* weights, void* ws, float* const* maps, float* logits, float* flow,
                     float* flow_up, void* stream);

#ifdef __cplusplus
}
#endif
#endif
