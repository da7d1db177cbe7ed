/* C ABI of the backward of one level of the flow-warped control pyramid (csrc/pyramid_grad.hip), compiled into libdiffcodec_hip.so
 * next to the entry points of the five other headers and bound by diffcodec_amd.lib.PYRAMID_SIGNATURES.
 * diffcodec_amd.pyramid_train wraps them in an autograd function (`warp_fuse`) and a module (`BiDirFeatureExtractor`).
 *
 * The operator is extractors.py:293-310 with control_utils.py:49-72 inlined, everything fp32 NCHW:
 *   wf = dc_splat_soft_f32(first, flow_f, metric_f, occ_f),  wl = dc_splat_soft_f32(last, flow_b, metric_b, occ_b)
 *   fused = dc_fuse_warped_f32(wf, wl, metric_f, metric_b, occ_f, occ_b)            (include/diffcodec_hip.h)
 * and its backward to first, last, metric_f and metric_b (a metric is both the splat's exponent and the fusion's confidence) is
 *   e = exp(metric)                                        dc_pyramid_exp_f32       per side
 *   den = dc_splat_sum_f32(e, flow)                        (include/diffcodec_hip.h) per side: the normaliser, recomputed
 *   per-pixel planes of the fusion and the normaliser      dc_pyramid_fuse_grad_f32 once
 *   the gradients of one side's feature map and metric     dc_pyramid_warp_grad_f32 per side
 * No tensor of C channels is written between the launches.
 *
 * Every launcher only enqueues kernels on `stream` (a hipStream_t; null = the default stream; no memset or copy nodes) and touches
 * no memory but the caller's tensors, so a chain of them is capturable into a graph.  There is no workspace and no size query:
 * every intermediate is a named output of documented shape that the caller allocates.  fp32 with a fixed summation order that
 * depends on (C, H * W) only, no float atomics, every output element written exactly once (nothing needs zeroing): bitwise
 * reproducible, and an image's results do not depend on its position in the batch or on N.  Return 0, -1 for an invalid argument
 * (nothing is launched), -2 when the launch fails.
 *
 * Sizes every entry accepts: N and C in 1..65535, H and W in 1..16384 with H * W <= 2^28.  "plane" below: contiguous [N][H][W]. */
#ifndef DIFFCODEC_PYRAMID_HIP_H
#define DIFFCODEC_PYRAMID_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* e[i] = exp(metric[i]) for n contiguous floats (expf, as the forward's gather evaluates it). */
int dc_pyramid_exp_f32(const float* metric, float* e, long long n, void* stream);

/* Target side.  g, wf, wl: contiguous [N][C][H][W] (the incoming gradient and the two masked warps the forward produced);
 * cf, cb, occ_f, occ_b: planes (the confidences = the metrics, and the occlusion masks); den_f, den_b: planes, the normalisers
 * sum_s e b of each side, either may be null when that side's gradients are not wanted (not both).  With A = sum_c g wf,
 * B = sum_c g wl, p = max(cf, 0), q = max(cb, 0), S = (p + q) + 1e-6, hole = occ_f + occ_b > 1.5, D = den + 1e-7 it writes the planes
 *   g_cf = [cf >= 0] (A (S - p) - B q) / S^2,   g_cb = [cb >= 0] (B (S - q) - A p) / S^2      (0 in a hole; the gate is >=, as
 *                                                                                              torch.clamp(min=0) differentiates)
 *   coef_f = (1 - occ_f) w0 / D_f,  gden_f = -w0 A / D_f     with w0 = p / S (0.5 in a hole); only when den_f is given
 *   coef_b = (1 - occ_b) w1 / D_b,  gden_b = -w1 B / D_b     with w1 = q / S (0.5 in a hole); only when den_b is given
 * g_cf and g_cb are always written; the outputs of a side whose den is given must not be null. */
int dc_pyramid_fuse_grad_f32(const float* g, const float* wf, const float* wl, const float* cf, const float* cb, const float* occ_f,
                             const float* occ_b, const float* den_f, const float* den_b, float* g_cf, float* g_cb, float* coef_f,
                             float* gden_f, float* coef_b, float* gden_b, int N, int C, int H, int W, void* stream);

/* Source side of one warp.  x: contiguous [N][C][H][W], the feature map that was splatted (read only when gm is given);
 * e: plane, exp(metric); flow: contiguous [N][2][H][W]; g: the incoming gradient of the fused map; coef, gden: that side's planes
 * from dc_pyramid_fuse_grad_f32; g_conf: that side's g_cf or g_cb.  With b the bilinear weight of source s at each of its four
 * corner targets t (corners outside the map are skipped, bounds tested before every read) it writes
 *   gx[n][c][s] = e A_c,                   A_c = sum_corners b coef(t) g_c(t)              contiguous [N][C][H][W], or null
 *   gm[n][s] = e (sum_c x_c A_c + sum_corners b gden(t)) + g_conf(s)                      plane, or null
 * (not both null; gden and g_conf are read only when gm is given).  A source whose landing point is not finite, or that has no corner
 * inside the map, gets gx = 0 and gm = g_conf. */
int dc_pyramid_warp_grad_f32(const float* x, const float* e, const float* flow, const float* g, const float* coef, const float* gden,
                             const float* g_conf, float* gx, float* gm, int N, int C, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif
