/* C ABI of the trainable FDN injection (csrc/fdn_grad.hip): the fp32 GroupNorm-and-modulate of control_utils.py:28-34, forward and
 * backward, compiled into libdiffcodec_hip.so next to the entry points of the six other headers and bound by
 * diffcodec_amd.lib.FDN_SIGNATURES.  diffcodec_amd.fdn_train wraps the pair in an autograd function (`fdn`) and the modules `FDN`
 * and `DualFlowControlLayers`.
 *
 *   out = GroupNorm(32, C, affine=False)(x) * (1 + gamma) + beta                      (control_utils.py:28-34)
 *
 * Everything is fp32 NCHW.  C is a multiple of 32 (nn.GroupNorm(32, C) refuses anything else); a group of sample n is the
 * m = (C / 32) * H * W contiguous floats of x.  x, y, g and g_x are dense [N][C][H][W].  gamma, beta and g_gamma are a pointer plus a
 * batch stride in elements: their [C][H][W] planes are dense, the batch stride is free (>= 0 for the two inputs, >= C * H * W for
 * g_gamma), so the two halves of one [N][2C][H][W] tensor are passed as they lie.  Loads and stores are 16 bytes wide where m and an
 * operand's address allow, 4 bytes wide otherwise, with the same bits either way.
 *
 * Every launcher only enqueues one kernel on `stream` (a hipStream_t; null = the default stream; no memset or copy nodes) and touches
 * no memory but the caller's tensors: capturable into a graph, no workspace, no size query.  One 256-thread workgroup per
 * (sample, group); every sum has a fixed order that depends on m only, no float atomics, nothing accumulated across workgroups, every
 * output element written exactly once: bitwise reproducible, and a sample's results do not depend on N or on its position in the
 * batch.  Return 0, -1 for an invalid argument (nothing is launched), -2 when the launch fails.
 *
 * Sizes every entry accepts: N in 1..65535, C a multiple of 32 in 32..65535, H and W in 1..16384 with H * W <= 2^28 and m <= 2^30. */
#ifndef DIFFCODEC_FDN_HIP_H
#define DIFFCODEC_FDN_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* Forward (control_utils.py:28-34).  Per (sample, group), in three passes over the group's block:
 *   mean0 = sum(x) / m
 *   c = sum(x - mean0) / m,  mean = mean0 + c,  var = sum((x - mean0)^2) / m - c^2
 *   rstd = 1 / sqrt(var + eps)         eps > 0 (with eps = 0 a constant group would have rstd = inf: refused)
 *   y    = (x - mean) * rstd * (1 + gamma) + beta
 * var is the biased variance, as F.group_norm forms it, from sums of centred data (never E[x^2] - mean^2).  This is the two-pass
 * form with one refinement: the centred pass also yields c, the rounding left in mean0 (about 1e-7 |mean0|), the stored mean is
 * mean0 + c, and c^2 is the exact shift of the centred sum of squares from mean0 to mean0 + c.  c is itself rounded, so the stored
 * var belongs to the stored mean up to about 1e-10 var.  A constant group gets mean = its value and var = 0.
 * mean, rstd: contiguous [N][32], written for the backward.  No pointer may be null. */
int dc_fdn_f32(const float* x, const float* gamma, long long gamma_stride, const float* beta, long long beta_stride, float* y,
               float* mean, float* rstd, int N, int C, int H, int W, float eps, void* stream);

/* Backward of control_utils.py:28-34.  g: the gradient of the output; x, mean, rstd: the forward's.  With xh = (x - mean) * rstd
 * recomputed, gh = g * (1 + gamma), and per (sample, group) S1 = sum(gh), S2 = sum(gh * xh):
 *   g_x     = rstd * (gh - S1 / m - xh * S2 / m)      dense [N][C][H][W], or null: the reduction pass is then not run, and gamma is
 *                                                     not read (it may be null)
 *   g_gamma = g * xh                                  planes with batch stride g_gamma_stride, or null
 * Not both null.  The gradient of beta is g itself: nothing is written for it. */
int dc_fdn_grad_f32(const float* g, const float* x, const float* gamma, long long gamma_stride, const float* mean, const float* rstd,
                    float* g_x, float* g_gamma, long long g_gamma_stride, int N, int C, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif
