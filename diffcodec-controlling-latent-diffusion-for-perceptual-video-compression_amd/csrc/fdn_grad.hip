// The FDN injection (control_utils.py:28-34) for gfx950 in exact fp32 NCHW, forward and backward (include/diffcodec_fdn_hip.h):
//
//   y = GroupNorm(32, C, affine=False)(x) * (1 + gamma) + beta
//
// A group of sample n is m = (C / 32) * H * W contiguous floats of x.  One 256-thread workgroup per (sample, group):
//
//   forward (fdn_kernel), three passes over the group's block, the later ones served from L2:
//     mean0 = sum(x) / m
//     c = sum(x - mean0) / m,  var = sum((x - mean0)^2) / m - c^2,  mean = mean0 + c       one pass, both sums centred
//     rstd = 1 / sqrt(var + eps),  y = (x - mean) * rstd * (1 + gamma) + beta
//   The refinement by c costs one accumulator: mean0 carries the rounding of a sum of m terms (about 1e-7 |mean|, which at
//   |mean| = 100 sigma is 1e-5 sigma in every x - mean), c brings it down to the rounding of the stored mean itself, and a constant
//   group gets mean = its value, xh = 0 and var = 0 exactly.  c^2 is the exact shift of the variance to the refined mean (about 1e-10 var).
//
//   backward (fdn_grad_kernel), with xh = (x - mean) * rstd recomputed from the saved statistics and gh = g * (1 + gamma):
//     S1 = sum(gh), S2 = sum(gh * xh)                                    skipped when g_x is not wanted
//     g_x = rstd * (gh - S1 / m - xh * S2 / m),  g_gamma = g * xh        the gradient of beta is g itself: nothing is written
//
// The order of every sum is a function of m alone.  Element i belongs to quad q = i / 4; thread t owns the quads t, t + 256, ... and
// keeps one accumulator per position in the quad, each adding its elements in ascending order; the four meet as (a0 + a1) + (a2 + a3),
// the 64 lanes of a wave by an xor butterfly (both partners of a step add the same two numbers, so every lane holds the same bits),
// the four waves through LDS as (w0 + w1) + (w2 + w3).  A quad is one 16-byte access where m % 4 == 0 and the operand's group base is
// 16-byte aligned, else four 4-byte accesses of the same elements (odd H * W, a channel-slice view at an odd offset): the same
// assignment, so the same bits.  No float atomics, nothing accumulated across workgroups, every launch only enqueues its kernel.
// Multiply-adds are written out (fmaf, contraction off), so that two unrolled copies of one expression cannot round differently.
#include "dc_common.h"
#include "../../include/diffcodec_fdn_hip.h"

namespace {

constexpr int GROUPS = 32;                                               // control_utils.py:25
constexpr int THREADS = 256;
// which operands take the 16-byte path (bits of `vec`)
constexpr int V_X = 1, V_GAMMA = 2, V_BETA = 4, V_OUT = 8, V_G = 16, V_GGAMMA = 32;

// elements i .. i + 3 of a group's block; past the block's end (4-byte path only): zeros
__device__ __forceinline__ f32x4 load_quad(const float* __restrict__ p, long long i, long long m, bool vec)
{
    if (vec) return *(const f32x4*)(p + i);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i + j < m) v[j] = p[i + j];
    return v;
}

__device__ __forceinline__ void store_quad(float* __restrict__ p, long long i, long long m, bool vec, f32x4 v)
{
    if (vec) {
        *(f32x4*)(p + i) = v;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i + j < m) p[i + j] = v[j];
}

__device__ __forceinline__ float quad_sum(f32x4 a) { return (a[0] + a[1]) + (a[2] + a[3]); }

// two sums over the workgroup at once; every thread returns the same bits.  The leading barrier ends the previous use of `part`.
__device__ __forceinline__ void block_sum2(float& a, float& b, float (*part)[2])
{
    a = dc_wave_sum(a);
    b = dc_wave_sum(b);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6][0] = a;
        part[threadIdx.x >> 6][1] = b;
    }
    __syncthreads();
    a = (part[0][0] + part[1][0]) + (part[2][0] + part[3][0]);
    b = (part[0][1] + part[1][1]) + (part[2][1] + part[3][1]);
}

__global__ __launch_bounds__(THREADS) void fdn_kernel(const float* __restrict__ x, const float* __restrict__ gamma, long long gamma_stride,
                                                      const float* __restrict__ beta, long long beta_stride, float* __restrict__ y,
                                                      float* __restrict__ mean_out, float* __restrict__ rstd_out, long long m, float eps, int vec)
{
#pragma clang fp contract(off)
    __shared__ float part[THREADS / 64][2];
    const long long n = blockIdx.x / GROUPS, grp = blockIdx.x % GROUPS;
    const float* xp = x + (long long)blockIdx.x * m;
    const float* gp = gamma + n * gamma_stride + grp * m;
    const float* bp = beta + n * beta_stride + grp * m;
    float* yp = y + (long long)blockIdx.x * m;
    const bool vx = vec & V_X, vg = vec & V_GAMMA, vb = vec & V_BETA, vo = vec & V_OUT;
    const float fm = (float)m;

    f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (long long i = 4LL * threadIdx.x; i < m; i += 4 * THREADS) a += load_quad(xp, i, m, vx);
    float s = quad_sum(a), unused = 0.f;
    block_sum2(s, unused, part);
    const float mean0 = s / fm;

    f32x4 d1 = {0.f, 0.f, 0.f, 0.f}, d2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (long long i = 4LL * threadIdx.x; i < m; i += 4 * THREADS) {
        const f32x4 v = load_quad(xp, i, m, vx);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = (vx || i + j < m) ? v[j] - mean0 : 0.f;
            d1[j] += d;
            d2[j] = __builtin_fmaf(d, d, d2[j]);
        }
    }
    float s1 = quad_sum(d1), s2 = quad_sum(d2);
    block_sum2(s1, s2, part);
    const float c = s1 / fm;
    const float mean = mean0 + c;
    const float var = fmaxf(__builtin_fmaf(-c, c, s2 / fm), 0.f);
    const float rstd = 1.0f / sqrtf(var + eps);
    if (threadIdx.x == 0) {
        mean_out[blockIdx.x] = mean;
        rstd_out[blockIdx.x] = rstd;
    }

#pragma unroll 2
    for (long long i = 4LL * threadIdx.x; i < m; i += 4 * THREADS) {
        const f32x4 v = load_quad(xp, i, m, vx), gv = load_quad(gp, i, m, vg), bv = load_quad(bp, i, m, vb);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = __builtin_fmaf((v[j] - mean) * rstd, 1.0f + gv[j], bv[j]);
        store_quad(yp, i, m, vo, o);
    }
}

__global__ __launch_bounds__(THREADS) void fdn_grad_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                           const float* __restrict__ gamma, long long gamma_stride,
                                                           const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                           float* __restrict__ g_x, float* __restrict__ g_gamma, long long g_gamma_stride,
                                                           long long m, int vec)
{
#pragma clang fp contract(off)
    __shared__ float part[THREADS / 64][2];
    const long long n = blockIdx.x / GROUPS, grp = blockIdx.x % GROUPS;
    const float* gop = g + (long long)blockIdx.x * m;
    const float* xp = x + (long long)blockIdx.x * m;
    const bool vx = vec & V_X, vg = vec & V_GAMMA, vo = vec & V_OUT, vgo = vec & V_G, vgg = vec & V_GGAMMA;
    const float mean = mean_in[blockIdx.x], rstd = rstd_in[blockIdx.x];

    float s1m = 0.f, s2m = 0.f;
    const float* gp = nullptr;
    float* gxp = nullptr;
    if (g_x) {                                                            // uniform over the grid: every thread reaches the barriers
        gp = gamma + n * gamma_stride + grp * m;
        gxp = g_x + (long long)blockIdx.x * m;
        f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (long long i = 4LL * threadIdx.x; i < m; i += 4 * THREADS) {
            const f32x4 gv = load_quad(gop, i, m, vgo), v = load_quad(xp, i, m, vx), ga = load_quad(gp, i, m, vg);
#pragma unroll
            for (int j = 0; j < 4; ++j) {                                 // past the end g = 0, so gh = 0 and neither sum moves
                const float gh = gv[j] * (1.0f + ga[j]);
                const float xh = (v[j] - mean) * rstd;
                a1[j] += gh;
                a2[j] = __builtin_fmaf(gh, xh, a2[j]);
            }
        }
        float s1 = quad_sum(a1), s2 = quad_sum(a2);
        block_sum2(s1, s2, part);
        const float fm = (float)m;
        s1m = s1 / fm;
        s2m = s2 / fm;
    }
    float* ggp = g_gamma ? g_gamma + n * g_gamma_stride + grp * m : nullptr;

#pragma unroll 2
    for (long long i = 4LL * threadIdx.x; i < m; i += 4 * THREADS) {
        const f32x4 gv = load_quad(gop, i, m, vgo), v = load_quad(xp, i, m, vx);
        f32x4 xh;
#pragma unroll
        for (int j = 0; j < 4; ++j) xh[j] = (v[j] - mean) * rstd;
        if (gxp) {
            const f32x4 ga = load_quad(gp, i, m, vg);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float gh = gv[j] * (1.0f + ga[j]);
                o[j] = rstd * __builtin_fmaf(-xh[j], s2m, gh - s1m);
            }
            store_quad(gxp, i, m, vo, o);
        }
        if (ggp) {
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = gv[j] * xh[j];
            store_quad(ggp, i, m, vgg, o);
        }
    }
}

inline bool shape_ok(int N, int C, int H, int W)
{
    return N >= 1 && N <= 65535 && C >= GROUPS && C <= 65535 && C % GROUPS == 0 && H >= 1 && H <= 16384 && W >= 1 && W <= 16384 &&
           (long long)H * W <= (1LL << 28) && (long long)(C / GROUPS) * H * W <= (1LL << 30);
}

// a group's block starts at base + n * stride + group * m: 16-byte aligned for every (n, group) when all three terms are
inline bool aligned16(const void* p, long long stride, long long m) { return p && (uintptr_t)p % 16 == 0 && stride % 4 == 0 && m % 4 == 0; }

}  // namespace

extern "C" int dc_fdn_f32(const float* x, const float* gamma, long long gamma_stride, const float* beta, long long beta_stride, float* y,
                          float* mean, float* rstd, int N, int C, int H, int W, float eps, void* stream)
{
    if (!x || !gamma || !beta || !y || !mean || !rstd || !shape_ok(N, C, H, W)) return DC_ERR_INVALID;
    if (gamma_stride < 0 || beta_stride < 0 || !(eps > 0.f) || !(eps <= 3.0e38f)) return DC_ERR_INVALID;
    const long long m = (long long)(C / GROUPS) * H * W;
    const int vec = (aligned16(x, 0, m) ? V_X : 0) | (aligned16(gamma, gamma_stride, m) ? V_GAMMA : 0) |
                    (aligned16(beta, beta_stride, m) ? V_BETA : 0) | (aligned16(y, 0, m) ? V_OUT : 0);
    hipLaunchKernelGGL(fdn_kernel, dim3(N * GROUPS), dim3(THREADS), 0, (hipStream_t)stream, x, gamma, gamma_stride, beta, beta_stride, y, mean,
                       rstd, m, eps, vec);
    return dc_launch_status();
}

extern "C" int dc_fdn_grad_f32(const float* g, const float* x, const float* gamma, long long gamma_stride, const float* mean,
                               const float* rstd, float* g_x, float* g_gamma, long long g_gamma_stride, int N, int C, int H, int W,
                               void* stream)
{
    if (!g || !x || !mean || !rstd || !shape_ok(N, C, H, W)) return DC_ERR_INVALID;
    if (!g_x && !g_gamma) return DC_ERR_INVALID;
    if (g_x && (!gamma || gamma_stride < 0)) return DC_ERR_INVALID;
    if (g_gamma && g_gamma_stride < (long long)C * H * W) return DC_ERR_INVALID;
    const long long m = (long long)(C / GROUPS) * H * W;
    const int vec = (aligned16(x, 0, m) ? V_X : 0) | (g_x && aligned16(gamma, gamma_stride, m) ? V_GAMMA : 0) | (aligned16(g, 0, m) ? V_G : 0) |
                    (aligned16(g_x, 0, m) ? V_OUT : 0) | (aligned16(g_gamma, g_gamma_stride, m) ? V_GGAMMA : 0);
    hipLaunchKernelGGL(fdn_grad_kernel, dim3(N * GROUPS), dim3(THREADS), 0, (hipStream_t)stream, g, x, gamma, gamma_stride, mean, rstd, g_x,
                       g_gamma, g_gamma_stride, m, vec);
    return dc_launch_status();
}
