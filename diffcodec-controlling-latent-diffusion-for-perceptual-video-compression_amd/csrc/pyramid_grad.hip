// Backward of one level of the flow-warped control pyramid for gfx950, fp32 NCHW (include/diffcodec_pyramid_hip.h): two 'soft'
// splats, the (1 - occ) multiply, the clamped-confidence fusion and the hole fill (extractors.py:293-310 with control_utils.py:49-72
// inlined), differentiated as ONE operator.  With e = exp(metric), b(s, t) the bilinear corner weight of source s at target t,
// den(t) = sum_s e b, D = den + 1e-7, wf = num / D (1 - occ), p = max(cf, 0), q = max(cb, 0), S = (p + q) + 1e-6 and g the incoming
// gradient:
//
//   target side (fuse_grad_kernel), one channel reduction per pixel:
//     A = sum_c g wf, B = sum_c g wl
//     g_cf = [cf >= 0] (A (S - p) - B q) / S^2,  g_cb = [cb >= 0] (B (S - q) - A p) / S^2          (0 in a hole)
//     w0 = p / S, w1 = q / S                                                                      (0.5 each in a hole)
//     coef = (1 - occ) w / D,  gden = -w A / D         per side; A carries the (1 - occ) of wf, so gden = -coef sum_c g num_c / D
//   source side (warp_grad_kernel), one launch per side:
//     A_c(s) = sum_corners b coef(t) g_c(t),  g_x_c = e A_c,  g_m(s) = e (sum_c x_c A_c + sum_corners b gden(t)) + g_conf(s)
//
// No C-channel intermediate exists between the two: g_wf = w0 g is formed in registers from the per-pixel plane `coef`.  Both are
// gathers, so nothing is accumulated across threads in global memory.  A workgroup of 256 threads holds 256 / SL pixels x SL channel
// slices; slice s adds the channels s, s + SL, s + 2 SL, ... in ascending order, the SL partial sums meet in LDS and are added in
// ascending s.  SL depends on (C, H * W) only, so the order of every sum is a fixed function of the image's shape: bit-identical
// from launch to launch, and the same bits whatever N the image is batched into.  Corners by dc_splat_corners.h: bounds tested
// before every read, a source whose landing point is not finite (or that has no corner inside the map) gets zeros.
#include "dc_common.h"
#include "dc_splat_corners.h"                    // Corners, corners_of: the set-up dc_splat_ingrad_f32 uses
#include "../../include/diffcodec_pyramid_hip.h"

namespace {

constexpr float EPS_SPLAT = 0.0000001f;                                  // softsplat.py:257
constexpr float EPS_FUSE = 1e-6f;                                        // extractors.py:298

__global__ __launch_bounds__(256) void exp_kernel(const float* __restrict__ m, float* __restrict__ e, long long n)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) e[i] = expf(m[i]);
}

// SL channel slices per pixel, PIX = 256 / SL pixels per workgroup: thread t = slice (t / PIX), pixel (t % PIX)
template <int SL>
__global__ __launch_bounds__(256) void fuse_grad_kernel(const float* __restrict__ g, const float* __restrict__ wf, const float* __restrict__ wl,
                                                        const float* __restrict__ cf, const float* __restrict__ cb,
                                                        const float* __restrict__ of, const float* __restrict__ ob,
                                                        const float* __restrict__ den_f, const float* __restrict__ den_b,
                                                        float* __restrict__ g_cf, float* __restrict__ g_cb, float* __restrict__ coef_f,
                                                        float* __restrict__ gden_f, float* __restrict__ coef_b, float* __restrict__ gden_b,
                                                        int N, int C, long long hw)
{
    constexpr int PIX = 256 / SL;
    __shared__ float part[SL > 1 ? SL : 1][PIX][2];
    const long long total = (long long)N * hw;
    const int slice = threadIdx.x / PIX, lane = threadIdx.x % PIX;
    // the trip count depends on the workgroup alone, so every thread of it reaches the barriers below
    for (long long base = (long long)blockIdx.x * PIX; base < total; base += (long long)gridDim.x * PIX) {
        const long long i = base + lane;
        const bool live = i < total;
        float a = 0.f, b = 0.f;
        if (live) {
            const long long n = i / hw, p = i - n * hw;
            const long long at = n * C * hw + p;
#pragma unroll 4
            for (int ch = slice; ch < C; ch += SL) {
                const long long j = at + ch * hw;
                const float gv = g[j];
                a += gv * wf[j];
                b += gv * wl[j];
            }
        }
        if (SL > 1) {
            part[slice][lane][0] = a;
            part[slice][lane][1] = b;
            __syncthreads();
            if (slice == 0 && live) {
#pragma unroll
                for (int s = 1; s < SL; ++s) a += part[s][lane][0], b += part[s][lane][1];
            }
            __syncthreads();                                              // the next trip overwrites part[][]
        }
        if (slice == 0 && live) {
            const float vf = cf[i], vb = cb[i];
            const float p = fmaxf(vf, 0.f), q = fmaxf(vb, 0.f);
            const float s = (p + q) + EPS_FUSE;
            const bool hole = of[i] + ob[i] > 1.5f;                       // extractors.py:307: fused = 0.5 (wf + wl), no confidence
            const float w0 = hole ? 0.5f : p / s, w1 = hole ? 0.5f : q / s;
            const float s2 = s * s;
            g_cf[i] = (!hole && vf >= 0.f) ? (a * (s - p) - b * q) / s2 : 0.f;    // clamp(min=0) passes the gradient at exactly 0
            g_cb[i] = (!hole && vb >= 0.f) ? (b * (s - q) - a * p) / s2 : 0.f;
            if (den_f) {
                const float d = den_f[i] + EPS_SPLAT;
                coef_f[i] = (1.0f - of[i]) * w0 / d;
                gden_f[i] = -(w0 * a) / d;
            }
            if (den_b) {
                const float d = den_b[i] + EPS_SPLAT;
                coef_b[i] = (1.0f - ob[i]) * w1 / d;
                gden_b[i] = -(w1 * b) / d;
            }
        }
    }
}

template <int SL>
__global__ __launch_bounds__(256) void warp_grad_kernel(const float* __restrict__ x, const float* __restrict__ e, const float* __restrict__ flow,
                                                        const float* __restrict__ g, const float* __restrict__ coef,
                                                        const float* __restrict__ gden, const float* __restrict__ g_conf,
                                                        float* __restrict__ gx, float* __restrict__ gm, int N, int C, int H, int W)
{
    constexpr int PIX = 256 / SL;
    __shared__ float part[SL > 1 ? SL : 1][PIX];
    const long long hw = (long long)H * W;
    const long long total = (long long)N * hw;
    const int slice = threadIdx.x / PIX, lane = threadIdx.x % PIX;
    for (long long base = (long long)blockIdx.x * PIX; base < total; base += (long long)gridDim.x * PIX) {
        const long long i = base + lane;
        const bool live = i < total;
        float acc = 0.f, ev = 0.f, bw[4] = {0.f, 0.f, 0.f, 0.f};
        bool any = false;
        Corners c;
        long long n = 0;
        if (live) {
            n = i / hw;
            const long long p = i - n * hw;
            c = corners_of(flow, n, hw, p, H, W);
            any = c.ok[0] || c.ok[1] || c.ok[2] || c.ok[3];
            ev = any ? e[i] : 0.f;                                        // a source that reaches no target: zeros, whatever e is
            bw[0] = c.ax * c.ay, bw[1] = c.bx * c.ay, bw[2] = c.ax * c.by, bw[3] = c.bx * c.by;      // nw, ne, sw, se
            float cw[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) cw[k] = c.ok[k] ? bw[k] * coef[n * hw + c.off[k]] : 0.f;
            const long long at = n * C * hw;
#pragma unroll 4
            for (int ch = slice; ch < C; ch += SL) {
                const long long plane = at + ch * hw;
                float q[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) q[k] = g[plane + c.off[k]];   // off = 0 for a corner outside: a valid address, unused
                float ac = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c.ok[k]) ac += cw[k] * q[k];
                if (gx) gx[plane + p] = any ? ev * ac : 0.f;
                if (gm) acc += x[plane + p] * ac;
            }
        }
        if (!gm) continue;                                                // uniform over the grid: no barrier is skipped by a part of a workgroup
        if (SL > 1) {
            part[slice][lane] = acc;
            __syncthreads();
            if (slice == 0 && live) {
#pragma unroll
                for (int s = 1; s < SL; ++s) acc += part[s][lane];
            }
            __syncthreads();
        }
        if (slice == 0 && live) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c.ok[k]) t += bw[k] * gden[n * hw + c.off[k]];
            gm[i] = (any ? ev * (acc + t) : 0.f) + g_conf[i];
        }
    }
}

inline int grid_for(long long items, int per_block) { return (int)min((long long)8192, (items + per_block - 1) / per_block); }

// channel slices per pixel: a function of (C, H * W) only
inline int slices(int C, long long hw) { return C < 16 ? 1 : hw >= 1024 ? 4 : 16; }

inline bool shape_ok(int N, int C, int H, int W)
{
    return N >= 1 && N <= 65535 && C >= 1 && C <= 65535 && H >= 1 && H <= 16384 && W >= 1 && W <= 16384 && (long long)H * W <= (1LL << 28);
}

}  // namespace

extern "C" int dc_pyramid_exp_f32(const float* metric, float* e, long long n, void* stream)
{
    if (!metric || !e || n <= 0) return DC_ERR_INVALID;
    hipLaunchKernelGGL(exp_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, metric, e, n);
    return dc_launch_status();
}

extern "C" int dc_pyramid_fuse_grad_f32(const float* g, const float* wf, const float* wl, const float* cf, const float* cb,
                                        const float* occ_f, const float* occ_b, const float* den_f, const float* den_b, float* g_cf,
                                        float* g_cb, float* coef_f, float* gden_f, float* coef_b, float* gden_b, int N, int C, int H,
                                        int W, void* stream)
{
    if (!g || !wf || !wl || !cf || !cb || !occ_f || !occ_b || !g_cf || !g_cb || !shape_ok(N, C, H, W)) return DC_ERR_INVALID;
    if (!den_f && !den_b) return DC_ERR_INVALID;
    if ((den_f && (!coef_f || !gden_f)) || (den_b && (!coef_b || !gden_b))) return DC_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const long long hw = (long long)H * W, total = (long long)N * hw;
    switch (slices(C, hw)) {
    case 1:
        hipLaunchKernelGGL(fuse_grad_kernel<1>, dim3(grid_for(total, 256)), dim3(256), 0, st, g, wf, wl, cf, cb, occ_f, occ_b, den_f, den_b,
                           g_cf, g_cb, coef_f, gden_f, coef_b, gden_b, N, C, hw);
        break;
    case 4:
        hipLaunchKernelGGL(fuse_grad_kernel<4>, dim3(grid_for(total, 64)), dim3(256), 0, st, g, wf, wl, cf, cb, occ_f, occ_b, den_f, den_b,
                           g_cf, g_cb, coef_f, gden_f, coef_b, gden_b, N, C, hw);
        break;
    default:
        hipLaunchKernelGGL(fuse_grad_kernel<16>, dim3(grid_for(total, 16)), dim3(256), 0, st, g, wf, wl, cf, cb, occ_f, occ_b, den_f, den_b,
                           g_cf, g_cb, coef_f, gden_f, coef_b, gden_b, N, C, hw);
        break;
    }
    return dc_launch_status();
}

extern "C" int dc_pyramid_warp_grad_f32(const float* x, const float* e, const float* flow, const float* g, const float* coef,
                                        const float* gden, const float* g_conf, float* gx, float* gm, int N, int C, int H, int W,
                                        void* stream)
{
    if (!e || !flow || !g || !coef || !shape_ok(N, C, H, W)) return DC_ERR_INVALID;
    if (!gx && !gm) return DC_ERR_INVALID;
    if (gm && (!x || !gden || !g_conf)) return DC_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const long long hw = (long long)H * W, total = (long long)N * hw;
    switch (slices(C, hw)) {
    case 1:
        hipLaunchKernelGGL(warp_grad_kernel<1>, dim3(grid_for(total, 256)), dim3(256), 0, st, x, e, flow, g, coef, gden, g_conf, gx, gm, N, C, H,
                           W);
        break;
    case 4:
        hipLaunchKernelGGL(warp_grad_kernel<4>, dim3(grid_for(total, 64)), dim3(256), 0, st, x, e, flow, g, coef, gden, g_conf, gx, gm, N, C, H,
                           W);
        break;
    default:
        hipLaunchKernelGGL(warp_grad_kernel<16>, dim3(grid_for(total, 16)), dim3(256), 0, st, x, e, flow, g, coef, gden, g_conf, gx, gm, N, C, H,
                           W);
        break;
    }
    return dc_launch_status();
}
