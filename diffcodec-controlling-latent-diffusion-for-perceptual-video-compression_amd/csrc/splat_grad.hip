// Backward of forward (summation) splatting for gfx950, fp32 NCHW: the reference's `softsplat_ingrad` (controlnet/softsplat.py:368-435)
// and `softsplat_flowgrad` (softsplat.py:439-524).  Both are gathers already — a source pixel reads the four targets around its
// landing point — so no binning is needed and nothing is accumulated across threads in global memory.
//
// ingrad:   one thread per source and channel group, four individually rounded products added in the order NW, NE, SW, SE.
// flowgrad: one pass over the channels yields both components (the reference runs one thread per component and reads `in` and
//           `outgrad` twice).  A workgroup of 256 threads holds 256 / S sources x S channel slices; slice s adds the channels
//           s, s + S, s + 2S, ... in ascending order (corners NW, NE, SW, SE inside a channel), the S partial sums meet in LDS and
//           are added in ascending s by the slice-0 lane.  S = split(C, H*W) only — 1 for few channels, 4 on maps of >= 1024
//           pixels, 16 below (C = 641 at 8x8: 64 sources per image) — so the order of every source's sum is a fixed function of
//           (C, H, W): bit-identical from launch to launch, and the same bits whatever N the image is batched into.
// Every product that feeds an addition passes through rounded() (see splat.hip): nothing is contracted.
#include "dc_common.h"
#include "dc_splat_corners.h"                    // Corners, corners_of: shared with pyramid_grad.hip
#include "../../include/diffcodec_hip.h"

namespace {

__device__ __forceinline__ float rounded(float v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// grid.x strides over the N*H*W sources, grid.y over the channels: a thread forms its source's corners once and serves every
// channel ch = blockIdx.y, blockIdx.y + gridDim.y, ...
__global__ __launch_bounds__(256) void splat_ingrad_kernel(const float* __restrict__ flow, const float* __restrict__ outgrad,
                                                           float* __restrict__ ingrad, int N, int C, int H, int W)
{
    const long long hw = (long long)H * W;
    const long long total = (long long)N * hw;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
        const long long n = g / hw, p = g - n * hw;
        const Corners c = corners_of(flow, n, hw, p, H, W);
        const float w[4] = {rounded(c.ax * c.ay), rounded(c.bx * c.ay), rounded(c.ax * c.by), rounded(c.bx * c.by)};
#pragma unroll 4
        for (int ch = blockIdx.y; ch < C; ch += gridDim.y) {
            const long long plane = (n * C + ch) * hw;
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = outgrad[plane + c.off[k]];     // off = 0 for a corner outside: a valid address, unused
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c.ok[k]) acc += rounded(v[k] * w[k]);
            ingrad[plane + p] = acc;                                          // 0 for a non-finite source: written, not skipped
        }
    }
}

// S channel slices per source, PIX = 256 / S sources per workgroup: thread t = slice (t / PIX), source (t % PIX)
template <int S>
__global__ __launch_bounds__(256) void splat_flowgrad_kernel(const float* __restrict__ in, const float* __restrict__ flow,
                                                             const float* __restrict__ outgrad, float* __restrict__ flowgrad, int N,
                                                             int C, int H, int W)
{
    constexpr int PIX = 256 / S;
    __shared__ float part[S > 1 ? S : 1][PIX][2];
    const long long hw = (long long)H * W;
    const long long total = (long long)N * hw;
    const int slice = threadIdx.x / PIX, lane = threadIdx.x % PIX;
    // the trip count depends on the workgroup alone, so every thread of it reaches the barriers below
    for (long long base = (long long)blockIdx.x * PIX; base < total; base += (long long)gridDim.x * PIX) {
        const long long g = base + lane;
        const bool live = g < total;
        float gx = 0.f, gy = 0.f;
        long long n = 0, p = 0;
        if (live) {
            n = g / hw, p = g - n * hw;
            const Corners c = corners_of(flow, n, hw, p, H, W);
            // d w / d fx (softsplat.py:477-481) and d w / d fy (:483-487): nw, ne, sw, se
            const float dwx[4] = {-c.ay, c.ay, -c.by, c.by};
            const float dwy[4] = {-c.ax, -c.bx, c.ax, c.bx};
            const float* src = in + n * C * hw + p;
            const float* og = outgrad + n * C * hw;
#pragma unroll 8
            for (int ch = slice; ch < C; ch += S) {
                const float v = src[ch * hw];
                const float* o = og + ch * hw;
                float q[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) q[k] = o[c.off[k]];               // off = 0 for a corner outside: a valid address, unused
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c.ok[k]) {
                        const float t = rounded(q[k] * v);
                        gx += rounded(t * dwx[k]);
                        gy += rounded(t * dwy[k]);
                    }
            }
        }
        if (S > 1) {
            part[slice][lane][0] = gx;
            part[slice][lane][1] = gy;
            __syncthreads();
            if (slice == 0 && live) {
#pragma unroll
                for (int s = 1; s < S; ++s) gx += part[s][lane][0], gy += part[s][lane][1];
            }
            __syncthreads();                                              // the next trip overwrites part[][]
        }
        if (slice == 0 && live) {
            flowgrad[(n * 2 + 0) * hw + p] = gx;
            flowgrad[(n * 2 + 1) * hw + p] = gy;
        }
    }
}

inline int grid_for(long long items, int per_block) { return (int)min((long long)8192, (items + per_block - 1) / per_block); }

}  // namespace

// channel slices per source of dc_splat_flowgrad_f32: a function of (C, H*W) only
static inline int flowgrad_split(int C, long long hw) { return C < 16 ? 1 : hw >= 1024 ? 4 : 16; }

extern "C" int dc_splat_ingrad_f32(const float* flow, const float* outgrad, float* ingrad, int N, int C, int H, int W, void* stream)
{
    if (!flow || !outgrad || !ingrad || N <= 0 || C <= 0 || H <= 0 || W <= 0) return DC_ERR_INVALID;
    const int gx = grid_for((long long)N * H * W, 256);
    const int gy = min(C, max(1, 4096 / gx));                            // enough workgroups on a small map, few corner set-ups on a large one
    hipLaunchKernelGGL(splat_ingrad_kernel, dim3(gx, gy), dim3(256), 0, (hipStream_t)stream, flow, outgrad, ingrad, N, C, H, W);
    return dc_launch_status();
}

extern "C" int dc_splat_flowgrad_f32(const float* in, const float* flow, const float* outgrad, float* flowgrad, int N, int C, int H,
                                     int W, void* stream)
{
    if (!in || !flow || !outgrad || !flowgrad || N <= 0 || C <= 0 || H <= 0 || W <= 0) return DC_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const long long hw = (long long)H * W, total = (long long)N * hw;
    switch (flowgrad_split(C, hw)) {
    case 1:
        hipLaunchKernelGGL(splat_flowgrad_kernel<1>, dim3(grid_for(total, 256)), dim3(256), 0, st, in, flow, outgrad, flowgrad, N, C, H, W);
        break;
    case 4:
        hipLaunchKernelGGL(splat_flowgrad_kernel<4>, dim3(grid_for(total, 64)), dim3(256), 0, st, in, flow, outgrad, flowgrad, N, C, H, W);
        break;
    default:
        hipLaunchKernelGGL(splat_flowgrad_kernel<16>, dim3(grid_for(total, 16)), dim3(256), 0, st, in, flow, outgrad, flowgrad, N, C, H, W);
        break;
    }
    return dc_launch_status();
}
