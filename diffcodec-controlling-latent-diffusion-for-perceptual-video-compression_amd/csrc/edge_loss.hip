// Sobel edge loss of the reference's training step (controlnet/edge_loss.py:22-38, train_controlnet.py:1149-1156) and its gradient,
// fp32 for gfx950.  With v = (x + 1) / 2 per channel plane, gx / gy = the Sobel x / y correlations with zero padding 1 and
// e = sqrt(gx^2 + gy^2 + 1e-6), the loss is l1_loss(e(pred), e(target), reduction).
//   forward: one launch; a workgroup stages a 16 x 64 tile of both planes with halo 1, forms |e_p - e_t| per pixel and either
//     stores it ('none') or reduces it to one fp64 partial; a second launch sums the partials in a fixed order ('mean' | 'sum').
//   backward: one gather launch per differentiable operand.  The tile is staged with halo 2, the fields
//     A = g sign(e_p - e_t) gx / e and B = g sign(e_p - e_t) gy / e of the operand's own plane are recomputed on the tile with halo
//     1 (zero outside the image), and every pixel gathers d = 1/2 sum_taps (SX A + SY B) from its 8 neighbours: every output
//     element is written once, nothing is accumulated in memory.  sign(0) = 0, so equal operands give a zero gradient.
#include "dc_f32_mfma.h"
#include "../../include/diffcodec_loss_hip.h"

namespace {

constexpr int SB_TH = 16, SB_TW = 64;        // pixels per workgroup

struct sb_field {
    float gx, gy, e;
};

// p: the pixel's own element of a staged tile of v = (x + 1) / 2 with row pitch `pitch` (zero outside the image)
__device__ __forceinline__ sb_field sb_sobel(const float* p, int pitch)
{
#pragma clang fp contract(off)
    const float a = p[-pitch - 1], b = p[-pitch], c = p[-pitch + 1], d = p[-1], f = p[1], g = p[pitch - 1], h = p[pitch], i = p[pitch + 1];
    sb_field o;
    o.gx = ((c - a) + 2.f * (f - d)) + (i - g);
    o.gy = ((g - a) + 2.f * (h - b)) + (i - c);
    o.e = sqrtf((o.gx * o.gx + o.gy * o.gy) + 1e-6f);
    return o;
}

template <int HALO>
__device__ __forceinline__ void sb_stage(float* tile, const float* __restrict__ src, long long sh, long long sw, int y0, int x0, int H, int W)
{
#pragma clang fp contract(off)
    constexpr int PH = SB_TH + 2 * HALO, PW = SB_TW + 2 * HALO;
    for (int e = threadIdx.x; e < PH * PW; e += 256) {
        const int py = e / PW, px = e - py * PW;
        const int y = y0 - HALO + py, x = x0 - HALO + px;
        tile[e] = (y >= 0 && y < H && x >= 0 && x < W) ? (src[y * sh + x * sw] + 1.f) / 2.f : 0.f;
    }
}

struct sb_tile {
    int y0, x0;
    long long plane;
};
__device__ __forceinline__ sb_tile sb_where(int tiles_x, int tiles)
{
    const long long b = blockIdx.x;
    const int t = (int)(b % tiles);
    return {(t / tiles_x) * SB_TH, (t % tiles_x) * SB_TW, b / tiles};
}

__global__ __launch_bounds__(256) void sobel_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target, dc_strides4 sp,
                                                         dc_strides4 st, int C, int H, int W, int tiles_x, int tiles,
                                                         float* __restrict__ out_map, double* __restrict__ part)
{
    constexpr int PW = SB_TW + 2;
    __shared__ float P[(SB_TH + 2) * PW], T[(SB_TH + 2) * PW];
    __shared__ double red[4];
    const sb_tile w = sb_where(tiles_x, tiles);
    const long long n = w.plane / C, c = w.plane % C;
    sb_stage<1>(P, pred + n * sp.n + c * sp.c, sp.h, sp.w, w.y0, w.x0, H, W);
    sb_stage<1>(T, target + n * st.n + c * st.c, st.h, st.w, w.y0, w.x0, H, W);
    __syncthreads();
    const int lx = threadIdx.x & 63, ly0 = threadIdx.x >> 6;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < SB_TH / 4; ++k) {
        const int ly = ly0 + 4 * k, y = w.y0 + ly, x = w.x0 + lx;
        if (y < H && x < W) {
            const int o = (ly + 1) * PW + lx + 1;
            const float v = fabsf(sb_sobel(P + o, PW).e - sb_sobel(T + o, PW).e);
            if (out_map) out_map[(w.plane * H + y) * W + x] = v;
            s += (double)v;
        }
    }
    if (!part) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lx == 0) red[ly0] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one wave: lane t sums partials t, t + 64, ... in order, a fixed butterfly sums the lanes
__global__ __launch_bounds__(64) void sobel_finalize_kernel(const double* __restrict__ part, long long count, double divide,
                                                            double* __restrict__ out)
{
    double s = 0.0;
    for (long long i = threadIdx.x; i < count; i += 64) s += part[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) out[0] = s / divide;
}

__global__ __launch_bounds__(256) void sobel_grad_kernel(const float* __restrict__ pred, const float* __restrict__ target, dc_strides4 sp,
                                                         dc_strides4 st, int C, int H, int W, int tiles_x, int tiles, int side,
                                                         const float* __restrict__ gout, int per_element, float scale,
                                                         float* __restrict__ grad)
{
#pragma clang fp contract(off)
    constexpr int PW = SB_TW + 4, FW = SB_TW + 2, FH = SB_TH + 2;
    __shared__ float P[(SB_TH + 4) * PW], T[(SB_TH + 4) * PW];
    __shared__ float A[FH * FW], B[FH * FW];
    const sb_tile w = sb_where(tiles_x, tiles);
    const long long n = w.plane / C, c = w.plane % C;
    sb_stage<2>(P, pred + n * sp.n + c * sp.c, sp.h, sp.w, w.y0, w.x0, H, W);
    sb_stage<2>(T, target + n * st.n + c * st.c, st.h, st.w, w.y0, w.x0, H, W);
    __syncthreads();
    for (int e = threadIdx.x; e < FH * FW; e += 256) {
        const int fy = e / FW, fx = e - fy * FW;
        const int y = w.y0 - 1 + fy, x = w.x0 - 1 + fx;
        float av = 0.f, bv = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const int o = (fy + 1) * PW + fx + 1;
            const sb_field p = sb_sobel(P + o, PW), t = sb_sobel(T + o, PW);
            const float diff = side ? t.e - p.e : p.e - t.e;
            const float sg = diff > 0.f ? 1.f : diff < 0.f ? -1.f : 0.f;
            const float gq = (per_element ? gout[(w.plane * H + y) * W + x] : gout[0]) * scale * sg;
            const sb_field own = side ? t : p;
            av = gq * own.gx / own.e;
            bv = gq * own.gy / own.e;
        }
        A[e] = av;
        B[e] = bv;
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, ly0 = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < SB_TH / 4; ++k) {
        const int ly = ly0 + 4 * k, y = w.y0 + ly, x = w.x0 + lx;
        if (y < H && x < W) {
            // gx(q) holds v(p) with SX[p - q]: p collects A(q) SX[p - q] + B(q) SY[p - q] over its neighbours q
            const float* a = A + (ly + 1) * FW + lx + 1;
            const float* b = B + (ly + 1) * FW + lx + 1;
            const float dxs = ((a[FW - 1] - a[FW + 1]) + 2.f * (a[-1] - a[1])) + (a[-FW - 1] - a[-FW + 1]);
            const float dys = ((b[-FW - 1] - b[FW - 1]) + 2.f * (b[-FW] - b[FW])) + (b[-FW + 1] - b[FW + 1]);
            grad[(w.plane * H + y) * W + x] = (dxs + dys) / 2.f;
        }
    }
}

bool sb_shape(int N, int C, int H, int W, int& tiles_x, int& tiles, long long& blocks)
{
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || H > 32768 || W > 32768 || (long long)N * C > (1ll << 30)) return false;
    tiles_x = (W + SB_TW - 1) / SB_TW;
    tiles = tiles_x * ((H + SB_TH - 1) / SB_TH);
    blocks = (long long)N * C * tiles;
    return blocks <= 0x7fffffffll;
}

}  // namespace

extern "C" long long dc_sobel_edge_ws_bytes(int N, int C, int H, int W)
{
    int tx, t;
    long long blocks;
    return sb_shape(N, C, H, W, tx, t, blocks) ? blocks * 8 : -1;
}

extern "C" int dc_sobel_edge_loss(const float* pred, const float* target, const long long* strides, int N, int C, int H, int W,
                                  int reduction, void* ws, float* out_map, double* out, void* stream)
{
    int tiles_x, tiles;
    long long blocks;
    if (!pred || !target || !strides || reduction < 0 || reduction > 2 || !sb_shape(N, C, H, W, tiles_x, tiles, blocks) ||
        (reduction == 0 ? !out_map : (!ws || !out)))
        return DC_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const dc_strides4 sp(strides), stt(strides + 4);
    hipLaunchKernelGGL(sobel_loss_kernel, dim3((unsigned)blocks), dim3(256), 0, st, pred, target, sp, stt, C, H, W, tiles_x, tiles,
                       reduction == 0 ? out_map : (float*)nullptr, reduction == 0 ? (double*)nullptr : (double*)ws);
    if (reduction != 0)
        hipLaunchKernelGGL(sobel_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, blocks,
                           reduction == 1 ? (double)N * C * H * W : 1.0, out);
    return dc_launch_status();
}

extern "C" int dc_sobel_edge_grad(const float* pred, const float* target, const long long* strides, int N, int C, int H, int W, int side,
                                  const float* gout, int per_element, float scale, float* grad, void* stream)
{
    int tiles_x, tiles;
    long long blocks;
    if (!pred || !target || !strides || !gout || !grad || side < 0 || side > 1 || !sb_shape(N, C, H, W, tiles_x, tiles, blocks))
        return DC_ERR_INVALID;
    const dc_strides4 sp(strides), stt(strides + 4);
    hipLaunchKernelGGL(sobel_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pred, target, sp, stt, C, H, W,
                       tiles_x, tiles, side, gout, per_element ? 1 : 0, scale, grad);
    return dc_launch_status();
}
