// Backward of the NormFix LPIPS (AlexNet) value of lpips.hip to its images, in exact fp32 for gfx950: the loss of the reference's
// training step (train_controlnet.py:951-955 with controlnet/lpips_loss.py).  The weights are frozen: data gradients only.
//
// The forward runs once (dc_lpips_alex on a caller-owned buffer, so the five post-ReLU maps of the 2N images stay); the backward
// runs on the M = N or 2N images whose operand wants a gradient:
//   tail gradient, one launch per layer: lanes along pixels, the 4 waves split the channels as lpips_tail_kernel does; pass 1 sums
//     the squares, pass 2 the dot product sum_k u_k t_k, pass 3 writes (t_c - u_c dot) / n, masked by the ReLU below (map > 0).
//   conv5 .. conv2 data gradients on v_mfma_f32_32x32x2_f32: a stride-1 "same" convolution of the output-gradient map with
//     K = (co, ky, kx), the taps mirrored (in the packed weights) and the forward's input channels as output channels: the loop of
//     lpips_conv_kernel<KS, CK> (64 x (4 x 32) tile, chunk staged one ahead, ragged edges masked).  The epilogue adds the tail
//     gradient that already lies in the output buffer and applies the ReLU mask of the layer below, so every dgrad reads its
//     operand (tail + above) * (map > 0) straight from its producer.
//   max-pool 3/2 gradients in gather form: every element of the pooled map recomputes the argmax of the at most 2 x 2 windows that
//     contain it (first maximum in raster order) and adds their gradients in window raster order.
//   conv1 data gradient (64 -> 3, 11x11, stride 4), a VALU gather by phase: pixel row iy receives from ky = r, r + 4, r + 8 (< 11),
//     r = (iy + 2) mod 4, at oy = (iy + 2 - ky) / 4.  A wave takes one row phase and its lanes pixels 4 apart, so the tap set and
//     the weight rows are wave-uniform (scalar loads of the K-major forward matrix) and a lane's reads of the LDS-staged gradient
//     tile are consecutive; one LDS read feeds the three image channels.  1 / scale_c and the x2 of normalize are fused in the store.
// Every sum runs in a fixed order and every output element is written once: no atomics, nothing to zero.
#include "dc_f32_mfma.h"
#include "dc_lpips_geom.h"
#include "../../include/diffcodec_hip.h"
#include "../../include/diffcodec_loss_hip.h"

namespace {

constexpr int LG_CO = 64, LG_COLS = 32, LG_ROWS = 4;        // the tile of lpips_conv_kernel
constexpr int LG_LAYERS = 5;
constexpr int LG_CH[LG_LAYERS] = {64, 192, 384, 256, 256};
constexpr int LG_CIN[LG_LAYERS] = {3, 64, 192, 384, 256};
constexpr int LG_KS[LG_LAYERS] = {11, 5, 3, 3, 3};
constexpr int LG_K1 = 364;
constexpr int LG_TAIL_PX = 64;

// ------------------------------------------------------------------------------------------------ tail gradient
// f: [2N][C][HW].  Image m of the M gradient images: m < nx is pair m's first side, the others pair m - nx's second side.
__global__ __launch_bounds__(256) void lpips_tail_grad_kernel(const float* __restrict__ f, int N, int C, int HW,
                                                              const float* __restrict__ lin, const float* __restrict__ g, int nx,
                                                              float* __restrict__ out)
{
#pragma clang fp contract(off)
    __shared__ float sq[2][4][LG_TAIL_PX];
    __shared__ float dt[4][LG_TAIL_PX];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m = blockIdx.y;
    const int p = blockIdx.x * LG_TAIL_PX + lane;
    const bool in = p < HW;
    const bool first = m < nx;
    const int pair = first ? m : m - nx;
    const float* __restrict__ sb = f + (long long)(first ? pair : N + pair) * C * HW + p;      // this side
    const float* __restrict__ ob = f + (long long)(first ? N + pair : pair) * C * HW + p;      // the other side
    float ss = 0.f, so = 0.f;
    for (int c = wv; c < C; c += 4) {
        const float a = in ? sb[(long long)c * HW] : 0.f, b = in ? ob[(long long)c * HW] : 0.f;
        ss = __builtin_fmaf(a, a, ss);
        so = __builtin_fmaf(b, b, so);
    }
    sq[0][wv][lane] = ss;
    sq[1][wv][lane] = so;
    __syncthreads();
    const float ns = sqrtf((((sq[0][0][lane] + sq[0][1][lane]) + sq[0][2][lane]) + sq[0][3][lane]) + (float)C * 1e-8f);
    const float no = sqrtf((((sq[1][0][lane] + sq[1][1][lane]) + sq[1][2][lane]) + sq[1][3][lane]) + (float)C * 1e-8f);
    const float coef = 2.f * g[pair] / (float)HW;
    float s = 0.f;
    for (int c = wv; c < C; c += 4) {
        const float a = in ? sb[(long long)c * HW] : 0.f, b = in ? ob[(long long)c * HW] : 0.f;
        const float u = a / ns;
        const float t = coef * lin[c] * (u - b / no);
        s = __builtin_fmaf(u, t, s);
    }
    dt[wv][lane] = s;
    __syncthreads();
    const float dot = ((dt[0][lane] + dt[1][lane]) + dt[2][lane]) + dt[3][lane];
    if (!in) return;
    float* __restrict__ o = out + (long long)m * C * HW + p;
    for (int c = wv; c < C; c += 4) {
        const float a = sb[(long long)c * HW], b = ob[(long long)c * HW];
        const float u = a / ns;
        const float t = coef * lin[c] * (u - b / no);
        o[(long long)c * HW] = a > 0.f ? (t - u * dot) / ns : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ conv2 .. conv5 data gradient
// x: the gradient at the convolution's output [M][Cin = forward Cout][H][W]; wp: [(co, ky, kx)][Cout = forward Cin], mirrored taps.
// y = (add ? add : 0) + conv, 0 where map <= 0; y may alias add (an element is read and written by the same lane).
template <int KS, int CK>
__global__ __launch_bounds__(256, 2) void lpips_dgrad_kernel(const float* __restrict__ x, const float* __restrict__ wp, const float* add,
                                                             const float* __restrict__ map, float* y, int Cin, int H, int W, int Cout,
                                                             int tiles_x)
{
    constexpr int KK = KS * KS, PAD = KS / 2;
    constexpr int PH = LG_ROWS - 1 + KS, PW = LG_COLS - 1 + KS;
    constexpr int PE = CK * PH * PW, NPE = (PE + 255) / 256;
    constexpr int WROWS = CK * KK;
    constexpr int WP4 = WROWS * (LG_CO / 4), NWP = (WP4 + 255) / 256;
    __shared__ __attribute__((aligned(16))) float Wl[WROWS * LG_CO];
    __shared__ float Pl[PE];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ch = wave & 1, ph = wave >> 1;
    const int j = lane & 31, h = lane >> 5;
    const int ty0 = (blockIdx.x / tiles_x) * LG_ROWS, tx0 = (blockIdx.x % tiles_x) * LG_COLS;
    const int co0 = blockIdx.y * LG_CO, n = blockIdx.z;
    const float* __restrict__ xn = x + (long long)n * Cin * H * W;

    int goff[NPE];
#pragma unroll
    for (int i = 0; i < NPE; ++i) {
        const int e = tid + 256 * i;
        goff[i] = -1;
        if (e < PE) {
            const int ci = e / (PH * PW), r = e - ci * (PH * PW);
            const int py = r / PW, px = r - py * PW;
            const int iy = ty0 - PAD + py, ix = tx0 - PAD + px;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) goff[i] = (ci * H + iy) * W + ix;
        }
    }
    const float* __restrict__ wt = wp + co0;

    float rp[NPE];
    f32x4 rw[NWP];
    auto load_chunk = [&](int c0) {
        const float* xc = xn + (long long)c0 * H * W;
#pragma unroll
        for (int i = 0; i < NPE; ++i) rp[i] = goff[i] >= 0 ? xc[goff[i]] : 0.f;
#pragma unroll
        for (int i = 0; i < NWP; ++i) {
            const int p = tid + 256 * i;
            rw[i] = p < WP4 ? *(const f32x4*)(wt + ((long long)c0 * KK + (p >> 4)) * Cout + (p & 15) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < NPE; ++i) {
            const int e = tid + 256 * i;
            if (e < PE) Pl[e] = rp[i];
        }
#pragma unroll
        for (int i = 0; i < NWP; ++i) {
            const int p = tid + 256 * i;
            if (p < WP4) *(f32x4*)(Wl + p * 4) = rw[i];
        }
    };

    int pbase[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) pbase[b] = (ph * 2 + b) * PW + j + h * (PH * PW);
    const int abase = h * KK * LG_CO + ch * 32 + j;

    f32x16 acc[2];
    dc_f32_zero(acc);

    const int nchunk = Cin / CK;
    load_chunk(0);
    for (int c = 0; c < nchunk; ++c) {
        __syncthreads();
        store_chunk();
        __syncthreads();
        if (c + 1 < nchunk) load_chunk((c + 1) * CK);
#pragma unroll
        for (int cp = 0; cp < CK / 2; ++cp) {
#pragma unroll
            for (int tap = 0; tap < KK; ++tap) {
                const float a = Wl[abase + (cp * 2 * KK + tap) * LG_CO];
                const int poff = cp * 2 * (PH * PW) + (tap / KS) * PW + (tap % KS);
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Pl[pbase[b] + poff], acc[b], 0, 0, 0);
            }
        }
    }

    // epilogue: + the gradient already in place (the tail's), then the ReLU mask of the layer below; masked at the ragged edges
    const int ox = tx0 + j;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int oy = ty0 + ph * 2 + b;
        if (oy < H && ox < W) {
            const long long base = (((long long)n * Cout + co0 + ch * 32) * H + oy) * W + ox;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long i = base + (long long)dc_f32_channel(r, h) * H * W;
                float v = acc[b][r];
                if (add) v += add[i];
                if (map) v = map[i] > 0.f ? v : 0.f;
                y[i] = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ max_pool2d(3, 2) gradient
__device__ __forceinline__ int lg_window_argmax(const float* __restrict__ p, int W)
{
    float m = p[0];
    int arg = 0;
#pragma unroll
    for (int q = 1; q < 9; ++q) {
        const float v = p[(q / 3) * W + (q % 3)];
        if (v > m) m = v, arg = q;                         // strict: the first maximum in raster order keeps the gradient
    }
    return arg;
}

__global__ __launch_bounds__(256) void lpips_pool_grad_kernel(const float* __restrict__ gp, const float* __restrict__ map, const float* add,
                                                              float* y, int H, int W, int Ho, int Wo, long long total)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int x = (int)(i % W);
        const long long t = i / W;
        const int yy = (int)(t % H);
        const long long plane = t / H;
        float v = add ? add[i] : 0.f;
        if (map[i] > 0.f) {
            const float* __restrict__ mp = map + plane * H * W;
            const float* __restrict__ g = gp + plane * Ho * Wo;
            const int oy_lo = yy >= 2 ? (yy - 1) >> 1 : 0, oy_hi = min(yy >> 1, Ho - 1);
            const int ox_lo = x >= 2 ? (x - 1) >> 1 : 0, ox_hi = min(x >> 1, Wo - 1);
            for (int oy = oy_lo; oy <= oy_hi; ++oy)
                for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                    const int arg = lg_window_argmax(mp + (2 * oy) * W + 2 * ox, W);
                    if (arg == (yy - 2 * oy) * 3 + (x - 2 * ox)) v += g[oy * Wo + ox];
                }
        } else {
            v = 0.f;
        }
        y[i] = v;
    }
}

// ------------------------------------------------------------------------------------------------ conv1 data gradient
constexpr int G1_TH = 16, G1_TW = 64;                        // image pixels per workgroup
constexpr int G1_GH = G1_TH / 4 + 3, G1_GW = G1_TW / 4 + 3;   // gradient tile: 7 x 19 per channel
constexpr int G1_GP = G1_GH * G1_GW;

__global__ __launch_bounds__(256) void lpips_conv1_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ wp,
                                                                float* __restrict__ dx, float* __restrict__ dy, int nx, int H, int W,
                                                                int Ho, int Wo, int tiles_x, int normalize)
{
#pragma clang fp contract(off)
    __shared__ float Gl[LG_CO * G1_GP];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int y0 = (blockIdx.x / tiles_x) * G1_TH, x0 = (blockIdx.x % tiles_x) * G1_TW, m = blockIdx.z;
    const int gy0 = y0 / 4 - 2, gx0 = x0 / 4 - 2;
    const float* __restrict__ gm = g + (long long)m * LG_CO * Ho * Wo;
    for (int e = tid; e < LG_CO * G1_GP; e += 256) {
        const int co = e / G1_GP, r = e - co * G1_GP;
        const int py = r / G1_GW, px = r - py * G1_GW;
        const int oy = gy0 + py, ox = gx0 + px;
        Gl[e] = (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo) ? gm[((long long)co * Ho + oy) * Wo + ox] : 0.f;
    }
    __syncthreads();

    const int a = lane >> 4, b = lane & 15;
    const int iy = y0 + 4 * a + wave;                         // the wave's row phase
    const int ry = (wave + 2) & 3, qy = (wave + 2) >> 2;
    float* __restrict__ dst = m < nx ? dx + (long long)m * 3 * H * W : dy + (long long)(m - nx) * 3 * H * W;
    const float two = normalize ? 2.f : 1.f;
#pragma unroll
    for (int px = 0; px < 4; ++px) {                          // column phase
        const int ix = x0 + 4 * b + px;
        const int rx = (px + 2) & 3, qx = (px + 2) >> 2;
        float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
        for (int ty = 0; ty < 3; ++ty) {
            const int ky = ry + 4 * ty;
            if (ky >= 11) break;
            const int gy = a + qy - ty + 2;
#pragma unroll
            for (int tx = 0; tx < 3; ++tx) {
                const int kx = rx + 4 * tx;
                if (kx >= 11) break;
                const float* gl = Gl + gy * G1_GW + (b + qx - tx + 2);
                const float* __restrict__ w0 = wp + (long long)(ky * 11 + kx) * LG_CO;      // k = (c, ky, kx), K-major rows of 64
                const float* __restrict__ w1 = w0 + 121 * LG_CO;
                const float* __restrict__ w2 = w0 + 242 * LG_CO;
#pragma unroll 8
                for (int co = 0; co < LG_CO; ++co) {
                    const float gv = gl[co * G1_GP];
                    acc0 = __builtin_fmaf(w0[co], gv, acc0);
                    acc1 = __builtin_fmaf(w1[co], gv, acc1);
                    acc2 = __builtin_fmaf(w2[co], gv, acc2);
                }
            }
        }
        if (iy < H && ix < W) {
            const long long o = (long long)iy * W + ix;
            dst[o] = acc0 / .458f * two;
            dst[o + (long long)H * W] = acc1 / .448f * two;
            dst[o + 2ll * H * W] = acc2 / .450f * two;
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct lg_dweights {
    long long w[LG_LAYERS], total;           // w[l]: conv(l + 1)'s mirrored matrix, l = 1 .. 4
};
lg_dweights lg_dweight_layout()
{
    lg_dweights o;
    long long off = 0;
    o.w[0] = 0;
    for (int l = 1; l < LG_LAYERS; ++l) {
        o.w[l] = off;
        off += (long long)LG_CH[l] * LG_KS[l] * LG_KS[l] * LG_CIN[l];
    }
    o.total = off;
    return o;
}

// offsets (floats) of the forward vector: per layer [K][Cout] then the bias, then the five lin vectors (lpips.hip)
void lg_forward_layout(long long& w1, long long lin[LG_LAYERS])
{
    long long off = 0;
    w1 = 0;
    for (int l = 0; l < LG_LAYERS; ++l) off += (long long)(l == 0 ? LG_K1 : LG_CIN[l] * LG_KS[l] * LG_KS[l]) * LG_CH[l] + LG_CH[l];
    for (int l = 0; l < LG_LAYERS; ++l) {
        lin[l] = off;
        off += LG_CH[l];
    }
}

struct lg_plan {
    dc_lpips_geom g;
    int M;
    long long d_off[LG_LAYERS], p_off[2], total;     // bytes: the gradient at relu(l + 1); at pooled relu1, relu2
};

bool make_lg_plan(int N, int H, int W, int sides, lg_plan& p)
{
    if (N <= 0 || N > 32767 || sides < 1 || sides > 3 || !dc_lpips_geometry(2 * N, N, H, W, &p.g)) return false;
    p.M = sides == 3 ? 2 * N : N;
    dc_f32_bump<1> ws;
    for (int l = 0; l < LG_LAYERS; ++l) p.d_off[l] = ws.take((long long)p.M * LG_CH[l] * p.g.h[l] * p.g.w[l] * 4);
    for (int l = 0; l < 2; ++l) p.p_off[l] = ws.take((long long)p.M * LG_CH[l] * p.g.h[l + 1] * p.g.w[l + 1] * 4);
    p.total = ws.off;
    return true;
}

bool lg_tail_grad(int layer, const float* f, int N, int HW, int sides, const float* weights, const float* g, float* out, hipStream_t st)
{
    if (!f || !weights || !g || !out || layer < 0 || layer >= LG_LAYERS || N <= 0 || N > 32767 || HW <= 0 || HW > (1 << 28) ||
        sides < 1 || sides > 3)
        return false;
    long long w1, lin[LG_LAYERS];
    lg_forward_layout(w1, lin);
    const int M = sides == 3 ? 2 * N : N, nx = (sides & 1) ? N : 0;
    hipLaunchKernelGGL(lpips_tail_grad_kernel, dim3((HW + LG_TAIL_PX - 1) / LG_TAIL_PX, M), dim3(256), 0, st, f, N, LG_CH[layer], HW,
                       weights + lin[layer], g, nx, out);
    return true;
}

bool lg_conv_dgrad(int layer, const float* gin, int M, int H, int W, const float* dw, const float* add, const float* map, float* y,
                   hipStream_t st)
{
    if (!gin || !dw || !y || y == gin || layer < 1 || layer >= LG_LAYERS || M <= 0 || M > 65535 || H <= 0 || W <= 0 || H > 4096 || W > 4096)
        return false;
    const float* w = dw + lg_dweight_layout().w[layer];
    const int tiles_x = (W + LG_COLS - 1) / LG_COLS, tiles_y = (H + LG_ROWS - 1) / LG_ROWS;
    const dim3 grid(tiles_x * tiles_y, LG_CIN[layer] / LG_CO, M);
    if (layer == 1)
        hipLaunchKernelGGL((lpips_dgrad_kernel<5, 4>), grid, dim3(256), 0, st, gin, w, add, map, y, LG_CH[layer], H, W, LG_CIN[layer], tiles_x);
    else
        hipLaunchKernelGGL((lpips_dgrad_kernel<3, 8>), grid, dim3(256), 0, st, gin, w, add, map, y, LG_CH[layer], H, W, LG_CIN[layer], tiles_x);
    return true;
}

bool lg_pool_grad(const float* gp, const float* map, const float* add, long long planes, int H, int W, float* y, hipStream_t st)
{
    if (!gp || !map || !y || y == gp || planes <= 0 || H < 3 || W < 3 || H > 16384 || W > 16384 || planes * H * W > (1ll << 40)) return false;
    const long long total = planes * H * W;
    hipLaunchKernelGGL(lpips_pool_grad_kernel, dim3(dc_f32_blocks(total, 8192)), dim3(256), 0, st, gp, map, add, y, H, W, (H - 3) / 2 + 1,
                       (W - 3) / 2 + 1, total);
    return true;
}

bool lg_conv1_dgrad(const float* gin, int M, int nx, int H, int W, int normalize, const float* weights, float* dx, float* dy, hipStream_t st)
{
    dc_lpips_geom g;
    if (!gin || !weights || M <= 0 || M > 65535 || nx < 0 || nx > M || (nx > 0 && !dx) || (nx < M && !dy) || !dc_lpips_geometry(M, 0, H, W, &g))
        return false;
    const int tiles_x = (W + G1_TW - 1) / G1_TW, tiles_y = (H + G1_TH - 1) / G1_TH;
    hipLaunchKernelGGL(lpips_conv1_dgrad_kernel, dim3(tiles_x * tiles_y, 1, M), dim3(256), 0, st, gin, weights, dx, dy, nx, H, W, g.h[0],
                       g.w[0], tiles_x, normalize);
    return true;
}

}  // namespace

extern "C" int dc_lpips_dgrad_weight_floats(void) { return (int)lg_dweight_layout().total; }

extern "C" long long dc_lpips_keep_ws_bytes(int N, int H, int W) { return dc_lpips_ws_bytes(N, H, W); }

extern "C" long long dc_lpips_train_ws_bytes(int N, int H, int W, int sides)
{
    lg_plan p;
    return make_lg_plan(N, H, W, sides, p) ? p.total : -1;
}

extern "C" int dc_lpips_alex_keep(const float* x, const float* y, const long long* strides, int N, int H, int W, int normalize,
                                  const float* weights, void* keep, double* out, void* stream)
{
    return dc_lpips_alex(x, y, 0, strides, N, H, W, normalize, 1, weights, keep, out, stream);
}

extern "C" int dc_lpips_tail_grad(int layer, const float* f, int N, int HW, int sides, const float* weights, const float* g, float* out,
                                  void* stream)
{
    return lg_tail_grad(layer, f, N, HW, sides, weights, g, out, (hipStream_t)stream) ? dc_launch_status() : DC_ERR_INVALID;
}

extern "C" int dc_lpips_conv_dgrad(int layer, const float* gin, int M, int H, int W, const float* dweights, const float* add,
                                   const float* map, float* y, void* stream)
{
    return lg_conv_dgrad(layer, gin, M, H, W, dweights, add, map, y, (hipStream_t)stream) ? dc_launch_status() : DC_ERR_INVALID;
}

extern "C" int dc_lpips_pool_grad(const float* gp, const float* map, const float* add, int planes, int H, int W, float* y, void* stream)
{
    return lg_pool_grad(gp, map, add, planes, H, W, y, (hipStream_t)stream) ? dc_launch_status() : DC_ERR_INVALID;
}

extern "C" int dc_lpips_conv1_dgrad(const float* gin, int M, int nx, int H, int W, int normalize, const float* weights, float* dx,
                                    float* dy, void* stream)
{
    return lg_conv1_dgrad(gin, M, nx, H, W, normalize, weights, dx, dy, (hipStream_t)stream) ? dc_launch_status() : DC_ERR_INVALID;
}

extern "C" int dc_lpips_alex_backward(const void* keep, const float* g, int N, int H, int W, int normalize, int sides,
                                      const float* weights, const float* dweights, void* ws, float* dx, float* dy, void* stream)
{
    lg_plan p;
    if (!keep || !g || !weights || !dweights || !ws || !make_lg_plan(N, H, W, sides, p) || ((sides & 1) && !dx) || ((sides & 2) && !dy))
        return DC_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int M = p.M, nx = (sides & 1) ? N : 0;
    const float* f[LG_LAYERS];      // the kept maps of all 2N images
    const float* fm[LG_LAYERS];     // the maps of the M gradient images (contiguous: all 2N, the first N or the last N)
    float* d[LG_LAYERS];
    for (int l = 0; l < LG_LAYERS; ++l) {
        f[l] = (const float*)((const char*)keep + p.g.feat_off[l]);
        fm[l] = f[l] + (sides == 2 ? (long long)N * LG_CH[l] * p.g.h[l] * p.g.w[l] : 0);
        d[l] = (float*)((char*)ws + p.d_off[l]);
    }
    float* pl[2] = {(float*)((char*)ws + p.p_off[0]), (float*)((char*)ws + p.p_off[1])};
    for (int l = 0; l < LG_LAYERS; ++l)
        if (!lg_tail_grad(l, f[l], N, p.g.h[l] * p.g.w[l], sides, weights, g + (long long)l * N, d[l], st)) return DC_ERR_INVALID;
    bool ok = lg_conv_dgrad(4, d[4], M, p.g.h[4], p.g.w[4], dweights, d[3], fm[3], d[3], st);
    ok = ok && lg_conv_dgrad(3, d[3], M, p.g.h[3], p.g.w[3], dweights, d[2], fm[2], d[2], st);
    ok = ok && lg_conv_dgrad(2, d[2], M, p.g.h[2], p.g.w[2], dweights, nullptr, nullptr, pl[1], st);
    ok = ok && lg_pool_grad(pl[1], fm[1], d[1], (long long)M * LG_CH[1], p.g.h[1], p.g.w[1], d[1], st);
    ok = ok && lg_conv_dgrad(1, d[1], M, p.g.h[1], p.g.w[1], dweights, nullptr, nullptr, pl[0], st);
    ok = ok && lg_pool_grad(pl[0], fm[0], d[0], (long long)M * LG_CH[0], p.g.h[0], p.g.w[0], d[0], st);
    ok = ok && lg_conv1_dgrad(d[0], M, nx, H, W, normalize, weights, dx, dy, st);
    return ok ? dc_launch_status() : DC_ERR_INVALID;
}
