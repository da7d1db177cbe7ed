// FID features (test_utils.py:14,39: torchmetrics FrechetInceptionDistance(feature=64)): the InceptionV3 stem of the FID network up
// to its first max-pool, 64 pooled features per image, and the per-side sums the Frechet distance is formed from.  Exact fp32 for
// gfx950 on v_mfma_f32_32x32x2_f32; every sum runs in a fixed order and there are no float atomics, so results are bitwise
// reproducible, an image's features do not depend on its position in the batch, and the launches only enqueue on the caller's
// stream (graph-capturable).
//
//   resize    TF1-legacy bilinear to 299 x 299 (no half-pixel offset: p = o * (I / 299), i0 = floor(p), i1 = min(i0 + 1, I - 1)),
//             then (x - 128) / 128, written as a [N,3,299,299] fp32 plane by its own kernel.  The source position is formed in fp64
//             (299 x 2 values per image, exact against the restatement); the taps are blended in fp32.  A separate plane rather than a
//             gather inside conv1's patch load: conv1 reads every resized pixel 2.25 times, and an arbitrary H x W source makes the
//             patch a per-tile rectangle of unknown size; 1.07 MB per image of extra traffic is noise next to the 11 MB of maps.
//   conv      three conv + BatchNorm(eval) + ReLU blocks, implicit GEMM  D[co][pixel] += W[co][k] * X[k][pixel], the scheme of
//             lpips.hip: weights packed K-major ([K = (ci, ky, kx)][Cout]), a chunk of CK input channels and its weight rows staged in
//             LDS, ragged edges masked in the patch load (zero padding materialised in LDS) and in the store.  Workgroup = 4 waves,
//             tile = Cout channels x (4 rows x 32 columns); wave w takes row w and all Cout / 32 channel tiles (one B read per
//             Cout / 32 MFMAs).  One k-step is a pair of consecutive k of the chunk: lane half h takes k = 2 kp + h.  conv1's K = 27
//             is padded to 28 with a zero weight row (the padded k reads the tap before it).  BatchNorm is one fmaf(acc, s, t) per
//             channel, s and t formed in fp64 when the weights are packed.
//   pool      max-pool 3 x 3 stride 2 (no padding) of the 64 x 147 x 147 map and its spatial mean: one workgroup per (image,
//             channel), per-thread fp64 sums in a fixed order, a fixed butterfly, one fp32 feature.
//   state     n, sum f [64], sum f f^T [64][64] in fp64: one thread per entry adds the rows image by image in batch order, so
//             update(a); update(b) leaves the bits of update(cat(a, b)).
#include "dc_f32_mfma.h"
#include "../../include/diffcodec_hip.h"

namespace {

constexpr int FD_SIZE = 299;                // the network's input
constexpr int FD_COLS = 32, FD_ROWS = 4;    // output pixels per workgroup: FD_ROWS rows of FD_COLS columns
constexpr int FD_FEAT = 64;
constexpr int FD_STATE = 1 + FD_FEAT + FD_FEAT * FD_FEAT;
constexpr int FD_H1 = 149, FD_H2 = 147, FD_HP = 73;

// ------------------------------------------------------------------------------------------------ resize + scale
template <typename T>
__device__ __forceinline__ float fd_load(const T* __restrict__ p, long long i)
{
#pragma clang fp contract(off)
    if constexpr (sizeof(T) == 1) {
        return (float)p[i];
    } else {                                               // a [0,1] float image is taken as (x * 255) truncated to uint8
        const float v = fminf(fmaxf(p[i] * 255.f, 0.f), 255.f);
        return truncf(v);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void fid_resize_kernel(const T* __restrict__ x, dc_strides4 s, int H, int W, float* __restrict__ y,
                                                         long long total)
{
#pragma clang fp contract(off)
    const double sy = (double)H / (double)FD_SIZE, sx = (double)W / (double)FD_SIZE;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ox = (int)(i % FD_SIZE);
        long long t = i / FD_SIZE;
        const int oy = (int)(t % FD_SIZE);
        t /= FD_SIZE;
        const int c = (int)(t % 3);
        const long long n = t / 3;
        const double py = (double)oy * sy, px = (double)ox * sx;
        const int y0 = (int)floor(py), x0 = (int)floor(px);
        const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
        const float ly = (float)(py - (double)y0), lx = (float)(px - (double)x0);
        const long long b = n * s.n + c * s.c;
        const float tl = fd_load(x, b + y0 * s.h + x0 * s.w), tr = fd_load(x, b + y0 * s.h + x1 * s.w);
        const float bl = fd_load(x, b + y1 * s.h + x0 * s.w), br = fd_load(x, b + y1 * s.h + x1 * s.w);
        const float top = tl + (tr - tl) * lx, bot = bl + (br - bl) * lx;
        y[i] = ((top + (bot - top) * ly) - 128.f) / 128.f;
    }
}

// ------------------------------------------------------------------------------------------------ conv 3x3 + BatchNorm + ReLU
template <int CK, int S>
struct fd_geom {
    static constexpr int PH = (FD_ROWS - 1) * S + 3, PW = (FD_COLS - 1) * S + 3;
    static constexpr int PE = CK * PH * PW;
    static constexpr int KC = CK * 9, KCP = (KC + 1) & ~1;               // k rows of a chunk, padded to whole pairs
    static __device__ constexpr int off(int k) { return dc_f32_patch_off<3, PW, PH * PW, KC>(k); }   // k = (ci, ky, kx)
};

// x [N][CIN][H][W] -> y [N][CO][Ho][Wo], wp [(CIN / CK) * KC (+ pad)][CO] K-major, bn_s / bn_t [CO]
template <int CIN, int CK, int CO, int S, int PAD>
__global__ __launch_bounds__(256) void fid_conv_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                       const float* __restrict__ bn_s, const float* __restrict__ bn_t,
                                                       float* __restrict__ y, int H, int W, int Ho, int Wo, int tiles_x)
{
    using G = fd_geom<CK, S>;
    constexpr int NC = CO / 32, NCHUNK = CIN / CK;
    static_assert(CIN % CK == 0 && CO % 32 == 0 && (NCHUNK == 1 || G::KC == G::KCP), "chunks must tile K");
    __shared__ __attribute__((aligned(16))) float Wl[G::KCP * CO];
    __shared__ float Pl[G::PE];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int ty0 = (blockIdx.x / tiles_x) * FD_ROWS, tx0 = (blockIdx.x % tiles_x) * FD_COLS;
    const int n = blockIdx.z;
    const float* __restrict__ xn = x + (long long)n * CIN * H * W;
    const int iy0 = ty0 * S - PAD, ix0 = tx0 * S - PAD;

    f32x16 acc[NC];
    dc_f32_zero(acc);

    const int pbase = wave * S * G::PW + j * S;
    const int abase = h * CO + j;
    for (int c = 0; c < NCHUNK; ++c) {
        if (c) __syncthreads();                                          // everyone is done reading the previous chunk
        const f32x4* __restrict__ wc = (const f32x4*)(wp + (long long)c * G::KC * CO);
        for (int p = tid; p < G::KCP * CO / 4; p += 256) ((f32x4*)Wl)[p] = wc[p];
        const float* __restrict__ xc = xn + (long long)c * CK * H * W;
        for (int e = tid; e < G::PE; e += 256) {
            const int ci = e / (G::PH * G::PW), r = e - ci * (G::PH * G::PW);
            const int py = r / G::PW, px = r - py * G::PW;
            const int iy = iy0 + py, ix = ix0 + px;
            Pl[e] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? xc[((long long)ci * H + iy) * W + ix] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kp = 0; kp < G::KCP / 2; ++kp) {                       // lane half h takes k = 2 kp + h
            const int poff = h ? G::off(2 * kp + 1) : G::off(2 * kp);
            dc_f32_kpair(acc, NC, &Wl[abase + kp * 2 * CO], Pl[pbase + poff]);
        }
    }

    // epilogue: BatchNorm as one fma + ReLU, masked at the ragged edges
    const int oy = ty0 + wave, ox = tx0 + j;
    if (oy < Ho && ox < Wo) {
        float* __restrict__ yo = y + (((long long)n * CO) * Ho + oy) * Wo + ox;
#pragma unroll
        for (int q = 0; q < NC; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int col = dc_f32_channel(r, h, q * 32);
                yo[(long long)col * Ho * Wo] = fmaxf(__builtin_fmaf(acc[q][r], bn_s[col], bn_t[col]), 0.f);
            }
    }
}

// ------------------------------------------------------------------------------------------------ max-pool 3/2 + spatial mean
// x [N][C][H][W] -> feat [N][C] (and pooled [N][C][Hp][Wp] when given); grid (C, N): one workgroup per plane
__global__ __launch_bounds__(256) void fid_pool_mean_kernel(const float* __restrict__ x, float* __restrict__ pooled,
                                                            float* __restrict__ feat, int H, int W, int Hp, int Wp)
{
    __shared__ double red[4];
    const long long plane = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    const float* __restrict__ xp = x + plane * H * W;
    const int area = Hp * Wp;
    double s = 0.0;
    for (int i = threadIdx.x; i < area; i += 256) {
        const int oy = i / Wp, ox = i - oy * Wp;
        const float* p = xp + (2 * oy) * W + 2 * ox;                     // every window lies inside the map
        float m = p[0];
#pragma unroll
        for (int q = 1; q < 9; ++q) m = fmaxf(m, p[(q / 3) * W + (q % 3)]);
        if (pooled) pooled[plane * area + i] = m;
        s += (double)m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) feat[plane] = (float)((((red[0] + red[1]) + red[2]) + red[3]) / (double)area);
}

// ------------------------------------------------------------------------------------------------ state
// state [1 + 64 + 64 * 64] fp64: n, sum f, sum f f^T (row-major); one thread per entry, rows added in batch order
__global__ __launch_bounds__(256) void fid_accumulate_kernel(const float* __restrict__ f, int N, double* __restrict__ state)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= FD_STATE) return;
    double s = state[idx];
    if (idx == 0) {
        for (int i = 0; i < N; ++i) s += 1.0;
    } else if (idx <= FD_FEAT) {
        const int a = idx - 1;
        for (int i = 0; i < N; ++i) s += (double)f[(long long)i * FD_FEAT + a];
    } else {
        const int e = idx - 1 - FD_FEAT, a = e >> 6, b = e & 63;
        for (int i = 0; i < N; ++i) s += (double)f[(long long)i * FD_FEAT + a] * (double)f[(long long)i * FD_FEAT + b];   // exact product
    }
    state[idx] = s;
}

// ------------------------------------------------------------------------------------------------ host side
// packed weights (floats): per block the K-major matrix [K (padded)][Cout], then s [Cout], t [Cout]
constexpr int FD_K[3] = {28, 288, 288};
constexpr int FD_CO[3] = {32, 32, 64};
struct fd_weights {
    long long w[3], s[3], t[3], total;
};
fd_weights fd_weight_layout()
{
    fd_weights o;
    long long off = 0;
    for (int l = 0; l < 3; ++l) {
        o.w[l] = off;
        off += (long long)FD_K[l] * FD_CO[l];
        o.s[l] = off;
        off += FD_CO[l];
        o.t[l] = off;
        off += FD_CO[l];
    }
    o.total = off;
    return o;
}

struct fd_plan {
    long long resized, m1, m2, m3, total;        // byte offsets into the workspace
};
bool make_fd_plan(int N, int H, int W, fd_plan& p)
{
    if (N <= 0 || N > 65535 || H < 1 || W < 1 || H > 16384 || W > 16384) return false;
    dc_f32_bump<1> ws;
    p.resized = ws.take((long long)N * 3 * FD_SIZE * FD_SIZE * 4);
    p.m1 = ws.take((long long)N * 32 * FD_H1 * FD_H1 * 4);
    p.m2 = ws.take((long long)N * 32 * FD_H2 * FD_H2 * 4);
    p.m3 = ws.take((long long)N * 64 * FD_H2 * FD_H2 * 4);
    p.total = ws.off;
    return true;
}

template <int CIN, int CK, int CO, int S, int PAD>
void launch_conv(const float* x, const float* w, const float* s, const float* t, float* y, int N, int H, int W, int Ho, int Wo,
                 hipStream_t st)
{
    const int tiles_x = (Wo + FD_COLS - 1) / FD_COLS, tiles_y = (Ho + FD_ROWS - 1) / FD_ROWS;
    hipLaunchKernelGGL((fid_conv_kernel<CIN, CK, CO, S, PAD>), dim3(tiles_x * tiles_y, 1, N), dim3(256), 0, st, x, w, s, t, y, H, W, Ho,
                       Wo, tiles_x);
}

void run_stem(const void* x, int u8, dc_strides4 sx, int N, int H, int W, const float* wts, float* resized, float* m1, float* m2,
              float* m3, float* pooled, float* feat, hipStream_t st)
{
    const fd_weights o = fd_weight_layout();
    const long long total = (long long)N * 3 * FD_SIZE * FD_SIZE;
    const int grid = dc_f32_blocks(total, 8192);
    if (u8)
        hipLaunchKernelGGL(fid_resize_kernel<uint8_t>, dim3(grid), dim3(256), 0, st, (const uint8_t*)x, sx, H, W, resized, total);
    else
        hipLaunchKernelGGL(fid_resize_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)x, sx, H, W, resized, total);
    launch_conv<3, 3, 32, 2, 0>(resized, wts + o.w[0], wts + o.s[0], wts + o.t[0], m1, N, FD_SIZE, FD_SIZE, FD_H1, FD_H1, st);
    launch_conv<32, 8, 32, 1, 0>(m1, wts + o.w[1], wts + o.s[1], wts + o.t[1], m2, N, FD_H1, FD_H1, FD_H2, FD_H2, st);
    launch_conv<32, 8, 64, 1, 1>(m2, wts + o.w[2], wts + o.s[2], wts + o.t[2], m3, N, FD_H2, FD_H2, FD_H2, FD_H2, st);
    hipLaunchKernelGGL(fid_pool_mean_kernel, dim3(FD_FEAT, N), dim3(256), 0, st, (const float*)m3, pooled, feat, FD_H2, FD_H2, FD_HP,
                       FD_HP);
}

}  // namespace

extern "C" int dc_fid_weight_floats(void) { return (int)fd_weight_layout().total; }

extern "C" long long dc_fid_ws_bytes(int N, int H, int W)
{
    fd_plan p;
    return make_fd_plan(N, H, W, p) ? p.total : -1;
}

extern "C" int dc_fid_features(const void* x, int x_u8, const long long* strides, int N, int H, int W, const float* weights, void* ws,
                               float* out, void* stream)
{
    fd_plan p;
    if (!x || !strides || !weights || !ws || !out || !make_fd_plan(N, H, W, p)) return DC_ERR_INVALID;
    char* base = (char*)ws;
    run_stem(x, x_u8, dc_strides4(strides), N, H, W, weights, (float*)(base + p.resized), (float*)(base + p.m1), (float*)(base + p.m2),
             (float*)(base + p.m3), nullptr, out, (hipStream_t)stream);
    return dc_launch_status();
}

extern "C" int dc_fid_maps(const void* x, int x_u8, const long long* strides, int N, int H, int W, const float* weights, float* resized,
                           float* m1, float* m2, float* m3, float* pooled, float* out, void* stream)
{
    fd_plan p;
    if (!x || !strides || !weights || !resized || !m1 || !m2 || !m3 || !pooled || !out || !make_fd_plan(N, H, W, p)) return DC_ERR_INVALID;
    run_stem(x, x_u8, dc_strides4(strides), N, H, W, weights, resized, m1, m2, m3, pooled, out, (hipStream_t)stream);
    return dc_launch_status();
}

extern "C" int dc_fid_conv(int layer, const float* x, int N, const float* weights, float* y, void* stream)
{
    if (!x || !weights || !y || layer < 0 || layer > 2 || N <= 0 || N > 65535) return DC_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const fd_weights o = fd_weight_layout();
    const float *w = weights + o.w[layer], *s = weights + o.s[layer], *t = weights + o.t[layer];
    if (layer == 0)
        launch_conv<3, 3, 32, 2, 0>(x, w, s, t, y, N, FD_SIZE, FD_SIZE, FD_H1, FD_H1, st);
    else if (layer == 1)
        launch_conv<32, 8, 32, 1, 0>(x, w, s, t, y, N, FD_H1, FD_H1, FD_H2, FD_H2, st);
    else
        launch_conv<32, 8, 64, 1, 1>(x, w, s, t, y, N, FD_H2, FD_H2, FD_H2, FD_H2, st);
    return dc_launch_status();
}

extern "C" int dc_fid_accumulate(const float* features, int N, double* state, void* stream)
{
    if (!features || !state || N <= 0) return DC_ERR_INVALID;
    hipLaunchKernelGGL(fid_accumulate_kernel, dim3((FD_STATE + 255) / 256), dim3(256), 0, (hipStream_t)stream, features, N, state);
    return dc_launch_status();
}
