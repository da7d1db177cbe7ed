// Backward of the fp32 extractor conv (dc_conv3x3_nchw_f32: NCHW, 3x3, padding 1, stride 1 | 2 | 4, + SiLU) in exact fp32 for gfx950:
// what fine-tuning the control extractors needs (the reference's train_controlnet.py trains exactly these convolutions).
//   z = conv(x, w) + b,  y = silu ? SiLU(z) : z
//   SiLU gradient  gz = gy * (s + z s (1 - s)), s = dc_sigmoid(z): the sigmoid form of the forward's dc_silu.
//   data gradient  dx[n][ci][iy][ix] = sum_{co, ky, kx} gz[n][co][oy][ox] w[co][ci][ky][kx], oy s + ky - 1 = iy, ox s + kx - 1 = ix:
//     a gather per dx element.  Only the taps of a pixel's phase (iy mod s, ix mod s) contribute: tap k of a dimension reaches
//     phase p where (p + 1 - k) mod s = 0, at o = (i + 1 - k) / s.  Per image (grid z), so an image's bits do not depend on the batch.
//   weight gradient  dw[co][ci][ky][kx] = sum_{n, oy, ox} gz[n][co][oy][ox] x[n][ci][oy s + ky - 1][ox s + kx - 1], db[co] = sum gz:
//     K = the N Ho Wo pixels, split over a partition fixed by the shape (image groups x row-block ranges); every part writes its
//     partial, a finish launch adds the partials in part order.  No atomics anywhere.
// Two forms per gradient, chosen by cg_route_of (the launchers and the query dc_conv3x3_f32_grad_route read the same decision):
//   MFMA (v_mfma_f32_32x32x2_f32, the pieces of dc_f32_mfma.h), stride 1 | 2, Cin and Cout >= 32 and multiples of 8, any map size:
//     dgrad: implicit GEMM D[ci][pixel] += W[ci][(co, tap)] G[(co, tap)][pixel] per phase: a phase's pixels (iy, ix) = (a s + py,
//       b s + px) form a dense grid (a, b) on which the gradient is a stride-1 correlation of gz with that phase's taps (1, 2, 2, 4
//       of the 9 at stride 2; all 9 at stride 1).  Tile = 64 | 32 input channels x 128 phase pixels (rows_t x cols_t); K runs over
//       chunks of 8 output channels whose gz patch (one-pixel halo, zero padding materialised) and weight slice are staged in LDS.
//       The weight slice is read from OIHW as it is (per output channel one contiguous run of 9 * channels floats) and transposed
//       on the way into LDS: nothing is packed between calls, the weight being a live parameter.
//     wgrad: D[co][ci] += G[co][pixel] X_tap[pixel][ci], one accumulator tile per tap (9 x 32 x 32 per wave), tile = 64 output x 64
//       input channels; a K step is 32 output pixels (rows_c x cols_c) whose gz values (transposed) and x patch are staged in LDS.
//   VALU (everything else: 1 or 3 channels, stride 4): one thread per dx element / per dw element and part.
#include "dc_f32_mfma.h"
#include "../../include/diffcodec_train_hip.h"

namespace {

constexpr int CG_CK = 8;                       // dgrad MFMA: output channels (K) per LDS chunk
constexpr int CG_PT = 128;                     // dgrad MFMA: phase pixels per workgroup
constexpr int CG_DPATCH = CG_CK * 6 * 34;      // dgrad MFMA: largest gz patch, (4 + 2) x (32 + 2) per channel
constexpr int CG_WT = 64;                      // wgrad MFMA: channels per workgroup, both ways
constexpr int CG_KPX = 32;                     // wgrad MFMA: output pixels per K step
constexpr int CG_GP = CG_WT + 1;               // wgrad MFMA: pitch of the transposed gz tile [pixel][co] (odd: conflict-free writes)
constexpr int CG_XPS = 3 * 65;                 // wgrad MFMA: largest x patch per channel (stride 2, 1 x 32 pixels); always odd
constexpr int CG_MAX_GROUPS = 8;               // wgrad: image groups of the K partition
constexpr int CG_MFMA_UNITS = 20;              // wgrad MFMA: K steps a part should at least have
constexpr int CG_VALU_ROWS = 4;                // wgrad VALU: output rows a part should at least have

// ------------------------------------------------------------------------------------------------ routing
struct cg_route {
    int form;       // DC_F32GRAD_MFMA | DC_F32GRAD_VALU
    int stride_t;   // MFMA: the STRIDE template argument; VALU: 0
    int ch_t;       // MFMA: channels per workgroup; VALU: 0
    int cols_t, rows_t;
    int groups, p1, upp;      // wgrad: image groups, parts per group, K steps (units) per part
    int units_x, units_img;   // wgrad: K steps per output-row block, per image
};

int cg_route_of(int kind, int N, int Cin, int H, int W, int Cout, int stride, cg_route& r)
{
    if ((kind != DC_F32GRAD_DGRAD && kind != DC_F32GRAD_WGRAD) || N <= 0 || N > 65535 || Cin <= 0 || Cin > 65535 || Cout <= 0 ||
        Cout > 65535 || H <= 0 || H > 16384 || W <= 0 || W > 16384 || (long long)H * W > (1ll << 28) ||
        (stride != 1 && stride != 2 && stride != 4) ||
        (kind == DC_F32GRAD_WGRAD && (long long)Cout * Cin * 9 > 0x7fffffffll - 65536))      // dw is indexed in 32 bits
        return DC_ERR_INVALID;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const bool mfma = stride != 4 && Cin >= 32 && Cout >= 32 && Cin % 8 == 0 && Cout % 8 == 0;
    r = cg_route{};
    r.form = mfma ? DC_F32GRAD_MFMA : DC_F32GRAD_VALU;
    r.stride_t = mfma ? stride : 0;
    if (kind == DC_F32GRAD_DGRAD) {
        if (mfma) {
            const int Wa = (W + stride - 1) / stride;                       // columns of phase 0's grid, the widest
            r.ch_t = (Cin % 64 == 0 || Cin % 64 > 32) ? 64 : 32;
            r.cols_t = Wa >= 32 ? 32 : Wa >= 16 ? 16 : 8;
            r.rows_t = CG_PT / r.cols_t;
        } else {
            r.cols_t = 256, r.rows_t = 1;                                   // 256 consecutive dx elements of one channel plane
        }
        return DC_OK;
    }
    int cap;
    if (mfma) {
        r.ch_t = CG_WT;
        r.cols_t = Wo >= 32 ? 32 : Wo >= 16 ? 16 : 8;
        r.rows_t = CG_KPX / r.cols_t;
        const int tiles = ((Cout + CG_WT - 1) / CG_WT) * ((Cin + CG_WT - 1) / CG_WT);
        cap = 256 / tiles > 1 ? 256 / tiles : 1;
    } else {
        r.cols_t = Wo, r.rows_t = 1;
        cap = 64;
    }
    r.units_x = (Wo + r.cols_t - 1) / r.cols_t;
    r.units_img = ((Ho + r.rows_t - 1) / r.rows_t) * r.units_x;
    const int least = mfma ? CG_MFMA_UNITS : CG_VALU_ROWS;
    int p1 = (r.units_img + least - 1) / least;
    p1 = p1 < cap ? p1 : cap;
    r.upp = (r.units_img + p1 - 1) / p1;
    r.p1 = (r.units_img + r.upp - 1) / r.upp;                               // no empty part
    r.groups = N < CG_MAX_GROUPS ? N : CG_MAX_GROUPS;
    return DC_OK;
}

// ------------------------------------------------------------------------------------------------ SiLU gradient
__global__ __launch_bounds__(256) void cg_silu_grad_kernel(const float* __restrict__ z, const float* gy, float* gz, long long n)
{
#pragma clang fp contract(off)
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = z[i], s = dc_sigmoid(v);
        gz[i] = gy[i] * (s + (v * s) * (1.0f - s));
    }
}

// ------------------------------------------------------------------------------------------------ data gradient, VALU form
// grid (pixel blocks, Cin, N): the channel is workgroup-uniform, so the weight reads are scalar loads
__global__ __launch_bounds__(256) void cg_dgrad_valu_kernel(const float* __restrict__ gz, const float* __restrict__ w,
                                                            float* __restrict__ dx, int Cin, int H, int W, int Cout, int Ho, int Wo,
                                                            int stride)
{
    const int p = blockIdx.x * 256 + threadIdx.x, ci = blockIdx.y, n = blockIdx.z;
    if (p >= H * W) return;
    const int iy = p / W, ix = p - iy * W;
    int oy[3], ox[3];                                        // per tap: the output row / column it reaches this pixel from, or -1
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int ty = iy + 1 - k, tx = ix + 1 - k;
        oy[k] = (ty >= 0 && ty % stride == 0 && ty / stride < Ho) ? ty / stride : -1;
        ox[k] = (tx >= 0 && tx % stride == 0 && tx / stride < Wo) ? tx / stride : -1;
    }
    const float* __restrict__ gn = gz + (long long)n * Cout * Ho * Wo;
    float acc = 0.f;
    for (int co = 0; co < Cout; ++co) {
        const float* __restrict__ gc = gn + (long long)co * Ho * Wo;
        const float* __restrict__ wc = w + ((long long)co * Cin + ci) * 9;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
                if (oy[ky] >= 0 && ox[kx] >= 0) acc = __builtin_fmaf(gc[oy[ky] * Wo + ox[kx]], wc[ky * 3 + kx], acc);
    }
    dx[((long long)n * Cin + ci) * H * W + p] = acc;
}

// ------------------------------------------------------------------------------------------------ data gradient, MFMA form
// Tap t of a dimension at phase p: kernel index k and offset `off` into the patch (whose origin is one pixel before the tile):
// stride 1: k = t, off = 2 - t (3 taps); stride 2: phase 0: k = 1, off = 1 (1 tap); phase 1: k = 2 t, off = 2 - t (2 taps).
template <int STRIDE>
__device__ __forceinline__ void cg_tap(int phase, int t, int& k, int& off)
{
    if (STRIDE == 1 || phase) k = STRIDE == 1 ? t : 2 * t, off = 2 - t;
    else k = 1, off = 1;
}

template <int STRIDE, int NQ>
__global__ __launch_bounds__(256, 2) void cg_dgrad_mfma_kernel(const float* __restrict__ gz, const float* __restrict__ w,
                                                               float* __restrict__ dx, int Cin, int H, int W, int Cout, int Ho, int Wo,
                                                               int cols_t, int tiles_x, int tiles)
{
    constexpr int CI_T = 32 * NQ;                          // input channels per workgroup: every wave holds all NQ 32-channel tiles
    constexpr int WP = CI_T + 4;                           // pitch of the weight slice [(co, tap)][ci] (spreads the transposing writes)
    __shared__ float Wl[CG_CK * 9 * WP];
    __shared__ float Pl[CG_DPATCH];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int phase = blockIdx.x / tiles, tile = blockIdx.x - phase * tiles;
    const int py = phase / STRIDE, px = phase - py * STRIDE;
    const int rows_t = CG_PT / cols_t;
    const int a0 = (tile / tiles_x) * rows_t, b0 = (tile % tiles_x) * cols_t;
    const int Ha = (H - py + STRIDE - 1) / STRIDE, Wa = (W - px + STRIDE - 1) / STRIDE;      // this phase's grid
    if (a0 >= Ha || b0 >= Wa) return;                      // workgroup-uniform: the tile grid is phase 0's, the largest
    const int ci0 = blockIdx.y * CI_T, n = blockIdx.z;
    const int PH = rows_t + 2, PW = cols_t + 2, PS = PH * PW;
    const float* __restrict__ gn = gz + (long long)n * Cout * Ho * Wo;

    // this lane's pixel of the wave's 32: (ty, tx) inside the tile
    const int p = wave * 32 + j;
    const int ty = p / cols_t, tx = p - ty * cols_t;
    const int pbase = ty * PW + tx + h * PS;               // lane half h reads the odd channel of the pair
    const float* abase = Wl + h * 9 * WP + j;
    const int nq = min(NQ, (Cin - ci0 + 31) / 32);
    const int nty = STRIDE == 1 ? 3 : 1 + py, ntx = STRIDE == 1 ? 3 : 1 + px;

    f32x16 acc[NQ];
    dc_f32_zero(acc);

    for (int c0 = 0; c0 < Cout; c0 += CG_CK) {
        __syncthreads();                                   // everyone is done reading the previous chunk
        for (int e = tid; e < CG_CK * PS; e += 256) {
            const int c = e / PS, r = e - c * PS;
            const int pr = r / PW, pc = r - pr * PW;
            const int oy = a0 - 1 + pr, ox = b0 - 1 + pc;
            Pl[e] = (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo) ? gn[((long long)(c0 + c) * Ho + oy) * Wo + ox] : 0.f;
        }
        for (int e = tid; e < CG_CK * 9 * CI_T; e += 256) {
            const int c = e / (9 * CI_T), f = e - c * (9 * CI_T);          // f: index into the run w[c0 + c][ci0 ..][tap]
            const int ci = f / 9, tap = f - ci * 9;
            Wl[(c * 9 + tap) * WP + ci] = ci0 + ci < Cin ? w[((long long)(c0 + c) * Cin + ci0) * 9 + f] : 0.f;
        }
        __syncthreads();
        for (int t = 0; t < nty; ++t) {
            int ky, offy;
            cg_tap<STRIDE>(py, t, ky, offy);
            for (int u = 0; u < ntx; ++u) {
                int kx, offx;
                cg_tap<STRIDE>(px, u, kx, offx);
                const float* a = abase + (ky * 3 + kx) * WP;
                const float* b = Pl + pbase + offy * PW + offx;
#pragma unroll
                for (int cp = 0; cp < CG_CK / 2; ++cp) dc_f32_kpair(acc, nq, a + cp * 2 * 9 * WP, b[cp * 2 * PS]);
            }
        }
    }

    // register r of lane half h = channel dc_f32_channel(r, h) of the tile, lane & 31 = pixel
    const int iy = (a0 + ty) * STRIDE + py, ix = (b0 + tx) * STRIDE + px;
    if (iy < H && ix < W) {
        float* __restrict__ o = dx + (((long long)n * Cin + ci0) * H + iy) * W + ix;
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = dc_f32_channel(r, h, q * 32);
                if (ci0 + ci < Cin) o[(long long)ci * H * W] = acc[q][r];
            }
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
// The K partition: part = group * p1 + q takes the images [group N / groups, (group + 1) N / groups) and of each the K steps
// (units) [q upp, min((q + 1) upp, units_img)); unit u = output rows (u / units_x) rows_c .. and columns (u % units_x) cols_c ..
struct cg_parts {
    int N, groups, p1, upp, units_x, units_img, cols_c, rows_c;
};
__device__ __forceinline__ void cg_part_range(const cg_parts& k, int part, int& n0, int& n1, int& u0, int& u1)
{
    const int g = part / k.p1, q = part - g * k.p1;
    n0 = (int)((long long)g * k.N / k.groups), n1 = (int)((long long)(g + 1) * k.N / k.groups);
    u0 = q * k.upp, u1 = min(k.units_img, u0 + k.upp);
}

// VALU form: one thread per (dw element, part); a unit is one whole output row
__global__ __launch_bounds__(256) void cg_wgrad_valu_kernel(const float* __restrict__ x, long long xbs, const float* __restrict__ gz,
                                                            float* __restrict__ dwp, cg_parts k, int Cin, int H, int W, int Cout,
                                                            int Ho, int Wo, int stride)
{
    const int total = Cout * Cin * 9, e = blockIdx.x * 256 + threadIdx.x, part = blockIdx.y;
    if (e >= total) return;
    const int co = e / (Cin * 9), r = e - co * (Cin * 9);
    const int ci = r / 9, tap = r - ci * 9;
    const int ky = tap / 3, kx = tap - ky * 3;
    int n0, n1, u0, u1;
    cg_part_range(k, part, n0, n1, u0, u1);
    float acc = 0.f;
    for (int n = n0; n < n1; ++n) {
        const float* __restrict__ gc = gz + ((long long)n * Cout + co) * Ho * Wo;
        const float* __restrict__ xc = x + (long long)n * xbs + (long long)ci * H * W;
        for (int oy = u0; oy < u1; ++oy) {
            const int iy = oy * stride + ky - 1;
            if (iy < 0 || iy >= H) continue;
            for (int ox = 0; ox < Wo; ++ox) {
                const int ix = ox * stride + kx - 1;
                if (ix >= 0 && ix < W) acc = __builtin_fmaf(gc[oy * Wo + ox], xc[(long long)iy * W + ix], acc);
            }
        }
    }
    dwp[(long long)part * total + e] = acc;
}

// MFMA form: grid (Cin tiles, Cout tiles, parts); wave = 32 output channels (cq) x 32 input channels (iq) x 9 taps
template <int STRIDE>
__global__ __launch_bounds__(256) void cg_wgrad_mfma_kernel(const float* __restrict__ x, long long xbs, const float* __restrict__ gz,
                                                            float* __restrict__ dwp, cg_parts k, int lc, int Cin, int H, int W,
                                                            int Cout, int Ho, int Wo)
{
    __shared__ float Gl[CG_KPX * CG_GP];                   // [pixel][co]
    __shared__ float Xl[CG_WT * CG_XPS];                   // [ci][PH][PW], channel pitch PS (odd)

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int cq = wave & 1, iq = wave >> 1;
    const int ci0 = blockIdx.x * CG_WT, co0 = blockIdx.y * CG_WT, part = blockIdx.z;
    const int cols_c = k.cols_c, rows_c = k.rows_c;
    const int PH = (rows_c - 1) * STRIDE + 3, PW = (cols_c - 1) * STRIDE + 3, PS = (PH * PW) | 1;
    int n0, n1, u0, u1;
    cg_part_range(k, part, n0, n1, u0, u1);

    f32x16 acc[9];
    dc_f32_zero(acc);
    const float* ga = Gl + h * CG_GP + cq * 32 + j;        // A: gz of pixel 2 kp + h, output channel j of the wave's 32
    const float* xb = Xl + (iq * 32 + j) * PS;             // B: the patch of input channel j of the wave's 32

    for (int n = n0; n < n1; ++n) {
        const float* __restrict__ gn = gz + (long long)n * Cout * Ho * Wo;
        const float* __restrict__ xn = x + (long long)n * xbs;
        for (int u = u0; u < u1; ++u) {
            const int oy0 = (u / k.units_x) * rows_c, ox0 = (u % k.units_x) * cols_c;
            __syncthreads();                               // everyone is done reading the previous step
            for (int e = tid; e < CG_KPX * CG_WT; e += 256) {
                const int co = e >> 5, kk = e & 31;
                const int oy = oy0 + (kk >> lc), ox = ox0 + (kk & (cols_c - 1));
                Gl[kk * CG_GP + co] = (co0 + co < Cout && oy < Ho && ox < Wo) ? gn[((long long)(co0 + co) * Ho + oy) * Wo + ox] : 0.f;
            }
            for (int e = tid; e < CG_WT * PH * PW; e += 256) {
                const int ci = e / (PH * PW), r = e - ci * (PH * PW);
                const int pr = r / PW, pc = r - pr * PW;
                const int iy = oy0 * STRIDE - 1 + pr, ix = ox0 * STRIDE - 1 + pc;
                Xl[ci * PS + r] = (ci0 + ci < Cin && iy >= 0 && iy < H && ix >= 0 && ix < W)
                                      ? xn[((long long)(ci0 + ci) * H + iy) * W + ix] : 0.f;
            }
            __syncthreads();
#pragma unroll 4
            for (int kp = 0; kp < CG_KPX / 2; ++kp) {
                const int kk = 2 * kp + h;
                const float a = ga[kp * 2 * CG_GP];
                const float* b = xb + ((kk >> lc) * STRIDE) * PW + (kk & (cols_c - 1)) * STRIDE;
#pragma unroll
                for (int tap = 0; tap < 9; ++tap)
                    acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[(tap / 3) * PW + (tap % 3)], acc[tap], 0, 0, 0);
            }
        }
    }

    // lane & 31 = input channel, register r of lane half h = output channel dc_f32_channel(r, h): a lane's 9 taps are contiguous
    const int ci = ci0 + iq * 32 + j;
    if (ci < Cin) {
        float* __restrict__ o = dwp + (long long)part * Cout * Cin * 9;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + dc_f32_channel(r, h, cq * 32);
            if (co < Cout) {
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) o[((long long)co * Cin + ci) * 9 + tap] = acc[tap][r];
            }
        }
    }
}

// bias partial of one image: grid (Cout, N); 256 strided sums, then a fixed tree
__global__ __launch_bounds__(256) void cg_bias_part_kernel(const float* __restrict__ gz, float* __restrict__ dbp, int Cout, int HWo)
{
    __shared__ float red[256];
    const int co = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const float* __restrict__ g = gz + ((long long)n * Cout + co) * HWo;
    float s = 0.f;
    for (int i = tid; i < HWo; i += 256) s += g[i];
    red[tid] = s;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (tid < d) red[tid] += red[tid + d];
        __syncthreads();
    }
    if (tid == 0) dbp[(long long)n * Cout + co] = red[0];
}

// dw[i] = the partials in part order; db[co] = the image partials in image order
__global__ __launch_bounds__(256) void cg_wgrad_finish_kernel(const float* __restrict__ dwp, const float* __restrict__ dbp,
                                                              float* __restrict__ dw, float* __restrict__ db, int total, int parts,
                                                              int Cout, int N)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < total) {
        float s = 0.f;
        for (int p = 0; p < parts; ++p) s += dwp[(long long)p * total + i];
        dw[i] = s;
    } else if (db && i - total < Cout) {
        const int co = i - total;
        float s = 0.f;
        for (int n = 0; n < N; ++n) s += dbp[(long long)n * Cout + co];
        db[co] = s;
    }
}

int cg_log2(int v) { return v == 32 ? 5 : v == 16 ? 4 : 3; }

}  // namespace

extern "C" int dc_conv3x3_f32_grad_route(int kind, int N, int Cin, int H, int W, int Cout, int stride, int* info)
{
    if (!info) return DC_ERR_INVALID;
    for (int i = 0; i < DC_F32GRAD_ROUTE_INFO_INTS; ++i) info[i] = 0;
    cg_route r;
    const int rc = cg_route_of(kind, N, Cin, H, W, Cout, stride, r);
    if (rc != DC_OK) return rc;
    info[0] = r.form, info[1] = r.stride_t, info[2] = r.ch_t, info[3] = r.cols_t, info[4] = r.rows_t;
    info[5] = r.groups, info[6] = r.p1, info[7] = r.upp;
    return DC_OK;
}

extern "C" int dc_silu_grad_f32(const float* z, const float* gy, float* gz, long long n, void* stream)
{
    if (!z || !gy || !gz || n <= 0) return DC_ERR_INVALID;
    hipLaunchKernelGGL(cg_silu_grad_kernel, dim3(dc_f32_blocks(n, 16384)), dim3(256), 0, (hipStream_t)stream, z, gy, gz, n);
    return dc_launch_status();
}

extern "C" int dc_conv3x3_f32_dgrad(const float* gz, const float* w, float* dx, int N, int Cin, int H, int W, int Cout, int stride,
                                    void* stream)
{
    cg_route r;
    if (!gz || !w || !dx || cg_route_of(DC_F32GRAD_DGRAD, N, Cin, H, W, Cout, stride, r) != DC_OK) return DC_ERR_INVALID;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    hipStream_t st = (hipStream_t)stream;
    if (r.form == DC_F32GRAD_VALU) {
        hipLaunchKernelGGL(cg_dgrad_valu_kernel, dim3((H * W + 255) / 256, Cin, N), dim3(256), 0, st, gz, w, dx, Cin, H, W, Cout, Ho, Wo,
                           stride);
        return dc_launch_status();
    }
    const int Ha = (H + stride - 1) / stride, Wa = (W + stride - 1) / stride;
    const int tiles_x = (Wa + r.cols_t - 1) / r.cols_t, tiles = tiles_x * ((Ha + r.rows_t - 1) / r.rows_t);
    const dim3 grid(tiles * stride * stride, (Cin + r.ch_t - 1) / r.ch_t, N);
#define CG_GO(S, Q) \
    if (r.stride_t == S && r.ch_t == 32 * Q) \
        hipLaunchKernelGGL((cg_dgrad_mfma_kernel<S, Q>), grid, dim3(256), 0, st, gz, w, dx, Cin, H, W, Cout, Ho, Wo, r.cols_t, tiles_x, tiles)
    CG_GO(1, 1);
    CG_GO(1, 2);
    CG_GO(2, 1);
    CG_GO(2, 2);
#undef CG_GO
    return dc_launch_status();
}

extern "C" long long dc_conv3x3_f32_wgrad_ws_bytes(int N, int Cin, int H, int W, int Cout, int stride)
{
    cg_route r;
    if (cg_route_of(DC_F32GRAD_WGRAD, N, Cin, H, W, Cout, stride, r) != DC_OK) return -1;
    return 4ll * ((long long)r.groups * r.p1 * Cout * Cin * 9 + (long long)N * Cout);
}

extern "C" int dc_conv3x3_f32_wgrad(const float* x, long long x_batch_stride, const float* gz, float* dw, float* db, void* ws, int N,
                                    int Cin, int H, int W, int Cout, int stride, void* stream)
{
    cg_route r;
    if (!x || !gz || !dw || !ws || cg_route_of(DC_F32GRAD_WGRAD, N, Cin, H, W, Cout, stride, r) != DC_OK ||
        x_batch_stride < (long long)Cin * H * W)
        return DC_ERR_INVALID;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const int total = Cout * Cin * 9, parts = r.groups * r.p1;
    hipStream_t st = (hipStream_t)stream;
    float* dwp = (float*)ws;
    float* dbp = dwp + (long long)parts * total;
    const cg_parts k{N, r.groups, r.p1, r.upp, r.units_x, r.units_img, r.cols_t, r.rows_t};
    if (r.form == DC_F32GRAD_VALU) {
        hipLaunchKernelGGL(cg_wgrad_valu_kernel, dim3((total + 255) / 256, parts), dim3(256), 0, st, x, x_batch_stride, gz, dwp, k, Cin,
                           H, W, Cout, Ho, Wo, stride);
    } else {
        const dim3 grid((Cin + CG_WT - 1) / CG_WT, (Cout + CG_WT - 1) / CG_WT, parts);
        if (r.stride_t == 1)
            hipLaunchKernelGGL(cg_wgrad_mfma_kernel<1>, grid, dim3(256), 0, st, x, x_batch_stride, gz, dwp, k, cg_log2(r.cols_t), Cin, H, W,
                               Cout, Ho, Wo);
        else
            hipLaunchKernelGGL(cg_wgrad_mfma_kernel<2>, grid, dim3(256), 0, st, x, x_batch_stride, gz, dwp, k, cg_log2(r.cols_t), Cin, H, W,
                               Cout, Ho, Wo);
    }
    if (db) hipLaunchKernelGGL(cg_bias_part_kernel, dim3(Cout, N), dim3(256), 0, st, gz, dbp, Cout, Ho * Wo);
    hipLaunchKernelGGL(cg_wgrad_finish_kernel, dim3((total + Cout + 255) / 256), dim3(256), 0, st, dwp, dbp, dw, db, total, parts, Cout, N);
    return dc_launch_status();
}
