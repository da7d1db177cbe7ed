// FVD features (test_utils.py:45-70, fvd_utils/models/fvd): the Inception-v1 I3D network, 400 logits per video.  Exact fp32 for
// gfx950 on v_mfma_f32_32x32x2_f32; every sum runs in a fixed order and there are no float atomics, so results are bitwise
// reproducible, a video's features do not depend on its position in the batch or on the batch size, and the launches only enqueue
// on the caller's stream (graph-capturable).
//
//   preprocess  per frame: bilinear resize (align_corners = False, no antialias) of the shorter side to 224, centre crop to
//               224 x 224, (v - 0.5) * 2, written as a [N,3,T,224,224] fp32 volume.  Only the cropped region is computed; source
//               positions are formed in fp64, the taps are blended in fp32.  Values are not clamped.
//   conv        Unit3D = conv3d (TF "SAME" padding: per axis pad = max(k - s, 0) when size % s == 0, else max(k - size % s, 0),
//               front = pad / 2, back = the rest; output ceil(size / s)) + eval BatchNorm as one fmaf(acc, s, t) + ReLU.
//               Implicit GEMM  D[co][pixel] += W[co][k] * X[k][pixel], the scheme of fid.hip with a time axis: weights packed
//               K-major with k = (ci, kt, kh, kw); K runs in chunks whose weight rows and input patch (zero padding materialised)
//               are staged in LDS.  Workgroup = 4 waves; one k-step is a pair of consecutive k of the chunk (lane half h takes
//               k = 2 kp + h); a workgroup takes 64 output channels (two 32-channel MFMA tiles, the second skipped when the padded
//               Cout ends first), the channel blocks are grid.y.  Cout is zero-padded to a multiple of 32 in the packed matrix and
//               masked in the store; the store goes to a channel offset of a wider map (the Inception branches land in their
//               concatenated map with no copy).
//                 7x7x7 / 2   chunk = one (ci, kt) slab of 49 taps + one zero row (50); tile 4 rows x 32 columns of one output
//                             time; patch 13 x 69.  A slab whose input time lies in the padding is skipped (it adds zeros).
//                 3x3x3 / 1   chunk = 4 input channels x 27 taps (108 rows); tile 4 x 32; patch 4 x 3 x 6 x 34.
//                 1x1x1       a plain GEMM over the flattened T*H*W positions: chunk = 32 input channels, tile 128 positions.
//   max-pool    SAME padding by the same rule; the padded positions are zeros that ENTER the max (F.pad, then pool).
//   head        mean over [2,7,7] windows (stride 1) of Mixed_5c in fp64 in a fixed order, the 1x1x1 logits conv with bias (the
//               conv kernel with s = 1, t = bias, no ReLU), the mean over the remaining time positions in fp64.
#include "dc_f32_mfma.h"
#include "../../include/diffcodec_hip.h"

namespace {

constexpr int FV_SIZE = 224;                // the network's input
constexpr int FV_COLS = 32, FV_ROWS = 4;    // output pixels per workgroup of the spatial kernels
constexpr int FV_COB = 64;                  // output channels per workgroup
constexpr int FV_PCI = 32, FV_PPOS = 128;   // 1x1x1: input channels per chunk, positions per workgroup
constexpr int FV_FEAT = 400;
constexpr int FV_ENDPOINTS = 16;

struct fv_strides {
    long long n, t, c, h, w;
};

// ------------------------------------------------------------------------------------------------ preprocess
template <typename T>
__global__ __launch_bounds__(256) void fvd_preprocess_kernel(const T* __restrict__ x, fv_strides s, int Tn, int H, int W, int RH, int RW,
                                                             int div255, float* __restrict__ y, long long total)
{
#pragma clang fp contract(off)
    const double sy = (double)H / (double)RH, sx = (double)W / (double)RW;
    const int y0c = (RH - FV_SIZE) / 2, x0c = (RW - FV_SIZE) / 2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ox = (int)(i % FV_SIZE);
        long long r = i / FV_SIZE;
        const int oy = (int)(r % FV_SIZE);
        r /= FV_SIZE;
        const int t = (int)(r % Tn);
        r /= Tn;
        const int c = (int)(r % 3);
        const long long n = r / 3;
        const double py = fmax(((double)(oy + y0c) + 0.5) * sy - 0.5, 0.0), px = fmax(((double)(ox + x0c) + 0.5) * sx - 0.5, 0.0);
        const int iy0 = min((int)py, H - 1), ix0 = min((int)px, W - 1);
        const int iy1 = iy0 + (iy0 < H - 1), ix1 = ix0 + (ix0 < W - 1);
        const float ly = (float)(py - (double)iy0), lx = (float)(px - (double)ix0);
        const float hy = 1.f - ly, hx = 1.f - lx;
        const long long b = n * s.n + t * s.t + c * s.c;
        float tl = (float)x[b + iy0 * s.h + ix0 * s.w], tr = (float)x[b + iy0 * s.h + ix1 * s.w];
        float bl = (float)x[b + iy1 * s.h + ix0 * s.w], br = (float)x[b + iy1 * s.h + ix1 * s.w];
        if (div255) {
            tl /= 255.f;
            tr /= 255.f;
            bl /= 255.f;
            br /= 255.f;
        }
        const float v = hy * (hx * tl + lx * tr) + ly * (hx * bl + lx * br);
        y[i] = (v - 0.5f) * 2.f;
    }
}

// ------------------------------------------------------------------------------------------------ Unit3D
// x [N][Cin][T][H][W] -> y [N][Ctot][To][Ho][Wo] at channels coff .. coff + Cout; wp [K rows (padded per chunk)][CoP] K-major
struct fv_conv {
    const float* x;
    const float* wp;
    const float* s;
    const float* t;
    float* y;
    int Cin, T, H, W, To, Ho, Wo, CoP, Cout, Ctot, coff, pt, ph, pw, relu, tiles_x, tiles_y;
};

template <int KS, int S, int CI, int KTC>
struct fv_geom {
    static constexpr int PH = (FV_ROWS - 1) * S + KS, PW = (FV_COLS - 1) * S + KS;
    static constexpr int PS = PH * PW;                                   // one (ci, kt) slice of the patch
    static constexpr int PE = CI * KTC * PS;
    static constexpr int KC = CI * KTC * KS * KS, KCP = (KC + 1) & ~1;   // k rows of a chunk, padded to whole pairs
    static constexpr int NKT = KS / KTC;                                 // chunks along the kernel's time axis
    static __device__ constexpr int off(int k) { return dc_f32_patch_off<KS, PW, PS, KC>(k); }   // k = (ci, kt, kh, kw)
};

__device__ __forceinline__ void fv_store(const fv_conv& a, const f32x16 (&acc)[2], int nq, int cb, int h, float* __restrict__ yo,
                                         long long cstride)
{
#pragma unroll
    for (int q = 0; q < 2; ++q)
        if (q < nq) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int col = dc_f32_channel(r, h, cb * FV_COB + q * 32);
                if (col < a.Cout) {
                    const float v = __builtin_fmaf(acc[q][r], a.s[col], a.t[col]);
                    yo[(long long)col * cstride] = a.relu ? fmaxf(v, 0.f) : v;
                }
            }
        }
}

template <int KS, int S, int CI, int KTC>
__global__ __launch_bounds__(256) void fvd_conv_kernel(fv_conv a)
{
    using G = fv_geom<KS, S, CI, KTC>;
    static_assert(KS % KTC == 0 && (G::NKT == 1 || CI == 1), "a chunk is whole channels or one time tap");
    __shared__ __attribute__((aligned(16))) float Wl[G::KCP * FV_COB];
    __shared__ float Pl[G::PE];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    int b = blockIdx.x;
    const int tx0 = (b % a.tiles_x) * FV_COLS;
    b /= a.tiles_x;
    const int ty0 = (b % a.tiles_y) * FV_ROWS, to = b / a.tiles_y;
    const int cb = blockIdx.y, n = blockIdx.z;
    const int wcols = min(FV_COB, a.CoP - cb * FV_COB), nq = wcols >> 5;
    const long long plane = (long long)a.H * a.W, vol = plane * a.T;
    const float* __restrict__ xn = a.x + (long long)n * a.Cin * vol;
    const int it0 = to * S - a.pt, iy0 = ty0 * S - a.ph, ix0 = tx0 * S - a.pw;

    f32x16 acc[2];
#pragma unroll
    for (int q = 0; q < 2; ++q)                                          // dc_f32_zero moves an s_nop of <3, 1, 4, 3>: the text stays
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

    const int pbase = wave * S * G::PW + j * S;
    const int abase = h * FV_COB + j;
    const int nchunk = ((a.Cin + CI - 1) / CI) * G::NKT;
    bool staged = false;
    for (int c = 0; c < nchunk; ++c) {
        const int cg = c / G::NKT, kt0 = (c % G::NKT) * KTC;
        if (KTC == 1) {                                                  // a slab that lies in the time padding adds zeros
            const int it = it0 + kt0;
            if (it < 0 || it >= a.T) continue;
        }
        if (staged) __syncthreads();                                     // everyone is done reading the previous chunk
        staged = true;
        dc_f32_copy_w<FV_COB>(Wl, a.wp + (long long)c * G::KCP * a.CoP + cb * FV_COB, a.CoP, G::KCP, FV_COB / 4, tid, wcols);
        for (int e = tid; e < G::PE; e += 256) {
            const int sl = e / G::PS, r = e - sl * G::PS;
            const int ci = sl / KTC, kt = sl - ci * KTC;
            const int py = r / G::PW, px = r - py * G::PW;
            const int cin = cg * CI + ci, it = it0 + kt0 + kt, iy = iy0 + py, ix = ix0 + px;
            const bool in = cin < a.Cin && it >= 0 && it < a.T && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            Pl[e] = in ? xn[(long long)cin * vol + (long long)it * plane + iy * a.W + ix] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kp = 0; kp < G::KCP / 2; ++kp) {                       // lane half h takes k = 2 kp + h
            const int poff = h ? G::off(2 * kp + 1) : G::off(2 * kp);
            dc_f32_kpair(acc, nq, &Wl[abase + kp * 2 * FV_COB], Pl[pbase + poff]);
        }
    }

    const int oy = ty0 + wave, ox = tx0 + j;
    if (oy < a.Ho && ox < a.Wo) {
        const long long cstride = (long long)a.To * a.Ho * a.Wo;
        float* __restrict__ yo = a.y + ((long long)n * a.Ctot + a.coff) * cstride + ((long long)to * a.Ho + oy) * a.Wo + ox;
        fv_store(a, acc, nq, cb, h, yo, cstride);
    }
}

// 1x1x1: y[co][p] = sum_ci w[ci][co] x[ci][p] over the flattened positions p of one video
__global__ __launch_bounds__(256) void fvd_pointwise_kernel(fv_conv a)
{
    __shared__ __attribute__((aligned(16))) float Wl[FV_PCI * FV_COB];
    __shared__ float Pl[FV_PCI * FV_PPOS];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int cb = blockIdx.y, n = blockIdx.z;
    const int wcols = min(FV_COB, a.CoP - cb * FV_COB), nq = wcols >> 5;
    const long long P = (long long)a.T * a.H * a.W;
    const long long p0 = (long long)blockIdx.x * FV_PPOS;
    const float* __restrict__ xn = a.x + (long long)n * a.Cin * P;

    f32x16 acc[2];
    dc_f32_zero(acc);

    const int pbase = wave * 32 + j;
    const int abase = h * FV_COB + j;
    const int nchunk = (a.Cin + FV_PCI - 1) / FV_PCI;
    for (int c = 0; c < nchunk; ++c) {
        if (c) __syncthreads();
        dc_f32_copy_w<FV_COB>(Wl, a.wp + (long long)c * FV_PCI * a.CoP + cb * FV_COB, a.CoP, FV_PCI, FV_COB / 4, tid, wcols);
        for (int e = tid; e < FV_PCI * FV_PPOS; e += 256) {
            const int ci = e / FV_PPOS, pp = e - ci * FV_PPOS;
            const int cin = c * FV_PCI + ci;
            const long long p = p0 + pp;
            Pl[e] = (cin < a.Cin && p < P) ? xn[(long long)cin * P + p] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kp = 0; kp < FV_PCI / 2; ++kp) dc_f32_kpair(acc, nq, &Wl[abase + kp * 2 * FV_COB], Pl[(2 * kp + h) * FV_PPOS + pbase]);
    }

    const long long p = p0 + pbase;
    if (p < P) {
        float* __restrict__ yo = a.y + ((long long)n * a.Ctot + a.coff) * P + p;
        fv_store(a, acc, nq, cb, h, yo, P);
    }
}

// ------------------------------------------------------------------------------------------------ max-pool, SAME, zeros enter
struct fv_pool {
    int T, H, W, To, Ho, Wo, kt, kh, kw, st, sh, sw, pt, ph, pw;
};

__global__ __launch_bounds__(256) void fvd_maxpool_kernel(const float* __restrict__ x, float* __restrict__ y, fv_pool g, long long total)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ox = (int)(i % g.Wo);
        long long r = i / g.Wo;
        const int oy = (int)(r % g.Ho);
        r /= g.Ho;
        const int ot = (int)(r % g.To);
        const long long nc = r / g.To;
        const float* __restrict__ xp = x + nc * g.T * g.H * g.W;
        float m = -INFINITY;
        for (int a = 0; a < g.kt; ++a) {
            const int it = ot * g.st - g.pt + a;
            for (int b = 0; b < g.kh; ++b) {
                const int iy = oy * g.sh - g.ph + b;
                for (int c = 0; c < g.kw; ++c) {
                    const int ix = ox * g.sw - g.pw + c;
                    const bool in = it >= 0 && it < g.T && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
                    m = fmaxf(m, in ? xp[((long long)it * g.H + iy) * g.W + ix] : 0.f);
                }
            }
        }
        y[i] = m;
    }
}

// ------------------------------------------------------------------------------------------------ head
// x [NC][T][49] -> y [NC][T - 1]: the mean of two consecutive 7 x 7 slices, summed in fp64 in index order
__global__ __launch_bounds__(256) void fvd_avgpool_kernel(const float* __restrict__ x, float* __restrict__ y, int T, long long total)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ot = (int)(i % (T - 1));
    const long long nc = i / (T - 1);
    const float* __restrict__ p = x + (nc * T + ot) * 49;
    double s = 0.0;
    for (int q = 0; q < 98; ++q) s += (double)p[q];
    y[i] = (float)(s / 98.0);
}

// x [NC][L] -> y [NC]: the mean over L in fp64 in index order
__global__ __launch_bounds__(256) void fvd_timemean_kernel(const float* __restrict__ x, float* __restrict__ y, int L, long long total)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    double s = 0.0;
    for (int q = 0; q < L; ++q) s += (double)x[i * L + q];
    y[i] = (float)(s / (double)L);
}

// ------------------------------------------------------------------------------------------------ host side
inline int fv_krows(int cin, int k)
{
    return k == 7 ? cin * 7 * 50 : k == 3 ? ((cin + 3) / 4) * 108 : ((cin + FV_PCI - 1) / FV_PCI) * FV_PCI;
}
inline long long fv_unit_floats(int cin, int cout, int k) { return ((long long)fv_krows(cin, k) + 2) * dc_f32_cop(cout); }
// TF "SAME": output size and front padding of one axis
inline void fv_same(int size, int k, int s, int& out, int& front)
{
    const int pad = size % s == 0 ? (k - s > 0 ? k - s : 0) : (k - size % s > 0 ? k - size % s : 0);
    out = (size + s - 1) / s;
    front = pad / 2;
}

// one Unit3D on contiguous maps; `packed` = its K-major matrix, then s [CoP], then t [CoP]
bool launch_unit(const float* x, int N, int Cin, int T, int H, int W, int k, int stride, const float* packed, int Cout, int relu,
                 float* y, int Ctot, int coff, hipStream_t st)
{
    if (!((k == 7 && stride == 2) || (k == 3 && stride == 1) || (k == 1 && stride == 1))) return false;
    if (N <= 0 || N > 65535 || Cin <= 0 || Cout <= 0 || T <= 0 || H <= 0 || W <= 0 || coff < 0 || coff + Cout > Ctot) return false;
    if ((long long)T * H * W > (1ll << 30)) return false;
    fv_conv a;
    a.x = x;
    a.y = y;
    a.CoP = dc_f32_cop(Cout);
    dc_f32_split(packed, fv_krows(Cin, k), a.CoP, a.wp, a.s, a.t);
    a.Cin = Cin, a.T = T, a.H = H, a.W = W, a.Cout = Cout, a.Ctot = Ctot, a.coff = coff, a.relu = relu;
    fv_same(T, k, stride, a.To, a.pt);
    fv_same(H, k, stride, a.Ho, a.ph);
    fv_same(W, k, stride, a.Wo, a.pw);
    a.tiles_x = (a.Wo + FV_COLS - 1) / FV_COLS;
    a.tiles_y = (a.Ho + FV_ROWS - 1) / FV_ROWS;
    const int cblocks = (a.CoP + FV_COB - 1) / FV_COB;
    if (k == 1) {
        const long long P = (long long)T * H * W;
        hipLaunchKernelGGL(fvd_pointwise_kernel, dim3((unsigned)((P + FV_PPOS - 1) / FV_PPOS), cblocks, N), dim3(256), 0, st, a);
    } else {
        const long long gx = (long long)a.tiles_x * a.tiles_y * a.To;
        if (gx > 0x7fffffffll) return false;
        if (k == 7)
            hipLaunchKernelGGL((fvd_conv_kernel<7, 2, 1, 1>), dim3((unsigned)gx, cblocks, N), dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL((fvd_conv_kernel<3, 1, 4, 3>), dim3((unsigned)gx, cblocks, N), dim3(256), 0, st, a);
    }
    return true;
}

bool launch_pool(const float* x, int N, int C, int T, int H, int W, int kt, int kh, int kw, int s_t, int s_h, int s_w, float* y,
                 hipStream_t st)
{
    if (N <= 0 || C <= 0 || T <= 0 || H <= 0 || W <= 0 || kt < 1 || kh < 1 || kw < 1 || s_t < 1 || s_h < 1 || s_w < 1) return false;
    fv_pool g;
    g.T = T, g.H = H, g.W = W, g.kt = kt, g.kh = kh, g.kw = kw, g.st = s_t, g.sh = s_h, g.sw = s_w;
    fv_same(T, kt, s_t, g.To, g.pt);
    fv_same(H, kh, s_h, g.Ho, g.ph);
    fv_same(W, kw, s_w, g.Wo, g.pw);
    const long long total = (long long)N * C * g.To * g.Ho * g.Wo;
    const int grid = dc_f32_blocks(total, 16384);
    hipLaunchKernelGGL(fvd_maxpool_kernel, dim3(grid), dim3(256), 0, st, x, y, g, total);
    return true;
}

// the six-branch modules: input channels, then b0, b1a, b1b, b2a, b2b, b3b
struct fv_mixed {
    int cin, c[6];
};
const fv_mixed FV_MIXED[9] = {{192, {64, 96, 128, 16, 32, 32}},     {256, {128, 128, 192, 32, 96, 64}},
                              {480, {192, 96, 208, 16, 48, 64}},    {512, {160, 112, 224, 24, 64, 64}},
                              {512, {128, 128, 256, 24, 64, 64}},   {512, {112, 144, 288, 32, 64, 64}},
                              {528, {256, 160, 320, 32, 128, 128}}, {832, {256, 160, 320, 32, 128, 128}},
                              {832, {384, 192, 384, 48, 128, 128}}};
inline int fv_mixed_cout(const fv_mixed& m) { return m.c[0] + m.c[2] + m.c[4] + m.c[5]; }

// packed weights: the 58 units in state-dict order (stem 1a, 2b, 2c; per module b0, b1a, b1b, b2a, b2b, b3b; logits)
struct fv_weights {
    long long stem[3], mixed[9][6], logits, total;
};
fv_weights fv_weight_layout()
{
    fv_weights o;
    long long off = 0;
    o.stem[0] = off, off += fv_unit_floats(3, 64, 7);
    o.stem[1] = off, off += fv_unit_floats(64, 64, 1);
    o.stem[2] = off, off += fv_unit_floats(64, 192, 3);
    for (int m = 0; m < 9; ++m) {
        const fv_mixed& M = FV_MIXED[m];
        const int cin[6] = {M.cin, M.cin, M.c[1], M.cin, M.c[3], M.cin};
        const int k[6] = {1, 1, 3, 1, 3, 1};
        for (int u = 0; u < 6; ++u) o.mixed[m][u] = off, off += fv_unit_floats(cin[u], M.c[u], k[u]);
    }
    o.logits = off, off += fv_unit_floats(1024, FV_FEAT, 1);
    o.total = off;
    return o;
}

struct fv_plan {
    int T1, T4, T5;
    long long prep, ep[FV_ENDPOINTS], tmp1, tmp2, tmp3, pooled, logits, total;   // byte offsets into the workspace
};
// channels, time and side of the 16 endpoint maps
void fv_endpoint_shape(const fv_plan& p, int e, int& C, int& T, int& S)
{
    static const int CH[FV_ENDPOINTS] = {64, 64, 64, 192, 192, 256, 480, 480, 512, 512, 512, 528, 832, 832, 832, 1024};
    static const int SD[FV_ENDPOINTS] = {112, 56, 56, 56, 28, 28, 28, 14, 14, 14, 14, 14, 14, 7, 7, 7};
    C = CH[e], S = SD[e], T = e < 7 ? p.T1 : e < 13 ? p.T4 : p.T5;
}
bool make_fv_plan(int N, int T, int H, int W, fv_plan& p)
{
    if (N <= 0 || N > 65535 || T < 9 || T > 4096 || H < 1 || W < 1 || H > 16384 || W > 16384) return false;
    p.T1 = (T + 1) / 2, p.T4 = (p.T1 + 1) / 2, p.T5 = (p.T4 + 1) / 2;
    dc_f32_bump<1> ws;
    p.prep = ws.take((long long)N * 3 * T * FV_SIZE * FV_SIZE * 4);
    for (int e = 0; e < FV_ENDPOINTS; ++e) {
        int C, Te, S;
        fv_endpoint_shape(p, e, C, Te, S);
        p.ep[e] = ws.take((long long)N * C * Te * S * S * 4);
    }
    // branch temporaries: the largest 1x1x1 reductions (128 channels at 28 x 28) and the largest pooled module input (256 at 28 x 28)
    long long t12 = 0, t3 = 0;
    for (int m = 0; m < 9; ++m) {
        const int Tm = m < 2 ? p.T1 : m < 7 ? p.T4 : p.T5, S = m < 2 ? 28 : m < 7 ? 14 : 7;
        const long long pix = (long long)N * Tm * S * S * 4;
        const int c12 = FV_MIXED[m].c[1] > FV_MIXED[m].c[3] ? FV_MIXED[m].c[1] : FV_MIXED[m].c[3];
        if (pix * c12 > t12) t12 = pix * c12;
        if (pix * FV_MIXED[m].cin > t3) t3 = pix * FV_MIXED[m].cin;
    }
    p.tmp1 = ws.take(t12);
    p.tmp2 = ws.take(t12);
    p.tmp3 = ws.take(t3);
    p.pooled = ws.take((long long)N * 1024 * (p.T5 - 1) * 4);
    p.logits = ws.take((long long)N * FV_FEAT * (p.T5 - 1) * 4);
    p.total = ws.off;
    return true;
}

bool launch_preprocess(const void* x, int u8, int div255, fv_strides s, int N, int T, int H, int W, int RH, int RW, float* y,
                       hipStream_t st)
{
    if (N <= 0 || T <= 0 || H < 1 || W < 1 || RH < FV_SIZE || RW < FV_SIZE || (RH != FV_SIZE && RW != FV_SIZE)) return false;
    const long long total = (long long)N * 3 * T * FV_SIZE * FV_SIZE;
    const int grid = dc_f32_blocks(total, 16384);
    if (u8)
        hipLaunchKernelGGL(fvd_preprocess_kernel<uint8_t>, dim3(grid), dim3(256), 0, st, (const uint8_t*)x, s, T, H, W, RH, RW, div255, y,
                           total);
    else
        hipLaunchKernelGGL(fvd_preprocess_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)x, s, T, H, W, RH, RW, div255, y,
                           total);
    return true;
}

// the whole chain on a preprocessed volume: ep[16] = the endpoint maps, out [N][400]
bool run_net(const float* prep, int N, int T, const fv_plan& p, const float* wts, float* const* ep, float* tmp1, float* tmp2, float* tmp3,
             float* pooled, float* logits, float* out, hipStream_t st)
{
    const fv_weights o = fv_weight_layout();
    const int T1 = p.T1, T4 = p.T4, T5 = p.T5;
    bool ok = launch_unit(prep, N, 3, T, FV_SIZE, FV_SIZE, 7, 2, wts + o.stem[0], 64, 1, ep[0], 64, 0, st);
    ok &= launch_pool(ep[0], N, 64, T1, 112, 112, 1, 3, 3, 1, 2, 2, ep[1], st);
    ok &= launch_unit(ep[1], N, 64, T1, 56, 56, 1, 1, wts + o.stem[1], 64, 1, ep[2], 64, 0, st);
    ok &= launch_unit(ep[2], N, 64, T1, 56, 56, 3, 1, wts + o.stem[2], 192, 1, ep[3], 192, 0, st);
    ok &= launch_pool(ep[3], N, 192, T1, 56, 56, 1, 3, 3, 1, 2, 2, ep[4], st);
    int e = 4;
    for (int m = 0; m < 9; ++m) {
        const fv_mixed& M = FV_MIXED[m];
        int Tm = m < 2 ? T1 : m < 7 ? T4 : T5, S = m < 2 ? 28 : m < 7 ? 14 : 7;
        if (m == 2) {
            ok &= launch_pool(ep[e], N, M.cin, T1, 28, 28, 3, 3, 3, 2, 2, 2, ep[e + 1], st);
            ++e;
        } else if (m == 7) {
            ok &= launch_pool(ep[e], N, M.cin, T4, 14, 14, 2, 2, 2, 2, 2, 2, ep[e + 1], st);
            ++e;
        }
        const float* in = ep[e];
        float* y = ep[e + 1];
        const int ct = fv_mixed_cout(M);
        const long long* w = o.mixed[m];
        ok &= launch_unit(in, N, M.cin, Tm, S, S, 1, 1, wts + w[0], M.c[0], 1, y, ct, 0, st);
        ok &= launch_unit(in, N, M.cin, Tm, S, S, 1, 1, wts + w[1], M.c[1], 1, tmp1, M.c[1], 0, st);
        ok &= launch_unit(tmp1, N, M.c[1], Tm, S, S, 3, 1, wts + w[2], M.c[2], 1, y, ct, M.c[0], st);
        ok &= launch_unit(in, N, M.cin, Tm, S, S, 1, 1, wts + w[3], M.c[3], 1, tmp2, M.c[3], 0, st);
        ok &= launch_unit(tmp2, N, M.c[3], Tm, S, S, 3, 1, wts + w[4], M.c[4], 1, y, ct, M.c[0] + M.c[2], st);
        ok &= launch_pool(in, N, M.cin, Tm, S, S, 3, 3, 3, 1, 1, 1, tmp3, st);
        ok &= launch_unit(tmp3, N, M.cin, Tm, S, S, 1, 1, wts + w[5], M.c[5], 1, y, ct, M.c[0] + M.c[2] + M.c[4], st);
        ++e;
    }
    const int L = T5 - 1;
    const long long np = (long long)N * 1024 * L, nf = (long long)N * FV_FEAT;
    hipLaunchKernelGGL(fvd_avgpool_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, (const float*)ep[15], pooled, T5, np);
    ok &= launch_unit(pooled, N, 1024, L, 1, 1, 1, 1, wts + o.logits, FV_FEAT, 0, logits, FV_FEAT, 0, st);
    hipLaunchKernelGGL(fvd_timemean_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, (const float*)logits, out, L, nf);
    return ok;
}

int run_chain(const void* x, int x_u8, int div255, const long long* strides, int N, int T, int H, int W, int RH, int RW,
              const float* weights, void* ws, float* const* maps, float* out, void* stream)
{
    fv_plan p;
    if (!x || !strides || !weights || !ws || !out || !make_fv_plan(N, T, H, W, p)) return DC_ERR_INVALID;
    char* base = (char*)ws;
    hipStream_t st = (hipStream_t)stream;
    const fv_strides sx{strides[0], strides[1], strides[2], strides[3], strides[4]};
    float* prep = (float*)(base + p.prep);
    if (!launch_preprocess(x, x_u8, div255, sx, N, T, H, W, RH, RW, prep, st)) return DC_ERR_INVALID;
    float* ep[FV_ENDPOINTS];
    for (int e = 0; e < FV_ENDPOINTS; ++e) {
        ep[e] = maps ? maps[e] : (float*)(base + p.ep[e]);
        if (!ep[e]) return DC_ERR_INVALID;
    }
    const bool ok = run_net(prep, N, T, p, weights, ep, (float*)(base + p.tmp1), (float*)(base + p.tmp2), (float*)(base + p.tmp3),
                            (float*)(base + p.pooled), (float*)(base + p.logits), out, st);
    const int rc = dc_launch_status();
    return ok ? rc : DC_ERR_INVALID;
}

}  // namespace

extern "C" int dc_fvd_weight_floats(void) { return (int)fv_weight_layout().total; }

extern "C" long long dc_fvd_ws_bytes(int N, int T, int H, int W)
{
    fv_plan p;
    return make_fv_plan(N, T, H, W, p) ? p.total : -1;
}

extern "C" int dc_fvd_features(const void* x, int x_u8, int div255, const long long* strides, int N, int T, int H, int W, int RH, int RW,
                               const float* weights, void* ws, float* out, void* stream)
{
    return run_chain(x, x_u8, div255, strides, N, T, H, W, RH, RW, weights, ws, nullptr, out, stream);
}

extern "C" int dc_fvd_endpoints(const void* x, int x_u8, int div255, const long long* strides, int N, int T, int H, int W, int RH, int RW,
                                const float* weights, void* ws, float* const* maps, float* out, void* stream)
{
    if (!maps) return DC_ERR_INVALID;
    return run_chain(x, x_u8, div255, strides, N, T, H, W, RH, RW, weights, ws, maps, out, stream);
}

extern "C" int dc_fvd_preprocess(const void* x, int x_u8, int div255, const long long* strides, int N, int T, int H, int W, int RH,
                                 int RW, float* y, void* stream)
{
    if (!x || !strides || !y) return DC_ERR_INVALID;
    const fv_strides sx{strides[0], strides[1], strides[2], strides[3], strides[4]};
    if (!launch_preprocess(x, x_u8, div255, sx, N, T, H, W, RH, RW, y, (hipStream_t)stream)) return DC_ERR_INVALID;
    return dc_launch_status();
}

extern "C" int dc_fvd_conv(const float* x, int N, int Cin, int T, int H, int W, int k, int stride, const float* packed, int Cout,
                           int relu, float* y, int Ctot, int c_off, void* stream)
{
    if (!x || !packed || !y) return DC_ERR_INVALID;
    if (!launch_unit(x, N, Cin, T, H, W, k, stride, packed, Cout, relu, y, Ctot, c_off, (hipStream_t)stream)) return DC_ERR_INVALID;
    return dc_launch_status();
}

extern "C" int dc_fvd_maxpool(const float* x, int N, int C, int T, int H, int W, int kt, int kh, int kw, int st, int sh, int sw, float* y,
                              void* stream)
{
    if (!x || !y) return DC_ERR_INVALID;
    if (!launch_pool(x, N, C, T, H, W, kt, kh, kw, st, sh, sw, y, (hipStream_t)stream)) return DC_ERR_INVALID;
    return dc_launch_status();
}
