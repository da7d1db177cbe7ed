// Conditional Motion Propagation (cmp/models/modules/cmp.py of the reference): the stages of the network that turns a few hundred
// guide vectors and an anchor frame into dense flow, in exact fp32 for gfx950 on v_mfma_f32_32x32x2_f32.  Inference only.  Every
// sum runs in a fixed order and there are no float atomics, so results are bitwise reproducible and a sample's values do not
// depend on its position in the batch or on the batch size; the launches only enqueue on the caller's stream (graph-capturable).
//
//   conv      2D convolution, kernel 1/3/5/7, stride 1/2, dilation 1/2/4, padding dilation * (k - 1) / 2, + eval BatchNorm as one
//             fmaf(acc, s, t) (+ residual) (+ ReLU), written to a channel offset of a wider map (the network's torch.cat's are
//             never materialised).  Implicit GEMM  D[co][pixel] += W[co][k] * X[k][pixel] with k = (ci, kh, kw): weights packed
//             K-major [rows][CoP] (rows = Cin k k rounded up to 32 with zero rows, CoP = Cout rounded up to 32 with zero columns),
//             then s [CoP], t [CoP].  Workgroup = 4 waves = 64 output channels (two 32-channel MFMA tiles, the second skipped when
//             the padded Cout ends first) x 128 output pixels of ONE sample, the pixels flattened over Ho * Wo so that an 8 x 8
//             map wastes half a tile, not fifteen sixteenths.  K runs in chunks of 32 rows; a chunk's weight rows and its im2col
//             slab [32][128] (zero padding materialised, stride and dilation applied in the gather) go global -> registers ->
//             LDS, the loads of chunk c + 1 in flight under the MFMAs of chunk c; one MFMA takes a pair of consecutive k (lane
//             half h holds k = 2 kp + h), as in fvd.hip.  The instruction sequence of an output element is fixed by (Cin, k)
//             alone, which is what makes the result reproducible; nothing is assumed about the order inside one MFMA.  The
//             operand is read through element strides; a uint8 operand (the frames, NHWC) becomes (v - mean_c) / div_c in
//             the gather.
//   head      the 1x1 head fused with the expectation: a workgroup holds all 2 nbins logits of its 128 pixels in accumulators
//             (up to seven 32-channel tiles per wave), takes the two maxima, the fp32 exponentials and the fp64 sums across
//             its registers and the two lane halves, and writes the flow; the logits are stored only on request.
//   max-pool  kernel k, stride s, padding p; the padding never enters the max (PyTorch's rule), NaN propagates.
//   avg-pool  2 x 2 / 2, floor size, into a channel slice.
//   upsample  bilinear, align_corners = True, into a channel slice; source positions in fp64, the blend in fp32.
//   convert   two nbins-bin softmaxes (x bins, then y bins) and the expectation over the bin centres, max-subtracted.
//   grid      dense flow -> [flow at the grid points, 0 elsewhere | mask], gather form.
#include "dc_f32_mfma.h"
#include "../../include/diffcodec_flow_hip.h"
#include <vector>

namespace {

constexpr int CM_COB = 64;      // output channels per workgroup
constexpr int CM_PIX = 128;     // output pixels per workgroup
constexpr int CM_KC = 32;       // k rows per chunk

struct cm_conv {
    const void* x;
    long long xn, xc, xh, xw;   // element strides of the operand
    const float* wp;
    const float* s;
    const float* t;
    const float* res;           // contiguous [N][Cout][Ho][Wo] or null
    float* y;
    int Cin, H, W, Ho, Wo, CoP, Cout, Ctot, coff, stride, dil, pad, relu, K;
    float mean[3], div[3];
};

template <int KS, bool U8>
__global__ __launch_bounds__(256) void cmp_conv_kernel(cm_conv a)
{
    __shared__ __attribute__((aligned(16))) float Wl[CM_KC * CM_COB];
    __shared__ float Pl[CM_KC * CM_PIX];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int cb = blockIdx.y, n = blockIdx.z;
    const int wcols = min(CM_COB, a.CoP - cb * CM_COB), nq = wcols >> 5;
    const int P = a.Ho * a.Wo, p0 = blockIdx.x * CM_PIX;

    // gather role: this thread fills column pp of rows kr0, kr0 + 2, ...
    const int pp = tid & (CM_PIX - 1), kr0 = tid >> 7;
    const int gp = p0 + pp;
    const bool gvalid = gp < P;
    const int goy = gvalid ? gp / a.Wo : 0, gox = gvalid ? gp - goy * a.Wo : 0;
    const int iy0 = goy * a.stride - a.pad, ix0 = gox * a.stride - a.pad;
    const char* __restrict__ xb = (const char*)a.x;
    const long long xoff = (long long)n * a.xn;

    f32x16 acc[2];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

    const int pbase = wave * 32 + j;
    const int abase = h * CM_COB + j;
    const int nchunk = (a.K + CM_KC - 1) / CM_KC;
    const int wrow = tid >> 4, wc4 = (tid & 15) * 4;                    // weight role: rows wrow and wrow + 16, columns wc4 .. wc4 + 3
    const float* __restrict__ wbase = a.wp + cb * CM_COB + wc4;

    // chunk c's operands travel global -> registers while chunk c - 1 is in the MFMAs, then registers -> LDS
    float pv[CM_KC / 2];
    f32x4 wv[2];
    auto fetch = [&](int c) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            wv[i] = wc4 < wcols ? *(const f32x4*)&wbase[(long long)(c * CM_KC + wrow + 16 * i) * a.CoP] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < CM_KC / 2; ++i) {
            const int k = c * CM_KC + kr0 + 2 * i;
            float v = 0.f;
            if (gvalid && k < a.K) {
                const int ci = k / (KS * KS), r = k - ci * (KS * KS);
                const int kh = r / KS, kw = r - kh * KS;
                const int iy = iy0 + kh * a.dil, ix = ix0 + kw * a.dil;
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                    const long long o = xoff + (long long)ci * a.xc + (long long)iy * a.xh + (long long)ix * a.xw;
                    if (U8) {
#pragma clang fp contract(off)
                        const float mu = ci == 0 ? a.mean[0] : ci == 1 ? a.mean[1] : a.mean[2];
                        const float dv = ci == 0 ? a.div[0] : ci == 1 ? a.div[1] : a.div[2];
                        v = ((float)((const unsigned char*)xb)[o] - mu) / dv;
                    } else {
                        v = ((const float*)xb)[o];
                    }
                }
            }
            pv[i] = v;
        }
    };
    fetch(0);
    for (int c = 0; c < nchunk; ++c) {
        if (c) __syncthreads();                                          // everyone is done reading the previous chunk
#pragma unroll
        for (int i = 0; i < 2; ++i) *(f32x4*)&Wl[(wrow + 16 * i) * CM_COB + wc4] = wv[i];
#pragma unroll
        for (int i = 0; i < CM_KC / 2; ++i) Pl[(kr0 + 2 * i) * CM_PIX + pp] = pv[i];
        __syncthreads();
        if (c + 1 < nchunk) fetch(c + 1);
#pragma unroll
        for (int kp = 0; kp < CM_KC / 2; ++kp) dc_f32_kpair(acc, nq, &Wl[abase + kp * 2 * CM_COB], Pl[(2 * kp + h) * CM_PIX + pbase]);
    }

    const int p = p0 + pbase;
    if (p < P) {
        float* __restrict__ yo = a.y + ((long long)n * a.Ctot + a.coff) * P + p;
        const float* __restrict__ ro = a.res ? a.res + (long long)n * a.Cout * P + p : nullptr;
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (q < nq) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ch = dc_f32_channel(r, h, cb * CM_COB + q * 32);
                    if (ch < a.Cout) {
                        float v = __builtin_fmaf(acc[q][r], a.s[ch], a.t[ch]);
                        if (ro) v += ro[(long long)ch * P];
                        yo[(long long)ch * P] = (a.relu && v < 0.f) ? 0.f : v;            // NaN stays NaN
                    }
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------ pools
__global__ __launch_bounds__(256) void cmp_maxpool_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int Ho, int Wo,
                                                          int k, int s, int pad, long long total)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ox = (int)(i % Wo);
        const long long r = i / Wo;
        const int oy = (int)(r % Ho);
        const float* __restrict__ xp = x + (r / Ho) * H * W;
        float m = -INFINITY;
        for (int b = 0; b < k; ++b) {
            const int iy = oy * s - pad + b;
            if (iy < 0 || iy >= H) continue;
            for (int c = 0; c < k; ++c) {
                const int ix = ox * s - pad + c;
                if (ix < 0 || ix >= W) continue;
                const float v = xp[(long long)iy * W + ix];
                m = (v > m || v != v) ? v : m;                           // NaN propagates, as in PyTorch
            }
        }
        y[i] = m;
    }
}

__global__ __launch_bounds__(256) void cmp_avgpool_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int H, int W, int Ho,
                                                          int Wo, int Ctot, int coff, long long total)
{
#pragma clang fp contract(off)
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ox = (int)(i % Wo);
        long long r = i / Wo;
        const int oy = (int)(r % Ho);
        r /= Ho;
        const int c = (int)(r % C);
        const long long n = r / C;
        const float* __restrict__ xp = x + (n * C + c) * H * W + (long long)(2 * oy) * W + 2 * ox;
        y[((n * Ctot + coff + c) * Ho + oy) * Wo + ox] = (((xp[0] + xp[1]) + xp[W]) + xp[W + 1]) * 0.25f;
    }
}

// ------------------------------------------------------------------------------------------------ upsample, align_corners = True
__global__ __launch_bounds__(256) void cmp_upsample_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int H, int W, int Ho,
                                                           int Wo, int Ctot, int coff, long long total)
{
#pragma clang fp contract(off)
    const double sy = Ho > 1 ? (double)(H - 1) / (double)(Ho - 1) : 0.0, sx = Wo > 1 ? (double)(W - 1) / (double)(Wo - 1) : 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ox = (int)(i % Wo);
        long long r = i / Wo;
        const int oy = (int)(r % Ho);
        r /= Ho;
        const int c = (int)(r % C);
        const long long n = r / C;
        const double py = (double)oy * sy, px = (double)ox * sx;
        const int y0 = min((int)py, H - 1), x0 = min((int)px, W - 1);
        const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
        const float ly = (float)(py - (double)y0), lx = (float)(px - (double)x0);
        const float hy = 1.f - ly, hx = 1.f - lx;
        const float* __restrict__ xp = x + (n * C + c) * H * W;
        const float tl = xp[(long long)y0 * W + x0], tr = xp[(long long)y0 * W + x1];
        const float bl = xp[(long long)y1 * W + x0], br = xp[(long long)y1 * W + x1];
        y[((n * Ctot + coff + c) * Ho + oy) * Wo + ox] = hy * (hx * tl + lx * tr) + ly * (hx * bl + lx * br);
    }
}

// ------------------------------------------------------------------------------------------------ logits -> flow
// logits [N][2 nbins][P] -> flow [N][2][P]: per pixel and half, sum_i softmax_i * centre_i with centre_i = (i + 1/2) step - fmax.
// The exponentials are fp32 of (logit - max) <= 0, the two sums run in fp64 in bin order.
__global__ __launch_bounds__(256) void cmp_convert_kernel(const float* __restrict__ lg, float* __restrict__ fl, int nbins, long long P,
                                                          double fmax_, long long total)
{
    const double step = 2.0 * fmax_ / (double)nbins;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long p = i % P, nh = i / P;                           // nh = n * 2 + half
        const float* __restrict__ lp = lg + nh * nbins * P + p;
        float m = lp[0];
        for (int b = 1; b < nbins; ++b) {
            const float v = lp[(long long)b * P];
            m = (v > m || v != v) ? v : m;
        }
        double se = 0.0, sm = 0.0;
        for (int b = 0; b < nbins; ++b) {
            const double e = (double)expf(lp[(long long)b * P] - m);
            se += e;
            sm += e * (((double)b + 0.5) * step - fmax_);
        }
        fl[i] = (float)(sm / se);
    }
}

// ------------------------------------------------------------------------------------------------ grid sampling
// flow [N][2][H][W] -> sp [N][4][H][W]: channels 0-1 the flow at the points y0 + a stride, x0 + b stride (0 elsewhere), 2-3 the mask
__global__ __launch_bounds__(256) void cmp_grid_kernel(const float* __restrict__ fl, float* __restrict__ sp, int H, int W, int stride, int y0,
                                                       int x0, long long total)
{
    const long long P = (long long)H * W;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long p = i % P, n = i / P;
        const int yy = (int)(p / W), xx = (int)(p % W);
        const bool on = yy >= y0 && xx >= x0 && (yy - y0) % stride == 0 && (xx - x0) % stride == 0;
        float* __restrict__ o = sp + n * 4 * P + p;
        o[0] = on ? fl[n * 2 * P + p] : 0.f;
        o[P] = on ? fl[(n * 2 + 1) * P + p] : 0.f;
        o[2 * P] = o[3 * P] = on ? 1.f : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ fused head
constexpr int CM_HT = 7;                    // 32-channel tiles of the head: 2 nbins <= 224
constexpr int CM_HC = CM_HT * 32;

struct cm_head {
    const float* x;                         // contiguous [N][Cin][P]
    const float* wp;
    const float* s;
    const float* t;
    float* logits;                          // [N][2 nbins][P] or null
    float* flow;                            // [N][2][P]
    int Cin, CoP, nbins, P;
    double fmax;
};

__global__ __launch_bounds__(256) void cmp_head_kernel(cm_head a)
{
    __shared__ __attribute__((aligned(16))) float Wl[CM_KC * CM_HC];
    __shared__ float Pl[CM_KC * CM_PIX];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int n = blockIdx.y, p0 = blockIdx.x * CM_PIX;
    const int nt = a.CoP >> 5, w4 = a.CoP >> 2;
    const int pp = tid & (CM_PIX - 1), kr0 = tid >> 7;
    const int gp = p0 + pp;
    const bool gvalid = gp < a.P;
    const float* __restrict__ xn = a.x + (long long)n * a.Cin * a.P;

    f32x16 acc[CM_HT];
    dc_f32_zero(acc);

    const int pbase = wave * 32 + j;
    const int nchunk = (a.Cin + CM_KC - 1) / CM_KC;
    for (int c = 0; c < nchunk; ++c) {
        if (c) __syncthreads();
        dc_f32_copy_w<CM_HC>(Wl, a.wp + (long long)c * CM_KC * a.CoP, a.CoP, CM_KC, w4, tid);
#pragma unroll
        for (int i = 0; i < CM_KC / 2; ++i) {
            const int kr = kr0 + 2 * i, k = c * CM_KC + kr;
            Pl[kr * CM_PIX + pp] = (gvalid && k < a.Cin) ? xn[(long long)k * a.P + gp] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kp = 0; kp < CM_KC / 2; ++kp) dc_f32_kpair(acc, nt, &Wl[(2 * kp + h) * CM_HC + j], Pl[(2 * kp + h) * CM_PIX + pbase]);
    }

    // this lane holds, for pixel p, the channels dc_f32_channel(r, h, 32 q); lane ^ 32 holds the others
    const int p = p0 + pbase, C2 = 2 * a.nbins;
    const bool pvalid = p < a.P;
    float mx[2] = {-INFINITY, -INFINITY};
#pragma unroll
    for (int q = 0; q < CM_HT; ++q)
        if (q < nt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ch = dc_f32_channel(r, h, q * 32);
                if (ch < C2) {
                    const float v = __builtin_fmaf(acc[q][r], a.s[ch], a.t[ch]);
                    acc[q][r] = v;
                    if (a.logits && pvalid) a.logits[((long long)n * C2 + ch) * a.P + p] = v;
                    const int half = ch >= a.nbins;
                    mx[half] = (v > mx[half] || v != v) ? v : mx[half];
                }
            }
        }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float o = __shfl_xor(mx[i], 32);
        mx[i] = (o > mx[i] || o != o) ? o : mx[i];
    }
    const double step = 2.0 * a.fmax / (double)a.nbins;
    double se[2] = {0.0, 0.0}, sm[2] = {0.0, 0.0};
#pragma unroll
    for (int q = 0; q < CM_HT; ++q)
        if (q < nt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ch = dc_f32_channel(r, h, q * 32);
                if (ch < C2) {
                    const int half = ch >= a.nbins, b = ch - half * a.nbins;
                    const double e = (double)expf(acc[q][r] - mx[half]);
                    se[half] += e;
                    sm[half] += e * (((double)b + 0.5) * step - a.fmax);
                }
            }
        }
    // the two lane halves add their partial sums as (h = 0) + (h = 1) on both sides: one value per pixel
    double tot_e[2], tot_m[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double oe = __shfl_xor(se[i], 32), om = __shfl_xor(sm[i], 32);
        tot_e[i] = h ? oe + se[i] : se[i] + oe;
        tot_m[i] = h ? om + sm[i] : sm[i] + om;
    }
    if (pvalid) a.flow[((long long)n * 2 + h) * a.P + p] = (float)(h ? tot_m[1] / tot_e[1] : tot_m[0] / tot_e[0]);
}

inline int cm_blocks(long long total) { return dc_f32_blocks(total, 65535 * 16); }
inline bool cm_dim(long long v) { return v > 0 && v <= (1 << 24); }
inline long long cm_rows(int K) { return (long long)((K + CM_KC - 1) / CM_KC) * CM_KC; }   // k rows of a packed unit: whole chunks

template <int KS>
void cm_launch(const cm_conv& a, int u8, dim3 grid, hipStream_t st)
{
    if (u8)
        hipLaunchKernelGGL((cmp_conv_kernel<KS, true>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((cmp_conv_kernel<KS, false>), grid, dim3(256), 0, st, a);
}

}  // namespace

extern "C" int dc_cmp_conv(const void* x, int x_u8, const long long* xstrides, const float* mean_div, int N, int Cin, int H, int W, int k,
                           int stride, int dilation, const float* packed, int Cout, const float* residual, int relu, float* y, int Ctot,
                           int c_off, void* stream)
{
    if (!x || !xstrides || !packed || !y) return DC_ERR_INVALID;
    if (k != 1 && k != 3 && k != 5 && k != 7) return DC_ERR_INVALID;
    if ((stride != 1 && stride != 2) || (dilation != 1 && dilation != 2 && dilation != 4)) return DC_ERR_INVALID;
    if (N <= 0 || N > 65535 || !cm_dim(Cin) || !cm_dim(Cout) || !cm_dim(H) || !cm_dim(W) || c_off < 0 || c_off + Cout > Ctot) return DC_ERR_INVALID;
    if ((long long)H * W > (1ll << 28) || (long long)Cin * k * k > (1ll << 28)) return DC_ERR_INVALID;
    if (x_u8 && (Cin != 3 || !mean_div)) return DC_ERR_INVALID;
    if (((uintptr_t)packed & 15) != 0) return DC_ERR_INVALID;
    cm_conv a;
    a.x = x;
    a.xn = xstrides[0], a.xc = xstrides[1], a.xh = xstrides[2], a.xw = xstrides[3];
    a.Cin = Cin, a.H = H, a.W = W, a.stride = stride, a.dil = dilation, a.pad = dilation * (k - 1) / 2;
    a.Ho = (H + 2 * a.pad - dilation * (k - 1) - 1) / stride + 1;
    a.Wo = (W + 2 * a.pad - dilation * (k - 1) - 1) / stride + 1;
    a.K = Cin * k * k;
    a.CoP = dc_f32_cop(Cout);
    a.Cout = Cout, a.Ctot = Ctot, a.coff = c_off, a.relu = relu;
    dc_f32_split(packed, cm_rows(a.K), a.CoP, a.wp, a.s, a.t);
    a.res = residual;
    a.y = y;
    for (int c = 0; c < 3; ++c) {
        a.mean[c] = x_u8 ? mean_div[c] : 0.f;
        a.div[c] = x_u8 ? mean_div[3 + c] : 1.f;
    }
    const long long tiles = ((long long)a.Ho * a.Wo + CM_PIX - 1) / CM_PIX;
    const int cbs = (a.CoP + CM_COB - 1) / CM_COB;
    if (tiles > 0x7fffffffll || cbs > 65535) return DC_ERR_INVALID;
    const dim3 grid((unsigned)tiles, (unsigned)cbs, (unsigned)N);
    const hipStream_t st = (hipStream_t)stream;
    switch (k) {
    case 1: cm_launch<1>(a, x_u8, grid, st); break;
    case 3: cm_launch<3>(a, x_u8, grid, st); break;
    case 5: cm_launch<5>(a, x_u8, grid, st); break;
    default: cm_launch<7>(a, x_u8, grid, st); break;
    }
    return dc_launch_status();
}

extern "C" int dc_cmp_maxpool(const float* x, int NC, int H, int W, int k, int stride, int pad, float* y, void* stream)
{
    if (!x || !y || !cm_dim(NC) || !cm_dim(H) || !cm_dim(W) || k < 1 || k > 8 || stride < 1 || pad < 0 || 2 * pad > k) return DC_ERR_INVALID;
    if (H + 2 * pad < k || W + 2 * pad < k) return DC_ERR_INVALID;      // an empty map
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    const long long total = (long long)NC * Ho * Wo;
    hipLaunchKernelGGL(cmp_maxpool_kernel, dim3(cm_blocks(total)), dim3(256), 0, (hipStream_t)stream, x, y, H, W, Ho, Wo, k, stride, pad,
                       total);
    return dc_launch_status();
}

extern "C" int dc_cmp_avgpool(const float* x, int N, int C, int H, int W, float* y, int Ctot, int c_off, void* stream)
{
    if (!x || !y || !cm_dim(N) || !cm_dim(C) || !cm_dim(H) || !cm_dim(W) || H < 2 || W < 2) return DC_ERR_INVALID;
    if (c_off < 0 || c_off + C > Ctot) return DC_ERR_INVALID;
    const int Ho = H / 2, Wo = W / 2;
    const long long total = (long long)N * C * Ho * Wo;
    hipLaunchKernelGGL(cmp_avgpool_kernel, dim3(cm_blocks(total)), dim3(256), 0, (hipStream_t)stream, x, y, C, H, W, Ho, Wo, Ctot, c_off,
                       total);
    return dc_launch_status();
}

extern "C" int dc_cmp_upsample(const float* x, int N, int C, int H, int W, int Ho, int Wo, float* y, int Ctot, int c_off, void* stream)
{
    if (!x || !y || !cm_dim(N) || !cm_dim(C) || !cm_dim(H) || !cm_dim(W) || !cm_dim(Ho) || !cm_dim(Wo)) return DC_ERR_INVALID;
    if (c_off < 0 || c_off + C > Ctot) return DC_ERR_INVALID;
    const long long total = (long long)N * C * Ho * Wo;
    hipLaunchKernelGGL(cmp_upsample_kernel, dim3(cm_blocks(total)), dim3(256), 0, (hipStream_t)stream, x, y, C, H, W, Ho, Wo, Ctot, c_off,
                       total);
    return dc_launch_status();
}

extern "C" int dc_cmp_convert_flow(const float* logits, int N, int nbins, int h, int w, float fmax, float* flow, void* stream)
{
    if (!logits || !flow || !cm_dim(N) || nbins < 1 || nbins > 4096 || !cm_dim(h) || !cm_dim(w) || !(fmax > 0.f)) return DC_ERR_INVALID;
    const long long P = (long long)h * w, total = (long long)N * 2 * P;
    hipLaunchKernelGGL(cmp_convert_kernel, dim3(cm_blocks(total)), dim3(256), 0, (hipStream_t)stream, logits, flow, nbins, P, (double)fmax,
                       total);
    return dc_launch_status();
}

extern "C" int dc_cmp_sparse_grid(const float* flow, int N, int H, int W, int stride, float* sparse, void* stream)
{
    if (!flow || !sparse || !cm_dim(N) || !cm_dim(H) || !cm_dim(W) || stride < 1) return DC_ERR_INVALID;
    const int y0 = (H - H / stride * stride) / 2, x0 = (W - W / stride * stride) / 2;
    const long long total = (long long)N * H * W;
    hipLaunchKernelGGL(cmp_grid_kernel, dim3(cm_blocks(total)), dim3(256), 0, (hipStream_t)stream, flow, sparse, H, W, stride, y0, x0, total);
    return dc_launch_status();
}

extern "C" int dc_cmp_head(const float* x, int N, int Cin, int h, int w, const float* packed, int nbins, float fmax, float* logits,
                           float* flow, void* stream)
{
    if (!x || !packed || !flow || N <= 0 || N > 65535 || !cm_dim(Cin) || !cm_dim(h) || !cm_dim(w)) return DC_ERR_INVALID;
    if (nbins < 1 || 2 * nbins > CM_HC || !(fmax > 0.f) || (long long)h * w > (1ll << 28) || ((uintptr_t)packed & 15) != 0) return DC_ERR_INVALID;
    cm_head a;
    a.x = x, a.Cin = Cin, a.P = h * w, a.nbins = nbins, a.fmax = (double)fmax;
    a.CoP = dc_f32_cop(2 * nbins);
    dc_f32_split(packed, cm_rows(Cin), a.CoP, a.wp, a.s, a.t);
    a.logits = logits, a.flow = flow;
    hipLaunchKernelGGL(cmp_head_kernel, dim3((a.P + CM_PIX - 1) / CM_PIX, N), dim3(256), 0, (hipStream_t)stream, a);
    return dc_launch_status();
}

// ------------------------------------------------------------------------------------------------ the whole network
namespace {

struct cm_spec {
    int cin, cout, k;
};
constexpr int CM_LAYERS[4][4] = {{64, 3, 1, 1}, {128, 4, 2, 1}, {256, 6, 1, 2}, {512, 3, 1, 4}};   // planes, blocks, stride, dilation
constexpr int CM_ENC = 256, CM_SP = 16;

// the convolutions in forward order (the order of `weights`): stem; per bottleneck [downsample], conv1, conv2, conv3; conv5; the two
// sparse convolutions; the decoder branches; SkipLayer: fusion8, skipconv4, fusion4, skipconv2, fusion2; the head
bool cm_specs(int arch, int nbins, std::vector<cm_spec>& t)
{
    if ((arch != 0 && arch != 1) || nbins < 1 || 2 * nbins > CM_HC) return false;
    t.push_back({3, 64, 7});
    int cin = 64;
    for (const auto& l : CM_LAYERS)
        for (int b = 0; b < l[1]; ++b) {
            if (b == 0) t.push_back({cin, l[0] * 4, 1});
            t.push_back({cin, l[0], 1});
            t.push_back({l[0], l[0], 3});
            t.push_back({l[0], l[0] * 4, 1});
            cin = l[0] * 4;
        }
    t.push_back({2048, CM_ENC, 1});
    t.push_back({4, 16, 5});
    t.push_back({16, CM_SP, 3});
    const int branches = arch == 0 ? 4 : 3, depth = arch == 0 ? 3 : 2;
    for (int b = 0; b < branches; ++b)
        for (int i = 0; i < depth; ++i) t.push_back({i == 0 ? CM_ENC + CM_SP : 128, 128, 3});
    if (arch == 0) {
        t.push_back({512, 256, 3});
        t.push_back({256, 128, 3});
        t.push_back({384, 128, 3});
        t.push_back({64, 32, 3});
        t.push_back({160, 64, 3});
        t.push_back({64, 2 * nbins, 1});
    } else {
        t.push_back({384, 2 * nbins, 1});
    }
    return true;
}
inline long long cm_packed_floats(const cm_spec& c)
{
    return (cm_rows(c.cin * c.k * c.k) + 2) * dc_f32_cop(c.cout);
}

struct cm_plan {
    int h2, w2, h4, w4, h8, w8, hs, ws;     // hs x ws: the sparse encoder's map after its first convolution and max-pool
    long long enc, stem, layer1, sp1, sp1p, sp2, cat, pool, bx, f8, cat4, f4, cat2, f2, flow, big[3], small[2], total;   // float offsets
};
inline int cm_half(int v) { return (v - 1) / 2 + 1; }

bool cm_make_plan(int arch, int N, int H, int W, int nbins, cm_plan& p)
{
    if ((arch != 0 && arch != 1) || N <= 0 || N > 65535 || H < 1 || W < 1 || H > 16384 || W > 16384 || nbins < 1 || 2 * nbins > CM_HC) return false;
    p.h2 = cm_half(H), p.w2 = cm_half(W), p.h4 = cm_half(p.h2), p.w4 = cm_half(p.w2), p.h8 = cm_half(p.h4), p.w8 = cm_half(p.w4);
    p.hs = p.h2 / 2, p.ws = p.w2 / 2;
    if (p.hs / 2 != p.h8 || p.ws / 2 != p.w8) return false;             // the two encoders disagree: the reference's torch.cat fails
    const int pool = arch == 0 ? 8 : 4;
    if (p.h8 < pool || p.w8 < pool) return false;                        // a decoder max-pool would be empty
    const long long P2 = (long long)p.h2 * p.w2, P4 = (long long)p.h4 * p.w4, P8 = (long long)p.h8 * p.w8, n = N;
    if (n * 2048 * P8 > (1ll << 34)) return false;
    dc_f32_bump<4> ws;
    p.enc = ws.take(n * (CM_ENC + CM_SP) * P8);
    p.stem = ws.take(n * 64 * P2);
    p.layer1 = ws.take(n * 256 * P4);
    p.sp1 = ws.take(n * 16 * P2);
    p.sp1p = ws.take(n * 16 * p.hs * p.ws);
    p.sp2 = ws.take(n * CM_SP * p.hs * p.ws);
    p.cat = ws.take(n * 128 * (arch == 0 ? 4 : 3) * P8);
    p.pool = ws.take(n * (CM_ENC + CM_SP) * (p.h8 / 2) * (p.w8 / 2));
    p.bx = ws.take(2 * n * 128 * P8);
    p.f8 = ws.take(arch == 0 ? n * 256 * P8 : 0);
    p.cat4 = ws.take(arch == 0 ? n * 384 * P4 : 0);
    p.f4 = ws.take(arch == 0 ? n * 128 * P4 : 0);
    p.cat2 = ws.take(arch == 0 ? n * 160 * P2 : 0);
    p.f2 = ws.take(arch == 0 ? n * 64 * P2 : 0);
    p.flow = ws.take(n * 2 * (arch == 0 ? P2 : P8));
    const long long big = n * (256 * P4 > 2048 * P8 ? 256 * P4 : 2048 * P8), small = n * (128 * P4 > 512 * P8 ? 128 * P4 : 512 * P8);
    for (auto& b : p.big) b = ws.take(big);
    for (auto& b : p.small) b = ws.take(small);
    p.total = ws.off;
    return true;
}

#define CM_CK(call)            \
    do {                       \
        const int rc_ = (call); \
        if (rc_) return rc_;   \
    } while (0)

// maps (optional): the endpoint tensors of dc_cmp_endpoints; logits / flow / flow_up: each written when non-null
int cm_run(int arch, const void* image, int u8, const long long* istr, const float* sparse, int N, int H, int W, int nbins, float fmax,
           const float* weights, void* wsv, float* logits, float* flow, float* flow_up, float* const* maps, void* st)
{
    cm_plan p;
    std::vector<cm_spec> t;
    if (!image || !istr || !sparse || !weights || !wsv || ((uintptr_t)weights & 15) || ((uintptr_t)wsv & 255)) return DC_ERR_INVALID;
    if (!cm_specs(arch, nbins, t) || !cm_make_plan(arch, N, H, W, nbins, p)) return DC_ERR_INVALID;
    float* ws = (float*)wsv;
    static const float mean_div[6] = {123.675f, 116.28f, 103.53f, 58.395f, 57.12f, 57.375f};
    const float* wq = weights;
    size_t ti = 0;
    // one convolution on contiguous maps, taking the next block of `weights`
    auto conv = [&](const float* x, int h, int w, int stride, int dil, const float* res, int relu, float* y, int ctot, int coff) {
        const cm_spec& c = t[ti++];
        const long long xs[4] = {(long long)c.cin * h * w, (long long)h * w, w, 1};
        const float* pk = wq;
        wq += cm_packed_floats(c);
        return dc_cmp_conv(x, 0, xs, nullptr, N, c.cin, h, w, c.k, stride, dil, pk, c.cout, res, relu, y, ctot, coff, st);
    };
    const int DIN = CM_ENC + CM_SP;
    float *enc = ws + p.enc, *stem = ws + p.stem, *layer1 = ws + p.layer1;

    {                                                                    // image encoder
        const cm_spec& c = t[ti++];
        CM_CK(dc_cmp_conv(image, u8, istr, mean_div, N, 3, H, W, 7, 2, 1, wq, 64, nullptr, 1, stem, 64, 0, st));
        wq += cm_packed_floats(c);
    }
    float* slots[3] = {ws + p.big[0], ws + p.big[1], ws + p.big[2]};
    float *s1 = ws + p.small[0], *s2 = ws + p.small[1];
    CM_CK(dc_cmp_maxpool(stem, N * 64, p.h2, p.w2, 3, 2, 1, slots[0], st));
    float* x = slots[0];
    int h = p.h4, w = p.w4;
    for (int l = 0; l < 4; ++l) {
        const int blocks = CM_LAYERS[l][1], stride = CM_LAYERS[l][2], dil = CM_LAYERS[l][3];
        for (int b = 0; b < blocks; ++b) {
            const int sb = b == 0 ? stride : 1;
            const int ho = (h - 1) / sb + 1, wo = (w - 1) / sb + 1;
            float* free_[2];
            int nf = 0;
            for (float* s : slots)
                if (s != x && nf < 2) free_[nf++] = s;
            const float* res = x;
            if (b == 0) {
                CM_CK(conv(x, h, w, sb, 1, nullptr, 0, free_[0], CM_LAYERS[l][0] * 4, 0));
                res = free_[0];
            }
            float* out = (l == 0 && b == blocks - 1) ? layer1 : free_[1];
            CM_CK(conv(x, h, w, 1, 1, nullptr, 1, s1, CM_LAYERS[l][0], 0));
            CM_CK(conv(s1, h, w, sb, dil, nullptr, 1, s2, CM_LAYERS[l][0], 0));
            CM_CK(conv(s2, ho, wo, 1, 1, res, 1, out, CM_LAYERS[l][0] * 4, 0));
            x = out, h = ho, w = wo;
        }
    }
    CM_CK(conv(x, h, w, 1, 1, nullptr, 0, enc, DIN, 0));                  // conv5 -> channels 0 .. 255 of the concatenation

    {                                                                    // sparse encoder -> channels 256 .. 271
        float *a1 = ws + p.sp1, *a2 = ws + p.sp1p, *a3 = ws + p.sp2;
        CM_CK(conv(sparse, H, W, 2, 1, nullptr, 1, a1, 16, 0));
        CM_CK(dc_cmp_maxpool(a1, N * 16, p.h2, p.w2, 2, 2, 0, a2, st));
        CM_CK(conv(a2, p.hs, p.ws, 1, 1, nullptr, 1, a3, CM_SP, 0));
        CM_CK(dc_cmp_avgpool(a3, N, CM_SP, p.hs, p.ws, enc, DIN, CM_ENC, st));
    }

    const int branches = arch == 0 ? 4 : 3, depth = arch == 0 ? 3 : 2, CT = 128 * branches;
    float *cat = ws + p.cat, *pool = ws + p.pool, *b0 = ws + p.bx, *b1 = b0 + (long long)N * 128 * p.h8 * p.w8;
    for (int br = 0; br < branches; ++br) {
        const int f = 1 << br, hb = p.h8 / f, wb = p.w8 / f;
        const float* cur = enc;
        if (br) {
            CM_CK(dc_cmp_maxpool(enc, N * DIN, p.h8, p.w8, f, f, 0, pool, st));
            cur = pool;
        }
        for (int i = 0; i < depth; ++i) {
            const bool direct = br == 0 && i == depth - 1;              // the full-resolution branch ends in its slice
            float* y = direct ? cat : (i & 1 ? b1 : b0);
            CM_CK(conv(cur, hb, wb, 1, 1, nullptr, 1, y, direct ? CT : 128, 0));
            cur = y;
        }
        if (br) CM_CK(dc_cmp_upsample(cur, N, 128, hb, wb, p.h8, p.w8, cat, CT, 128 * br, st));
    }

    const float* top = cat;
    int ht = p.h8, wt = p.w8, ctop = CT;
    float *f8 = ws + p.f8, *f4 = ws + p.f4, *f2 = ws + p.f2;
    if (arch == 0) {
        float *cat4 = ws + p.cat4, *cat2 = ws + p.cat2;
        CM_CK(conv(cat, p.h8, p.w8, 1, 1, nullptr, 1, f8, 256, 0));
        CM_CK(dc_cmp_upsample(f8, N, 256, p.h8, p.w8, p.h4, p.w4, cat4, 384, 0, st));
        CM_CK(conv(layer1, p.h4, p.w4, 1, 1, nullptr, 1, cat4, 384, 256));
        CM_CK(conv(cat4, p.h4, p.w4, 1, 1, nullptr, 1, f4, 128, 0));
        CM_CK(dc_cmp_upsample(f4, N, 128, p.h4, p.w4, p.h2, p.w2, cat2, 160, 0, st));
        CM_CK(conv(stem, p.h2, p.w2, 1, 1, nullptr, 1, cat2, 160, 128));
        CM_CK(conv(cat2, p.h2, p.w2, 1, 1, nullptr, 1, f2, 64, 0));
        top = f2, ht = p.h2, wt = p.w2, ctop = 64;
    }
    float* fl = flow ? flow : ws + p.flow;
    CM_CK(dc_cmp_head(top, N, ctop, ht, wt, wq, nbins, fmax, logits, fl, st));
    if (flow_up) {
        if (ht == H && wt == W)
            CM_CK(hipMemcpyAsync(flow_up, fl, sizeof(float) * N * 2 * H * W, hipMemcpyDeviceToDevice, (hipStream_t)st) == hipSuccess ? 0 : DC_ERR_LAUNCH);
        else
            CM_CK(dc_cmp_upsample(fl, N, 2, ht, wt, H, W, flow_up, 2, 0, st));
    }
    if (maps) {                                                          // copies of the workspace's maps; the slices of `enc` row by row
        const size_t P2 = (size_t)p.h2 * p.w2 * 4, P4 = (size_t)p.h4 * p.w4 * 4, P8 = (size_t)p.h8 * p.w8 * 4;
        auto copy = [&](float* dst, const float* src, size_t bytes) {
            return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)st) == hipSuccess ? 0 : DC_ERR_LAUNCH;
        };
        CM_CK(hipMemcpy2DAsync(maps[0], CM_SP * P8, enc + (long long)CM_ENC * p.h8 * p.w8, DIN * P8, CM_SP * P8, N, hipMemcpyDeviceToDevice,
                               (hipStream_t)st) == hipSuccess ? 0 : DC_ERR_LAUNCH);
        CM_CK(hipMemcpy2DAsync(maps[1], CM_ENC * P8, enc, DIN * P8, CM_ENC * P8, N, hipMemcpyDeviceToDevice, (hipStream_t)st) == hipSuccess
                  ? 0 : DC_ERR_LAUNCH);
        CM_CK(copy(maps[2], stem, N * 64 * P2));
        CM_CK(copy(maps[3], layer1, N * 256 * P4));
        if (arch == 0) {
            CM_CK(copy(maps[4], f8, N * 256 * P8));
            CM_CK(copy(maps[5], f4, N * 128 * P4));
            CM_CK(copy(maps[6], f2, N * 64 * P2));
        } else {
            CM_CK(copy(maps[4], cat, N * (size_t)CT * P8));
        }
    }
    return DC_OK;
}

}  // namespace

extern "C" int dc_cmp_weight_floats(int arch, int nbins)
{
    std::vector<cm_spec> t;
    if (!cm_specs(arch, nbins, t)) return -1;
    long long n = 0;
    for (const auto& c : t) n += cm_packed_floats(c);
    return (int)n;
}

extern "C" long long dc_cmp_ws_bytes(int arch, int N, int H, int W)
{
    cm_plan p;
    return cm_make_plan(arch, N, H, W, 99, p) ? p.total * 4 : -1;
}

extern "C" int dc_cmp_forward(int arch, const void* image, int image_u8, const long long* image_strides, const float* sparse, int N, int H,
                              int W, int nbins, float fmax, const float* weights, void* ws, float* logits, float* flow, void* stream)
{
    if (!logits && !flow) return DC_ERR_INVALID;
    return cm_run(arch, image, image_u8, image_strides, sparse, N, H, W, nbins, fmax, weights, ws, logits, flow, nullptr, nullptr, stream);
}

extern "C" int dc_cmp_flow(int arch, const void* image, int image_u8, const long long* image_strides, const float* sparse, int N, int H, int W,
                           int nbins, float fmax, const float* weights, void* ws, float* flow_up, void* stream)
{
    if (!flow_up) return DC_ERR_INVALID;
    return cm_run(arch, image, image_u8, image_strides, sparse, N, H, W, nbins, fmax, weights, ws, nullptr, nullptr, flow_up, nullptr, stream);
}

extern "C" int dc_cmp_endpoints(int arch, const void* image, int image_u8, const long long* image_strides, const float* sparse, int N, int H,
                                int W, int nbins, float fmax, const float* weights, void* ws, float* const* maps, float* logits, float* flow,
                                float* flow_up, void* stream)
{
    const int nm = arch == 0 ? 7 : 5;
    if (!maps || !logits || !flow || !flow_up || (arch != 0 && arch != 1)) return DC_ERR_INVALID;
    for (int i = 0; i < nm; ++i)
        if (!maps[i]) return DC_ERR_INVALID;
    return cm_run(arch, image, image_u8, image_strides, sparse, N, H, W, nbins, fmax, weights, ws, logits, flow, flow_up, maps, stream);
}
