// LPIPS (AlexNet, version 0.1) of decoded frames against their ground truth (test_utils.py:13,58: lpips.LPIPS(net='alex')), in exact
// fp32 for gfx950: five fp32 convolutions on v_mfma_f32_32x32x2_f32 (bias + ReLU in the epilogue), two max-pools and one fused
// distance tail per layer.  Every sum runs in a fixed order, there are no float atomics: results are bitwise reproducible, do not
// depend on the position of a pair in the batch, and the launches only enqueue on the caller's stream (graph-capturable).
//
// The 2N images of N pairs run as ONE batch of 2N (image z < N comes from x, the others from y), so one weight slice in cache
// serves both sides.  Weights arrive packed K-major ([K = (ci, ky, kx)][Cout], metrics.py packs them once at load): a weight slice
// is then a run of whole 256-byte rows, loaded coalesced and written to LDS as it is; this replaces the in-kernel transpose of
// conv_f32_mfma.hip (whose lanes each fetch from another weight row).
//
// Convolutions, implicit GEMM  D[co][pixel] += W[co][k] * X[k][pixel]:
//   workgroup = 4 waves, tile = 64 output channels x (4 rows x 32 columns) of one image; ragged edges are masked in the patch load
//   (zero padding materialised in LDS) and in the store, so any map size works (from 512^2: 127 / 63 / 31 wide, one column of the
//   32 idle).  Wave w takes channel half w & 1 and rows 2 (w >> 1), 2 (w >> 1) + 1: two accumulator tiles, one A read per two MFMAs.
//   MFMA operand and C/D layouts: dc_f32_mfma.h.
//   conv2-5 (5x5 | 3x3, stride 1): K runs over chunks of CK input channels (4 | 8); the chunk's patch and weight slice are staged in
//     LDS from registers loaded one chunk ahead; one k-step is a PAIR of input channels at one tap.
//   conv1 (3 -> 64, 11x11, stride 4, pad 2): K = (c, ky, kx) = 363, padded to 364 with a zero weight row; the whole weight matrix
//     and the tile's 3 x 23 x 135 patch are staged once.  The patch is read from the image operand itself (uint8 or fp32 through
//     element strides) with the input transform fused: x / 255 for uint8, the optional 2x - 1, then the ScalingLayer
//     (x - shift) / scale.  Padding is zero in the SCALED space (a padded tap contributes 0).  One k-step is a pair of consecutive k.
// Distance tail, one launch per layer: lanes along pixels (coalesced NCHW reads), the 4 waves split the channels; pass 1 sums the
//   squares, pass 2 sums w_c (x_c / (|x| + eps) - y_c / (|y| + eps))^2; the normalised maps never exist in memory.  One fp64 partial
//   per workgroup, then one finalize launch sums each (layer, image) slab in a fixed order into the spatial mean and the five means
//   into the value.
#include "dc_f32_mfma.h"
#include "dc_lpips_geom.h"
#include "../../include/diffcodec_hip.h"

namespace {

constexpr int LP_CO = 64;                  // output channels per workgroup
constexpr int LP_COLS = 32, LP_ROWS = 4;   // output pixels per workgroup: LP_ROWS rows of LP_COLS columns
constexpr int LP_LAYERS = 5;
constexpr int LP_CH[LP_LAYERS] = {64, 192, 384, 256, 256};
constexpr int LP_CIN[LP_LAYERS] = {3, 64, 192, 384, 256};
constexpr int LP_KS[LP_LAYERS] = {11, 5, 3, 3, 3};
constexpr int LP_K1 = 364;                 // conv1's K (3 * 11 * 11 = 363) padded to a whole number of pairs
constexpr int LP_MIN_HW = 31;              // smallest image: the maps are 7 / 3 / 1 / 1 / 1
constexpr int LP_TAIL_PX = 64;             // pixels per workgroup of the tail: one per lane

// ------------------------------------------------------------------------------------------------ conv2 .. conv5
template <int KS, int CK>
__global__ __launch_bounds__(256, 2) void lpips_conv_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                            const float* __restrict__ bias, float* __restrict__ y, int Cin, int H,
                                                            int W, int Cout, int tiles_x)
{
    constexpr int KK = KS * KS, PAD = KS / 2;
    constexpr int PH = LP_ROWS - 1 + KS, PW = LP_COLS - 1 + KS;
    constexpr int PE = CK * PH * PW, NPE = (PE + 255) / 256;          // patch floats, per thread
    constexpr int WROWS = CK * KK;                                   // k rows of the weight slice, LP_CO floats each
    constexpr int WP4 = WROWS * (LP_CO / 4), NWP = (WP4 + 255) / 256;   // float4 pieces, per thread
    __shared__ __attribute__((aligned(16))) float Wl[WROWS * LP_CO];
    __shared__ float Pl[PE];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ch = wave & 1, ph = wave >> 1;
    const int j = lane & 31, h = lane >> 5;
    const int ty0 = (blockIdx.x / tiles_x) * LP_ROWS, tx0 = (blockIdx.x % tiles_x) * LP_COLS;
    const int co0 = blockIdx.y * LP_CO, n = blockIdx.z;
    const float* __restrict__ xn = x + (long long)n * Cin * H * W;

    // patch staging plan: element e = tid + 256 i of [CK][PH][PW] -> offset inside the chunk, or -1 (padding / outside the map)
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
    for (int b = 0; b < 2; ++b) pbase[b] = (ph * 2 + b) * PW + j + h * (PH * PW);     // lane half h reads the odd channel of the pair
    const int abase = h * KK * LP_CO + ch * 32 + j;

    f32x16 acc[2];
    dc_f32_zero(acc);

    const int nchunk = Cin / CK;
    load_chunk(0);
    for (int c = 0; c < nchunk; ++c) {
        __syncthreads();                                   // everyone is done reading the previous chunk
        store_chunk();
        __syncthreads();
        if (c + 1 < nchunk) load_chunk((c + 1) * CK);      // flies under this chunk's MFMAs
#pragma unroll
        for (int cp = 0; cp < CK / 2; ++cp) {
#pragma unroll
            for (int tap = 0; tap < KK; ++tap) {
                const float a = Wl[abase + (cp * 2 * KK + tap) * LP_CO];
                const int poff = cp * 2 * (PH * PW) + (tap / KS) * PW + (tap % KS);
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Pl[pbase[b] + poff], acc[b], 0, 0, 0);
            }
        }
    }

    // epilogue: bias + ReLU, masked at the ragged edges
    const int ox = tx0 + j;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int oy = ty0 + ph * 2 + b;
        if (oy < H && ox < W) {
            float* __restrict__ yo = y + (((long long)n * Cout + co0 + ch * 32) * H + oy) * W + ox;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int col = dc_f32_channel(r, h);
                yo[(long long)col * H * W] = fmaxf(acc[b][r] + bias[co0 + ch * 32 + col], 0.f);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ conv1
constexpr int L1_KS = 11, L1_S = 4, L1_PAD = 2;
constexpr int L1_PH = (LP_ROWS - 1) * L1_S + L1_KS, L1_PW = (LP_COLS - 1) * L1_S + L1_KS;      // 23 x 135
constexpr int L1_PE = 3 * L1_PH * L1_PW;
constexpr int L1_LDS_BYTES = (LP_K1 * LP_CO + L1_PE) * 4;

__device__ constexpr int l1_off(int k) { return dc_f32_patch_off<L1_KS, L1_PW, L1_PH * L1_PW, 363>(k); }   // k = (c, ky, kx)

template <typename T>
__device__ __forceinline__ float l1_load(const T* __restrict__ p, long long i)
{
#pragma clang fp contract(off)
    if constexpr (sizeof(T) == 1) return (float)p[i] / 255.f;
    else return p[i];
}

template <typename T>
__global__ __launch_bounds__(256) void lpips_conv1_kernel(const T* __restrict__ x, const T* __restrict__ y, dc_strides4 sx, dc_strides4 sy,
                                                          int NX, const float* __restrict__ wp, const float* __restrict__ bias,
                                                          float* __restrict__ out, int H, int W, int Ho, int Wo, int tiles_x,
                                                          int normalize)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Wl = lds;                                       // [LP_K1][LP_CO]
    float* Pl = lds + LP_K1 * LP_CO;                       // [3][L1_PH][L1_PW], already scaled
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ch = wave & 1, ph = wave >> 1;
    const int j = lane & 31, h = lane >> 5;
    const int ty0 = (blockIdx.x / tiles_x) * LP_ROWS, tx0 = (blockIdx.x % tiles_x) * LP_COLS;
    const int n = blockIdx.z;
    const bool first = n < NX;
    const T* __restrict__ src = first ? x + n * sx.n : y + (n - NX) * sy.n;
    const dc_strides4 s = first ? sx : sy;

    dc_f32_copy_w<LP_CO>(Wl, wp, LP_CO, LP_K1, LP_CO / 4, tid);
    const int iy0 = ty0 * L1_S - L1_PAD, ix0 = tx0 * L1_S - L1_PAD;
    for (int e = tid; e < L1_PE; e += 256) {
        const int c = e / (L1_PH * L1_PW), r = e - c * (L1_PH * L1_PW);
        const int py = r / L1_PW, px = r - py * L1_PW;
        const int iy = iy0 + py, ix = ix0 + px;
        float v = 0.f;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
            v = l1_load(src, c * s.c + iy * s.h + ix * s.w);
            if (normalize) v = 2.f * v - 1.f;
            const float shift = c == 0 ? -.030f : c == 1 ? -.088f : -.188f;
            const float scale = c == 0 ? .458f : c == 1 ? .448f : .450f;
            v = (v - shift) / scale;
        }
        Pl[e] = v;
    }
    __syncthreads();

    int pbase[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) pbase[b] = (ph * 2 + b) * L1_S * L1_PW + j * L1_S;
    const int abase = h * LP_CO + ch * 32 + j;
    f32x16 acc[2];
    dc_f32_zero(acc);
#pragma unroll
    for (int kp = 0; kp < LP_K1 / 2; ++kp) {               // lane half h takes k = 2 kp + h
        const float a = Wl[abase + kp * 2 * LP_CO];
        const int poff = h ? l1_off(2 * kp + 1) : l1_off(2 * kp);
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Pl[pbase[b] + poff], acc[b], 0, 0, 0);
    }

    const int ox = tx0 + j;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int oy = ty0 + ph * 2 + b;
        if (oy < Ho && ox < Wo) {
            float* __restrict__ yo = out + (((long long)n * LP_CO + ch * 32) * Ho + oy) * Wo + ox;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int col = dc_f32_channel(r, h);
                yo[(long long)col * Ho * Wo] = fmaxf(acc[b][r] + bias[ch * 32 + col], 0.f);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ max_pool2d(3, stride 2), floor mode
__global__ __launch_bounds__(256) void lpips_pool_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int Ho, int Wo,
                                                         long long total)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ox = (int)(i % Wo);
        const long long t = i / Wo;
        const int oy = (int)(t % Ho);
        const float* p = x + ((t / Ho) * H + 2 * oy) * W + 2 * ox;           // every window lies inside the map
        float m = p[0];
#pragma unroll
        for (int q = 1; q < 9; ++q) m = fmaxf(m, p[(q / 3) * W + (q % 3)]);
        y[i] = m;
    }
}

// ------------------------------------------------------------------------------------------------ distance tail
// f: [2N][C][HW] post-ReLU maps (image n against image N + n).  part[n * gridDim.x + blockIdx.x] = this workgroup's fp64 sum.
__global__ __launch_bounds__(256) void lpips_tail_kernel(const float* __restrict__ f, int N, int C, int HW, const float* __restrict__ lin,
                                                         int normfix, double* __restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ float sq[2][4][LP_TAIL_PX];
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n = blockIdx.y;
    const int p = blockIdx.x * LP_TAIL_PX + lane;
    const bool in = p < HW;
    const float* __restrict__ xb = f + (long long)n * C * HW + p;
    const float* __restrict__ yb = f + (long long)(N + n) * C * HW + p;
    float sx = 0.f, sy = 0.f;
    for (int c = wv; c < C; c += 4) {                      // C is a multiple of 4: every wave takes C / 4 channels
        const float a = in ? xb[(long long)c * HW] : 0.f, b = in ? yb[(long long)c * HW] : 0.f;
        sx = __builtin_fmaf(a, a, sx);
        sy = __builtin_fmaf(b, b, sy);
    }
    sq[0][wv][lane] = sx;
    sq[1][wv][lane] = sy;
    __syncthreads();
    const float nx2 = ((sq[0][0][lane] + sq[0][1][lane]) + sq[0][2][lane]) + sq[0][3][lane];
    const float ny2 = ((sq[1][0][lane] + sq[1][1][lane]) + sq[1][2][lane]) + sq[1][3][lane];
    // lpips.normalize_tensor: x / (sqrt(sum x^2) + 1e-10); NormFix (controlnet/lpips_loss.py:27-29): x / sqrt(sum (x^2 + 1e-8))
    const float dx = normfix ? sqrtf(nx2 + (float)C * 1e-8f) : sqrtf(nx2) + 1e-10f;
    const float dy = normfix ? sqrtf(ny2 + (float)C * 1e-8f) : sqrtf(ny2) + 1e-10f;
    double s = 0.0;
    for (int c = wv; c < C; c += 4) {
        const float a = in ? xb[(long long)c * HW] : 0.f, b = in ? yb[(long long)c * HW] : 0.f;
        const float d = a / dx - b / dy;
        s += (double)(lin[c] * (d * d));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) red[wv] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[(long long)n * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

struct lp_segments {
    long long off[LP_LAYERS];                // first partial of layer l (doubles)
    int count[LP_LAYERS];                    // partials per image
    long long area[LP_LAYERS];               // pixels per map
};

// One wave per pair: lane t sums partials t, t + 64, ... of a layer in order, a fixed butterfly sums the lanes;
// out[l * N + n] = spatial mean of layer l, out[5 N + n] = their sum in layer order.
__global__ __launch_bounds__(64) void lpips_finalize_kernel(const double* __restrict__ part, lp_segments seg, int N, double* __restrict__ out)
{
    const int n = blockIdx.x;
    double total = 0.0;
    for (int l = 0; l < LP_LAYERS; ++l) {
        const double* src = part + seg.off[l] + (long long)n * seg.count[l];
        double s = 0.0;
        for (int i = threadIdx.x; i < seg.count[l]; i += 64) s += src[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const double m = s / (double)seg.area[l];
        if (threadIdx.x == 0) out[(long long)l * N + n] = m;
        total += m;
    }
    if (threadIdx.x == 0) out[(long long)LP_LAYERS * N + n] = total;
}

// ------------------------------------------------------------------------------------------------ host side
// Map sizes and workspace layout for M images (a call on N pairs has M = 2 N): the five post-ReLU maps, the two pooled maps,
// and (pairs only) the tail partials.
struct lp_plan {
    int h[LP_LAYERS], w[LP_LAYERS];          // map of layer l (relu1 .. relu5)
    int hp[2], wp[2];                        // pooled relu1, relu2
    long long feat_off[LP_LAYERS], pool_off[2], part_off, total;
    lp_segments seg;
};

bool make_lp_plan(int M, int pairs, int H, int W, lp_plan& p)
{
    if (M <= 0 || M > 65535 || H < LP_MIN_HW || W < LP_MIN_HW || H > 16384 || W > 16384) return false;
    p.h[0] = (H + 2 * L1_PAD - L1_KS) / L1_S + 1;
    p.w[0] = (W + 2 * L1_PAD - L1_KS) / L1_S + 1;
    p.hp[0] = (p.h[0] - 3) / 2 + 1;
    p.wp[0] = (p.w[0] - 3) / 2 + 1;
    p.h[1] = p.hp[0];
    p.w[1] = p.wp[0];
    p.hp[1] = (p.h[1] - 3) / 2 + 1;
    p.wp[1] = (p.w[1] - 3) / 2 + 1;
    for (int l = 2; l < LP_LAYERS; ++l) {
        p.h[l] = p.hp[1];
        p.w[l] = p.wp[1];
    }
    dc_f32_bump<1> ws;
    long long parts = 0;
    for (int l = 0; l < LP_LAYERS; ++l) {
        p.feat_off[l] = ws.take((long long)M * LP_CH[l] * p.h[l] * p.w[l] * 4);
        p.seg.off[l] = parts;
        p.seg.count[l] = (p.h[l] * p.w[l] + LP_TAIL_PX - 1) / LP_TAIL_PX;
        p.seg.area[l] = (long long)p.h[l] * p.w[l];
        parts += (long long)pairs * p.seg.count[l];
    }
    for (int l = 0; l < 2; ++l) p.pool_off[l] = ws.take((long long)M * LP_CH[l] * p.hp[l] * p.wp[l] * 4);
    p.part_off = ws.take(parts * 8);
    p.total = ws.off;
    return true;
}

// offsets (floats) into the packed weight buffer: per layer the K-major matrix [K][Cout] then the bias, then the five lin vectors
struct lp_weights {
    long long w[LP_LAYERS], b[LP_LAYERS], lin[LP_LAYERS], total;
};
lp_weights lp_weight_layout()
{
    lp_weights o;
    long long off = 0;
    for (int l = 0; l < LP_LAYERS; ++l) {
        o.w[l] = off;
        off += (long long)(l == 0 ? LP_K1 : LP_CIN[l] * LP_KS[l] * LP_KS[l]) * LP_CH[l];
        o.b[l] = off;
        off += LP_CH[l];
    }
    for (int l = 0; l < LP_LAYERS; ++l) {
        o.lin[l] = off;
        off += LP_CH[l];
    }
    o.total = off;
    return o;
}

template <int KS, int CK>
void launch_conv(const float* x, const float* w, const float* b, float* y, int M, int Cin, int H, int W, int Cout, hipStream_t st)
{
    const int tiles_x = (W + LP_COLS - 1) / LP_COLS, tiles_y = (H + LP_ROWS - 1) / LP_ROWS;
    hipLaunchKernelGGL((lpips_conv_kernel<KS, CK>), dim3(tiles_x * tiles_y, Cout / LP_CO, M), dim3(256), 0, st, x, w, b, y, Cin, H, W,
                       Cout, tiles_x);
}

template <typename T>
void launch_conv1(const void* x, const void* y, dc_strides4 sx, dc_strides4 sy, int NX, int M, const float* w, const float* b, float* out,
                  int H, int W, int Ho, int Wo, int normalize, hipStream_t st)
{
    auto kern = lpips_conv1_kernel<T>;
    static std::atomic<unsigned long long> attr_done{0};
    dc_set_max_dyn_lds((const void*)kern, L1_LDS_BYTES, attr_done);
    const int tiles_x = (Wo + LP_COLS - 1) / LP_COLS, tiles_y = (Ho + LP_ROWS - 1) / LP_ROWS;
    hipLaunchKernelGGL(kern, dim3(tiles_x * tiles_y, 1, M), dim3(256), L1_LDS_BYTES, st, (const T*)x, (const T*)y, sx, sy, NX, w, b, out,
                       H, W, Ho, Wo, tiles_x, normalize);
}

void launch_pool(const float* x, float* y, int planes, int H, int W, int Ho, int Wo, hipStream_t st)
{
    const long long total = (long long)planes * Ho * Wo;
    const int grid = dc_f32_blocks(total, 8192);
    hipLaunchKernelGGL(lpips_pool_kernel, dim3(grid), dim3(256), 0, st, x, y, H, W, Ho, Wo, total);
}

// The five post-ReLU maps of M images (the first NX from x, the rest from y) into f[0..4]; pool[0..1] take the pooled maps.
void run_features(const void* x, const void* y, int u8, dc_strides4 sx, dc_strides4 sy, int NX, int M, int H, int W, int normalize,
                  const float* wts, const lp_plan& p, float* const f[LP_LAYERS], float* const pool[2], hipStream_t st)
{
    const lp_weights o = lp_weight_layout();
    if (u8)
        launch_conv1<uint8_t>(x, y, sx, sy, NX, M, wts + o.w[0], wts + o.b[0], f[0], H, W, p.h[0], p.w[0], normalize, st);
    else
        launch_conv1<float>(x, y, sx, sy, NX, M, wts + o.w[0], wts + o.b[0], f[0], H, W, p.h[0], p.w[0], normalize, st);
    launch_pool(f[0], pool[0], M * LP_CH[0], p.h[0], p.w[0], p.hp[0], p.wp[0], st);
    launch_conv<5, 4>(pool[0], wts + o.w[1], wts + o.b[1], f[1], M, LP_CIN[1], p.h[1], p.w[1], LP_CH[1], st);
    launch_pool(f[1], pool[1], M * LP_CH[1], p.h[1], p.w[1], p.hp[1], p.wp[1], st);
    launch_conv<3, 8>(pool[1], wts + o.w[2], wts + o.b[2], f[2], M, LP_CIN[2], p.h[2], p.w[2], LP_CH[2], st);
    launch_conv<3, 8>(f[2], wts + o.w[3], wts + o.b[3], f[3], M, LP_CIN[3], p.h[3], p.w[3], LP_CH[3], st);
    launch_conv<3, 8>(f[3], wts + o.w[4], wts + o.b[4], f[4], M, LP_CIN[4], p.h[4], p.w[4], LP_CH[4], st);
}

}  // namespace

bool dc_lpips_geometry(int M, int pairs, int H, int W, dc_lpips_geom* g)
{
    lp_plan p;
    if (!make_lp_plan(M, pairs, H, W, p)) return false;
    for (int l = 0; l < LP_LAYERS; ++l) g->h[l] = p.h[l], g->w[l] = p.w[l], g->feat_off[l] = p.feat_off[l];
    g->total = p.total;
    return true;
}

extern "C" int dc_lpips_weight_floats(void) { return (int)lp_weight_layout().total; }

extern "C" long long dc_lpips_ws_bytes(int N, int H, int W)
{
    lp_plan p;
    return N > 0 && N <= 32767 && make_lp_plan(2 * N, N, H, W, p) ? p.total : -1;
}

extern "C" long long dc_lpips_features_ws_bytes(int N, int H, int W)
{
    lp_plan p;
    return make_lp_plan(N, 0, H, W, p) ? p.total - p.pool_off[0] : -1;
}

extern "C" int dc_lpips_alex(const void* x, const void* y, int x_u8, const long long* strides, int N, int H, int W, int normalize,
                             int normfix, const float* weights, void* ws, double* out, void* stream)
{
    lp_plan p;
    if (!x || !y || !strides || !weights || !ws || !out || N <= 0 || N > 32767 || !make_lp_plan(2 * N, N, H, W, p)) return DC_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    float* f[LP_LAYERS];
    for (int l = 0; l < LP_LAYERS; ++l) f[l] = (float*)(base + p.feat_off[l]);
    float* pool[2] = {(float*)(base + p.pool_off[0]), (float*)(base + p.pool_off[1])};
    const dc_strides4 sx(strides), sy(strides + 4);
    run_features(x, y, x_u8, sx, sy, N, 2 * N, H, W, normalize, weights, p, f, pool, st);
    const lp_weights o = lp_weight_layout();
    double* part = (double*)(base + p.part_off);
    for (int l = 0; l < LP_LAYERS; ++l)
        hipLaunchKernelGGL(lpips_tail_kernel, dim3(p.seg.count[l], N), dim3(256), 0, st, (const float*)f[l], N, LP_CH[l],
                           p.h[l] * p.w[l], weights + o.lin[l], normfix, part + p.seg.off[l]);
    hipLaunchKernelGGL(lpips_finalize_kernel, dim3(N), dim3(64), 0, st, (const double*)part, p.seg, N, out);
    return dc_launch_status();
}

extern "C" int dc_lpips_alex_features(const void* x, int x_u8, const long long* strides, int N, int H, int W, int normalize,
                                      const float* weights, void* ws, float* f1, float* f2, float* f3, float* f4, float* f5, void* stream)
{
    lp_plan p;
    if (!x || !strides || !weights || !ws || !f1 || !f2 || !f3 || !f4 || !f5 || !make_lp_plan(N, 0, H, W, p)) return DC_ERR_INVALID;
    float* f[LP_LAYERS] = {f1, f2, f3, f4, f5};
    float* pool[2] = {(float*)ws, (float*)((char*)ws + (p.pool_off[1] - p.pool_off[0]))};   // this entry's scratch: the pooled maps only
    const dc_strides4 sx(strides);
    run_features(x, x, x_u8, sx, sx, N, N, H, W, normalize, weights, p, f, pool, (hipStream_t)stream);
    return dc_launch_status();
}

extern "C" int dc_lpips_conv(int layer, const void* x, int x_u8, const long long* strides, int M, int H, int W, int normalize,
                             const float* weights, float* y, void* stream)
{
    if (!x || !weights || !y || layer < 0 || layer >= LP_LAYERS || M <= 0 || M > 65535 || H <= 0 || W <= 0 || H > 16384 || W > 16384)
        return DC_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const lp_weights o = lp_weight_layout();
    const float *w = weights + o.w[layer], *b = weights + o.b[layer];
    if (layer == 0) {
        lp_plan p;
        if (!strides || !make_lp_plan(M, 0, H, W, p)) return DC_ERR_INVALID;
        const dc_strides4 sx(strides);
        if (x_u8)
            launch_conv1<uint8_t>(x, x, sx, sx, M, M, w, b, y, H, W, p.h[0], p.w[0], normalize, st);
        else
            launch_conv1<float>(x, x, sx, sx, M, M, w, b, y, H, W, p.h[0], p.w[0], normalize, st);
    } else if (H > 4096 || W > 4096) {
        return DC_ERR_INVALID;
    } else if (layer == 1) {
        launch_conv<5, 4>((const float*)x, w, b, y, M, LP_CIN[1], H, W, LP_CH[1], st);
    } else {
        launch_conv<3, 8>((const float*)x, w, b, y, M, LP_CIN[layer], H, W, LP_CH[layer], st);
    }
    return dc_launch_status();
}
