// Image-quality metrics of a decoded frame against its ground truth (validation.py:120-155, test_utils.py:23-55): PSNR and
// SSIM / MS-SSIM with the semantics of pytorch_msssim 1.0 (restated in metrics.py), for gfx950.
//
// Operands are logical [N][C][H][W] images with arbitrary element strides, uint8 (converted to fp32 on load) or fp32, so that an
// NHWC uint8 frame or a permuted fp32 view is read in place.  Every sum runs in a fixed order and no float atomics are used:
// the results are bitwise identical from run to run.  Launches only enqueue on the caller's stream (graph-capturable); scratch
// comes from the caller, sized by dc_ssim_ws_bytes / dc_psnr_ws_bytes.
//
// SSIM, per scale, one fused launch: a 64 x 32 output tile of one (n, c) plane and its (ws - 1) halo are staged in LDS as fp32,
// each lane runs the separable window over the five products (x, y, x^2, y^2, xy) for one column and 8 output rows (horizontal
// pass from LDS, vertical pass in registers), forms ssim_map / cs_map per pixel and the workgroup writes one fp64 (sum ssim, sum
// cs) partial.  Values are shifted by -L/2 on load: sigma = E[x'^2] - mean'^2 is shift-invariant, and the smaller magnitudes cut
// the cancellation error of the fp32 second moments (the luminance term adds the shift back).  Between scales a separate launch
// applies avg_pool2d(2, padding = (H % 2, W % 2), count_include_pad) into fp32 planes.  A reduce launch sums each (scale, n, c)
// slab in fp64 in a fixed order; the finalize launch applies relu, the weight powers, the product and the means.
#include "dc_common.h"
#include "../../include/diffcodec_hip.h"

namespace {

constexpr int MT_TW = 64;                 // output columns per workgroup: one per lane
constexpr int MT_TH = 32;                 // output rows per workgroup: MT_R per wave, 4 waves
constexpr int MT_R = MT_TH / 4;
constexpr int MT_MAX_WS = 15;
constexpr int MT_MAX_LEVELS = 8;
constexpr int MT_PSNR_BLOCKS = 64;        // SSE partials per image (= one wave in the finalize)

struct img_strides {
    long long n, c, h, w;
};
struct ssim_consts {
    float g[MT_MAX_WS];
    float c1, c2, shift;
};

template <typename T>
__device__ __forceinline__ float mt_load(const T* __restrict__ p, long long i) { return (float)p[i]; }

__device__ __forceinline__ double2 mt_block_sum2(double a, double b, double2* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wv] = double2{a, b};
    __syncthreads();
    double2 s = red[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) {
        s.x += red[i].x;
        s.y += red[i].y;
    }
    return s;                                // valid in every thread, the same sequence of additions in each
}

template <typename T, int WS>
__global__ __launch_bounds__(256) void ssim_scale_kernel(const T* __restrict__ x, const T* __restrict__ y, img_strides sx,
                                                         img_strides sy, int C, int H, int W, int tiles_x, ssim_consts k,
                                                         double2* __restrict__ part)
{
#pragma clang fp contract(off)
    constexpr int LW = MT_TW + WS - 1, LH = MT_TH + WS - 1;
    __shared__ float lx[LH * LW], ly[LH * LW];
    __shared__ double2 red[4];
    const int nc = blockIdx.y, n = nc / C, c = nc - n * C;
    const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int ox0 = tx * MT_TW, oy0 = ty * MT_TH;
    const T* xb = x + n * sx.n + c * sx.c;
    const T* yb = y + n * sy.n + c * sy.c;
    for (int i = threadIdx.x; i < LH * LW; i += 256) {
        const int r = i / LW, q = i - r * LW, gy = oy0 + r, gx = ox0 + q;
        float a = 0.f, b = 0.f;
        if (gy < H && gx < W) {
            a = mt_load(xb, gy * sx.h + gx * sx.w) - k.shift;
            b = mt_load(yb, gy * sy.h + gx * sy.w) - k.shift;
        }
        lx[i] = a;
        ly[i] = b;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float acc[MT_R][5];
#pragma unroll
    for (int r = 0; r < MT_R; ++r)
#pragma unroll
        for (int p = 0; p < 5; ++p) acc[r][p] = 0.f;
#pragma unroll
    for (int i = 0; i < MT_R + WS - 1; ++i) {                 // input rows of this lane's 8 output rows
        const float* rx = lx + (wv * MT_R + i) * LW + lane;
        const float* ry = ly + (wv * MT_R + i) * LW + lane;
        float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f, h4 = 0.f;
#pragma unroll
        for (int j = 0; j < WS; ++j) {                         // horizontal pass, taps in index order
            const float a = rx[j], b = ry[j], g = k.g[j];
            h0 = __builtin_fmaf(g, a, h0);
            h1 = __builtin_fmaf(g, b, h1);
            h2 = __builtin_fmaf(g, a * a, h2);
            h3 = __builtin_fmaf(g, b * b, h3);
            h4 = __builtin_fmaf(g, a * b, h4);
        }
#pragma unroll
        for (int r = 0; r < MT_R; ++r) {                       // vertical pass: output row r takes input rows r .. r + WS - 1 in order
            const int t = i - r;
            if (t >= 0 && t < WS) {
                const float g = k.g[t];
                acc[r][0] = __builtin_fmaf(g, h0, acc[r][0]);
                acc[r][1] = __builtin_fmaf(g, h1, acc[r][1]);
                acc[r][2] = __builtin_fmaf(g, h2, acc[r][2]);
                acc[r][3] = __builtin_fmaf(g, h3, acc[r][3]);
                acc[r][4] = __builtin_fmaf(g, h4, acc[r][4]);
            }
        }
    }

    const int Ho = H - WS + 1, Wo = W - WS + 1, ox = ox0 + lane;
    double s_ssim = 0.0, s_cs = 0.0;
#pragma unroll
    for (int r = 0; r < MT_R; ++r) {
        const int oy = oy0 + wv * MT_R + r;
        if (oy < Ho && ox < Wo) {
            const float mx = acc[r][0], my = acc[r][1];
            const float sxx = __builtin_fmaf(-mx, mx, acc[r][2]);
            const float syy = __builtin_fmaf(-my, my, acc[r][3]);
            const float sxy = __builtin_fmaf(-mx, my, acc[r][4]);
            const float ux = mx + k.shift, uy = my + k.shift;
            const float cs = (2.f * sxy + k.c2) / ((sxx + syy) + k.c2);
            const float lum = (2.f * (ux * uy) + k.c1) / ((ux * ux + uy * uy) + k.c1);
            s_ssim += (double)(lum * cs);
            s_cs += (double)cs;
        }
    }
    const double2 s = mt_block_sum2(s_ssim, s_cs, red);
    if (threadIdx.x == 0) part[(long long)nc * gridDim.x + tile] = s;
}

// avg_pool2d(kernel 2, stride 2, padding (H % 2, W % 2), count_include_pad): output (i, j) covers input rows 2i - ph, 2i - ph + 1
// and columns 2j - pw, 2j - pw + 1; pad positions count as zero, the sum is divided by 4.  Output: contiguous fp32 [N*C][Ho][Wo].
template <typename T>
__global__ __launch_bounds__(256) void ssim_pool_kernel(const T* __restrict__ x, const T* __restrict__ y, img_strides sx,
                                                        img_strides sy, int C, int H, int W, float* __restrict__ px,
                                                        float* __restrict__ py, int Ho, int Wo, long long total)
{
#pragma clang fp contract(off)
    const int ph = H & 1, pw = W & 1;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int j = (int)(i % Wo);
        const long long t = i / Wo;
        const int r = (int)(t % Ho);
        const int nc = (int)(t / Ho), n = nc / C, c = nc - n * C;
        const T* xb = x + n * sx.n + c * sx.c;
        const T* yb = y + n * sy.n + c * sy.c;
        float vx[4], vy[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int yy = 2 * r - ph + (q >> 1), xx = 2 * j - pw + (q & 1);
            const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
            vx[q] = in ? mt_load(xb, yy * sx.h + xx * sx.w) : 0.f;
            vy[q] = in ? mt_load(yb, yy * sy.h + xx * sy.w) : 0.f;
        }
        px[i] = ((vx[0] + vx[1]) + (vx[2] + vx[3])) * 0.25f;
        py[i] = ((vy[0] + vy[1]) + (vy[2] + vy[3])) * 0.25f;
    }
}

struct ssim_segments {
    long long off[MT_MAX_LEVELS];            // first partial of scale s (double2 units)
    int count[MT_MAX_LEVELS];                // partials per (n, c) plane at scale s
    long long area[MT_MAX_LEVELS];           // ssim_map pixels per plane at scale s
};

// One workgroup per (plane, scale): thread t sums partials t, t + 256, ... in order, then a fixed-order block sum; writes the
// spatial means (ssim, cs) of the plane.
__global__ __launch_bounds__(256) void ssim_reduce_kernel(const double2* __restrict__ part, ssim_segments seg, int NC,
                                                          double2* __restrict__ means)
{
    __shared__ double2 red[4];
    const int nc = blockIdx.x, s = blockIdx.y, cnt = seg.count[s];
    const double2* src = part + seg.off[s] + (long long)nc * cnt;
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const double2 v = src[i];
        a += v.x;
        b += v.y;
    }
    const double2 t = mt_block_sum2(a, b, red);
    if (threadIdx.x == 0) means[(long long)s * NC + nc] = double2{t.x / (double)seg.area[s], t.y / (double)seg.area[s]};
}

struct ssim_final {
    float w[MT_MAX_LEVELS];
    int levels;
    int mode;                                // 0 = MS-SSIM, 1 = SSIM, 2 = SSIM with relu (nonnegative_ssim)
};

// out[nc] = per-(n, c) value, out[NC + n] = mean over c, out[NC + N] = mean over (n, c).  One workgroup.  relu is written
// v < 0 ? 0 : v, as torch.relu behaves: a NaN mean (a NaN pixel) stays NaN (fmax would turn it into 0) and reaches every mean
// it belongs to.
__global__ __launch_bounds__(256) void ssim_finalize_kernel(const double2* __restrict__ means, int N, int C, ssim_final f,
                                                            double* __restrict__ out)
{
    const int NC = N * C;
    for (int nc = threadIdx.x; nc < NC; nc += blockDim.x) {
        double v;
        if (f.mode == 0) {
            v = 1.0;
            for (int s = 0; s < f.levels; ++s) {
                const double2 m = means[(long long)s * NC + nc];
                const double b = s < f.levels - 1 ? m.y : m.x;                      // relu(cs) below the last scale, relu(ssim) at it
                v *= pow(b < 0.0 ? 0.0 : b, (double)f.w[s]);
            }
        } else {
            v = means[nc].x;
            if (f.mode == 2) v = v < 0.0 ? 0.0 : v;
        }
        out[nc] = v;
    }
    __syncthreads();
    __shared__ double rows[256];
    double total = 0.0;                                              // thread 0: sum over n of the per-n sums, in n order
    for (int n0 = 0; n0 < N; n0 += 256) {
        const int n = n0 + threadIdx.x;
        if (n < N) {
            double s = 0.0;
            for (int c = 0; c < C; ++c) s += out[n * C + c];
            out[NC + n] = s / (double)C;
            rows[threadIdx.x] = s;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < min(256, N - n0); ++i) total += rows[i];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[NC + N] = total / (double)NC;
}

// Per-image sum of squared differences: uint8 exactly in 64-bit integers, fp32 in fp64.  Workgroup b of image n takes the
// (c, h) rows b, b + MT_PSNR_BLOCKS, ...; one partial per workgroup.
template <typename T, typename Acc>
__global__ __launch_bounds__(256) void psnr_sse_kernel(const T* __restrict__ x, const T* __restrict__ y, img_strides sx,
                                                       img_strides sy, int C, int H, int W, Acc* __restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ Acc red[4];
    const int n = blockIdx.y, rows = C * H;
    const T* xb = x + n * sx.n;
    const T* yb = y + n * sy.n;
    Acc s = 0;
    for (int r = blockIdx.x; r < rows; r += MT_PSNR_BLOCKS) {
        const int c = r / H, h = r - c * H;
        const T* xr = xb + c * sx.c + h * sx.h;
        const T* yr = yb + c * sy.c + h * sy.h;
        for (int w = threadIdx.x; w < W; w += 256) {
            if constexpr (sizeof(T) == 1) {
                const int d = (int)xr[w * sx.w] - (int)yr[w * sy.w];
                s += (Acc)(d * d);
            } else {
                const double d = (double)xr[w * sx.w] - (double)yr[w * sy.w];
                s += d * d;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[(long long)n * MT_PSNR_BLOCKS + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// One wave per image: lane l takes partial l, a fixed butterfly sums them; out[n] = 10 log10(L^2 / mse), +inf when mse == 0.
template <typename Acc>
__global__ __launch_bounds__(64) void psnr_finalize_kernel(const Acc* __restrict__ part, double count, double peak2,
                                                           double* __restrict__ out)
{
    const int n = blockIdx.x;
    Acc s = part[(long long)n * MT_PSNR_BLOCKS + threadIdx.x];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) {
        const double mse = (double)s / count;
        out[n] = mse == 0.0 ? __builtin_huge_val() : 10.0 * log10(peak2 / mse);
    }
}

inline int mt_grid(long long total) { return (int)min((long long)8192, (total + 255) / 256); }
inline long long mt_align(long long b) { return (b + 255) & ~255ll; }

// Workspace of one SSIM / MS-SSIM call: pooled X / Y planes of scales 1 .. levels-1, the per-workgroup partials of every scale,
// the per-(scale, plane) means.
struct ssim_plan {
    int levels, h[MT_MAX_LEVELS], w[MT_MAX_LEVELS], tiles_x[MT_MAX_LEVELS], tiles[MT_MAX_LEVELS];
    long long plane_off[MT_MAX_LEVELS];      // bytes: X planes, Y planes follow at + plane_bytes
    long long plane_bytes[MT_MAX_LEVELS];
    long long part_off;                      // bytes
    ssim_segments seg;
    long long means_off, total;
};

bool make_ssim_plan(int N, int C, int H, int W, int ws, int levels, ssim_plan& p)
{
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || ws < 1 || ws > MT_MAX_WS || !(ws & 1) || levels < 1 || levels > MT_MAX_LEVELS ||
        (long long)N * C > 65535)
        return false;
    const long long NC = (long long)N * C;
    p.levels = levels;
    long long off = 0, parts = 0;
    for (int s = 0; s < levels; ++s) {
        p.h[s] = s == 0 ? H : (p.h[s - 1] + (p.h[s - 1] & 1)) / 2;
        p.w[s] = s == 0 ? W : (p.w[s - 1] + (p.w[s - 1] & 1)) / 2;
        if (p.h[s] < ws || p.w[s] < ws) return false;
        const int ho = p.h[s] - ws + 1, wo = p.w[s] - ws + 1;
        p.tiles_x[s] = (wo + MT_TW - 1) / MT_TW;
        p.tiles[s] = p.tiles_x[s] * ((ho + MT_TH - 1) / MT_TH);
        p.seg.off[s] = parts;
        p.seg.count[s] = p.tiles[s];
        p.seg.area[s] = (long long)ho * wo;
        parts += NC * p.tiles[s];
        p.plane_bytes[s] = s == 0 ? 0 : mt_align(NC * p.h[s] * p.w[s] * 4);
        p.plane_off[s] = off;
        off += 2 * p.plane_bytes[s];
    }
    p.part_off = off;
    off += mt_align(parts * 16);
    p.means_off = off;
    off += mt_align(NC * levels * 16);
    p.total = off;
    return true;
}

template <typename T, int WS>
void launch_scale(const void* x, const void* y, img_strides sx, img_strides sy, int N, int C, int H, int W, int tiles_x, int tiles,
                  const ssim_consts& k, double2* part, hipStream_t st)
{
    hipLaunchKernelGGL((ssim_scale_kernel<T, WS>), dim3(tiles, N * C), dim3(256), 0, st, (const T*)x, (const T*)y, sx, sy, C, H, W,
                       tiles_x, k, part);
}

template <typename T>
void launch_scale_ws(int ws, const void* x, const void* y, img_strides sx, img_strides sy, int N, int C, int H, int W, int tiles_x,
                     int tiles, const ssim_consts& k, double2* part, hipStream_t st)
{
#define MT_WS_CASE(V) \
    case V: launch_scale<T, V>(x, y, sx, sy, N, C, H, W, tiles_x, tiles, k, part, st); break;
    switch (ws) {
        MT_WS_CASE(1) MT_WS_CASE(3) MT_WS_CASE(5) MT_WS_CASE(7) MT_WS_CASE(9) MT_WS_CASE(11) MT_WS_CASE(13) MT_WS_CASE(15)
    }
#undef MT_WS_CASE
}

int run_ssim(const void* x, const void* y, int x_u8, const long long* strides, int N, int C, int H, int W, const float* win,
             int win_size, const float* weights, int levels, float K1, float K2, float data_range, int mode, void* ws, double* out,
             void* stream)
{
    ssim_plan p;
    if (!x || !y || !strides || !win || !ws || !out || (mode == 0 && !weights) || !make_ssim_plan(N, C, H, W, win_size, levels, p))
        return DC_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    ssim_consts k;
    for (int i = 0; i < MT_MAX_WS; ++i) k.g[i] = i < win_size ? win[i] : 0.f;
    const double c1 = (double)K1 * data_range, c2 = (double)K2 * data_range;
    k.c1 = (float)(c1 * c1);
    k.c2 = (float)(c2 * c2);
    k.shift = 0.5f * data_range;
    char* base = (char*)ws;
    double2* part = (double2*)(base + p.part_off);
    img_strides sx{strides[0], strides[1], strides[2], strides[3]}, sy{strides[4], strides[5], strides[6], strides[7]};
    const void *cx = x, *cy = y;
    int u8 = x_u8;
    for (int s = 0; s < levels; ++s) {
        if (s > 0) {                                              // pool scale s - 1 into the contiguous fp32 planes of scale s
            float* px = (float*)(base + p.plane_off[s]);
            float* py = (float*)(base + p.plane_off[s] + p.plane_bytes[s]);
            const long long total = (long long)N * C * p.h[s] * p.w[s];
            if (u8)
                hipLaunchKernelGGL(ssim_pool_kernel<uint8_t>, dim3(mt_grid(total)), dim3(256), 0, st, (const uint8_t*)cx,
                                   (const uint8_t*)cy, sx, sy, C, p.h[s - 1], p.w[s - 1], px, py, p.h[s], p.w[s], total);
            else
                hipLaunchKernelGGL(ssim_pool_kernel<float>, dim3(mt_grid(total)), dim3(256), 0, st, (const float*)cx,
                                   (const float*)cy, sx, sy, C, p.h[s - 1], p.w[s - 1], px, py, p.h[s], p.w[s], total);
            cx = px;
            cy = py;
            u8 = 0;
            const long long hw = (long long)p.h[s] * p.w[s];
            sx = sy = img_strides{C * hw, hw, p.w[s], 1};
        }
        if (u8)
            launch_scale_ws<uint8_t>(win_size, cx, cy, sx, sy, N, C, p.h[s], p.w[s], p.tiles_x[s], p.tiles[s], k, part + p.seg.off[s], st);
        else
            launch_scale_ws<float>(win_size, cx, cy, sx, sy, N, C, p.h[s], p.w[s], p.tiles_x[s], p.tiles[s], k, part + p.seg.off[s], st);
    }
    double2* means = (double2*)(base + p.means_off);
    hipLaunchKernelGGL(ssim_reduce_kernel, dim3(N * C, levels), dim3(256), 0, st, (const double2*)part, p.seg, N * C, means);
    ssim_final f;
    for (int s = 0; s < MT_MAX_LEVELS; ++s) f.w[s] = (mode == 0 && s < levels) ? weights[s] : 0.f;
    f.levels = levels;
    f.mode = mode;
    hipLaunchKernelGGL(ssim_finalize_kernel, dim3(1), dim3(256), 0, st, (const double2*)means, N, C, f, out);
    return dc_launch_status();
}

}  // namespace

extern "C" long long dc_ssim_ws_bytes(int N, int C, int H, int W, int win_size, int levels)
{
    ssim_plan p;
    return make_ssim_plan(N, C, H, W, win_size, levels, p) ? p.total : -1;
}

extern "C" int dc_ms_ssim(const void* x, const void* y, int x_u8, const long long* strides, int N, int C, int H, int W,
                          const float* win, int win_size, const float* weights, int levels, float K1, float K2, float data_range,
                          void* ws, double* out, void* stream)
{
    return run_ssim(x, y, x_u8, strides, N, C, H, W, win, win_size, weights, levels, K1, K2, data_range, 0, ws, out, stream);
}

extern "C" int dc_ssim(const void* x, const void* y, int x_u8, const long long* strides, int N, int C, int H, int W, const float* win,
                       int win_size, float K1, float K2, float data_range, int nonnegative, void* ws, double* out, void* stream)
{
    return run_ssim(x, y, x_u8, strides, N, C, H, W, win, win_size, nullptr, 1, K1, K2, data_range, nonnegative ? 2 : 1, ws, out,
                    stream);
}

extern "C" long long dc_psnr_ws_bytes(int N) { return N > 0 && N <= 65535 ? (long long)N * MT_PSNR_BLOCKS * 8 : -1; }

extern "C" int dc_psnr(const void* x, const void* y, int x_u8, const long long* strides, int N, int C, int H, int W,
                       double data_range, void* ws, double* out, void* stream)
{
    if (!x || !y || !strides || !ws || !out || N <= 0 || N > 65535 || C <= 0 || H <= 0 || W <= 0) return DC_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const img_strides sx{strides[0], strides[1], strides[2], strides[3]}, sy{strides[4], strides[5], strides[6], strides[7]};
    const double count = (double)C * H * W, peak2 = data_range * data_range;
    if (x_u8) {
        auto* part = (unsigned long long*)ws;
        hipLaunchKernelGGL((psnr_sse_kernel<uint8_t, unsigned long long>), dim3(MT_PSNR_BLOCKS, N), dim3(256), 0, st,
                           (const uint8_t*)x, (const uint8_t*)y, sx, sy, C, H, W, part);
        hipLaunchKernelGGL(psnr_finalize_kernel<unsigned long long>, dim3(N), dim3(64), 0, st, (const unsigned long long*)part, count,
                           peak2, out);
    } else {
        auto* part = (double*)ws;
        hipLaunchKernelGGL((psnr_sse_kernel<float, double>), dim3(MT_PSNR_BLOCKS, N), dim3(256), 0, st, (const float*)x,
                           (const float*)y, sx, sy, C, H, W, part);
        hipLaunchKernelGGL(psnr_finalize_kernel<double>, dim3(N), dim3(64), 0, st, (const double*)part, count, peak2, out);
    }
    return dc_launch_status();
}
