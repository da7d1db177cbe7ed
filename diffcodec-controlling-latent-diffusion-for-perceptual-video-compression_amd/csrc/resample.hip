// Pillow's 8-bit antialiased resize (Resample.c: BILINEAR, BICUBIC, LANCZOS) on the device, bit for bit.
//
// The arithmetic is integer once the coefficient table exists: the host builds, per axis, int32 coefficients K [out][ksize]
// (float64 filter values, normalised, scaled by 2^22 and rounded half away from zero) and int32 bounds [out][2] = (first input
// sample, tap count), and one output sample is clip(((1 << 21) + sum_x K[x] * in[xmin + x]) >> 22, 0, 255) in int32.  Pillow runs a
// horizontal pass (when the widths differ) into a uint8 image and then a vertical pass (when the heights differ) on it; so does
// this file: two launches, the uint8 intermediate [N, H_in, W_out, C] in caller-provided scratch, rounded and clipped to a byte
// exactly like the final image.  A pass whose sizes agree is skipped, not run with identity taps.
//
// One lane owns one output pixel (all C channels) and walks that pixel's own tap count: no compile-time tap limit (a 200 -> 3
// Lanczos pass has about 400 taps, the 1920 -> 512 bilinear one 8 or 9).  Horizontal pass: neighbouring lanes read neighbouring tap
// windows of one input row (windows overlap or abut, so a wave's loads fall in a few cache lines) and each lane its own table row.
// Vertical pass: bounds and coefficients are uniform over the workgroup (scalar loads) and the lanes read C consecutive bytes each
// of one row per tap.  The first pass reads the operand through element strides (a cropped window of a frame is resized in place).
// Both tap windows are clamped to the table's ksize and to the input extent in the kernel, so a wrong table cannot make it read
// outside the operand.
#include "dc_common.h"
#include "../../include/diffcodec_hip.h"

#include <math.h>

namespace {

constexpr int RS_SPAN = 256;              // output pixels of one row per workgroup: one per lane, 4 waves
constexpr int RS_PRECISION_BITS = 22;     // Pillow's PRECISION_BITS = 32 - 8 - 2

struct rs_strides {
    long long n, c, h, w;                 // element strides, in dc_psnr's order
};

__host__ __device__ __forceinline__ uint8_t rs_clip8(int acc)
{
    const int v = acc >> RS_PRECISION_BITS;                          // arithmetic shift
    return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// One output pixel (all C channels) of one pass.  VERT = false: filters along W (in_size = W_in, out rows = H);  VERT = true: filters
// along H (in_size = H_in, out columns = W).  `row` = n * out_h + y;  out is contiguous [N, out_h, out_w, C].
template <int C, bool VERT>
__host__ __device__ __forceinline__ void rs_pixel(int row, int x, const uint8_t* __restrict__ in, rs_strides s, int in_size, int out_h,
                                                  int out_w, const int* __restrict__ K, const int* __restrict__ bounds, int ksize,
                                                  uint8_t* __restrict__ out)
{
    const int n = row / out_h, y = row - n * out_h;
    const int o = VERT ? y : x;                                      // the output index along the filtered axis
    int first = bounds[2LL * o], taps = bounds[2LL * o + 1];
    first = first < 0 ? 0 : first > in_size ? in_size : first;
    const int room = in_size - first < ksize ? in_size - first : ksize;
    taps = taps < 0 ? 0 : taps > room ? room : taps;
    const int* __restrict__ k = K + (long long)o * ksize;
    const long long step = VERT ? s.h : s.w;
    const uint8_t* __restrict__ p = in + (long long)n * s.n + (VERT ? (long long)x * s.w : (long long)y * s.h) + (long long)first * step;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (RS_PRECISION_BITS - 1);
    for (int t = 0; t < taps; ++t) {
        const int kv = k[t];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += kv * (int)p[c * s.c];
        p += step;
    }
    uint8_t* __restrict__ q = out + ((long long)row * out_w + x) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) q[c] = rs_clip8(acc[c]);
}

// grid = (N * out_h, ceil(out_w / RS_SPAN)): one lane per output pixel of one row
template <int C, bool VERT>
__global__ __launch_bounds__(RS_SPAN) void resample_pass_kernel(const uint8_t* __restrict__ in, rs_strides s, int in_size, int out_h,
                                                                 int out_w, const int* __restrict__ K, const int* __restrict__ bounds,
                                                                 int ksize, uint8_t* __restrict__ out)
{
    const int x = blockIdx.y * RS_SPAN + threadIdx.x;
    if (x < out_w) rs_pixel<C, VERT>(blockIdx.x, x, in, s, in_size, out_h, out_w, K, bounds, ksize, out);
}

template <bool VERT>
void rs_launch(int C, dim3 grid, hipStream_t st, const uint8_t* in, rs_strides s, int in_size, int out_h, int out_w, const int* K,
               const int* bounds, int ksize, uint8_t* out)
{
    switch (C) {
    case 1: hipLaunchKernelGGL((resample_pass_kernel<1, VERT>), grid, dim3(RS_SPAN), 0, st, in, s, in_size, out_h, out_w, K, bounds, ksize, out); break;
    case 2: hipLaunchKernelGGL((resample_pass_kernel<2, VERT>), grid, dim3(RS_SPAN), 0, st, in, s, in_size, out_h, out_w, K, bounds, ksize, out); break;
    case 3: hipLaunchKernelGGL((resample_pass_kernel<3, VERT>), grid, dim3(RS_SPAN), 0, st, in, s, in_size, out_h, out_w, K, bounds, ksize, out); break;
    default: hipLaunchKernelGGL((resample_pass_kernel<4, VERT>), grid, dim3(RS_SPAN), 0, st, in, s, in_size, out_h, out_w, K, bounds, ksize, out); break;
    }
}

// ksize of one axis is ceil(support * max(in / out, 1)) * 2 + 1 with support 1, 2 or 3 (bilinear, bicubic, Lanczos): a table built
// for other sizes (or another filter family) does not have one of these three row lengths.
bool rs_ksize_ok(int in_size, int out_size, int ksize)
{
    const double scale = (double)in_size / out_size, fs = scale < 1.0 ? 1.0 : scale;
    for (int support = 1; support <= 3; ++support)
        if (ksize == (int)ceil(support * fs) * 2 + 1) return true;
    return false;
}

bool rs_grid_ok(long long rows, int out_w) { return rows <= 0x7fffffffLL && dc_cdiv(out_w, RS_SPAN) <= 65535; }

}  // namespace

extern "C" long long dc_resample_ws_bytes(int N, int H_in, int W_out, int C)
{
    if (N < 1 || H_in < 1 || W_out < 1 || C < 1 || C > 4) return -1;
    return (long long)N * H_in * W_out * C;
}

extern "C" int dc_resample_u8(const void* in, const long long* strides, int N, int H_in, int W_in, int C, int H_out, int W_out,
                              const int* k_h, const int* bounds_h, int ksize_h, const int* k_v, const int* bounds_v, int ksize_v,
                              void* scratch, void* out, void* stream)
{
    if (!in || !strides || !out || N < 1 || H_in < 1 || W_in < 1 || H_out < 1 || W_out < 1 || C < 1 || C > 4) return DC_ERR_INVALID;
    const bool horiz = W_out != W_in, vert = H_out != H_in;
    if (horiz != (k_h != nullptr) || horiz != (bounds_h != nullptr) || vert != (k_v != nullptr) || vert != (bounds_v != nullptr))
        return DC_ERR_INVALID;                                       // a null table means "sizes agree, pass skipped" and nothing else
    if (!horiz && !vert) return DC_ERR_INVALID;                      // nothing to resample: the caller copies
    if (horiz && !rs_ksize_ok(W_in, W_out, ksize_h)) return DC_ERR_INVALID;
    if (vert && !rs_ksize_ok(H_in, H_out, ksize_v)) return DC_ERR_INVALID;
    if (horiz && vert && !scratch) return DC_ERR_INVALID;
    if (!rs_grid_ok((long long)N * H_in, W_out) || !rs_grid_ok((long long)N * H_out, W_out)) return DC_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const rs_strides s{strides[0], strides[1], strides[2], strides[3]};
    const uint8_t* src = (const uint8_t*)in;
    rs_strides ss = s;
    if (horiz) {
        uint8_t* dst = (uint8_t*)(vert ? scratch : out);
        rs_launch<false>(C, dim3(N * H_in, dc_cdiv(W_out, RS_SPAN)), st, src, s, W_in, H_in, W_out, k_h, bounds_h, ksize_h, dst);
        src = dst;
        ss = rs_strides{(long long)H_in * W_out * C, 1, (long long)W_out * C, C};
    }
    if (vert)
        rs_launch<true>(C, dim3(N * H_out, dc_cdiv(W_out, RS_SPAN)), st, src, ss, H_in, H_out, W_out, k_v, bounds_v, ksize_v, (uint8_t*)out);
    return dc_launch_status();
}
