// Guide points for the CMP network: the 'watershed' strategy of the reference's flow_sampler (cmp/utils/data_utils.py: get_edge,
// distance_transform_edt, nms, remove_border, neighbor_elim) on the device, alone or united with its 'grid' strategy.  C ABI:
// include/diffcodec_guide_hip.h.
//
//   1  edge      flow[:, :, ::ds, ::ds] -> Sobel magnitude (fp32, one fixed operation order), its per-image peak (per-block maxima,
//                then one block per image: a max has no order), mag / max(peak, 0.01) > 0.1 -> a byte map
//   2  edt       exact squared Euclidean distance in int32, separably: per column the distance to the nearest edge pixel of that
//                column (two scans), then per row min over x' of (x - x')^2 + g(x')^2 against the row staged in LDS
//   3  nms       d2 >= its maximum over the ks x ks window clipped to the image (row maximum from LDS, then column maximum),
//                0 < d2 < GP_INF, the one-pixel border removed
//   4  select    row counts -> row offsets -> the candidates in row-major order (ballot prefix, nothing appended atomically), then one
//                wave per image walks them: a candidate survives iff no earlier survivor lies within |dy| < d and |dx| < d
//   5  scatter   (u, v, 1, 1) at the grid points and at the survivors
//
// The walk.  Two survivors never share a d x d tile (inside one tile |dy| < d and |dx| < d), so the survivors are kept as one
// packed (y, x) per tile, and only the tile rows ty - 1 and ty can hold a survivor that blocks a candidate of tile row ty (earlier
// means y' <= y): two tile rows in LDS, indexed by ty & 1.  A slot left over from tile row ty - 2 or before is never cleared: its
// survivor is more than d rows up and fails the |dy| < d test by itself.  The wave takes 64 candidates at a time: every lane tests
// its candidate against the 2 x 3 tiles around it, the lanes still standing are then resolved in order in registers (the lowest
// survives and knocks out the later ones in its box), so the serial steps of a chunk are its survivors, not its candidates.
#include "dc_common.h"
#include "../../include/diffcodec_guide_hip.h"

namespace {

constexpr int GP_SIDE = 800;                 // a working image has fewer rows and fewer columns than this
constexpr int GP_INF = 1 << 29;              // d2 of an image without an edge pixel; GP_INF + 800^2 fits an int

__device__ __forceinline__ int gp_wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------------------------------------ 1: edge map
// mag [N][h][w]: sum over the two channels of sqrt(ex^2 + ey^2); partial [N][nblk]: the maximum of each block's 256 pixels
__global__ __launch_bounds__(256) void gp_mag_kernel(const float* __restrict__ fl, float* __restrict__ mag, float* __restrict__ partial,
                                                     int H, int W, int h, int w, int ds)
{
#pragma clang fp contract(off)
    __shared__ float red[4];
    const int n = blockIdx.y, P = h * w, i = blockIdx.x * 256 + threadIdx.x;
    const long long FP = (long long)H * W;
    float m = 0.f;
    if (i < P) {
        const int y = i / w, x = i % w;
        const long long r0 = (long long)(max(y - 1, 0) * ds) * W, r1 = (long long)(y * ds) * W, r2 = (long long)(min(y + 1, h - 1) * ds) * W;
        const int c0 = max(x - 1, 0) * ds, c1 = x * ds, c2 = min(x + 1, w - 1) * ds;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float* __restrict__ p = fl + ((long long)n * 2 + c) * FP;
            const float a00 = p[r0 + c0], a01 = p[r0 + c1], a02 = p[r0 + c2];
            const float a10 = p[r1 + c0], a12 = p[r1 + c2];
            const float a20 = p[r2 + c0], a21 = p[r2 + c1], a22 = p[r2 + c2];
            const float ex = ((a00 - a02) + 2.f * (a10 - a12)) + (a20 - a22);
            const float ey = ((a00 - a20) + 2.f * (a01 - a21)) + (a02 - a22);
            s += sqrtf(ex * ex + ey * ey);
        }
        mag[(long long)n * P + i] = s;
        m = s;
    }
    m = dc_wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) partial[(long long)n * gridDim.x + blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void gp_peak_kernel(const float* __restrict__ partial, float* __restrict__ peak, int nblk)
{
    __shared__ float red[4];
    float m = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 256) m = fmaxf(m, partial[(long long)blockIdx.x * nblk + i]);
    m = dc_wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) peak[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void gp_thresh_kernel(const float* __restrict__ mag, const float* __restrict__ peak, float* __restrict__ norm,
                                                        unsigned char* __restrict__ edge, int P)
{
    const int n = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const float v = mag[(long long)n * P + i] / fmaxf(peak[n], 0.01f);
    if (norm) norm[(long long)n * P + i] = v;
    edge[(long long)n * P + i] = v > 0.1f ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ 2: squared distance
// g [N][h][w]: rows to the nearest edge pixel of the same column, GP_SIDE where the column has none.  One thread per column.
__global__ __launch_bounds__(64) void gp_cols_kernel(const unsigned char* __restrict__ edge, int* __restrict__ g, int h, int w)
{
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= w) return;
    const long long base = (long long)blockIdx.y * h * w + x;
    int dist = GP_SIDE;
    for (int y = 0; y < h; ++y) {
        dist = edge[base + (long long)y * w] ? 0 : min(dist + 1, GP_SIDE);
        g[base + (long long)y * w] = dist;
    }
    dist = GP_SIDE;
    for (int y = h - 1; y >= 0; --y) {
        dist = edge[base + (long long)y * w] ? 0 : min(dist + 1, GP_SIDE);
        if (dist < g[base + (long long)y * w]) g[base + (long long)y * w] = dist;      // this thread's own store of the first scan
    }
}

// d2 [N][h][w] = min over x' of (x - x')^2 + g(y, x')^2; one block per row
__global__ __launch_bounds__(256) void gp_rows_kernel(const int* __restrict__ g, int* __restrict__ d2, int h, int w)
{
    __shared__ __attribute__((aligned(16))) int g2[GP_SIDE];
    const long long base = ((long long)blockIdx.y * h + blockIdx.x) * w;
    const int wp = (w + 3) & ~3;
    for (int x = threadIdx.x; x < wp; x += 256) {
        const int v = x < w ? g[base + x] : GP_SIDE;
        g2[x] = v >= GP_SIDE ? GP_INF : v * v;
    }
    __syncthreads();
    for (int x = threadIdx.x; x < w; x += 256) {
        int best = GP_INF;
        for (int q = 0; q < wp; q += 4) {
            const int4 v = *(const int4*)&g2[q];
            const int e = x - q;
            best = min(best, v.x + e * e);
            best = min(best, v.y + (e - 1) * (e - 1));
            best = min(best, v.z + (e - 2) * (e - 2));
            best = min(best, v.w + (e - 3) * (e - 3));
        }
        d2[base + x] = best;
    }
}

// ------------------------------------------------------------------------------------------------ 3: non-maximum suppression
__global__ __launch_bounds__(256) void gp_rowmax_kernel(const int* __restrict__ d2, int* __restrict__ rmax, int h, int w, int r)
{
    __shared__ int row[GP_SIDE];
    const long long base = ((long long)blockIdx.y * h + blockIdx.x) * w;
    for (int x = threadIdx.x; x < w; x += 256) row[x] = d2[base + x];
    __syncthreads();
    for (int x = threadIdx.x; x < w; x += 256) {
        const int lo = max(x - r, 0), hi = min(x + r, w - 1);
        int m = row[lo];
        for (int q = lo + 1; q <= hi; ++q) m = max(m, row[q]);
        rmax[base + x] = m;
    }
}

__global__ __launch_bounds__(256) void gp_colmax_kernel(const int* __restrict__ d2, const int* __restrict__ rmax, unsigned char* __restrict__ cand,
                                                        int h, int w, int r)
{
    const int P = h * w, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const long long base = (long long)blockIdx.y * P;
    const int y = i / w, x = i % w;
    const int lo = max(y - r, 0), hi = min(y + r, h - 1);
    int m = 0;
    for (int q = lo; q <= hi; ++q) m = max(m, rmax[base + q * w + x]);
    const int v = d2[base + i];
    const bool inner = y > 0 && y < h - 1 && x > 0 && x < w - 1;
    cand[base + i] = (inner && v > 0 && v < GP_INF && v >= m) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ 4: compaction and elimination
__global__ __launch_bounds__(64) void gp_rowcnt_kernel(const unsigned char* __restrict__ cand, int* __restrict__ rowcnt, int h, int w)
{
    const long long row = (long long)blockIdx.y * h + blockIdx.x;
    int c = 0;
    for (int x = threadIdx.x; x < w; x += 64) c += cand[row * w + x] ? 1 : 0;
    c = gp_wave_sum(c);
    if (threadIdx.x == 0) rowcnt[row] = c;
}

// list [N][h w]: the candidates of image n as (y << 16) | x in row-major order; ncand [N]
__global__ __launch_bounds__(64) void gp_compact_kernel(const unsigned char* __restrict__ cand, const int* __restrict__ rowcnt,
                                                        int* __restrict__ list, int* __restrict__ ncand, int h, int w)
{
    const int n = blockIdx.y, y = blockIdx.x, lane = threadIdx.x;
    int off = 0;
    for (int q = lane; q < y; q += 64) off += rowcnt[(long long)n * h + q];
    int run = gp_wave_sum(off);
    const long long row = ((long long)n * h + y) * w;
    int* __restrict__ out = list + (long long)n * h * w;
    for (int x0 = 0; x0 < w; x0 += 64) {
        const int x = x0 + lane;
        const bool c = x < w && cand[row + x] != 0;
        const unsigned long long b = __ballot(c);
        if (c) out[run + __popcll(b & ((1ull << lane) - 1ull))] = (y << 16) | x;
        run += __popcll(b);
    }
    if (y == h - 1 && lane == 0) ncand[n] = run;
}

// one wave per image; counts [N], points [N][cap][2] = (y, x) * scale of the survivors in order, then -1
__global__ __launch_bounds__(64) void gp_walk_kernel(const int* __restrict__ list, const int* __restrict__ ncand, int* __restrict__ counts,
                                                     int* __restrict__ points, int h, int w, int d, int scale, int cap)
{
    __shared__ int ring[2][GP_SIDE];
    const int n = blockIdx.x, lane = threadIdx.x;
    for (int i = lane; i < 2 * GP_SIDE; i += 64) (&ring[0][0])[i] = -1;
    __syncthreads();
    const int* __restrict__ in = list + (long long)n * h * w;
    int* __restrict__ pts = points + (long long)n * cap * 2;
    const int count = min(ncand[n], h * w), tw = (w + d - 1) / d;
    int nsurv = 0;
    for (int base = 0; base < count; base += 64) {
        const bool valid = base + lane < count;
        const int c = valid ? in[base + lane] : 0;
        const int y = c >> 16, x = c & 0xffff, ty = y / d, tx = x / d;
        bool blocked = !valid;
        if (valid) {
            for (int a = ty > 0 ? ty - 1 : ty; a <= ty; ++a)
                for (int b = max(tx - 1, 0); b <= min(tx + 1, tw - 1); ++b) {
                    const int e = ring[a & 1][b];
                    if (e >= 0 && abs(y - (e >> 16)) < d && abs(x - (e & 0xffff)) < d) blocked = true;
                }
        }
        unsigned long long mask = __ballot(!blocked);
        while (mask) {
            const int i = __builtin_ctzll(mask);
            const int cy = __shfl(y, i, 64), cx = __shfl(x, i, 64);
            if (lane == i) {
                ring[ty & 1][tx] = c;
                if (nsurv < cap) {
                    pts[2 * nsurv] = y * scale;
                    pts[2 * nsurv + 1] = x * scale;
                }
            }
            ++nsurv;
            if (lane > i && abs(y - cy) < d && abs(x - cx) < d) blocked = true;
            mask = __ballot(!blocked) & (i == 63 ? 0ull : ~0ull << (i + 1));
        }
        __syncthreads();
    }
    if (lane == 0) counts[n] = min(nsurv, cap);
    for (int k = min(nsurv, cap) + lane; k < cap; k += 64) pts[2 * k] = pts[2 * k + 1] = -1;
}

// ------------------------------------------------------------------------------------------------ 5: scatter
// the grid points (as dc_cmp_sparse_grid; none for stride 0) and zeros elsewhere
__global__ __launch_bounds__(256) void gp_grid_kernel(const float* __restrict__ fl, float* __restrict__ sp, int H, int W, int stride, int y0, int x0,
                                                      long long total)
{
    const long long P = (long long)H * W;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long p = i % P, n = i / P;
        const int yy = (int)(p / W), xx = (int)(p % W);
        const bool on = stride > 0 && yy >= y0 && xx >= x0 && (yy - y0) % stride == 0 && (xx - x0) % stride == 0;
        float* __restrict__ o = sp + n * 4 * P + p;
        o[0] = on ? fl[n * 2 * P + p] : 0.f;
        o[P] = on ? fl[(n * 2 + 1) * P + p] : 0.f;
        o[2 * P] = o[3 * P] = on ? 1.f : 0.f;
    }
}

// after gp_grid_kernel on the same stream; a point that is also a grid point gets the same four values again
__global__ __launch_bounds__(256) void gp_points_kernel(const float* __restrict__ fl, float* __restrict__ sp, const int* __restrict__ counts,
                                                        const int* __restrict__ points, int cap, int H, int W)
{
    const int n = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    if (k >= cap || k >= counts[n]) return;
    const int y = points[((long long)n * cap + k) * 2], x = points[((long long)n * cap + k) * 2 + 1];
    if (y < 0 || y >= H || x < 0 || x >= W) return;
    const long long P = (long long)H * W, p = (long long)y * W + x;
    float* __restrict__ o = sp + (long long)n * 4 * P + p;
    o[0] = fl[(long long)n * 2 * P + p];
    o[P] = fl[((long long)n * 2 + 1) * P + p];
    o[2 * P] = o[3 * P] = 1.f;
}

// ------------------------------------------------------------------------------------------------ host
inline bool gp_dim(long long v) { return v > 0 && v <= (1 << 24); }
inline bool gp_batch(int N) { return N > 0 && N <= 65535; }
inline bool gp_side(int v) { return v > 0 && v < GP_SIDE; }
inline bool gp_ks(int ks) { return ks >= 3 && (ks & 1) == 1; }
inline int gp_d(int ks) { return min((ks - 1) / 2, GP_SIDE); }         // beyond the image every window and every box is the same
inline int gp_ds(int H, int W) { return max(1, max(H, W) / 400); }
inline long long gp_up(long long v) { return (v + 255) / 256 * 256; }

struct gp_ws {
    float* mag;              // [N][P] fp32, stage 1; then `list`
    int* list;
    int* g;                  // [N][P] column distances, stage 2; then `rmax`, stage 3
    int* rmax;
    int* d2;                 // [N][P]
    unsigned char* edge;     // [N][P]
    unsigned char* cand;     // [N][P]
    int* rowcnt;             // [N][h]
    int* ncand;              // [N]
    float* partial;          // [N][nblk]
    float* peak;             // [N]
    long long bytes;
};

gp_ws gp_plan(void* ws, int N, int h, int w)
{
    const long long P = (long long)h * w, nblk = (P + 255) / 256;
    char* p = (char*)ws;
    long long at = 0;
    gp_ws s;
    s.mag = (float*)(p + at), s.list = (int*)(p + at), at += gp_up(4 * N * P);
    s.g = (int*)(p + at), s.rmax = (int*)(p + at), at += gp_up(4 * N * P);
    s.d2 = (int*)(p + at), at += gp_up(4 * N * P);
    s.edge = (unsigned char*)(p + at), at += gp_up(N * P);
    s.cand = (unsigned char*)(p + at), at += gp_up(N * P);
    s.rowcnt = (int*)(p + at), at += gp_up(4ll * N * h);
    s.ncand = (int*)(p + at), at += gp_up(4ll * N);
    s.partial = (float*)(p + at), at += gp_up(4 * N * nblk);
    s.peak = (float*)(p + at), at += gp_up(4ll * N);
    s.bytes = at;
    return s;
}

inline hipStream_t gp_st(void* stream) { return (hipStream_t)stream; }

void gp_edge(const float* flow, int N, int H, int W, int h, int w, int ds, const gp_ws& s, float* norm, unsigned char* edge, void* stream)
{
    const int P = h * w, nblk = (P + 255) / 256;
    hipLaunchKernelGGL(gp_mag_kernel, dim3(nblk, N), dim3(256), 0, gp_st(stream), flow, s.mag, s.partial, H, W, h, w, ds);
    hipLaunchKernelGGL(gp_peak_kernel, dim3(N), dim3(256), 0, gp_st(stream), s.partial, s.peak, nblk);
    hipLaunchKernelGGL(gp_thresh_kernel, dim3(nblk, N), dim3(256), 0, gp_st(stream), s.mag, s.peak, norm, edge, P);
}

void gp_edt(const unsigned char* edge, int N, int h, int w, int* g, int* d2, void* stream)
{
    hipLaunchKernelGGL(gp_cols_kernel, dim3((w + 63) / 64, N), dim3(64), 0, gp_st(stream), edge, g, h, w);
    hipLaunchKernelGGL(gp_rows_kernel, dim3(h, N), dim3(256), 0, gp_st(stream), g, d2, h, w);
}

void gp_nms(const int* d2, int N, int h, int w, int r, int* rmax, unsigned char* cand, void* stream)
{
    hipLaunchKernelGGL(gp_rowmax_kernel, dim3(h, N), dim3(256), 0, gp_st(stream), d2, rmax, h, w, r);
    hipLaunchKernelGGL(gp_colmax_kernel, dim3((h * w + 255) / 256, N), dim3(256), 0, gp_st(stream), d2, rmax, cand, h, w, r);
}

void gp_select(const unsigned char* cand, int N, int h, int w, int d, int scale, const gp_ws& s, int* counts, int* points, int cap, void* stream)
{
    hipLaunchKernelGGL(gp_rowcnt_kernel, dim3(h, N), dim3(64), 0, gp_st(stream), cand, s.rowcnt, h, w);
    hipLaunchKernelGGL(gp_compact_kernel, dim3(h, N), dim3(64), 0, gp_st(stream), cand, s.rowcnt, s.list, s.ncand, h, w);
    hipLaunchKernelGGL(gp_walk_kernel, dim3(N), dim3(64), 0, gp_st(stream), s.list, s.ncand, counts, points, h, w, d, scale, cap);
}

void gp_scatter(const float* flow, int N, int H, int W, int stride, const int* counts, const int* points, int cap, float* sparse, void* stream)
{
    const int y0 = stride > 0 ? (H - H / stride * stride) / 2 : 0, x0 = stride > 0 ? (W - W / stride * stride) / 2 : 0;
    const long long total = (long long)N * H * W;
    const int blocks = (int)min((total + 255) / 256, (long long)65535 * 16);
    hipLaunchKernelGGL(gp_grid_kernel, dim3(blocks), dim3(256), 0, gp_st(stream), flow, sparse, H, W, stride, y0, x0, total);
    hipLaunchKernelGGL(gp_points_kernel, dim3((cap + 255) / 256, N), dim3(256), 0, gp_st(stream), flow, sparse, counts, points, cap, H, W);
}

inline long long gp_most(int h, int w, int d) { return (long long)((h + d - 1) / d) * ((w + d - 1) / d); }
inline bool gp_cap(int cap, int h, int w, int d) { return cap >= gp_most(h, w, d); }

}  // namespace

extern "C" long long dc_guide_ws_bytes(int N, int H, int W)
{
    if (!gp_batch(N) || !gp_dim(H) || !gp_dim(W)) return -1;
    const int ds = gp_ds(H, W);
    return gp_plan(nullptr, N, (H + ds - 1) / ds, (W + ds - 1) / ds).bytes;
}

extern "C" int dc_guide_edge(const float* flow, int N, int H, int W, void* ws, float* mag, unsigned char* edge, void* stream)
{
    if (!flow || !ws || !edge || !gp_batch(N) || !gp_dim(H) || !gp_dim(W)) return DC_ERR_INVALID;
    const int ds = gp_ds(H, W), h = (H + ds - 1) / ds, w = (W + ds - 1) / ds;
    gp_edge(flow, N, H, W, h, w, ds, gp_plan(ws, N, h, w), mag, edge, stream);
    return dc_launch_status();
}

extern "C" int dc_guide_edt(const unsigned char* edge, int N, int h, int w, void* ws, int* d2, void* stream)
{
    if (!edge || !ws || !d2 || !gp_batch(N) || !gp_side(h) || !gp_side(w)) return DC_ERR_INVALID;
    gp_edt(edge, N, h, w, gp_plan(ws, N, h, w).g, d2, stream);
    return dc_launch_status();
}

extern "C" int dc_guide_nms(const int* d2, int N, int h, int w, int ks, void* ws, unsigned char* cand, void* stream)
{
    if (!d2 || !ws || !cand || !gp_batch(N) || !gp_side(h) || !gp_side(w) || !gp_ks(ks)) return DC_ERR_INVALID;
    gp_nms(d2, N, h, w, gp_d(ks), gp_plan(ws, N, h, w).rmax, cand, stream);
    return dc_launch_status();
}

extern "C" int dc_guide_select(const unsigned char* cand, int N, int h, int w, int ks, int scale, void* ws, int* counts, int* points, int cap,
                               void* stream)
{
    if (!cand || !ws || !counts || !points || !gp_batch(N) || !gp_side(h) || !gp_side(w) || !gp_ks(ks)) return DC_ERR_INVALID;
    if (scale < 1 || scale > (1 << 15) || !gp_cap(cap, h, w, gp_d(ks))) return DC_ERR_INVALID;
    gp_select(cand, N, h, w, gp_d(ks), scale, gp_plan(ws, N, h, w), counts, points, cap, stream);
    return dc_launch_status();
}

extern "C" int dc_guide_scatter(const float* flow, int N, int H, int W, int stride, const int* counts, const int* points, int cap, float* sparse,
                                void* stream)
{
    if (!flow || !counts || !points || !sparse || !gp_batch(N) || !gp_dim(H) || !gp_dim(W) || stride < 0 || cap < 1) return DC_ERR_INVALID;
    gp_scatter(flow, N, H, W, stride, counts, points, cap, sparse, stream);
    return dc_launch_status();
}

extern "C" int dc_guide_watershed(const float* flow, int N, int H, int W, int ks, int stride, void* ws, int* counts, int* points, int cap,
                                  float* sparse, void* stream)
{
    if (!flow || !ws || !counts || !points || !gp_batch(N) || !gp_dim(H) || !gp_dim(W) || !gp_ks(ks) || stride < 0) return DC_ERR_INVALID;
    const int ds = gp_ds(H, W), h = (H + ds - 1) / ds, w = (W + ds - 1) / ds, d = gp_d(ks);
    if (!gp_cap(cap, h, w, d)) return DC_ERR_INVALID;
    const gp_ws s = gp_plan(ws, N, h, w);
    gp_edge(flow, N, H, W, h, w, ds, s, nullptr, s.edge, stream);
    gp_edt(s.edge, N, h, w, s.g, s.d2, stream);
    gp_nms(s.d2, N, h, w, d, s.rmax, s.cand, stream);
    gp_select(s.cand, N, h, w, d, ds, s, counts, points, cap, stream);          // the list takes the magnitude's place: stage 1 is done
    if (sparse) gp_scatter(flow, N, H, W, stride, counts, points, cap, sparse, stream);
    return dc_launch_status();
}
