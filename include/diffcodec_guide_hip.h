/* C ABI of the guide-point sampler (csrc/guide_points.hip), compiled into libdiffcodec_hip.so next to the entry points of the other
 * three headers and bound by diffcodec_amd.lib.GUIDE_SIGNATURES: the 'watershed' strategy of the reference's flow_sampler
 * (cmp/utils/data_utils.py), alone or united with its 'grid' strategy, on dense fp32 flow [N][2][H][W].
 *
 * The working image is flow[:, :, ::ds, ::ds] with ds = max(1, max(H, W) / 400): h = ceil(H / ds) rows of w = ceil(W / ds) pixels,
 * both below 800 for every H, W.  The stage entries that take a working image (edt, nms, select) refuse h or w >= 800.
 *
 * Every launcher only enqueues kernels on `stream` (a hipStream_t; null = the default stream; no memset or copy nodes) and touches
 * no memory but the caller's tensors and `ws`, so a chain of them is capturable into a graph.  Only the edge magnitude is floating
 * point (fp32, fixed operation order, no contraction; its peak is a max, which no order changes); everything after the threshold
 * is integer.  No atomics of any kind: bitwise reproducible and independent of the image's position in the batch.
 * Return 0, -1 for an invalid argument (nothing is launched), -2 when the launch fails.
 *
 * `ws`: dc_guide_ws_bytes(N, H, W) bytes, any contents, 256-byte aligned; for a stage entry on a working image, of
 * dc_guide_ws_bytes(N, h, w).  ks: the odd NMS window, >= 3; d = (ks - 1) / 2. */
#ifndef DIFFCODEC_GUIDE_HIP_H
#define DIFFCODEC_GUIDE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the scratch of every entry below for N flows of H x W; -1 for N < 1 or a dimension < 1. */
long long dc_guide_ws_bytes(int N, int H, int W);

/* Stage 1.  Per channel the 3x3 Sobel pair on the working image with clamped indices, sqrt(ex^2 + ey^2) summed over the two
 * channels, divided by max(peak of the image, 0.01).  mag (may be null): the normalised magnitude, fp32 [N][h][w];
 * edge: 1 where it is > 0.1, else 0, bytes [N][h][w]. */
int dc_guide_edge(const float* flow, int N, int H, int W, void* ws, float* mag, unsigned char* edge, void* stream);
/* Stage 2.  d2 [N][h][w] (int32): the exact squared Euclidean distance to the nearest pixel with edge != 0; 1 << 29 at every
 * pixel of an image that has no edge pixel. */
int dc_guide_edt(const unsigned char* edge, int N, int h, int w, void* ws, int* d2, void* stream);
/* Stage 3.  cand [N][h][w] bytes: 1 where 0 < d2 < (1 << 29) and d2 >= the maximum of d2 over the ks x ks window clipped to the
 * image, except on the one-pixel border; else 0. */
int dc_guide_nms(const int* d2, int N, int h, int w, int ks, void* ws, unsigned char* cand, void* stream);
/* Stage 4.  The candidates (cand != 0) in row-major order; one survives iff no earlier survivor lies within |dy| < d and |dx| < d.
 * counts [N]: the survivors of each image; points [N][cap][2] (int32): their (y * scale, x * scale) in row-major order, then -1.
 * cap >= ceil(h / d) * ceil(w / d), the most that can survive; scale >= 1. */
int dc_guide_select(const unsigned char* cand, int N, int h, int w, int ks, int scale, void* ws, int* counts, int* points, int cap,
                    void* stream);
/* Stage 5.  sparse [N][4][H][W] (fp32): (u, v, 1, 1) of the flow at the first counts[n] points of image n (full-resolution (y, x))
 * and, with stride >= 1, at the 'grid' points of dc_cmp_sparse_grid; 0 elsewhere.  stride 0: no grid points. */
int dc_guide_scatter(const float* flow, int N, int H, int W, int stride, const int* counts, const int* points, int cap, float* sparse,
                     void* stream);
/* The five stages in one call with ds as above: counts and points as dc_guide_select with scale = ds
 * (cap >= ceil(h / d) * ceil(w / d)), sparse as dc_guide_scatter or null for the points alone. */
int dc_guide_watershed(const float* flow, int N, int H, int W, int ks, int stride, void* ws, int* counts, int* points, int cap,
                       float* sparse, void* stream);

#ifdef __cplusplus
}
#endif
#endif
