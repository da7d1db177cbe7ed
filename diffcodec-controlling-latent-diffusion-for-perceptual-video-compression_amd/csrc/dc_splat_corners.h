// The corner set-up of a splat source, shared by every backward kernel that gathers from the four targets around a landing point
// (splat_grad.hip: dc_splat_ingrad_f32, dc_splat_flowgrad_f32; pyramid_grad.hip: dc_pyramid_warp_grad_f32), so that all of them
// decide validity the same way.
#pragma once
#include "dc_common.h"

// The four corners of source (x, y) of image n (softsplat.py:298-318, :384-404, :455-475): weight factors and validity.
//   ax = sex - fx, bx = fx - nwx, ay = sey - fy, by = fy - nwy;   w: nw ax*ay, ne bx*ay, sw ax*by, se bx*by
// off[k] = pixel offset of corner k inside a plane, ok[k] = the corner lies inside the map.  A landing point that is not finite,
// or so far out that no corner can be inside (its floor need not fit an int), has no valid corner.
struct Corners {
    float ax, bx, ay, by;
    long long off[4];
    bool ok[4];
};

__device__ __forceinline__ Corners corners_of(const float* __restrict__ flow, long long n, long long hw, long long p, int H, int W)
{
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const float fx = (float)x + flow[(n * 2 + 0) * hw + p];
    const float fy = (float)y + flow[(n * 2 + 1) * hw + p];
    Corners c;
    c.ax = c.bx = c.ay = c.by = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) c.off[k] = 0, c.ok[k] = false;
    if (isfinite(fx) && isfinite(fy) && fx >= -1.0f && fx < (float)W && fy >= -1.0f && fy < (float)H) {
        const int nwx = (int)floorf(fx), nwy = (int)floorf(fy);           // in [-1, W-1] x [-1, H-1]
        c.ax = (float)(nwx + 1) - fx, c.bx = fx - (float)nwx;
        c.ay = (float)(nwy + 1) - fy, c.by = fy - (float)nwy;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int cx = nwx + (k & 1), cy = nwy + (k >> 1);
            c.ok[k] = cx >= 0 && cx < W && cy >= 0 && cy < H;
            c.off[k] = c.ok[k] ? (long long)cy * W + cx : 0;
        }
    }
    return c;
}
