// The map geometry and workspace layout of lpips.hip's plan, for lpips_grad.hip: dc_lpips_alex leaves the five post-ReLU maps of
// its 2N images at feat_off[l] of its workspace, which is what dc_lpips_alex_keep hands to the backward.
#pragma once

struct dc_lpips_geom {
    int h[5], w[5];                  // relu1 .. relu5
    long long feat_off[5];           // bytes from the workspace base; map l is [M][C_l][h_l][w_l] fp32
    long long total;                 // bytes of the whole workspace
};

// false for a refused size (the rule of dc_lpips_ws_bytes); M images of which `pairs` pairs have tail partials
bool dc_lpips_geometry(int M, int pairs, int H, int W, dc_lpips_geom* g);
