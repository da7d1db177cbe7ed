// Host-side routing of the fp32 extractor conv (dc_conv3x3_nchw_f32): conv_direct.hip (the launch, the two VALU forms and the query
// dc_conv3x3_f32_route) and conv_f32_mfma.hip (the exact-fp32 MFMA form) see each other through these declarations only.
#pragma once
#include "dc_common.h"
#include "../../include/diffcodec_hip.h"

constexpr int DC_FM_CK = 8;                    // MFMA form: input channels per LDS chunk
constexpr int DC_FM_MAXE = 26;                 // MFMA form: patch floats per thread per chunk (largest patch: stride 2, 128 x 1 tile: 8*3*257)

// The launch decision for one (Cin, H, W, Cout, stride): decided once by dc_conv_f32_route_of, then read by the launch and by the
// query, so that they cannot disagree.  The fields name the launched instance completely.
struct dc_f32_route {
    int form;       // DC_F32CONV_*
    int stride;     // STRIDE template argument: 1 | 2 (| 4, one-pixel form only)
    int co_t;       // output channels per workgroup: mfma CO_T 64 | 32, blocked 64, one-pixel 16
    int pt;         // output pixels per workgroup: mfma PT 128 | 64, VALU forms 256 (16 x 16)
    int cols_t;     // pixel tile: columns ...
    int rows_t;     // ... x rows (cols_t * rows_t == pt)
};

// Returns DC_OK and fills `r`, or DC_ERR_INVALID for what the launch refuses.
static inline int dc_conv_f32_route_of(int Cin, int H, int W, int Cout, int stride, dc_f32_route& r)
{
    if (Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || (stride != 1 && stride != 2 && stride != 4)) return DC_ERR_INVALID;
    const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
    r.stride = stride;
    // GEMM-shaped layers take the exact-fp32 MFMA form when the GEMM dimensions are whole tiles: Cin a multiple of the 8-channel
    // chunk (>= 16), Cout a multiple of 32, stride 1 | 2 with exact halving, and an output map that splits into 128-pixel tiles
    // (maps below 128 pixels: 64-pixel tiles, which exist for 64-channel tiles only) of cols_t = min(Wo, tile) columns whose input
    // patch fits the staging registers.
    const bool gemm = stride != 4 && Cin >= 16 && Cin % DC_FM_CK == 0 && Cout % 32 == 0 && !(stride == 2 && ((H | W) & 1));
    if (gemm && Ho * Wo >= 64) {
        const int pt = Ho * Wo >= 128 ? 128 : 64;
        const int cols_t = Wo < pt ? Wo : pt;
        if (!(pt == 64 && Cout % 64) && pt % cols_t == 0 && Wo % cols_t == 0 && Ho % (pt / cols_t) == 0) {
            const int rows_t = pt / cols_t;
            if (DC_FM_CK * ((rows_t - 1) * stride + 3) * ((cols_t - 1) * stride + 3) <= DC_FM_MAXE * 256) {
                r.form = DC_F32CONV_MFMA;
                r.co_t = (pt == 64 || Cout % 64 == 0) ? 64 : 32;
                r.pt = pt, r.cols_t = cols_t, r.rows_t = rows_t;
                return DC_OK;
            }
        }
    }
    // the register-blocked form (16 x 16 pixels x 64 output channels per workgroup) wins where there are >= 64 output channels to
    // share an input patch and the map is at least 64 wide (or 32 wide with >= 160 channels); the one-pixel form (16 x 16 pixels x
    // 16 output channels) takes the rest, and every stride-4 launch
    const bool blk = stride != 4 && Cout >= 64 && (Wo >= 64 || (Wo >= 32 && Cout >= 160));
    r.form = blk ? DC_F32CONV_BLK : DC_F32CONV_DIRECT;
    r.co_t = blk ? 64 : 16;
    r.pt = 256, r.cols_t = 16, r.rows_t = 16;
    return DC_OK;
}

// conv_f32_mfma.hip: launches the instance conv3x3_f32_mfma_kernel<r.stride, r.co_t, r.pt> of a DC_F32CONV_MFMA route
int dc_conv_f32_mfma_launch(const float* x, long long xbs, const float* w, const float* bias, float* y, int N, int Cin, int H, int W,
                            int Cout, const dc_f32_route& r, int silu, hipStream_t st);
