// Host-side routing interface of the conv / linear path (dc_conv_igemm_bf16): the six kernel families of igemm.hip, conv3x3_tile.hip,
// gemm_dma.hip, gemm_wide.hip, gemm_p8.hip and gemm_rowpanel.hip see each other through these declarations only.
#pragma once
#include "dc_common.h"
#include "../../include/diffcodec_hip.h"

// The launch decision for one dc_conv_desc: decided once by conv_route (igemm.hip), then read by the launchers, by dc_conv_route /
// dc_conv_instance and by dc_conv_gn_part_chunks, so that none of them can disagree.  `kernel` and the template fields name the
// launched instance completely; a field a family's template does not have stays 0.
struct dc_route {
    int kernel;     // DC_ROUTE_*
    int variant;    // tile form as dc_conv_route reports it (info[1])
    int epi;        // EPI: specialised epilogue mode (0 = generic run-time flags)
    int splitk;     // effective split-K
    int ln_first;   // the LayerNorm finalize pass runs first, into ln_scratch
    int tm, tn;     // TM, TN (gemm_dma, conv3x3_tile, igemm); TN (gemm_wide)
    int nst;        // NST (gemm_dma), NSTB (conv3x3_tile)
    int st;         // ST (gemm_wide)
    int gn;         // GN: GroupNorm partials out (gemm_rowpanel), GroupNorm affine on load (conv3x3_tile, igemm)
    int ks3;        // KS3 (igemm)
    int fast, ups, sh;   // FAST, UPS, SH (conv3x3_tile)
    int gn_chunks;  // gn_part_out chunks per sample this launch writes (0: gn_part_out is not set)
};

// A family's route function returns DC_OK (the launch is its own: `r` names the instance), DC_ERR_INVALID (its own, and refused),
// or DC_ROUTE_PASS (not its launch: `r` is untouched and the next family is asked).
#define DC_ROUTE_PASS 1

// N tile of the host routing rules: 160 columns when Cout is a multiple of 160 (all SD-1.5 UNet widths) and the epilogue is
// plain, else 128 (the GEGLU epilogue pairs 16-column blocks of a 128-column tile).
static inline int dc_n_tile(const dc_conv_desc& d) { return (d.Cout % 160 == 0 && d.epilogue == 0) ? 160 : 128; }

// Each family: route decides from the descriptor; launch switches on the route only (the descriptor gives grid sizes and operands).
// gemm_dma.hip: the 1x1 / linear family.  Its route asks the three kernels below first (with r.epi set to the family's epilogue
// mode) and keeps the 128- / 64-row LDS-DMA tiles for itself; launches without a kernel of the family (GroupNorm + SiLU on load) pass.
int dc_gemm_dma_route(const dc_conv_desc& d, dc_route& r);
int dc_gemm_dma_launch(const dc_conv_desc& d, const dc_route& r, hipStream_t st);
// gemm_rowpanel.hip: the K = 320 kernel that keeps a 256-row activation panel in registers and streams only W
int dc_gemm_rowpanel_route(const dc_conv_desc& d, dc_route& r);
int dc_gemm_rowpanel_launch(const dc_conv_desc& d, const dc_route& r, hipStream_t st);
// gemm_p8.hip: the 256 x 256 four-phase kernel for the long-K, wide-N linears without residual / statistics
int dc_gemm_p8_route(const dc_conv_desc& d, dc_route& r);
int dc_gemm_p8_launch(const dc_conv_desc& d, const dc_route& r, hipStream_t st);
// gemm_wide.hip: the 256-row ping-pong kernel for long-K launches
int dc_gemm_wide_route(const dc_conv_desc& d, dc_route& r);
int dc_gemm_wide_launch(const dc_conv_desc& d, const dc_route& r, hipStream_t st);
// conv3x3_tile.hip: LDS-staged 2D-tile kernel for 3x3 stride-1 convs with tile-aligned outputs
int dc_conv3x3_tile_route(const dc_conv_desc& d, dc_route& r);
int dc_conv3x3_tile_launch(const dc_conv_desc& d, const dc_route& r, hipStream_t st);
// (igemm.hip, the gather GEMM, takes what is left: its route and launch are local to conv_route's file)
