/*
 * diffcodec_hip.h — C-ABI of the MI355X (gfx950) decode hot path of DiffCodec.
 *
 * One shared object (libdiffcodec_hip.so) of `extern "C"` launchers.  Every entry point:
 *   - takes plain device pointers + sizes (no torch / C++ types), the HIP stream as `void*`;
 *   - allocates nothing (workspaces are passed in); the only process-wide state is one lock-free bit per
 *     (kernel, device) recording that the kernel's dynamic-LDS limit was raised on that device;
 *   - enqueues on the given stream and returns immediately: 0 = ok, -1 = invalid argument,
 *     -2 = launch failure.  Safe to capture into a hipGraph.
 *
 * Tensor conventions: activations of the diffusion models are NHWC bf16 ("pixel rows x channels");
 * the control-pyramid stage (extractor + splat) is NCHW fp32 like the reference (softsplat.py:279
 * forces fp32).  Weights: conv [Cout][KH*KW][Cin] bf16 (repacked from the checkpoint's OIHW), linear
 * [Cout][Cin] bf16 (checkpoint layout).
 *
 * Each declaration cites the reference interface it replaces (paths relative to the reference repo).
 * The reference's only native interface on this path is the CuPy launch of `softsplat_out`
 * (controlnet/softsplat.py:284-345); everything else is reached through torch / diffusers module
 * calls, cited by call site.
 */
#ifndef DIFFCODEC_HIP_H
#define DIFFCODEC_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ forward splatting (fp32, NCHW) */
/* Replaces cuda_launch(cuda_kernel('softsplat_out', ...)) — controlnet/softsplat.py:284-345 — together
 * with the 'soft' wrapper math of softsplat.py:246-247,253-270 and the optional `warped*(1-mask)` of
 * control_utils.py:69-70.  Deterministic gather form (sources binned by landing cell, every target sums its sources in
 * ascending raster order): bit-identical from run to run.  ws: scratch of dc_splat_ws_bytes(N, H, W) bytes (any contents).
 * metric [N,1,H,W]; mask [N,1,H,W] or NULL. */
long long dc_splat_ws_bytes(int N, int H, int W);
int dc_splat_soft_f32(const float* in, const float* flow, const float* metric, const float* mask,
                      float* out, void* ws, int N, int C, int H, int W, void* stream);
/* 'sum' mode: out = splat(in, flow) (softsplat.py:235,251); bit-exact with the sequential restatement oracle/splat_oracle.c. */
int dc_splat_sum_f32(const float* in, const float* flow, float* out, void* ws, int N, int C, int H, int W, void* stream);
/* The normalised modes of the wrapper, fused (no-grad forward) — controlnet/softsplat.py:240-247 (the cat[...] that is never
 * materialised here), :251 (the splat) and :253-270 (the normaliser):
 *   mode DC_SPLAT_AVG    'avg'     out = sum in*w           / norm(sum w)            metric must be NULL
 *        DC_SPLAT_LINEAR 'linear'  out = sum (in*metric)*w  / norm(sum metric*w)
 *        DC_SPLAT_SOFT   'soft'    out = sum (in*exp(m))*w  / norm(sum exp(m)*w)
 *   eps  DC_SPLAT_ADDEPS  norm(d) = d + 1e-7 (:256-260)   DC_SPLAT_ZEROEPS  d == 0 ? 1 : d (:262-263)
 *        DC_SPLAT_CLIPEPS clip(d, 1e-7, None) (:265-266; a NaN d stays NaN, as under torch's clip)
 * Same gather, same ascending source order and individually rounded products / sums as dc_splat_sum_f32: 'avg' and 'linear' are
 * bit for bit splat_sum(cat[...]) followed by the fp32 normaliser; (DC_SPLAT_SOFT, DC_SPLAT_ADDEPS) is dc_splat_soft_f32's
 * instance.  mask [N,1,H,W] or NULL as in dc_splat_soft_f32; ws: dc_splat_ws_bytes(N, H, W) bytes. */
#define DC_SPLAT_AVG 0
#define DC_SPLAT_LINEAR 1
#define DC_SPLAT_SOFT 2
#define DC_SPLAT_ADDEPS 0
#define DC_SPLAT_ZEROEPS 1
#define DC_SPLAT_CLIPEPS 2
int dc_splat_norm_f32(const float* in, const float* flow, const float* metric, const float* mask, float* out, void* ws,
                      int N, int C, int H, int W, int mode, int eps, void* stream);
/* Replaces cuda_launch(cuda_kernel('softsplat_ingrad', ...)) — controlnet/softsplat.py:368-435 (arithmetic :376-423):
 * ingrad[n,c,y,x] = sum over the in-bounds corners (NW, NE, SW, SE) of outgrad[n,c,corner] * w_corner, every product and sum
 * rounded on its own.  Every element is written: a source whose landing point is not finite gets 0 (the reference starts from
 * a zeroed tensor), so `ingrad` may be uninitialised memory.  flow [N,2,H,W]; outgrad, ingrad [N,C,H,W].  No scratch. */
int dc_splat_ingrad_f32(const float* flow, const float* outgrad, float* ingrad, int N, int C, int H, int W, void* stream);
/* Replaces cuda_launch(cuda_kernel('softsplat_flowgrad', ...)) — controlnet/softsplat.py:439-524 (arithmetic :447-511):
 * flowgrad[n,k,y,x] = sum over channels and in-bounds corners of (outgrad[n,c,corner] * in[n,c,y,x]) * dw_k,corner with the dw of
 * :477-489; both components in one pass over the channels (the reference runs one thread per component).  The channel sum of a
 * source is split over S lanes of a workgroup (S a function of C and H*W only), each lane summing its channels c = s, s + S, ...
 * in ascending order, and the S partial sums are added in ascending s: a fixed order, no float atomics, bit-identical from
 * launch to launch and independent of N.  Non-finite landing points get 0 in both components; every element is written.
 * in, outgrad [N,C,H,W]; flow, flowgrad [N,2,H,W].  No scratch. */
int dc_splat_flowgrad_f32(const float* in, const float* flow, const float* outgrad, float* flowgrad, int N, int C, int H, int W,
                          void* stream);
/* compute_mask(a, b) — controlnet/control_utils.py:11-17: occ = (|| b + softsplat(a, b, ones, 'soft') ||_2 > 0.3).
 * ws: dc_splat_ws_bytes(N, H, W) bytes. */
int dc_occlusion_mask_f32(const float* flow_a, const float* flow_b, float* mask_out, void* ws,
                          int N, int H, int W, void* stream);
/* resize_and_normalize_flow_batched — controlnet/control_utils.py:74-97 (bilinear, align_corners=False,
 * then u/((w-1)/2), v/((h-1)/2)).  src [N,2,H,W] with batch stride `src_batch_stride` floats (lets the
 * caller pass flow[:, :2] / flow[:, 2:] views of the [N,4,H,W] control, extractors.py:268-269). */
int dc_flow_resize_normalize_f32(const float* src, long long src_batch_stride, float* dst,
                                 int N, int H, int W, int h, int w, void* stream);
/* Bi_Dir_ResidueExtractor's flow scaling — controlnet/extractors.py:181-183: bilinear (align_corners=False) then u/div_x,
 * v/div_y (div = 512/res: pixel rescale instead of the grid-style normalisation above). */
int dc_flow_resize_divide_f32(const float* src, long long src_batch_stride, float* dst, int N, int H, int W, int h, int w,
                              float div_x, float div_y, void* stream);
/* Confidence fusion + double-hole fill — controlnet/extractors.py:297-310. All [N,*,H,W] fp32.
 * occ_f = occ_b = NULL: fusion only (Bi_Dir_ResidueExtractor, extractors.py:199-203, has no hole fill). */
int dc_fuse_warped_f32(const float* warped_first, const float* warped_last, const float* conf_f,
                       const float* conf_b, const float* occ_f, const float* occ_b, float* fused,
                       int N, int C, int H, int W, void* stream);

/* ------------------------------------------------------------------ fp32 NCHW direct conv (extractor) */
/* nn.Conv2d(k=3, padding=1, stride s in {1,2,4}) [+ SiLU] of the control extractors — controlnet/extractors.py:215-262,
 * control_utils.py:43-47.  x [N,Cin,H,W] (batch stride given, for channel-sliced views), w OIHW fp32. */
int dc_conv3x3_nchw_f32(const float* x, long long x_batch_stride, const float* w, const float* bias, float* y,
                        int N, int Cin, int H, int W, int Cout, int stride, int silu, void* stream);
/* The kernel instance dc_conv3x3_nchw_f32 launches for a shape, without launching anything (host code; the same routing function
 * the launch switches on).  Returns 0, or DC_ERR_INVALID for a shape the launch would refuse (stride not in {1,2,4}, a dimension
 * <= 0), and fills info[DC_F32CONV_ROUTE_INFO_INTS]:
 *   info[0] form: one of DC_F32CONV_* — MFMA conv3x3_f32_mfma_kernel<STRIDE, CO_T, PT> (exact fp32 matrix instruction),
 *           BLK conv3x3_nchw_f32_blk_kernel<STRIDE, 16, 4, 4, 8> (register-blocked VALU: four pixels x 16 channels per thread),
 *           DIRECT conv3x3_nchw_f32_kernel<STRIDE, 8 | 2> (one pixel x 16 channels per thread; every stride-4 launch);
 *   info[1] STRIDE;
 *   info[2] output channels per workgroup: CO_T 64 | 32 (MFMA), 64 (BLK), 16 (DIRECT);
 *   info[3] output pixels per workgroup: PT 128 | 64 (MFMA), 256 (the VALU forms' 16 x 16 tile);
 *   info[4] columns and info[5] rows of that pixel tile (MFMA: min(Wo, PT) columns, whole tiles only; VALU: 16 x 16, ragged). */
#define DC_F32CONV_ROUTE_INFO_INTS 6
#define DC_F32CONV_MFMA 1
#define DC_F32CONV_BLK 2
#define DC_F32CONV_DIRECT 3
int dc_conv3x3_f32_route(int Cin, int H, int W, int Cout, int stride, int* info);

/* ------------------------------------------------------------------ layout / dtype */
int dc_nchw_f32_to_nhwc_bf16(const float* src, void* dst, int N, int C, int H, int W, void* stream);
int dc_nhwc_bf16_to_nchw_f32(const void* src, float* dst, int N, int C, int H, int W, void* stream);
int dc_nhwc_f32_to_nchw_f32(const float* src, float* dst, int N, int C, int H, int W, void* stream);
int dc_f32_to_bf16(const float* src, void* dst, long long n, void* stream);

/* ------------------------------------------------------------------ MFMA implicit GEMM (bf16 in, fp32 acc) */
/* One kernel family serves: F.conv2d 3x3 / 1x1 inside diffusers ResnetBlock2D / Downsample2D / Upsample2D /
 * Transformer2DModel.proj_in/out (call sites flownet.py:83-124, pipeline.py:358-367,391), every nn.Linear
 * (to_q/k/v/out, ff, time_emb_proj), the FDN gamma/beta convs (control_utils.py:31-32) and the ControlNet
 * zero-convs (flownet.py:120-128).  Fusions: GroupNorm-affine(+SiLU) on load, nearest-2x upsample on load,
 * channel-concat of two inputs on load (UNet skip connections), bias + per-sample channel add (time
 * embedding) + out_scale (conditioning_scale) + residual add, or GEGLU, on store. */
typedef struct dc_conv_desc {
    const void* x1;         /* NHWC bf16 [N,H,W,C1] */
    const void* x2;         /* NHWC bf16 [N,H,W,C2] or NULL (channel concat: cat[x1,x2]) */
    const void* w;          /* bf16 [Cout][ksize*ksize][C1+C2] */
    const float* bias;      /* [Cout] or NULL */
    const float* gn_ab;     /* [gn_batch][C1+C2][2] fp32 (scale, shift) applied on load, or NULL.  1x1 launches: with gn_silu == 0 and a
                             * shape the K = 320 row-panel GEMM takes (>= 65,536 rows, whole 256-row panels inside one sample) the affine is
                             * applied to the kernel's register-resident activations and `stats_out` / `gn_part_out` stay available (same
                             * bits as dc_gn_apply_nhwc_bf16 followed by the plain launch); other 1x1 launches take the gather GEMM,
                             * which has no statistics epilogue (DC_ERR_INVALID if one is requested). */
    const float* row_add;   /* [N][Cout] fp32 added per sample (time-embedding projection) or NULL */
    const void* residual;   /* NHWC bf16 [M][Cout] added after scaling, or NULL */
    void* out;              /* bf16 [M][Cout] (f32 if out_f32; [M][Cout/2] for GEGLU) */
    float* splitk_ws;       /* fp32 [splitk][M][Cout] when splitk > 1: one slab per split, summed by the finish pass */
    int N, H, W;            /* input dims (before the fused upsample) */
    int C1, C2, Cout;
    int ksize;              /* 1 or 3 */
    int stride;             /* 1 or 2 */
    int pad;                /* 1: symmetric pad 1; 0: F.pad(x,(0,1,0,1)) + pad 0 (VAE encoder downsample) */
    int upsample;           /* 1: F.interpolate(scale_factor=2, nearest) fused on load */
    int Ho, Wo;             /* output dims */
    int gn_silu;            /* SiLU after the GN affine */
    int epilogue;           /* 0: linear; 1: GEGLU (weights/bias rows pre-interleaved 16 hid | 16 gate) */
    int out_f32;
    float out_scale;
    int splitk;             /* >= 1: an explicit split-K request (shrunk until every split owns K steps); DC_SPLITK_AUTO: the
                             * library picks, see below; any other value below 1 means 1 (a zeroed descriptor runs unsplit) */
    int gn_batch;           /* rows of gn_ab (sample n uses row n % gn_batch) */
    int act;                /* 0 none, 1 SiLU, 2 quick-GELU x*sigmoid(1.702x) — applied after bias/row_add, before out_scale */
    long long row_add_stride; /* floats between consecutive samples of row_add (0 = Cout) */
    /* nn.LayerNorm folded into the following nn.Linear (BasicTransformerBlock.norm1/2/3 -> attn1.to_q/k/v, attn2.to_q,
     * ff.net.0.proj): with W' = W diag(gamma) and b' = b + W beta prepared by the caller,
     *   Linear(LN(x)) = rstd * (x W'^T - mean * colsum(W')) + b',
     * so the GEMM runs on the raw rows and the normalisation is two per-row scalars in the epilogue; the standalone
     * LayerNorm pass (read + write of the whole activation) disappears.  1x1 / linear descriptors only. */
    const float* ln_stats;  /* consumer: [M][2] fp32 (mean, rstd) of every input row (dc_ln_finalize), or NULL */
    const float* ln_colsum; /* consumer: [Cout] fp32 sum over k of the (bf16) weight row, required with ln_stats */
    float* stats_out;       /* producer: [M][dc_gemm_row_stats_parts(Cout)][2] partial (sum, sum sq) of every OUTPUT row, or NULL */
    /* GroupNorm statistics of the OUTPUT from the epilogue that produces it (ResnetBlock2D.norm1/norm2, Transformer2DModel.norm
     * and FDN read them next): [dc_conv_gn_part_chunks(desc)][N][Cout][2] fp32 per-(pixel tile, sample, channel) partial
     * (sum, sum of squares) — the operand dc_gn_finalize takes — instead of a separate read pass over the tensor.  NULL = off.
     * Only the launches for which dc_conv_gn_part_chunks returns > 0 accept it. */
    float* gn_part_out;
    /* The LayerNorm finalize folded into the consumer (round 3).  ln_parts > 0: `ln_stats` holds the RAW partials
     * [M][ln_parts][2] (sum, sum of squares) exactly as a producer's `stats_out` (or dc_row_stats_bf16, parts = 1) wrote them, and
     * the launch forms (mean, rstd) over the C1 + C2 input channels itself, with dc_ln_finalize's arithmetic and `ln_eps`: kernels
     * whose waves own whole rows do it in their prologue; for the other kernels the launcher runs the dc_ln_finalize pass into
     * `ln_scratch` ([M][2] floats, caller-owned, required) first — either way the same bits as finalizing beforehand.
     * ln_parts == 0: `ln_stats` is the finalized [M][2] (mean, rstd). */
    int ln_parts;
    float ln_eps;
    float* ln_scratch;
} dc_conv_desc;
/* dc_conv_desc.splitk = DC_SPLITK_AUTO: the library chooses the split for the launch's shape and kernel (1 wherever the route
 * accepts no other: ln_stats, stats_out, GEGLU, a Cout that is no multiple of 16).  dc_conv_igemm_bf16, dc_conv_route (info[3] is
 * the pick), dc_conv_instance, dc_conv_igemm_ws_bytes (the bytes of the pick) and dc_conv_gn_part_chunks (0 when the pick is above
 * 1) resolve it the same way; a pick above 1 needs splitk_ws as an explicit split does. */
#define DC_SPLITK_AUTO (-1)
int dc_conv_igemm_bf16(const dc_conv_desc* desc, void* stream);
/* The dispatcher's decision for `desc`, without launching anything: the same routing function dc_conv_igemm_bf16 runs.
 * Returns what the launch would return for its descriptor checks (0 or DC_ERR_INVALID; operand checks that do not steer the
 * route — splitk_ws and ln_scratch being set — are left to the launch) and fills info[DC_ROUTE_INFO_INTS]:
 *   info[0] kernel: one of DC_ROUTE_*;
 *   info[1] variant: gemm_dma TM*10000 + TN*1000 + stages*100 + A_REG*10 + PROD (its template; the A_REG digit is always 0 and
 *           the PROD digit always 1, kept so that recorded routes stay valid); igemm TM*10 + TN;
 *           conv3x3_tile its tile rows (2 / 4, 8 = two 8x8 images per tile); 0 for the other kernels;
 *   info[2] epilogue mode (gemm_dma family and conv3x3_tile: the specialised epilogue; 0 = generic run-time flags);
 *   info[3] effective split-K (after shrinking to the fixpoint where every split owns a non-empty K range);
 *   info[4] 1 if the LayerNorm finalize runs first as its own pass into `ln_scratch` (then required), else 0. */
#define DC_ROUTE_INFO_INTS 5
#define DC_ROUTE_GEMM_DMA 1
#define DC_ROUTE_GEMM_WIDE 2
#define DC_ROUTE_GEMM_P8 3
#define DC_ROUTE_GEMM_ROWPANEL 4
#define DC_ROUTE_CONV3X3_TILE 5
#define DC_ROUTE_IGEMM 6
int dc_conv_route(const dc_conv_desc* desc, int* info);
/* The kernel instance dc_conv_igemm_bf16 launches for `desc`, from the same routing function: returns as dc_conv_route does and
 * fills info[DC_CONV_INSTANCE_INTS] with info[0] = kernel (DC_ROUTE_*) followed by the template arguments of that kernel's instance
 * (unused slots 0):
 *   gemm_dma       gemm_dma_kernel<TM, TN, NST, EPI>: wave tile rows / columns in 16s, LDS stages, epilogue mode;
 *   gemm_wide      gemm_wide_kernel<TN, EPI, ST>: ST bit 0 = row statistics out, bit 1 = GroupNorm partials out;
 *   gemm_p8        gemm_p8_kernel<EPI>;
 *   gemm_rowpanel  gemm_rowpanel_kernel<EPI, GN>: GN = GroupNorm partials out;
 *   conv3x3_tile   conv3x3_tile_kernel<TM, TN, GN, NSTB, EPI, FAST, UPS, SH>: GN = GroupNorm affine on load, weight-ring stages,
 *                  half-step pipeline and its fused-upsample / 8-wide-map forms;
 *   igemm          igemm_kernel<2, 2, TM, TN, KS3, GN>: 3x3 gather, GroupNorm affine on load. */
#define DC_CONV_INSTANCE_INTS 9
int dc_conv_instance(const dc_conv_desc* desc, int* info);
/* Workspace bytes needed for splitk>1 (0 otherwise); under DC_SPLITK_AUTO, for the split the library picks. */
long long dc_conv_igemm_ws_bytes(const dc_conv_desc* desc);
/* Partials per output row that a 1x1 / linear launch with `stats_out` writes (one per wave column slice of the tile grid). */
int dc_gemm_row_stats_parts(int Cout);
/* Pixel-tile partials per sample that a launch of `desc` writes to gn_part_out; 0 if that launch cannot emit them (split-K,
 * GEGLU, fp32 output of a 1x1, kernels without the statistics epilogue, pixel tiles that straddle samples). */
int dc_conv_gn_part_chunks(const dc_conv_desc* desc);
/* Row statistics of a bf16 matrix x [M][C] for `ln_stats` when the producing launch cannot emit them (one partial per row):
 * stats [M][1][2] = (sum, sum of squares). */
int dc_row_stats_bf16(const void* x, float* stats, long long M, int C, void* stream);
/* Partials [M][parts][2] (from `stats_out` or dc_row_stats_bf16) -> mean_rstd [M][2] = (mean, 1/sqrt(var + eps)) over C channels:
 * the `ln_stats` operand.  One small launch per LayerNorm instead of the read + write pass over the activation. */
int dc_ln_finalize(const float* partials, float* mean_rstd, long long M, int parts, int C, float eps, void* stream);

/* Small-channel direct convs (NHWC bf16): Cin <= 8 (conv_in 4->320, VAE conv_in) and Cout <= 8
 * (conv_out 320->4, VAE conv_out 128->3 / 512->8, quant convs).  Same fusions on load as the igemm.
 * w_small_cin: bf16 [k*k][Cin][Cout]; w_small_cout: bf16 [Cout][k*k][Cin]. */
int dc_conv_small_cin_bf16(const void* x, const void* w, const float* bias, void* out, int N, int H, int W,
                           int Cin, int Cout, int ksize, int stride, int pad, int Ho, int Wo, void* stream);
int dc_conv_small_cout_bf16(const void* x, const void* w, const float* bias, const float* gn_ab, int gn_silu,
                            int gn_batch, void* out, int out_f32, int N, int H, int W, int Cin, int Cout, int ksize,
                            void* stream);

/* ------------------------------------------------------------------ normalisation */
/* GroupNorm (diffusers ResnetBlock2D.norm1/2, Transformer2DModel.norm, conv_norm_out; FDN.param_free_norm,
 * control_utils.py:24,29): per-(chunk,sample,channel) partial sums -> per-(sample,channel) scale/shift.
 * partials: fp32 [dc_gn_stats_chunks(HW,C)][N][C][2], fully written (no zeroing needed, no atomics). */
int dc_gn_stats_chunks(long long HW, int C);
int dc_gn_stats_nhwc_bf16(const void* x, float* partials, int N, long long HW, int C, void* stream);
/* Sums the chunk slabs, combines the channel sums of cat[x1,x2] into `groups` groups; writes ab [N][C1+C2][2].
 * gamma/beta may be NULL (affine=False, FDN). */
int dc_gn_finalize(const float* sums1, int C1, int chunks1, const float* sums2, int C2, int chunks2, const float* gamma,
                   const float* beta, float* ab, int N, int groups, long long HW, float eps, void* stream);
/* Same result as dc_gn_stats_nhwc_bf16 (+ a second source) followed by dc_gn_finalize, in one launch: one workgroup
 * per (sample, group) reads its channels of cat[x1, x2] directly.  For small maps (<= 16x16), where the two dependent
 * launches dominate.  Group width and C1, C2 must be even. */
int dc_gn_direct_nhwc_bf16(const void* x1, int C1, const void* x2, int C2, const float* gamma, const float* beta,
                           float* ab, int N, long long HW, int groups, float eps, void* stream);
/* y = (x*a+b) [SiLU]; x = cat[x1,x2] NHWC bf16. */
int dc_gn_apply_nhwc_bf16(const void* x1, int C1, const void* x2, int C2, const float* ab, void* y,
                          int N, long long HW, int silu, void* stream);
/* FDN modulation — control_utils.py:33: y = (x*a+b)*(1+gamma)+beta; gamma/beta NHWC bf16 [Bp,HW,C] (sample n uses n % Bp). */
int dc_fdn_modulate_nhwc_bf16(const void* x, const float* ab, const void* gamma, const void* beta, void* y,
                              int N, int Bp, long long HW, int C, void* stream);
/* nn.LayerNorm over the last dim (BasicTransformerBlock.norm1/2/3). x [M][C] bf16. */
int dc_layernorm_bf16(const void* x, const float* gamma, const float* beta, void* y, long long M, int C, float eps,
                      void* stream);

/* ------------------------------------------------------------------ attention */
/* softmax(Q K^T * scale) V, flash-style, heads interleaved on the channel dim (diffusers Attention /
 * F.scaled_dot_product_attention inside BasicTransformerBlock.attn1/attn2).  q [B][Nq][q_stride] etc.;
 * head h occupies columns [h*D, (h+1)*D).  D in {8,16,32,40,64,80,128,160}. */
int dc_attention_bf16(const void* q, const void* k, const void* v, void* out, int B, int heads, int Nq, int Nk, int D,
                      long long q_stride, long long k_stride, long long v_stride, long long o_stride, float scale,
                      void* stream);
/* The form dc_attention_bf16 launches for a shape, without launching anything (host code; the same form rule as the launch).
 * Returns 0, or DC_ERR_INVALID for a shape the launch would refuse, and fills info[DC_ATTN_ROUTE_INFO_INTS] with the template
 * arguments of the attn_kernel<D, QB, SHORT, RAGGED, PP> instance: head dim, 32-query blocks per wave, short-context form (both
 * key tiles resident), ragged last key tile (key masking compiled in), ping-pong form. */
#define DC_ATTN_ROUTE_INFO_INTS 5
int dc_attention_route(int B, int heads, int Nq, int Nk, int D, int* info);
/* Causal softmax(Q K^T * scale) V over a short context (T <= 128, D <= 128): CLIPTextModel self-attention behind
 * `encode_prompt` (pipeline.py:223-236).  Same operand layout as dc_attention_bf16; key j is visible to query i iff j <= i. */
int dc_attention_causal_small_bf16(const void* q, const void* k, const void* v, void* out, int B, int heads, int T, int D,
                                   long long q_stride, long long k_stride, long long v_stride, long long o_stride,
                                   float scale, void* stream);
/* CLIPTextEmbeddings: out[b][t][:] = tok_emb[ids[b][t]][:] + pos_emb[t][:]  (ids int64 [B][T]; tables and out bf16). */
int dc_embed_tokens_bf16(const long long* ids, const void* tok_emb, const void* pos_emb, void* out, int B, int T, int C,
                         int vocab, void* stream);
/* Row softmax fp32 -> bf16 (VAE single-head attention, d=512, done as GEMM/softmax/GEMM). */
int dc_softmax_rows_f32_to_bf16(const float* s, void* p, long long rows, int cols, float scale, void* stream);

/* ------------------------------------------------------------------ elementwise */
/* time_proj — flownet.py:74: sinusoidal embedding of the timestep t_dev[step_dev ? *step_dev : 0] (device-resident so
 * that a captured hipGraph of one denoising step can be replayed for every step). */
int dc_timestep_embedding_f32(const float* t_dev, const int* step_dev, float* out, int n, int dim, void* stream);
/* FreeU — pipe.enable_freeu(s1,s2,b1,b2) (validation.py:106) -> diffusers apply_freeu [recalled]: skip features of up-blocks
 * 0/1 get their 2x2 lowest-frequency block scaled by s (fourier_filter, threshold 1); the backbone's first C/2 channels get *b. */
int dc_freeu_lowfreq_nhwc_bf16(const void* x, void* y, int N, int H, int W, int C, float s, void* stream);
int dc_freeu_backbone_nhwc_bf16(const void* x, void* y, long long pixels, int C, float b, void* stream);
/* y = a*x0 + b*x1 + c*x2 + d*x3 on fp32 tensors (x1..x3 may be NULL): `scheduler.step` of the multistep schedulers the reference
 * instantiates (UniPCMultistepScheduler, validation.py:37) and the CFG combine of the generic loop (pipeline.py:370-375). */
int dc_lincomb4_f32(const float* x0, const float* x1, const float* x2, const float* x3, float a, float b, float c, float d,
                    float* y, long long n, void* stream);
/* dst[c][r] = src[r][c], bf16, batch of `batch` matrices (VAE attention: V -> V^T). */
int dc_transpose_bf16(const void* src, void* dst, int batch, int R, int C, void* stream);
/* DiagonalGaussianDistribution.sample() * scale — train_controlnet.py:1081, pipeline.ipynb cell 7:
 * moments NHWC fp32 [N,h,w,2*C] (mean | logvar), noise NCHW fp32 -> latents NCHW fp32. */
int dc_vae_sample_latents(const float* moments, const float* noise, float* latents, float scale, int N, int C, int H, int W, void* stream);
int dc_silu_f32(const float* x, float* y, long long n, void* stream);
int dc_add_bf16(const void* a, const void* b, void* y, long long n, void* stream);
int dc_add_f32(const float* a, const float* b, float* y, long long n, void* stream);   /* P + W pyramids, flow_resnet.py:90 */
/* CFG combine + DDIM step — pipeline.py:370-375.  eps fp32 NHWC [cfg?2B:B][h][w][4]; latents fp32 NCHW in/out;
 * coef_dev [steps][4] = {sqrt(1-a_t), sqrt(a_t), sqrt(a_prev), sqrt(1-a_prev)}; step_dev int32 counter (incremented).
 * Also writes the next model input NHWC bf16 [cfg?2B:B][h][w][C]. */
int dc_cfg_ddim_step(const float* eps, float* latents, void* model_in, const float* coef_dev, int* step_dev,
                     float guidance, int cfg, int B, int C, int H, int W, void* stream);
/* CFG combine + one UniPCMultistepScheduler.step (the scheduler validation.py:37 instantiates; bh2, predict_x0, order <= 2) in
 * one pass, for the captured denoising step of pipeline.py:308-385: same operand conventions as dc_cfg_ddim_step; m0 / m1 / last
 * fp32 [B,C,H,W] scheduler state (the two most recent x0-predictions, the previous predictor's start sample), updated in place;
 * coef_dev [steps][12] = {1/alpha_i, -sigma_i/alpha_i, flags (1 corrector | 2 corrector uses m1 | 4 predictor uses m1),
 * corrector coefficients of (last, m0, m_t, m1), predictor coefficients of (x, m_t, m1), 0, 0}.  Arithmetic = the
 * dc_lincomb4_f32 sequence of the scheduler's generic `step`, bit for bit. */
int dc_cfg_unipc_step(const float* eps, float* latents, float* m0, float* m1, float* last, void* model_in,
                      const float* coef_dev, int* step_dev, float guidance, int cfg, int B, int C, int H, int W, void* stream);
/* latents NCHW f32 [B,C,H,W] * mul -> NHWC bf16 [rep*B,H,W,C] (pipeline.py:313-320, :391 scaling) */
int dc_latents_to_model_input(const float* latents, void* model_in, float mul, int rep, int B, int C, int H, int W, void* stream);
/* image_processor.postprocess — pipeline.py:397-398: (x/2+0.5).clamp(0,1); x NHWC f32 [N,H,W,3] -> NCHW f32 and/or NHWC u8 */
int dc_postprocess_image(const float* x, float* out_nchw_f32, uint8_t* out_nhwc_u8, int N, int C, int H, int W,
                         int x_pixel_stride /* input elements per pixel, 0 = C (4 when conv_out ran with a padded 4th channel) */, void* stream);

/* ------------------------------------------------------------------ input side (controlnet/utils.py) */
/* resize_flow_to (utils.py:21-28) on the .flo payload layout: src [H][W][2] fp32 (pixel units) -> dst [2][th][tw] fp32,
 * bilinear with align_corners=True, then u *= tw/W and v *= th/H. */
int dc_flow_hw2_resize_scale_f32(const float* src_hw2, int H, int W, float* dst_2hw, int th, int tw, void* stream);
/* load_pair_to_sixch (utils.py:30-39) after the PIL resize: two RGB uint8 [H][W][3] images -> [6][H][W] fp32 in [0,1]
 * (TF.to_tensor's x/255, image 0 in planes 0-2, image 1 in planes 3-5). */
int dc_pack_sixch_u8_f32(const uint8_t* img0_hw3, const uint8_t* img1_hw3, float* dst_6hw, int H, int W, void* stream);

/* ------------------------------------------------------------------ tiled decode (patch_exp.ipynb / patch_utils.py) */
/* Blend of full-size decoded tiles into the frame with half-cosine ramps on inner tile edges (this package's
 * tiled-decode policy, tiling.merge_ramp; the reference's merge_costiles window is kept host-side for parity only).
 * tiles [T][C][th][tw] fp32 in [0,1]; coords int32 [T][4] = (y1, y2, x1, x2) with y2-y1 == th, x2-x1 == tw;
 * ramp [feather] fp32; out uint8 [H][W][C] = clip(rint(sum(scale*tile*w) / sum(w))); every pixel must be covered. */
int dc_blend_tiles_ramp_u8(const float* tiles_nchw, const int* coords_dev, int T, int C, int th, int tw,
                           const float* ramp_dev, int feather, uint8_t* out_hwc, int H, int W, float scale, void* stream);

/* ------------------------------------------------------------------ frame quality metrics (validation.py:120-155, test_utils.py:23-55) */
/* Operands: two logical [N][C][H][W] images, uint8 (x_u8 = 1: converted to fp32 on load) or fp32 (x_u8 = 0), read through element
 * strides: strides[0..3] = X's (n, c, h, w) strides, strides[4..7] = Y's (host array), so NHWC frames and permuted views need no copy.
 * Semantics of pytorch_msssim 1.0 (ms_ssim / ssim: Gaussian window applied as a valid separable correlation, C1 = (K1 L)^2,
 * C2 = (K2 L)^2, avg_pool2d(2, padding = (H % 2, W % 2)) between scales), computed in fp32 with fp64 sums in a fixed order:
 * bitwise reproducible, no float atomics.  win: host array of win_size (odd, <= 15) taps; weights: host array of `levels`
 * (<= 8) exponents.  ws: scratch of dc_ssim_ws_bytes(...) bytes (any contents).  out (device, fp64) [N*C + N + 1]: the value per
 * (n, c), its mean over c per n, the mean over (n, c).  Every scale must keep H, W >= win_size; dc_ssim_ws_bytes returns -1
 * for a shape / window / level count the kernels do not take (N * C <= 65535), and the launch then returns -1 and writes nothing.
 * NaN rule: relu is v < 0 ? 0 : v (torch.relu), in dc_ms_ssim and in dc_ssim with nonnegative = 1: a NaN pixel of a float operand
 * makes the value of its (n, c) plane, the mean of its sample and the overall mean NaN; other planes and samples are unaffected. */
long long dc_ssim_ws_bytes(int N, int C, int H, int W, int win_size, int levels);
int dc_ms_ssim(const void* x, const void* y, int x_u8, const long long* strides, int N, int C, int H, int W, const float* win,
               int win_size, const float* weights, int levels, float K1, float K2, float data_range, void* ws, double* out,
               void* stream);
/* single-scale SSIM (levels = 1 in dc_ssim_ws_bytes); nonnegative = 1 applies relu to the per-(n, c) value (nonnegative_ssim) */
int dc_ssim(const void* x, const void* y, int x_u8, const long long* strides, int N, int C, int H, int W, const float* win,
            int win_size, float K1, float K2, float data_range, int nonnegative, void* ws, double* out, void* stream);
/* PSNR per image: out (device, fp64) [N] = 10 log10(L^2 / mse) over the C*H*W elements of each image, +inf when mse = 0.  The
 * squared differences are summed exactly in 64-bit integers for uint8, in fp64 in a fixed order for fp32.
 * ws: dc_psnr_ws_bytes(N) bytes; 1 <= N <= 65535, otherwise dc_psnr_ws_bytes and the launch return -1. */
long long dc_psnr_ws_bytes(int N);
int dc_psnr(const void* x, const void* y, int x_u8, const long long* strides, int N, int C, int H, int W, double data_range,
            void* ws, double* out, void* stream);

/* LPIPS, AlexNet, version 0.1 (test_utils.py:13,58: lpips.LPIPS(net='alex')) of N image pairs, exact fp32 on the fp32 matrix
 * instruction, sums in a fixed order (bitwise reproducible, independent of a pair's position in the batch, no float atomics).
 * Operands as above with C = 3: uint8 is mapped to x / 255; normalize = 1 applies 2x - 1; then the ScalingLayer
 * (x - shift) / scale, the five conv + ReLU stages (zero padding in the scaled space), per layer the channel-unit-normalised
 * squared difference weighted by the lin vector, its spatial mean, and their sum.  normfix = 1 normalises by
 * sqrt(sum_c (x_c^2 + 1e-8)) (controlnet/lpips_loss.py:27-29) instead of sqrt(sum_c x_c^2) + 1e-10.
 * weights (device, fp32, 16-byte aligned, dc_lpips_weight_floats() elements): for conv1..conv5 the K-major matrix
 * [K = (ci, ky, kx)][Cout] followed by the bias [Cout] (conv1's K = 363 is followed by one zero row: 364 rows), then the five
 * lin vectors [64][192][384][256][256].  ws: dc_lpips_ws_bytes(N, H, W) bytes (-1 when H or W < 31 or N is out of range).
 * out (device, fp64) [5 N + N]: the per-layer values [layer][n], then their sum per pair. */
int dc_lpips_weight_floats(void);
long long dc_lpips_ws_bytes(int N, int H, int W);
int dc_lpips_alex(const void* x, const void* y, int x_u8, const long long* strides, int N, int H, int W, int normalize, int normfix,
                  const float* weights, void* ws, double* out, void* stream);
/* The five post-ReLU maps of one operand (strides[0..3]), contiguous fp32 NCHW: f1 [N,64,H1,W1], f2 [N,192,H2,W2],
 * f3 [N,384,H3,W3], f4 / f5 [N,256,H3,W3] with H1 = (H - 7) / 4 + 1, H2 = (H1 - 3) / 2 + 1, H3 = (H2 - 3) / 2 + 1 (floor).
 * ws: dc_lpips_features_ws_bytes(N, H, W) bytes. */
long long dc_lpips_features_ws_bytes(int N, int H, int W);
int dc_lpips_alex_features(const void* x, int x_u8, const long long* strides, int N, int H, int W, int normalize,
                           const float* weights, void* ws, float* f1, float* f2, float* f3, float* f4, float* f5, void* stream);
/* One conv + bias + ReLU stage on its own (tools/bench_metrics.py times the layers through it).  layer 0: x is the image operand
 * (x_u8, strides[0..3], M images of H x W) and y is [M,64,H1,W1]; layer 1..4: x is a contiguous fp32 map [M,Cin,H,W] (x_u8 and
 * strides are ignored; H, W <= 4096) and y is [M,Cout,H,W]. */
int dc_lpips_conv(int layer, const void* x, int x_u8, const long long* strides, int M, int H, int W, int normalize,
                  const float* weights, float* y, void* stream);

/* FID features, feature = 64 (test_utils.py:14,39: torchmetrics FrechetInceptionDistance(feature=64)): the stem of the FID
 * InceptionV3 up to its first max-pool, exact fp32 on the fp32 matrix instruction, sums in a fixed order (bitwise reproducible,
 * independent of an image's position in the batch, no float atomics).  Operand as above with C = 3 and any H, W >= 1
 * (strides[0..3]); a float image (x_u8 = 0) holds [0,1] values and is taken as (x * 255) truncated to uint8.  Resize to 299 x 299
 * (TF1-legacy bilinear: p = o * (I / 299), i0 = floor(p), i1 = min(i0 + 1, I - 1)), (x - 128) / 128, then conv 3->32 3x3 / 2,
 * conv 32->32 3x3, conv 32->64 3x3 pad 1, each followed by eval BatchNorm (one fma per channel) and ReLU, max-pool 3x3 / 2 and
 * the spatial mean.  weights (device, fp32, 16-byte aligned, dc_fid_weight_floats() elements): per block the K-major matrix
 * [K = (ci, ky, kx)][Cout] (block 1: K = 27 followed by one zero row), then s [Cout] = bn.weight / sqrt(running_var + 1e-3) and
 * t [Cout] = bn.bias - running_mean * s.  ws: dc_fid_ws_bytes(N, H, W) bytes (-1 when N, H or W is out of range).
 * out (device, fp32) [N][64]. */
int dc_fid_weight_floats(void);
long long dc_fid_ws_bytes(int N, int H, int W);
int dc_fid_features(const void* x, int x_u8, const long long* strides, int N, int H, int W, const float* weights, void* ws,
                    float* out, void* stream);
/* The same with every intermediate written to the caller's contiguous fp32 NCHW tensors (needs no workspace): resized
 * [N,3,299,299], the three post-ReLU maps m1 [N,32,149,149], m2 [N,32,147,147], m3 [N,64,147,147], pooled [N,64,73,73]. */
int dc_fid_maps(const void* x, int x_u8, const long long* strides, int N, int H, int W, const float* weights, float* resized,
                float* m1, float* m2, float* m3, float* pooled, float* out, void* stream);
/* One conv + BatchNorm + ReLU block on its own (tools/bench_metrics.py times the blocks through it): layer 0..2, x the block's
 * contiguous fp32 input [N,3,299,299] / [N,32,149,149] / [N,32,147,147], y its output map. */
int dc_fid_conv(int layer, const float* x, int N, const float* weights, float* y, void* stream);
/* state (device, fp64) [1 + 64 + 64 * 64] = n, sum f, sum f f^T (row-major) += the N rows of features [N][64], added image by image
 * in batch order: two calls leave the bits of one call on the concatenation. */
int dc_fid_accumulate(const float* features, int N, double* state, void* stream);

/* FVD features (test_utils.py:45-70; fvd_utils/models/fvd): the Inception-v1 I3D network, 400 logits per video, exact fp32 on the
 * fp32 matrix instruction, sums in a fixed order (bitwise reproducible, independent of a video's position in the batch and of the
 * batch size, no float atomics).  Operand: N videos of T >= 9 frames, logical [N][T][3][H][W], uint8 (x_u8 = 1) or fp32, read
 * through the five element strides (n, t, c, h, w) of `strides` (host array), so uint8 NTHWC frames need no copy; div255 = 1
 * divides every tap by 255 first.  Per frame: bilinear resize (align_corners = False, no antialias) to RH x RW, where the shorter
 * side is 224 and the other the caller's ceil(side * 224 / min(H, W)), centre crop to 224 x 224 from (size - 224) / 2, (v - 0.5) * 2,
 * no clamping.  Then the I3D chain: every Unit3D is conv3d with TF "SAME" padding (per axis pad = max(k - s, 0) when
 * size % s == 0, else max(k - size % s, 0); front = pad / 2; output ceil(size / s)), eval BatchNorm as one fma per channel, ReLU;
 * the max-pools pad by the same rule with zeros that enter the max; the head is the [2,7,7] mean of Mixed_5c, the logits conv
 * with bias, and the mean over the remaining time positions.
 * weights (device, fp32, 16-byte aligned, dc_fvd_weight_floats() elements): the 58 units in state-dict order (Conv3d_1a_7x7,
 * Conv3d_2b_1x1, Conv3d_2c_3x3; per Mixed_* module b0, b1a, b1b, b2a, b2b, b3b; logits), each as dc_fvd_conv's `packed`.
 * ws: dc_fvd_ws_bytes(N, T, H, W) bytes (-1 when T < 9 or a size is out of range).  out (device, fp32) [N][400]. */
int dc_fvd_weight_floats(void);
long long dc_fvd_ws_bytes(int N, int T, int H, int W);
int dc_fvd_features(const void* x, int x_u8, int div255, const long long* strides, int N, int T, int H, int W, int RH, int RW,
                    const float* weights, void* ws, float* out, void* stream);
/* The same with the 16 endpoint maps (Conv3d_1a_7x7 .. Mixed_5c, contiguous fp32 [N][C][T'][S][S]) written to the caller's tensors:
 * maps = host array of 16 device pointers. */
int dc_fvd_endpoints(const void* x, int x_u8, int div255, const long long* strides, int N, int T, int H, int W, int RH, int RW,
                     const float* weights, void* ws, float* const* maps, float* out, void* stream);
/* The preprocess on its own: y = contiguous fp32 [N][3][T][224][224]. */
int dc_fvd_preprocess(const void* x, int x_u8, int div255, const long long* strides, int N, int T, int H, int W, int RH, int RW,
                      float* y, void* stream);
/* One Unit3D on caller-given shapes: x contiguous fp32 [N][Cin][T][H][W]; (k, stride) is (7, 2), (3, 1) or (1, 1) on all three axes;
 * y [N][Ctot][To][Ho][Wo], of which channels c_off .. c_off + Cout are written (the others are left alone); relu = 0 leaves the
 * fma's value.  packed (device, fp32, 16-byte aligned): the K-major matrix [rows][CoP], CoP = Cout rounded up to 32 (zero
 * columns), rows in (ci, kt, kh, kw) order and zero-padded per chunk: k = 7 one zero row after the 49 taps of every (ci, kt);
 * k = 3 up to a multiple of 4 input channels (108 rows); k = 1 up to a multiple of 32 input channels; then s [CoP], t [CoP] with
 * y = s * conv + t (BatchNorm folded; s = 1, t = bias for a plain conv). */
int dc_fvd_conv(const float* x, int N, int Cin, int T, int H, int W, int k, int stride, const float* packed, int Cout, int relu,
                float* y, int Ctot, int c_off, void* stream);
/* SAME-padded max-pool of a contiguous fp32 [N][C][T][H][W] map, kernel (kt, kh, kw), stride (st, sh, sw); the padded positions
 * are zeros that enter the max.  y [N][C][ceil(T / st)][ceil(H / sh)][ceil(W / sw)]. */
int dc_fvd_maxpool(const float* x, int N, int C, int T, int H, int W, int kt, int kh, int kw, int st, int sh, int sw, float* y,
                   void* stream);

/* Pillow's 8-bit antialiased resize (Image.resize with BILINEAR, BICUBIC or LANCZOS; no box=, no reducing_gap=), bit for bit.
 * in: uint8 [N][H_in][W_in][C], C in 1..4, read through element strides (n, c, h, w) in dc_psnr's order (a cropped window of a
 * frame is an operand).  out: contiguous uint8 [N][H_out][W_out][C].  Per axis whose sizes differ the caller passes the table
 * Pillow's precompute_coeffs + normalize_coeffs_8bpc build (device, int32): k [out][ksize] = the float64 filter values,
 * normalised, times 2^22, rounded half away from zero; bounds [out][2] = (first input sample, tap count <= ksize); ksize =
 * ceil(support * max(in / out, 1)) * 2 + 1.  One output sample is clip(((1 << 21) + sum_x k[x] * in[first + x]) >> 22, 0, 255) in
 * int32.  The horizontal pass runs first, into `scratch` (dc_resample_ws_bytes(N, H_in, W_out, C) bytes, any contents; only read
 * when both passes run), as bytes rounded and clipped like the result; then the vertical pass.  Null tables for an axis mean
 * "sizes agree, pass skipped" and are an error otherwise; equal sizes on both axes are an error (copy instead).  Errors (a size
 * < 1, C outside 1..4, a null pointer, a ksize that is not one of the three filters' for the axis sizes) are returned before
 * anything is launched.  No allocation, no synchronisation. */
long long dc_resample_ws_bytes(int N, int H_in, int W_out, int C);
int dc_resample_u8(const void* in, const long long* strides, int N, int H_in, int W_in, int C, int H_out, int W_out, const int* k_h,
                   const int* bounds_h, int ksize_h, const int* k_v, const int* bounds_v, int ksize_v, void* scratch, void* out,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif
