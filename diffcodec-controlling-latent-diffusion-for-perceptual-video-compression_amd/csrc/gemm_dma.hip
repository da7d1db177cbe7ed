// Row-major GEMM  out[m][n] = sum_k X[m][k] * W[n][k]  for gfx950 with a multi-stage LDS-DMA pipeline — the 1x1 conv /
// nn.Linear path (Transformer2DModel.proj_out, attention to_q/k/v/out, GEGLU feed-forward, time_emb_proj, conv_shortcut,
// ControlNet zero-convs: call sites flownet.py:87-124, pipeline.py:358-367) whenever no transform is needed on load.
//
// Per workgroup: 256 threads = 4 waves as 2(m) x 2(n), tile BM x BN, BK = 64 (one 128-byte line per row per K-step).
// Both operand tiles go global -> LDS by LDS-DMA in the swizzled stage layout of dc_kstage.h.  NST LDS stages form a ring: the DMA of
// K-step k+NST-1 is issued right after the barrier that opens step k, and a counted `s_waitcnt vmcnt(N)` (never 0 in
// the loop) leaves NST-2 stages in flight across every raw `s_barrier` — one barrier per K-step.
#include "dc_epilogue.h"
#include <cstdlib>

// Developer-only phase stamps (tools/gemm_stamp.py builds this file with -DDC_STAMP into a scratch .so): s_memtime at
// kernel entry / after the first stage landed / after the K loop / at exit, written to the (otherwise unused) split-K
// workspace.  Never defined in the product build.
#ifdef DC_STAMP
#define DC_STAMP_AT(i)                                                                         \
    do {                                                                                       \
        if (threadIdx.x == 0 && d.splitk_ws) {                                                 \
            unsigned long long t_;                                                             \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");         \
            ((unsigned long long*)d.splitk_ws)[(long long)blockIdx.x * 8 + (i)] = t_;          \
        }                                                                                      \
    } while (0)
#else
#define DC_STAMP_AT(i)
#endif

namespace {

// EPI: epilogue specialisation chosen by the launcher from the descriptor.  With every fusion a run-time flag, the unrolled
// (tm, tn) epilogue was 6,300 instructions in 336 basic blocks — a branch (and often a wait) per flag per 4 outputs — and took
// 10.7k cycles per workgroup against 9k for the whole K loop at K = 320 (phase stamps, tools/gemm_stamp.py).  The common
// fusions are compile-time here, so their epilogues are straight-line code:
//   0 generic (run-time flags: row_add, act, fp32 out, split-K, any mix)      1 bias        2 bias + scale + residual
//   3 folded LayerNorm + bias                                               4 GEGLU       5 folded LayerNorm + GEGLU
// stats_out / gn_part_out stay run-time in modes 1-2: one workgroup-uniform test outside the loops.
template <int TM, int TN, int NST, int EPI>
__global__ __launch_bounds__(256, 2) void gemm_dma_kernel(const dc_conv_desc d)
{
    constexpr bool GENERIC = EPI == 0;
    const bool e_geglu = GENERIC ? d.epilogue == 1 : EPI >= 4;
    const bool e_ln = GENERIC ? d.ln_stats != nullptr : (EPI == 3 || EPI == 5);
    const bool e_res = GENERIC ? d.residual != nullptr : EPI == 2;
    const bool e_rowadd = GENERIC && d.row_add != nullptr;
    const int e_act = GENERIC ? d.act : 0;
    const int e_flags = (e_ln ? DC_EPI_LN : 0) | DC_EPI_BIAS | (e_res ? DC_EPI_RES : 0);       // (+ DC_EPI_ROWADD per fragment inside Cout)
    const bool e_stats = (GENERIC || EPI == 1 || EPI == 2) && d.stats_out != nullptr;
    const bool e_gnpart = (GENERIC || EPI == 1 || EPI == 2) && d.gn_part_out != nullptr;
    constexpr int WM = 2, WN = 2;
    constexpr int BM = WM * TM * 16, BN = WN * TN * 16;
    constexpr int ROWS = BM + BN;
    constexpr int STAGE = ROWS * 128;
    constexpr int NGW = ROWS / 32;                    // DMA wave-instructions per wave per stage (8 rows each)
    static_assert(ROWS % 32 == 0 && BN % 32 == 0, "rows per stage must split over 4 waves x 8-row pieces");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;
    const int fr = lane & 15, fq = lane >> 4;
    DC_STAMP_AT(0);

    const int HoWo = d.Ho * d.Wo;
    const int M = d.N * HoWo;
    const int K = d.C1 + d.C2;
    const int KT = K >> 6;
    const int n_tiles = (d.Cout + BN - 1) / BN;
    const int m_tiles = (M + BM - 1) / BM;
    const int nblk = n_tiles * m_tiles;
    const int bid = dc_xcd_remap(blockIdx.x, nblk);
    const int tile_n = bid % n_tiles, tile_m = bid / n_tiles;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    int kt_begin = 0, kt_end = KT;
    if (d.splitk > 1) {
        const int per = (KT + d.splitk - 1) / d.splitk;
        kt_begin = blockIdx.y * per;
        kt_end = min(KT, kt_begin + per);
        if (kt_begin >= kt_end) return;
    }
    const int nk = kt_end - kt_begin;

    // ---- per-lane DMA sources: piece g = wave + 4 i of the stage (dc_kstage.h)
    const char* src1[NGW];                            // row base in x1 (or W) incl. the swizzled chunk offset
    const char* src2[NGW];                            // row base in x2 (second K range) — A rows only
    int ldsoff[NGW];
    const int c1_steps = d.C1 >> 6;
#pragma unroll
    for (int i = 0; i < NGW; ++i) {
        const int g = wave + 4 * i;
        const int row = g * 8 + (lane >> 3);
        const int chunk = dc_kstage_src_chunk(lane, row);
        ldsoff[i] = g * DC_KPIECE;
        if (g * 8 < BM) {
            int m = m0 + row;
            m = m < M ? m : M - 1;                    // clamp: rows past M are computed and discarded
            src1[i] = (const char*)d.x1 + ((long long)m * d.C1 + chunk * 8) * 2;
            src2[i] = d.x2 ? (const char*)d.x2 + ((long long)m * d.C2 + chunk * 8) * 2 : nullptr;
        } else {
            int n = n0 + row - BM;
            n = n < d.Cout ? n : d.Cout - 1;
            src1[i] = (const char*)d.w + ((long long)n * K + chunk * 8) * 2;
            src2[i] = nullptr;
        }
    }
    auto issue_stage = [&](int kt, int slot) {
        kt = kt < kt_end ? kt : kt_end - 1;           // past-the-end stages re-read the last one (keeps vmcnt counts constant)
        char* base = smem + slot * STAGE;
        if (kt < c1_steps) {                          // first K range (the only one without a channel concat): no per-piece select
            // (the builtin, not dc_dma16: see dc_kstage.h)
#pragma unroll
            for (int i = 0; i < NGW; ++i)
                __builtin_amdgcn_global_load_lds((dc_gptr_t)(src1[i] + (long long)kt * 128), (dc_lptr_t)(base + ldsoff[i]), 16, 0, 0);
            return;
        }
#pragma unroll
        for (int i = 0; i < NGW; ++i) {
            const bool is_a = (wave + 4 * i) * 8 < BM;                    // wave-uniform
            const char* p = is_a ? src2[i] + (long long)(kt - c1_steps) * 128 : src1[i] + (long long)kt * 128;
            __builtin_amdgcn_global_load_lds((dc_gptr_t)p, (dc_lptr_t)(base + ldsoff[i]), 16, 0, 0);
        }
    };

    f32x4 acc[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // One K-step: all 2 x (TN + TM) fragment reads up front, the next stage's NGW LDS-DMA pieces issued AFTER them in program order and
    // spread between the MFMAs (dc_sched_reads_mfma_dma in dc_kstage.h says why).
    bf16x8 wf[2][TN], xf[2][TM];
    auto load_frags = [&](int slot) {
        const char* sA = smem + slot * STAGE;
        const char* sB = sA + BM * 128;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int swz = dc_kstage_frag_off(s, fq, fr);
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) xf[s][tm] = *(const bf16x8*)(sA + ((wm * TM + tm) * 16 + fr) * 128 + swz);
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) wf[s][tn] = *(const bf16x8*)(sB + ((wn * TN + tn) * 16 + fr) * 128 + swz);
        }
    };
    auto mfma_frags = [&]() {
        dc_mfma_kstep(acc, wf, xf);
        dc_sched_reads_mfma_dma<2 * TN * TM, 2 * (TN + TM), NGW>();
    };

    // bias for this lane's output channels: fetched now so its latency hides under the K loop
    const int nb0 = n0 + wn * TN * 16 + 4 * fq;        // this lane's first output channel
    f32x4 bv[TN];
    dc_epi_load_cols<TN>(bv, d.bias, nb0, d.Cout);

    // LayerNorm folded into this linear (dc_conv_desc.ln_stats): this lane's rows' (mean, rstd) and the weight column sums,
    // fetched here next to the bias and first used in the epilogue, so the loads fly under the whole K loop (consuming them
    // here would put a full memory round trip in front of the first DMA stage of every workgroup)
    f32x2 ln_mr[TM] = {};
    f32x4 cs[TN] = {};
    if (e_ln) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            int m = m0 + (wm * TM + tm) * 16 + fr;
            m = m < M ? m : M - 1;
            ln_mr[tm] = *(const f32x2*)(d.ln_stats + (long long)m * 2);
        }
        dc_epi_load_cols<TN>(cs, d.ln_colsum, nb0, d.Cout);
    }

    // ---- pipeline
#pragma unroll
    for (int s = 0; s < NST - 1; ++s) issue_stage(kt_begin + s, s);
    for (int k = 0; k < nk; ++k) {
        dc_ring_sync<NGW * (NST - 2)>();               // this wave's pieces of stage k have landed and its reads of stage k-1 have
                                                      // returned; after the barrier: everyone else's too
        if (k == 0) DC_STAMP_AT(1);
        load_frags(k % NST);
        issue_stage(kt_begin + k + NST - 1, (k + NST - 1) % NST);
        mfma_frags();
    }
    wait_vmcnt<0>();
    DC_STAMP_AT(2);

    // ---- epilogue.  bf16 outputs go through LDS so that global stores (and residual loads) are whole 16-byte pieces of
    //      contiguous output rows: the MFMA layout gives each lane 4 channels of one pixel, i.e. 32-byte row fragments
    //      per store instruction; staged, every row leaves as BN*2 contiguous bytes.
    const bool staged = !GENERIC || (!d.out_f32 && d.splitk <= 1);   // specialised modes are staged by construction
    if (staged) {
        constexpr int OC = BN;                                  // staged columns (GEGLU halves it below)
        constexpr int PITCH = OC * 2 + 16;                      // bytes per staged row (+16: spread rows over banks)
        static_assert(BM * PITCH <= NST * STAGE, "output tile must fit in the stage buffers");
        __syncthreads();                                        // all waves are done reading the last stage
        DC_STAMP_AT(4);
        // all epilogue operands are fetched up front (independent loads in flight together): issued one (tm, tn) tile at
        // a time behind `if (bias)` / `if (residual)` they serialise into ~20 dependent L2 round trips per workgroup
        bf16x4 rr[TM][TN] = {};
        if (e_res && !e_geglu) dc_epi_load_residual<TM, TN>(rr, d.residual, m0 + wm * TM * 16 + fr, M, nb0, d.Cout);
        f32x4 gs[TN], gq[TN];                                   // GroupNorm partials over this wave's rows (gn_part_out)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) gs[tn] = gq[tn] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            const int row = (wm * TM + tm) * 16 + fr;
            const int m = m0 + row;
            const int nimg = e_rowadd ? (m < M ? m : M - 1) / HoWo : 0;
            if (e_geglu) {
#pragma unroll
                for (int tp = 0; tp < TN / 2; ++tp) {
                    *(bf16x4*)(smem + row * PITCH + (((((wn * TN + 2 * tp) * 16) / 2 + 4 * fq) * 2) ^ dc_stage_swz(row))) =
                        dc_epi_geglu(acc[2 * tp][tm], acc[2 * tp + 1][tm], e_flags, ln_mr[tm][0], ln_mr[tm][1], cs[2 * tp], cs[2 * tp + 1],
                                     bv[2 * tp], bv[2 * tp + 1]);
                }
            } else {
                float st1 = 0.f, st2 = 0.f;                     // partial (sum, sum of squares) of this output row: stats_out
                const float rowmask = m < M ? 1.f : 0.f;        // rows past M are clamped duplicates: keep them out of the sums
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) {
                    const int nl = (wn * TN + tn) * 16 + 4 * fq;
                    const int nb = n0 + nl;
                    const f32x4 v = dc_epi_plain_with(
                        acc[tn][tm], e_flags | (e_rowadd && nb < d.Cout ? DC_EPI_ROWADD : 0), e_act, ln_mr[tm][0], ln_mr[tm][1], cs[tn],
                        [&] { return bv[tn]; }, [&] { return *(const f32x4*)(d.row_add + (long long)nimg * d.row_add_stride + nb); }, d.out_scale,
                        [&] { return rr[tm][tn]; });
                    *(bf16x4*)(smem + row * PITCH + ((nl * 2) ^ dc_stage_swz(row))) = dc_pack_bf16x4(v);
                    if (GENERIC || EPI == 1 || EPI == 2) {      // the sums are a handful of FMAs: always formed, stored on request
                        dc_row_stats_add(st1, st2, v, nb < d.Cout ? 1.f : 0.f);
                        dc_gn_part_add(gs[tn], gq[tn], v, rowmask);
                    }
                }
                if (e_stats)
                    dc_row_stats_store(st1, st2, d.stats_out + ((long long)m * (2 * n_tiles) + tile_n * 2 + wn) * 2, fq == 0 && m < M);
            }
        }
        if (e_gnpart) {
            // chunk = (row tile within the sample, wave row); the launcher guarantees HoWo % BM == 0, so a tile has one sample
            const int n_img = m0 / HoWo;
            const int chunk = ((m0 - n_img * HoWo) / BM) * 2 + wm;
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const int nb = n0 + (wn * TN + tn) * 16 + 4 * fq;
                dc_gn_partial_store(gs[tn], gq[tn], d.gn_part_out + (((long long)chunk * d.N + n_img) * d.Cout + nb) * 2,
                                    fr == 0 && nb < d.Cout);
            }
        }
        DC_STAMP_AT(5);
        __syncthreads();
        DC_STAMP_AT(6);
        // cooperative store: consecutive lanes -> consecutive 16-byte pieces of one output row
        const int out_cols = e_geglu ? d.Cout >> 1 : d.Cout;
        const int col0 = e_geglu ? n0 >> 1 : n0;
        bf16_t* __restrict__ o = (bf16_t*)d.out;
        if (e_geglu) dc_stage_store_rows<BM, PITCH, OC / 16, 256>(smem, o, m0, M, col0, out_cols);     // 16-byte pieces per staged
        else dc_stage_store_rows<BM, PITCH, OC / 8, 256>(smem, o, m0, M, col0, out_cols);              // row: a compile-time divisor
        DC_STAMP_AT(3);
        return;
    }
    // ---- direct epilogue (fp32 outputs, split-K partials): the one igemm.hip runs
    dc_epi_direct<TM, TN>(acc, d, m0, n0, wm, wn, fr, fq);
}

template <int TM, int TN, int NST, int EPI>
int launch_gemm_e(const dc_conv_desc& d, hipStream_t st)
{
    constexpr int BM = 2 * TM * 16, BN = 2 * TN * 16;
    const int M = d.N * d.Ho * d.Wo;
    const int nblk = dc_cdiv(M, BM) * dc_cdiv(d.Cout, BN);
    const dim3 grid(nblk, d.splitk > 1 ? d.splitk : 1);
    const size_t lds = (size_t)NST * (BM + BN) * 128;
    auto kern = gemm_dma_kernel<TM, TN, NST, EPI>;
    static std::atomic<unsigned long long> attr_done{0};
    dc_set_max_dyn_lds((const void*)kern, (int)lds, attr_done);
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, d);
    return dc_launch_status();
}

// epilogue mode of a descriptor (see the kernel's EPI comment); 0 = the generic run-time-flag epilogue
int epi_mode(const dc_conv_desc& d)
{
    if (d.out_f32 || d.splitk > 1 || d.row_add || d.act) return 0;
    if (d.epilogue == 1) return (d.residual || d.stats_out || d.gn_part_out) ? 0 : (d.ln_stats ? 5 : 4);
    if (d.ln_stats) return (d.residual || d.stats_out || d.gn_part_out) ? 0 : 3;
    return d.residual ? 2 : 1;
}

template <int TM, int TN, int NST>
int launch_gemm(const dc_conv_desc& d, int epi, hipStream_t st)
{
    switch (epi) {
        case 1: return launch_gemm_e<TM, TN, NST, 1>(d, st);
        case 2: return launch_gemm_e<TM, TN, NST, 2>(d, st);
        case 3: return launch_gemm_e<TM, TN, NST, 3>(d, st);
        case 4: return launch_gemm_e<TM, TN, NST, 4>(d, st);
        case 5: return launch_gemm_e<TM, TN, NST, 5>(d, st);
        default: return launch_gemm_e<TM, TN, NST, 0>(d, st);
    }
}

}  // namespace

extern "C" int dc_gemm_row_stats_parts(int Cout) { return dc_row_stats_parts_rule(Cout); }

// The decision for a 1x1 descriptor: kernel, gemm_dma template (variant = TM*10000 + TN*1000 + stages*100 + A_REG*10 + PROD, where
// the A_REG digit is always 0 and the PROD digit always 1: kept so that recorded routes stay valid), epilogue mode, and whether the
// LayerNorm finalize runs first.  A GroupNorm affine on load exists in the row-panel kernel only: such a launch belongs to the family
// exactly when that kernel takes it (the gather GEMM of igemm.hip serves the others).
int dc_gemm_dma_route(const dc_conv_desc& d, dc_route& r)
{
    if (d.ksize != 1) return DC_ROUTE_PASS;
    r.epi = epi_mode(d);
    int rc = dc_gemm_rowpanel_route(d, r);
    if (rc == DC_ROUTE_PASS && d.gn_ab) {
        r.epi = 0;
        return DC_ROUTE_PASS;
    }
    // the folded LayerNorm and the row / GroupNorm statistics live in the staged (bf16, unsplit) epilogue only
    if ((d.ln_stats || d.stats_out || d.gn_part_out) && (d.out_f32 || d.splitk > 1)) return DC_ERR_INVALID;
    if (d.gn_part_out && (d.epilogue != 0 || d.ln_stats)) return DC_ERR_INVALID;
    if (rc != DC_ROUTE_PASS) return rc;
    if (d.ln_stats && d.ln_parts > 0) {
        // raw LayerNorm partials and a kernel whose waves do not own whole rows: the finalize pass runs first, into the
        // caller's scratch, and the launch proceeds on (mean, rstd) pairs — the same bits as finalizing beforehand
        dc_conv_desc q = d;
        if (q.ln_scratch) q.ln_stats = q.ln_scratch;
        q.ln_parts = 0;
        rc = dc_gemm_dma_route(q, r);
        r.ln_first = 1;
        return rc;
    }
    if (d.ln_stats && !d.ln_colsum) return DC_ERR_INVALID;
    rc = dc_gemm_p8_route(d, r);
    if (rc == DC_ROUTE_PASS) rc = dc_gemm_wide_route(d, r);
    if (rc != DC_ROUTE_PASS) return rc;
    if (d.stats_out && d.epilogue != 0) return DC_ERR_INVALID;
    const long long M = (long long)d.N * d.Ho * d.Wo, hw = (long long)d.Ho * d.Wo;
    const int bn = dc_n_tile(d), sk = d.splitk > 1 ? d.splitk : 1, KT = (d.C1 + d.C2) >> 6;
    const long long big = ((M + 127) / 128) * ((d.Cout + bn - 1) / bn) * sk;
    const long long small = ((M + 63) / 64) * ((d.Cout + bn - 1) / bn) * sk;
    r.kernel = DC_ROUTE_GEMM_DMA;
    r.tn = bn / 32;
    // 2 LDS stages for the big tiles keep two workgroups resident per CU (2 waves per SIMD: one computes while the
    // other waits for its DMA); the small tiles afford 3 stages at the same residency.
    // (Staging the activation tile through registers and only the weights by LDS-DMA was measured: no gain over all-DMA.)
    if (big >= 256) r.tm = 4, r.nst = 2;
    // Grids that cannot even put one workgroup on every CU (the 16x16 / 8x8 levels of a one- or two-frame decode) are bound by
    // the serial K loop: one LDS-DMA round trip per 64-wide step.  They take a deeper ring — the whole CU's LDS for one
    // workgroup, three or four stages in flight instead of one — with the same tile shape (so the statistics / GroupNorm partial
    // layouts are unchanged).  M = 512, N = 1280, K = 1280: 26 -> see tools/bench_gemm.py 2.
    else if (small <= 256 && KT >= 6) r.tm = 2, r.nst = bn == 160 ? 4 : 5;
    else r.tm = 2, r.nst = bn == 160 ? 2 : 3;
    r.variant = r.tm * 10000 + r.tn * 1000 + r.nst * 100 + 1;
    // GroupNorm partials: chunk = (row tile within the sample, wave row); a row tile must not straddle two samples
    if (d.gn_part_out && hw % (32 * r.tm) == 0) r.gn_chunks = (int)(hw / (32 * r.tm)) * 2;
    return DC_OK;
}

int dc_gemm_dma_launch(const dc_conv_desc& d, const dc_route& r, hipStream_t st)
{
    switch (r.variant) {
#define DC_DMA_VARIANT(TM, TN, NST) \
    case TM * 10000 + TN * 1000 + NST * 100 + 1: return launch_gemm<TM, TN, NST>(d, r.epi, st);
        DC_DMA_VARIANT(4, 5, 2)
        DC_DMA_VARIANT(4, 4, 2)
        DC_DMA_VARIANT(2, 5, 4)
        DC_DMA_VARIANT(2, 4, 5)
        DC_DMA_VARIANT(2, 5, 2)
        DC_DMA_VARIANT(2, 4, 3)
#undef DC_DMA_VARIANT
        default: return DC_ERR_INVALID;
    }
}
