// Wide-tile GEMM  out[m][n] = sum_k X[m][k] * W[n][k]  for gfx950: the long-K 1x1 / linear launches (attention out-projections,
// feed-forward, time-embedding-free shortcuts; same call sites as gemm_dma.hip) where the 128-row kernel is bound by the
// bytes it pulls through the CU's vector-memory path, not by the matrix pipe (gemm_dma with the K-loop DMA switched off ran
// 1.15-1.65x faster on these shapes: tools/ab experiment of round 2).
//
// One 512-thread workgroup per CU owns a 256 x BN output tile (BN = 160 | 128): 28 % fewer operand bytes per FLOP than two
// 128-row workgroups, which is what the LDS-DMA path is short of.  With a single workgroup per CU nothing overlaps for free,
// so the two halves of the workgroup are run in anti-phase ("ping-pong"):
//   group 0 = waves 0-3 (rows 0-127), group 1 = waves 4-7 (rows 128-255); each group is a 2(m) x 2(n) arrangement of
//   64 x (BN/2) wave tiles — the per-wave code of gemm_dma.hip;
//   a K-step of a wave is  [barrier] L: fragment reads + its share of the LDS-DMA for stage k+2  [barrier] M: the MFMAs;
//   group 1 passes one extra barrier up front, so while one group computes the other loads: each SIMD hosts one wave of
//   each group, its matrix pipe always has a wave in its M phase, and LDS reads / DMA issue hide behind the partner's MFMAs.
// Ring of 3 stages (the whole 160 KB of LDS).  Hazards, with I(2k) / I(2k+1) the barrier intervals in which group 0 / 1 read
// stage k:  RAW — every wave waits for its own pieces of stage k+1 (counted vmcnt, stage k+2 stays in flight) and for its
// fragment reads (lgkmcnt(0)) at the END of its L phase, i.e. before the barrier that precedes every read of stage k+1 by
// either group;  WAR — stage k+2 reuses the slot of stage k-1, whose last reads (group 1, I(2k-1)) are retired by that
// same lgkmcnt(0) before the barrier that opens I(2k), the earliest interval in which a piece of stage k+2 is issued.
// No DMA is issued past the last stage (the epilogue stages its rows through the ring's LDS), so the final waits are vmcnt(0).
#include "dc_epilogue.h"
#include <cstdlib>
#include <type_traits>

namespace {

// EPI as in gemm_dma.hip: 1 bias, 2 bias + scale + residual, 3 folded LayerNorm + bias, 4 GEGLU, 5 folded LayerNorm + GEGLU.
// ST (EPI 1 / 2): bit 0 = LayerNorm row statistics of the output requested (`stats_out`), bit 1 = GroupNorm partials (`gn_part_out`).
// A compile-time choice: the sums cost 24 vector operations per 16 x 16 block (480 per wave and tile), most launches of this kernel
// request one kind or none (the feed-forward down-projection), and run-time branches around them inside the unrolled epilogue make
// hipcc spill thousands of dwords.
template <int TN, int EPI, int ST>
__global__ __launch_bounds__(512, 2) void gemm_wide_kernel(const dc_conv_desc d)
{
    constexpr int TM = 4, NST = 3;
    constexpr int BM = 256, BN = 2 * TN * 16;
    constexpr int ROWS = BM + BN;
    constexpr int STAGE = ROWS * 128;
    constexpr int NP = ROWS / 8;                      // LDS-DMA pieces (8 rows x 128 B) per stage
    constexpr int PMAX = (NP + 7) / 8;                // pieces per wave (waves with index < NP % 8 issue PMAX, the rest PMAX - 1)
    constexpr bool e_geglu = EPI >= 4, e_ln = EPI == 3 || EPI == 5, e_res = EPI == 2;
    static_assert(NP % 8 == 0 || NP % 8 == 4, "the two wave groups must be uniform in their piece count");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;                        // 0: rows 0-127, 1: rows 128-255
    const int wm = wave & 1, wn = (wave >> 1) & 1;
    const int fr = lane & 15, fq = lane >> 4;
    const int wrow = grp * 128 + wm * TM * 16;        // first row of this wave's tiles inside the workgroup tile
    static_assert(ST == 0 || EPI == 1 || EPI == 2, "statistics ride on the bias / residual epilogues only");
    constexpr bool e_stats = (ST & 1) != 0, e_gnpart = (ST & 2) != 0;
    constexpr int e_flags = (e_ln ? DC_EPI_LN : 0) | DC_EPI_BIAS | (e_res ? DC_EPI_RES : 0);

    const int HoWo = d.Ho * d.Wo;
    const int M = d.N * HoWo;
    const int K = d.C1 + d.C2;
    const int nk = K >> 6;
    const int n_tiles = (d.Cout + BN - 1) / BN;
    const int m_tiles = (M + BM - 1) / BM;
    const int nblk = n_tiles * m_tiles;
    const int bid = dc_xcd_remap(blockIdx.x, nblk);
    const int tile_n = bid % n_tiles, tile_m = bid / n_tiles;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    // ---- per-lane DMA sources: piece g = wave + 8 i of the stage (dc_kstage.h)
    //      Addresses are a workgroup-uniform base (SGPRs: tile origin of the operand) + a 32-bit per-lane offset that also carries the K
    //      offset of the stage (one v_add_u32 per piece; a 64-bit per-lane pointer costs two registers and a 64-bit vector add per piece,
    //      issued while the partner group's MFMAs hold the vector port — gemm_p8.hip measured 2-3 % for the same change).
    uint32_t off1[PMAX], off2[PMAX];
    const int c1_steps = d.C1 >> 6;
    const int my_pieces = (NP - wave + 7) / 8;        // wave-uniform: PMAX or PMAX - 1
    const char* const bx1 = (const char*)d.x1 + (long long)m0 * d.C1 * 2;
    const char* const bx2 = d.x2 ? (const char*)d.x2 + (long long)m0 * d.C2 * 2 : nullptr;
    const char* const bw = (const char*)d.w + (long long)n0 * K * 2;
#pragma unroll
    for (int i = 0; i < PMAX; ++i) {
        int g = wave + 8 * i;
        g = g < NP ? g : NP - 1;
        const int row = g * 8 + (lane >> 3);
        const int chunk = dc_kstage_src_chunk(lane, row);
        if (row < BM) {
            int m = m0 + row;
            m = m < M ? m : M - 1;                    // clamp: rows past M are computed and discarded
            off1[i] = (uint32_t)((m - m0) * d.C1 + chunk * 8) * 2u;
            off2[i] = (uint32_t)((m - m0) * d.C2 + chunk * 8) * 2u;
        } else {
            int n = n0 + row - BM;
            n = n < d.Cout ? n : d.Cout - 1;
            off1[i] = (uint32_t)((n - n0) * K + chunk * 8) * 2u;
            off2[i] = 0;
        }
    }
    auto issue_stage = [&](int kt, int slot) {
        char* base = smem + slot * STAGE;
        const bool second = kt >= c1_steps;
        const uint32_t ko1 = (uint32_t)kt * 128u, ko2 = (uint32_t)(kt - c1_steps) * 128u;
#pragma unroll
        for (int i = 0; i < PMAX; ++i) {
            if (i == PMAX - 1 && my_pieces < PMAX) break;                        // wave-uniform
            const int g = wave + 8 * i;
            const bool is_a = g * 8 < BM;                                        // wave-uniform
            const char* p = is_a ? ((second ? bx2 : bx1) + (size_t)(uint32_t)((second ? off2[i] : off1[i]) + (second ? ko2 : ko1)))
                                 : (bw + (size_t)(uint32_t)(off1[i] + ko1));
            dc_dma16(p, base + g * DC_KPIECE);
        }
    };

    f32x4 acc[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    bf16x8 wf[2][TN], xf[2][TM];
    auto load_frags = [&](int slot) {
        const char* sA = smem + slot * STAGE;
        const char* sB = sA + BM * 128;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int swz = dc_kstage_frag_off(s, fq, fr);
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) xf[s][tm] = *(const bf16x8*)(sA + (wrow + tm * 16 + fr) * 128 + swz);
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) wf[s][tn] = *(const bf16x8*)(sB + ((wn * TN + tn) * 16 + fr) * 128 + swz);
        }
    };
    auto mfma_frags = [&]() {
        __builtin_amdgcn_s_setprio(1);
        dc_mfma_kstep(acc, wf, xf);
        __builtin_amdgcn_s_setprio(0);
    };

    // bias / LayerNorm operands for this lane's outputs: fetched now, first used in the epilogue
    const int nb0 = n0 + wn * TN * 16 + 4 * fq;       // this lane's first output channel
    f32x4 bv[TN];
    dc_epi_load_cols<TN>(bv, d.bias, nb0, d.Cout);
    f32x2 ln_mr[TM] = {};
    f32x4 cs[TN] = {};
    if (e_ln) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            int m = m0 + wrow + tm * 16 + fr;
            m = m < M ? m : M - 1;
            ln_mr[tm] = *(const f32x2*)(d.ln_stats + (long long)m * 2);
        }
        dc_epi_load_cols<TN>(cs, d.ln_colsum, nb0, d.Cout);
    }
    // the operand loads above are ordinary VMEM operations in front of the DMA pieces in this wave's queue: retire them now so
    // that the counted waits below see DMA pieces only
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- pipeline.  P = this wave's pieces per stage; the two groups differ when NP is not a multiple of 8.
    auto pipeline = [&](auto pc) {
        constexpr int P = decltype(pc)::value;
        issue_stage(0, 0);
        if (nk > 1) issue_stage(1, 1);
        if (nk > 1) dc_wait_vm_lgkm<P>();
        else dc_wait_vm_lgkm<0>();                       // this wave's pieces of stage 0 have landed
        if (grp == 1) dc_wg_barrier();                   // the extra barrier that puts group 1 half a K-step behind group 0
        for (int k = 0; k < nk; ++k) {
            dc_wg_barrier();                             // opens this group's L phase: every wave's pieces of stage k have landed
            load_frags(k % NST);
            const bool more = k + 2 < nk;
            if (more) issue_stage(k + 2, (k + 2) % NST);
            if (more) dc_wait_vm_lgkm<P>();              // own pieces of stage k+1 landed (stage k+2 stays in flight), reads returned
            else dc_wait_vm_lgkm<0>();
            dc_wg_barrier();                             // opens this group's M phase (and the other group's L phase)
            mfma_frags();
        }
        if (grp == 0) dc_wg_barrier();                   // pairs with group 1's last L-to-M barrier
    };
    if (my_pieces == PMAX) pipeline(std::integral_constant<int, PMAX>{});
    else pipeline(std::integral_constant<int, PMAX - 1>{});

    // ---- epilogue: rows staged through LDS (every DMA has landed, every fragment read has returned: see the header), then
    //      written as whole 16-byte pieces of contiguous output rows.  Group 0 arrives while group 1 still runs its last MFMAs,
    //      which touch no LDS.
    constexpr int OC = BN;
    constexpr int PITCH = OC * 2 + 16;
    static_assert(BM * PITCH <= NST * STAGE, "output tile must fit in the stage buffers");
    bf16x4 rr[TM][TN] = {};
    if (e_res) dc_epi_load_residual<TM, TN>(rr, d.residual, m0 + wrow + fr, M, nb0, d.Cout);
    f32x4 gs[TN], gq[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) gs[tn] = gq[tn] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        const int row = wrow + tm * 16 + fr;
        const int m = m0 + row;
        if (e_geglu) {
#pragma unroll
            for (int tp = 0; tp < TN / 2; ++tp) {
                *(bf16x4*)(smem + row * PITCH + (((((wn * TN + 2 * tp) * 16) / 2 + 4 * fq) * 2) ^ dc_stage_swz(row))) =
                    dc_epi_geglu(acc[2 * tp][tm], acc[2 * tp + 1][tm], e_flags, ln_mr[tm][0], ln_mr[tm][1], cs[2 * tp], cs[2 * tp + 1],
                                 bv[2 * tp], bv[2 * tp + 1]);
            }
        } else {
            float st1 = 0.f, st2 = 0.f;
            const float rowmask = m < M ? 1.f : 0.f;
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const int nl = (wn * TN + tn) * 16 + 4 * fq;
                const int nb = n0 + nl;
                const f32x4 v = dc_epi_plain(acc[tn][tm], e_flags, 0, ln_mr[tm][0], ln_mr[tm][1], cs[tn], bv[tn], f32x4{0.f, 0.f, 0.f, 0.f},
                                             d.out_scale, rr[tm][tn]);
                *(bf16x4*)(smem + row * PITCH + ((nl * 2) ^ dc_stage_swz(row))) = dc_pack_bf16x4(v);
                if (e_stats) dc_row_stats_add(st1, st2, v, nb < d.Cout ? 1.f : 0.f);      // compile-time
                if (e_gnpart) dc_gn_part_add(gs[tn], gq[tn], v, rowmask);
            }
            if (e_stats) dc_row_stats_store(st1, st2, d.stats_out + ((long long)m * (2 * n_tiles) + tile_n * 2 + wn) * 2, fq == 0 && m < M);
        }
        __builtin_amdgcn_sched_barrier(0);            // one row group at a time (register pressure)
    }
    if (e_gnpart) {
        // chunks of 64 rows (one wave row): the launcher guarantees HoWo % 256 == 0, so a tile has one sample
        const int n_img = m0 / HoWo;
        const int chunk = ((m0 - n_img * HoWo) / 64) + grp * 2 + wm;
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int nb = n0 + (wn * TN + tn) * 16 + 4 * fq;
            dc_gn_partial_store(gs[tn], gq[tn], d.gn_part_out + (((long long)chunk * d.N + n_img) * d.Cout + nb) * 2,
                                fr == 0 && nb < d.Cout);
        }
    }
    __syncthreads();
    const int out_cols = e_geglu ? d.Cout >> 1 : d.Cout;
    const int col0 = e_geglu ? n0 >> 1 : n0;
    bf16_t* __restrict__ o = (bf16_t*)d.out;
    dc_stage_store_rows<BM, PITCH, (e_geglu ? OC / 16 : OC / 8), 512>(smem, o, m0, M, col0, out_cols);      // 16-byte pieces per staged row
}

template <int TN, int EPI, int ST>
int launch_wide_st(const dc_conv_desc& d, hipStream_t st)
{
    constexpr int BN = 2 * TN * 16;
    const int M = d.N * d.Ho * d.Wo;
    const int nblk = dc_cdiv(M, 256) * dc_cdiv(d.Cout, BN);
    const size_t lds = (size_t)3 * (256 + BN) * 128;
    auto kern = gemm_wide_kernel<TN, EPI, ST>;
    static std::atomic<unsigned long long> attr_done{0};
    dc_set_max_dyn_lds((const void*)kern, (int)lds, attr_done);
    hipLaunchKernelGGL(kern, dim3(nblk), dim3(512), lds, st, d);
    return dc_launch_status();
}

template <int TN, int EPI>
int launch_wide(const dc_conv_desc& d, int stats, hipStream_t st)
{
    if constexpr (EPI == 1 || EPI == 2) {
        switch (stats) {
            case 1: return launch_wide_st<TN, EPI, 1>(d, st);
            case 2: return launch_wide_st<TN, EPI, 2>(d, st);
            case 3: return launch_wide_st<TN, EPI, 3>(d, st);
            default: return launch_wide_st<TN, EPI, 0>(d, st);
        }
    } else {
        return launch_wide_st<TN, EPI, 0>(d, st);
    }
}

}  // namespace

// The wide kernel takes a launch when the specialised epilogue modes apply, K is long enough for the 3-stage ring to pay for
// the unoverlapped prologue / epilogue of a one-workgroup-per-CU kernel, and the tile grid fills the chip.
int dc_gemm_wide_route(const dc_conv_desc& d, dc_route& r)
{
    constexpr int min_k = 640;
    const int epi = r.epi;
    if (epi < 1 || epi > 5 || d.ksize != 1 || d.gn_ab || d.splitk > 1 || d.out_f32) return DC_ROUTE_PASS;
    const int K = d.C1 + d.C2;
    const long long M = (long long)d.N * d.Ho * d.Wo, hw = (long long)d.Ho * d.Wo;
    const int bn = dc_n_tile(d);
    if (d.Cout % bn) return DC_ROUTE_PASS;                  // whole N tiles only (the 128-row kernel clamps ragged ones)
    if ((d.stats_out || d.gn_part_out) && hw % 256) return DC_ROUTE_PASS;
    const long long tiles = ((M + 255) / 256) * (d.Cout / bn);
    // measured (tools/bench_gemm.py, same box, model batch 32): +4..13 % for K 640-2560, 0..-2 % at K 640 x N 640, -4 % at K 5120
    if (!(K >= min_k && K <= 2560 && M % 256 == 0 && tiles >= 192)) return DC_ROUTE_PASS;
    r.kernel = DC_ROUTE_GEMM_WIDE;
    r.tn = bn / 32;
    r.st = epi <= 2 ? (d.stats_out ? 1 : 0) | (d.gn_part_out ? 2 : 0) : 0;
    if (d.gn_part_out) r.gn_chunks = (int)(hw / 64);        // GroupNorm partials: one chunk per 64-row wave row
    return DC_OK;
}

int dc_gemm_wide_launch(const dc_conv_desc& d, const dc_route& r, hipStream_t st)
{
    const bool n160 = r.tn == 5;
    switch (r.epi) {
        case 1: return n160 ? launch_wide<5, 1>(d, r.st, st) : launch_wide<4, 1>(d, r.st, st);
        case 2: return n160 ? launch_wide<5, 2>(d, r.st, st) : launch_wide<4, 2>(d, r.st, st);
        case 3: return n160 ? launch_wide<5, 3>(d, r.st, st) : launch_wide<4, 3>(d, r.st, st);
        case 4: return launch_wide<4, 4>(d, r.st, st);
        case 5: return launch_wide<4, 5>(d, r.st, st);
        default: return DC_ERR_INVALID;
    }
}
