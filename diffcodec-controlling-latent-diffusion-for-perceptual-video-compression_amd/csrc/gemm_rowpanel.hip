// Row-panel GEMM  out[m][n] = sum_k X[m][k] * W[n][k]  for K = 320 on gfx950: the 64x64-resolution linears of the SD-1.5
// transformer blocks (attn to_q/k/v with the folded LayerNorm, to_out + residual, GEGLU feed-forward, proj_in / proj_out; same
// call sites as gemm_dma.hip: flownet.py:87-124, pipeline.py:358-367) at model batches whose row count fills the chip.
//
// Why a separate kernel.  With K = 320 a tiled GEMM workgroup runs five K-steps between a prologue and an epilogue in which
// nothing is in flight, and both operand tiles stream through LDS once per output tile: the 128-row kernel reached 360-590
// TFLOP/s on these shapes with the matrix pipe 22 % busy (round-2 PMC), although every one of them is within 2x of its HBM
// floor.  Here the whole K of the ACTIVATION lives in registers instead:
//   * one 512-thread workgroup per CU owns a panel of 256 rows; wave w keeps its 32 rows x 320 of X as MFMA operand fragments
//     (80 VGPRs, loaded once straight from global memory) and walks over ALL output columns;
//   * only W streams through LDS: stages of 64 output columns x 320 (40 KB, N-major, so a stage is one contiguous block of the
//     [N][K] weight matrix) in a 3-deep LDS-DMA ring shared by the 8 waves, refilled across the whole column loop — one barrier
//     per stage, the ring never drains between "tiles"; the stage's 64 bias (and LayerNorm column-sum) floats ride in the same
//     slot.  LDS-fill bytes per FLOP are 1/256 (128-row tile kernel: 1/71), LDS reads 0.5 per MFMA, none for X;
//   * the epilogue of a stage (bias / folded LayerNorm / scale + residual / GEGLU, row statistics, GroupNorm partials) runs
//     right after that stage's 80 MFMAs on 32 accumulator registers, goes through a wave-private 4 KB staging area (no
//     workgroup barrier) and leaves as whole 128-byte row pieces, while the ring keeps prefetching;
//   * residual rows go by LDS-DMA too: at the top of their stage straight into the wave's staging area (row layout, whole
//     lines), where the epilogue picks them up in the MFMA layout and overwrites them in place with the outputs; a
//     one-dword-per-half-line DMA "touch" into a scratch corner two stages earlier has pulled them into L2 by then.  No load
//     of the loop has a VGPR destination: hipcc would drain the DMA ring with a vmcnt(0) at the first use of an ordinary
//     load's result, and it may copy the destination registers of an inline-asm load while the load is still in flight
//     (seen in the first build of this kernel: v_mov of the residual registers in front of the hand-placed wait).
// Every vector-memory operation of the loop is counted by hand: per stage and wave, in issue order,
//   [touch T] [residual pieces R] [W pieces P (+1 bias, +1 colsum piece on waves 0 / 1)] ... MFMAs ... [row stores F] [GN partials G]
// so the wait in front of the barrier that opens stage s (its pieces were issued two stages earlier) is
// vmcnt(P + T + R + 2 (F + G)) and the wait in front of the first read of the residual rows is vmcnt(P).
// The accumulators see the same k order as gemm_dma.hip (ten 32-wide steps in sequence, v_mfma_f32_16x16x32_bf16) and the
// epilogue arithmetic is the same expressions, so the bf16 outputs are bit-identical to the tile kernels'.
#include "dc_epilogue.h"
#include <cstdlib>
#include <type_traits>

// Developer-only phase stamps (tools/rowpanel_stamp.py builds this file with -DDC_STAMP into a scratch .so): s_memtime of wave 0
// of every workgroup at kernel entry / after the prologue / per stage after its barrier, after its MFMAs and after its epilogue,
// written to the (otherwise unused) split-K workspace.  Never defined in the product build.
#ifdef DC_STAMP
#define RP_STAMP_AT(i)                                                                         \
    do {                                                                                       \
        if (threadIdx.x == 0 && d.splitk_ws && (i) < 64) {                                     \
            unsigned long long t_;                                                             \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");         \
            ((unsigned long long*)d.splitk_ws)[(long long)blockIdx.x * 64 + (i)] = t_;         \
        }                                                                                      \
    } while (0)
#else
#define RP_STAMP_AT(i)
#endif

namespace {

constexpr int RP_K = 320;                          // the only K this kernel is built for
constexpr int RP_KS = RP_K / 32;                   // 32-wide MFMA k-steps
constexpr int RP_SC = 64;                          // output columns per stage
constexpr int RP_TN = RP_SC / 16, RP_TM = 2;       // 16x16 tiles per wave and stage: 4 (n) x 2 (m)
constexpr int RP_WBYTES = RP_SC * RP_K * 2;        // 40,960: the W rows of a stage
constexpr int RP_STAGE = RP_WBYTES + 512;          // + 64 bias floats + 64 colsum floats
constexpr int RP_NST = 3;
constexpr int RP_P = RP_WBYTES / 1024 / 8;         // 1 KB LDS-DMA pieces per wave and stage: 5
constexpr int RP_STG = 4096;                       // wave-private output staging: 32 rows x 128 B
constexpr int RP_TOUCH = 256;                      // wave-private landing pad of the touch DMA (never read)
constexpr int RP_LDS = RP_NST * RP_STAGE + 8 * RP_STG + 8 * RP_TOUCH;
static_assert(RP_LDS <= 160 * 1024, "LDS budget");

// EPI as in gemm_dma.hip: 1 bias, 2 bias + scale + residual, 3 folded LayerNorm + bias, 4 GEGLU, 5 folded LayerNorm + GEGLU.
// GN: GroupNorm partials of the output requested (modes 1-2) — compile-time because its stores enter the vmcnt arithmetic.
template <int EPI, bool GN>
__global__ __launch_bounds__(512, 2) void gemm_rowpanel_kernel(const dc_conv_desc d)
{
    constexpr bool e_geglu = EPI >= 4, e_ln = EPI == 3 || EPI == 5, e_res = EPI == 2;
    constexpr int T = e_res ? 1 : 0, R = e_res ? 4 : 0;
    // (the chain multiplies by out_scale even when it is 1.0f, which this kernel used to skip: x * 1.0f is x, and no register moved)
    constexpr int e_flags = (e_ln ? DC_EPI_LN : 0) | DC_EPI_BIAS | (e_res ? DC_EPI_RES : 0);
    constexpr int F = e_geglu ? 2 : 4, G = GN ? 2 * RP_TN : 0;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const int S = d.Cout / RP_SC;                                   // stages
    const long long mw = (long long)blockIdx.x * 256 + wave * 32;   // this wave's first row
    const bool e_stats = (EPI == 1 || EPI == 2) && d.stats_out != nullptr;
    const int extra = wave == 0 || (wave == 1 && e_ln);             // wave-uniform: one small DMA piece more per stage

    // ---- this wave's activation rows as MFMA B-operand fragments: xf[tm][k] = X[mw + 16 tm + fr][32 k + 8 fq .. + 8)
    bf16x8 xf[RP_TM][RP_KS];
#pragma unroll
    for (int tm = 0; tm < RP_TM; ++tm) {
        const char* p = (const char*)d.x1 + ((mw + tm * 16 + fr) * RP_K + fq * 8) * 2;
#pragma unroll
        for (int k = 0; k < RP_KS; ++k) xf[tm][k] = *(const bf16x8*)(p + k * 64);
    }
    if (d.gn_ab) {
        // GroupNorm affine on load (dc_conv_desc.gn_ab, no SiLU: the transformer's norm in front of proj_in): the panel lies inside one
        // sample, so every row takes the same (scale, shift) per channel; applied once to the register-resident fragments with the
        // arithmetic of the standalone pass (dc_gn_affine_pair) — the normalized tensor is never written or re-read.
        const long long hw = (long long)d.Ho * d.Wo;
        const float* __restrict__ abp = d.gn_ab + ((long long)((mw / hw) % d.gn_batch) * RP_K + fq * 8) * 2;
#pragma unroll
        for (int k = 0; k < RP_KS; ++k) {
            f32x4 g[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = *(const f32x4*)(abp + k * 64 + 4 * j);
#pragma unroll
            for (int tm = 0; tm < RP_TM; ++tm) {
                u32x4 v = *(const u32x4*)&xf[tm][k];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = dc_gn_affine_pair(v[j], g[j]);
                xf[tm][k] = *(const bf16x8*)&v;
            }
        }
    }
    f32x2 ln_mr[RP_TM] = {};
    if (e_ln) {
        if (d.ln_parts > 0) {                                       // raw partials: the finalize pass folded into this prologue — every
            dc_ln_row_partials rp[RP_TM];                           // row's pairs fetched first (loads in flight together), then summed
#pragma unroll
            for (int tm = 0; tm < RP_TM; ++tm) dc_ln_fetch_partials(rp[tm], d.ln_stats + (mw + tm * 16 + fr) * d.ln_parts * 2, d.ln_parts);
#pragma unroll
            for (int tm = 0; tm < RP_TM; ++tm) {
                float mean, rstd;
                dc_ln_mean_rstd(rp[tm], d.ln_parts, 1.0f / (float)RP_K, d.ln_eps, mean, rstd);
                ln_mr[tm] = f32x2{mean, rstd};
            }
        } else {
#pragma unroll
            for (int tm = 0; tm < RP_TM; ++tm) ln_mr[tm] = *(const f32x2*)(d.ln_stats + (mw + tm * 16 + fr) * 2);
        }
    }

    // ---- W stage image in LDS: 64 rows x 640 B, the row-panel layout of dc_kstage.h.  Piece g = 5 wave + i covers LDS bytes
    //      [1024 g, 1024 g + 1024): lane s lands at flat chunk 64 g + s = (row n, position q).
    int woff[RP_P];
#pragma unroll
    for (int i = 0; i < RP_P; ++i) {
        const int flat = (wave * RP_P + i) * 64 + lane;
        const int n = flat / 40, q = flat - n * 40;
        woff[i] = n * DC_RP_KROW + (dc_kstage_rp_src_chunk(q, n) << 4);
    }
    auto issue_w = [&](int s, int slot) {
        s = s < S ? s : S - 1;                                      // past-the-end stages re-read the last one into a dead slot
        const char* src = (const char*)d.w + (long long)s * RP_WBYTES;
        char* base = smem + slot * RP_STAGE;
#pragma unroll
        for (int i = 0; i < RP_P; ++i)              // (the builtin, not dc_dma16 / dc_dma4: see dc_kstage.h)
            __builtin_amdgcn_global_load_lds((dc_gptr_t)(src + woff[i]), (dc_lptr_t)(base + (wave * RP_P + i) * DC_KPIECE), 16, 0, 0);
        if (extra) {
            const float* v = (wave == 0 ? d.bias : d.ln_colsum) + s * RP_SC + lane;
            __builtin_amdgcn_global_load_lds((dc_gptr_t)v, (dc_lptr_t)(base + RP_WBYTES + wave * 256), 4, 0, 0);
        }
    };

    // fragment read addresses: W row 16 tn + fr, k-step k (dc_kstage_rp_frag_off: + (k >> 1) * 128 from the even / odd base)
    const int x7 = fr & 7;
    const int rd_even = fr * DC_RP_KROW + dc_kstage_rp_frag_off(0, fq, fr);
    const int rd_odd = fr * DC_RP_KROW + dc_kstage_rp_frag_off(1, fq, fr);

    // wave-private staging (non-GEGLU: 32 rows x 128 B; GEGLU: 32 rows x 64 B), bank-conflict-free for the 8-byte MFMA-layout
    // writes and the 16-byte row reads: chunk XOR row bits, 8-byte halves swapped on alternate 8-row groups (dc_stage_swz)
    char* stg = smem + RP_NST * RP_STAGE + wave * RP_STG;
    const bf16_t* __restrict__ resid = (const bf16_t*)d.residual;
    bf16_t* __restrict__ o = (bf16_t*)d.out;
    const int out_cols = e_geglu ? d.Cout >> 1 : d.Cout;

    float st1[RP_TM], st2[RP_TM];
#pragma unroll
    for (int tm = 0; tm < RP_TM; ++tm) st1[tm] = st2[tm] = 0.f;
    // residual rows by LDS-DMA: piece i = rows [8 i, 8 i + 8) of the wave's panel, lane l -> row 8 i + (l >> 3), staging chunk
    // position l & 7, which holds source chunk (l & 7) ^ (row & 7) (the staging swizzle; no half swap on the way in)
    const char* res_lane = nullptr;
    const char* touch_lane = nullptr;
    if (e_res) {
        res_lane = (const char*)resid + ((mw + (lane >> 3)) * d.Cout) * 2 + (((lane & 7) ^ ((lane >> 3) & 7)) << 4);
        touch_lane = (const char*)resid + ((mw + (lane & 31)) * d.Cout) * 2 + (lane >> 5) * 64;
    }

    // ---- prologue: two stages in flight, everything landed before the loop (so the steady-state counts hold from stage 1 on)
    RP_STAMP_AT(0);
    issue_w(0, 0);
    issue_w(1, 1);
    dc_ring_sync<0>();
    RP_STAMP_AT(1);
    for (int s = 0; s < S; ++s) {
        if (s > 0) {
            __builtin_amdgcn_sched_barrier(0);
            if (extra) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(RP_P + 1 + T + R + 2 * (F + G)) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(RP_P + T + R + 2 * (F + G)) : "memory");
            dc_wg_barrier();
        }
        RP_STAMP_AT(2 + 3 * s);
        // ---- top of the stage: touch (s+2), residual (s), W (s+2)
        if (e_res) {
            const int s2 = s + 2 < S ? s + 2 : S - 1;
            dc_dma4(touch_lane + s2 * (RP_SC * 2), smem + RP_NST * RP_STAGE + 8 * RP_STG + wave * RP_TOUCH);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                dc_dma16(res_lane + (long long)i * 8 * d.Cout * 2 + s * (RP_SC * 2), stg + i * 1024);
        }
        issue_w(s + 2, (s + 2) % RP_NST);

        // ---- 80 MFMAs: D[n][m] tiles, W fragments from the slot, X fragments from registers
        const char* sb = smem + (s % RP_NST) * RP_STAGE;
        f32x4 acc[RP_TN][RP_TM];
#pragma unroll
        for (int tn = 0; tn < RP_TN; ++tn)
#pragma unroll
            for (int tm = 0; tm < RP_TM; ++tm) acc[tn][tm] = f32x4{0.f, 0.f, 0.f, 0.f};
        // fragment reads run one k-step ahead of the MFMAs that consume them (two register sets)
        bf16x8 wf[2][RP_TN];
        auto read_w = [&](int k, bf16x8* dst) {
#pragma unroll
            for (int tn = 0; tn < RP_TN; ++tn)
                dst[tn] = *(const bf16x8*)(sb + ((k & 1) ? rd_odd : rd_even) + tn * 10240 + (k >> 1) * 128);
        };
        read_w(0, wf[0]);
        __builtin_amdgcn_sched_group_barrier(0x100, RP_TN, 0);      // (the scheduler fills groups in order: name this one too)
#pragma unroll
        for (int k = 0; k < RP_KS; ++k) {
            if (k + 1 < RP_KS) read_w(k + 1, wf[(k + 1) & 1]);
#pragma unroll
            for (int tn = 0; tn < RP_TN; ++tn)
#pragma unroll
                for (int tm = 0; tm < RP_TM; ++tm)
                    acc[tn][tm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[k & 1][tn], xf[tm][k], acc[tn][tm], 0, 0, 0);
            if (k + 1 < RP_KS) __builtin_amdgcn_sched_group_barrier(0x100, RP_TN, 0);       // the next step's reads first ...
            __builtin_amdgcn_sched_group_barrier(0x008, RP_TN * RP_TM, 0);                  // ... then this step's MFMAs
        }
        RP_STAMP_AT(3 + 3 * s);

        // ---- epilogue of the stage
        f32x4 bv[RP_TN], cs[RP_TN] = {};
#pragma unroll
        for (int tn = 0; tn < RP_TN; ++tn) {
            bv[tn] = *(const f32x4*)(sb + RP_WBYTES + (tn * 16 + 4 * fq) * 4);
            if (e_ln) cs[tn] = *(const f32x4*)(sb + RP_WBYTES + 256 + (tn * 16 + 4 * fq) * 4);
        }
        if (e_res) {                                                // this wave's residual pieces of the stage have landed
            __builtin_amdgcn_sched_barrier(0);
            if (extra) wait_vmcnt<RP_P + 1>();
            else wait_vmcnt<RP_P>();
            __builtin_amdgcn_sched_barrier(0);
        }
        f32x4 gs[RP_TN], gq[RP_TN];
#pragma unroll
        for (int tn = 0; tn < RP_TN; ++tn) gs[tn] = gq[tn] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tm = 0; tm < RP_TM; ++tm) {
            const int row = tm * 16 + fr;
            if (e_geglu) {
#pragma unroll
                for (int tp = 0; tp < RP_TN / 2; ++tp) {
                    const bf16x4 pk = dc_epi_geglu(acc[2 * tp][tm], acc[2 * tp + 1][tm], e_flags, ln_mr[tm][0], ln_mr[tm][1], cs[2 * tp],
                                                   cs[2 * tp + 1], bv[2 * tp], bv[2 * tp + 1]);
                    const int chunk = (tp * 2 + (fq >> 1)) ^ ((row >> 1) & 3);
                    const int half = (fq & 1) ^ ((row >> 3) & 1);
                    *(bf16x4*)(stg + row * 64 + chunk * 16 + half * 8) = pk;
                }
            } else {
#pragma unroll
                for (int tn = 0; tn < RP_TN; ++tn) {
                    const int chunk = (tn * 2 + (fq >> 1)) ^ x7;
                    bf16x4 rr = {};
                    if (e_res) rr = *(const bf16x4*)(stg + row * 128 + chunk * 16 + (fq & 1) * 8);
                    const f32x4 v = dc_epi_plain(acc[tn][tm], e_flags, 0, ln_mr[tm][0], ln_mr[tm][1], cs[tn], bv[tn], f32x4{0.f, 0.f, 0.f, 0.f},
                                                 d.out_scale, rr);
                    const int half = (fq & 1) ^ ((row >> 3) & 1);
                    *(bf16x4*)(stg + row * 128 + chunk * 16 + half * 8) = dc_pack_bf16x4(v);
                    if (EPI == 1 || EPI == 2) {
                        if (e_stats) dc_row_stats_add(st1[tm], st2[tm], v, 1.f);
                        if (GN) dc_gn_part_add(gs[tn], gq[tn], v, 1.f);
                    }
                }
            }
        }
        // rows out: consecutive lanes -> consecutive 16-byte pieces of one output row (whole 128-byte lines; 64 B for GEGLU)
        if (e_geglu) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = (lane >> 2) + 16 * i, c = lane & 3;
                u32x4 v = *(const u32x4*)(stg + row * 64 + ((c ^ ((row >> 1) & 3)) << 4));
                if ((row >> 3) & 1) v = u32x4{v[2], v[3], v[0], v[1]};
                *(u32x4*)(o + (mw + row) * out_cols + s * (RP_SC / 2) + c * 8) = v;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = (lane >> 3) + 8 * i, c = lane & 7;
                u32x4 v = *(const u32x4*)(stg + row * 128 + ((c ^ (row & 7)) << 4));
                if (i & 1) v = u32x4{v[2], v[3], v[0], v[1]};
                *(u32x4*)(o + (mw + row) * out_cols + s * RP_SC + c * 8) = v;
            }
        }
        RP_STAMP_AT(4 + 3 * s);
        if (GN) {
            // chunk = 32 rows (one wave); the launcher guarantees HoWo % 256 == 0, so a panel lies inside one sample
            const long long hw = (long long)d.Ho * d.Wo;
            const int n_img = (int)(mw / hw);
            const int chunk = (int)((mw - n_img * hw) >> 5);
#pragma unroll
            for (int tn = 0; tn < RP_TN; ++tn) {
                const int nb = s * RP_SC + tn * 16 + 4 * fq;
                dc_gn_partial_store(gs[tn], gq[tn], d.gn_part_out + (((long long)chunk * d.N + n_img) * d.Cout + nb) * 2, fr == 0);
            }
        }
    }
    if (e_stats) {
        // a wave owns whole rows: part 0 carries the row's (sum, sum of squares), the other parts the launcher promised are zero
        const int parts = dc_row_stats_parts_rule(d.Cout);
#pragma unroll
        for (int tm = 0; tm < RP_TM; ++tm) {
            float a = st1[tm], b = st2[tm];
            dc_row_stats_reduce(a, b);
            float* dst = d.stats_out + (mw + tm * 16 + fr) * parts * 2;
            for (int p = fq; p < parts; p += 4) *(f32x2*)(dst + p * 2) = p == 0 ? f32x2{a, b} : f32x2{0.f, 0.f};
        }
    }
}

template <int EPI, bool GN>
int launch_rowpanel(const dc_conv_desc& d, hipStream_t st)
{
    const long long M = (long long)d.N * d.Ho * d.Wo;
    auto kern = gemm_rowpanel_kernel<EPI, GN>;
    static std::atomic<unsigned long long> attr_done{0};
    dc_set_max_dyn_lds((const void*)kern, RP_LDS, attr_done);
    hipLaunchKernelGGL(kern, dim3((unsigned)(M / 256)), dim3(512), RP_LDS, st, d);
    return dc_launch_status();
}

}  // namespace

// Takes a launch when K = 320 (one source; load-side transform: none, or a GroupNorm affine without SiLU), a specialised epilogue mode applies, the columns split
// into whole 64-wide stages and the row panels fill the chip (>= one workgroup per CU).  Never depends on whether the optional
// statistics outputs are set, so that the chunk query and the launch agree.
int dc_gemm_rowpanel_route(const dc_conv_desc& d, dc_route& r)
{
    const int epi = r.epi;
    if (epi < 1 || epi > 5 || d.ksize != 1 || d.splitk > 1 || d.out_f32) return DC_ROUTE_PASS;
    if (d.gn_ab && (d.gn_silu || d.gn_batch <= 0)) return DC_ROUTE_PASS;   // the affine on load only (the X prologue has no SiLU)
    if (d.ln_parts > DC_LN_PARTS_MAX) return DC_ROUTE_PASS;            // (the dispatcher finalizes first and comes back with pairs)
    if (d.C1 != RP_K || d.C2 != 0 || d.x2 || !d.bias) return DC_ROUTE_PASS;
    const long long M = (long long)d.N * d.Ho * d.Wo, hw = (long long)d.Ho * d.Wo;
    if (M % 256 || M < 256 * 256) return DC_ROUTE_PASS;
    if (d.Cout % RP_SC || d.Cout < 5 * RP_SC) return DC_ROUTE_PASS;
    if (hw % 256) return DC_ROUTE_PASS;                     // GroupNorm partials need a panel inside one sample
    if ((epi == 3 || epi == 5) && !d.ln_colsum) return DC_ERR_INVALID;
    r.kernel = DC_ROUTE_GEMM_ROWPANEL;
    r.gn = d.gn_part_out != nullptr;                        // (epilogue modes 1 / 2 only: the others are never chosen with gn_part_out)
    if (r.gn) r.gn_chunks = (int)(hw / 32);                 // GroupNorm partials: one chunk per 32-row wave panel
    return DC_OK;
}

int dc_gemm_rowpanel_launch(const dc_conv_desc& d, const dc_route& r, hipStream_t st)
{
    switch (r.epi) {
        case 1: return r.gn ? launch_rowpanel<1, true>(d, st) : launch_rowpanel<1, false>(d, st);
        case 2: return r.gn ? launch_rowpanel<2, true>(d, st) : launch_rowpanel<2, false>(d, st);
        case 3: return launch_rowpanel<3, false>(d, st);
        case 4: return launch_rowpanel<4, false>(d, st);
        case 5: return launch_rowpanel<5, false>(d, st);
        default: return DC_ERR_INVALID;
    }
}
