// The ONE epilogue of the six bf16 matrix kernels (gemm_dma.hip, gemm_wide.hip, gemm_p8.hip, gemm_rowpanel.hip, igemm.hip,
// conv3x3_tile.hip): what happens to one lane's f32x4 accumulator fragment (4 consecutive output channels of one pixel row) between
// the last MFMA and the store, written once, so that every kernel rounds in the same order and gives the same bits
//
//     LN fold -> + bias -> + row_add -> act -> * out_scale | * out_scale + residual -> bf16
//
// plus the LayerNorm row-statistics and GroupNorm partial sums taken from the fp32 values on the way.  The functions own no tiling,
// no LDS addressing and no loop over (tm, tn): those stay in the kernels, whose layouts differ.  The leaves (dc_ln_fold,
// dc_scale_res, dc_act, dc_gelu_erf) are in dc_common.h with their contraction pragmas; nothing else in the chain is a multiply
// feeding an add, so the chain itself has nothing the compiler could fuse differently from one call site to the next.  The sums of
// dc_row_stats_add / dc_gn_part_add DO contract (v * v + ...): they carry no pragma, exactly as the kernels wrote them, and the fused
// forms are pinned per instance by tests/test_gpu_conv_bits.py.
#pragma once
#include "dc_conv_route.h"
#include "dc_kstage.h"                       // the other half of each kernel: the K loop's operand stage

// which steps of the chain run: compile-time constants in the specialised epilogues (the call folds to straight-line code), run-time
// values in the generic ones
enum { DC_EPI_LN = 1, DC_EPI_BIAS = 2, DC_EPI_ROWADD = 4, DC_EPI_RES = 8 };

// The plain chain -> the fp32 values about to be rounded (or stored, for out_f32).  bias / row_add / residual are callables that
// return the operand: a step that is off never evaluates its own, so a generic epilogue hands in the load itself and keeps its
// one-branch-per-flag shape (operands selected against zero instead cost the gather GEMM 330 vector instructions per wave).
// The GEMMs add bias, then row_add.  conv3x3_tile.hip ALONE pre-sums the two per channel (bias + row_add, once per workgroup
// instead of once per pixel) and passes the sum as `bias` without DC_EPI_ROWADD: acc + (bias + row_add) rounds differently from
// (acc + bias) + row_add, and its outputs are pinned to that order.
template <class FB, class FA, class FR>
__device__ __forceinline__ f32x4 dc_epi_plain_with(f32x4 v, int flags, int act, float mean, float rstd, f32x4 colsum, FB bias, FA row_add,
                                                   float out_scale, FR residual)
{
    if (flags & DC_EPI_LN) v = dc_ln_fold(v, mean, rstd, colsum);
    if (flags & DC_EPI_BIAS) v += bias();
    if (flags & DC_EPI_ROWADD) v += row_add();
    if (act) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = dc_act(v[r], act);
    }
    if (flags & DC_EPI_RES) v = dc_scale_res(v, out_scale, residual());
    else v *= out_scale;
    return v;
}
// the same on operands already in registers (the prefetching epilogues)
__device__ __forceinline__ f32x4 dc_epi_plain(f32x4 v, int flags, int act, float mean, float rstd, f32x4 colsum, f32x4 bias, f32x4 row_add,
                                              float out_scale, bf16x4 residual)
{
    return dc_epi_plain_with(v, flags, act, mean, rstd, colsum, [&] { return bias; }, [&] { return row_add; }, out_scale, [&] { return residual; });
}

__device__ __forceinline__ bf16x4 dc_pack_bf16x4(f32x4 v)
{
    bf16x4 pk;
#pragma unroll
    for (int r = 0; r < 4; ++r) pk[r] = (bf16_t)v[r];
    return pk;
}

// The GEGLU chain of a (value, gate) fragment pair: LN fold -> + bias -> value * gelu(gate) -> bf16
// Its vector operands come in by const reference ON PURPOSE: taken by value, hipcc's SLP pass vectorizes the chain 4-wide instead
// of 2-wide after inlining and schedules the row-panel LayerNorm + GEGLU epilogue 2 % slower (M = 131072, N = 2560: 37.5 -> 38.3 ms
// per step; the same bits).  By reference both row-panel GEGLU instances are the instruction stream of the hand-written chain.
__device__ __forceinline__ bf16x4 dc_epi_geglu(const f32x4& acc_h, const f32x4& acc_g, int flags, float mean, float rstd, const f32x4& cs_h,
                                               const f32x4& cs_g, const f32x4& bias_h, const f32x4& bias_g)
{
    f32x4 h = acc_h, g = acc_g;
    if (flags & DC_EPI_LN) {
        h = dc_ln_fold(h, mean, rstd, cs_h);
        g = dc_ln_fold(g, mean, rstd, cs_g);
    }
    if (flags & DC_EPI_BIAS) {
        h += bias_h;
        g += bias_g;
    }
    bf16x4 pk;
#pragma unroll
    for (int r = 0; r < 4; ++r) pk[r] = (bf16_t)(h[r] * dc_gelu_erf(g[r]));
    return pk;
}

// LayerNorm row statistics of the output (stats_out): this lane's (sum, sum of squares) of one row over its fragments, a fragment
// past Cout masked out by colmask = 0
__device__ __forceinline__ void dc_row_stats_add(float& st1, float& st2, f32x4 v, float colmask)
{
    st1 += colmask * ((v[0] + v[1]) + (v[2] + v[3]));
    st2 += colmask * ((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]));
}
// lanes fr, fr + 16, fr + 32, fr + 48 hold the same row: fixed-order tree, every lane ends with the row's pair ...
__device__ __forceinline__ void dc_row_stats_reduce(float& st1, float& st2)
{
    st1 += __shfl_xor(st1, 16, 64);
    st2 += __shfl_xor(st2, 16, 64);
    st1 += __shfl_xor(st1, 32, 64);
    st2 += __shfl_xor(st2, 32, 64);
}
// ... and the writer lane stores it as one (sum, sum of squares) partial (gemm_rowpanel.hip stores its own: it zero-fills the other parts)
__device__ __forceinline__ void dc_row_stats_store(float st1, float st2, float* __restrict__ dst, bool writer)
{
    dc_row_stats_reduce(st1, st2);
    if (writer) *(f32x2*)dst = f32x2{st1, st2};
}
// GroupNorm partials of the output (gn_part_out, stored by dc_gn_partial_store): per-channel (sum, sum of squares) over this lane's
// rows; a row past M (a clamped duplicate) masked out by rowmask = 0
__device__ __forceinline__ void dc_gn_part_add(f32x4& gs, f32x4& gq, f32x4 v, float rowmask)
{
    gs += rowmask * v;
    gq += rowmask * (v * v);
}

// Epilogue operand prefetch of the two LDS-DMA tile kernels (gemm_dma.hip, gemm_wide.hip), issued in front of the K loop so the loads
// fly under it.  Per-column fp32 operand (bias, LayerNorm weight column sums) of this lane's 4 channels in each of its TN 16-column
// blocks from column nb0 on; zeros past Cout or without the operand.
template <int TN>
__device__ __forceinline__ void dc_epi_load_cols(f32x4 (&dst)[TN], const float* __restrict__ src, int nb0, int Cout)
{
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int nb = nb0 + tn * 16;
        dst[tn] = (src && nb < Cout) ? *(const f32x4*)(src + nb) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}
// the residual fragments of rows mrow0 + 16 tm: all fetched up front (independent loads in flight together): issued one (tm, tn) tile
// at a time behind `if (residual)` they serialise into ~20 dependent L2 round trips per workgroup
template <int TM, int TN>
__device__ __forceinline__ void dc_epi_load_residual(bf16x4 (&rr)[TM][TN], const void* __restrict__ residual, int mrow0, int M, int nb0, int Cout)
{
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        const int m = mrow0 + tm * 16;
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int nb = nb0 + tn * 16;
            rr[tm][tn] = (m < M && nb < Cout) ? *(const bf16x4*)((const bf16_t*)residual + (long long)m * Cout + nb)
                                              : bf16x4{(bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
        }
    }
}

// Cooperative store of a staged bf16 tile (BM rows of PITCH bytes, PIECES 16-byte pieces each, written through dc_stage_swz):
// consecutive lanes -> consecutive 16-byte pieces of one output row; rows from M on and columns from out_cols on are dropped.
template <int BM, int PITCH, int PIECES, int NTHREADS>
__device__ __forceinline__ void dc_stage_store_rows(const char* smem, bf16_t* __restrict__ o, int m0, int M, int col0, int out_cols)
{
    for (int i = threadIdx.x; i < BM * PIECES; i += NTHREADS) {
        const int row = i / PIECES, pc = i - row * PIECES;
        const int m = m0 + row, c = col0 + pc * 8;
        if (m < M && c < out_cols) *(u32x4*)(o + (long long)m * out_cols + c) = dc_stage_unswz(*(const u32x4*)(smem + row * PITCH + pc * 16), row);
    }
}

// The direct epilogue of igemm_kernel and of gemm_dma_kernel's non-staged path (fp32 outputs, split-K slabs, direct bf16 / GEGLU
// stores): lane (fr, fq) of wave (wm, wn) holds out[m0 + (wm TM + tm) 16 + fr][n0 + (wn TN + tn) 16 + 4 fq + 0..3] in acc[tn][tm].
template <int TM, int TN>
__device__ __forceinline__ void dc_epi_direct(const f32x4 (&acc)[TN][TM], const dc_conv_desc& d, int m0, int n0, int wm, int wn, int fr, int fq)
{
    const int HoWo = d.Ho * d.Wo;
    const int M = d.N * HoWo;
    const long long slab = (long long)M * d.Cout;           // elements per split-K slab
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int flags = (d.bias ? DC_EPI_BIAS : 0) | (d.row_add ? DC_EPI_ROWADD : 0) | (d.residual ? DC_EPI_RES : 0);
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        const int m = m0 + (wm * TM + tm) * 16 + fr;
        if (m >= M) continue;
        const int nimg = m / HoWo;
        if (d.epilogue == 1) {
            const int half = d.Cout >> 1;
            bf16_t* __restrict__ o = (bf16_t*)d.out;
#pragma unroll
            for (int tp = 0; tp < TN / 2; ++tp) {
                const int nb = n0 + (wn * TN + 2 * tp) * 16 + 4 * fq;      // packed row of the hidden half
                if (nb >= d.Cout) continue;
                f32x4 bh = zero, bg = zero;                                // (GEGLU on this path is rare: operands selected, not branched on)
                if (d.bias) {
                    bh = *(const f32x4*)(d.bias + nb);
                    bg = *(const f32x4*)(d.bias + nb + 16);
                }
                const int col = ((n0 + (wn * TN + 2 * tp) * 16) >> 1) + 4 * fq;
                *(bf16x4*)(o + (long long)m * half + col) = dc_epi_geglu(acc[2 * tp][tm], acc[2 * tp + 1][tm], flags, 0.f, 0.f, zero, zero, bh, bg);
            }
            continue;
        }
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int nb = n0 + (wn * TN + tn) * 16 + 4 * fq;
            if (nb >= d.Cout) continue;
            const long long off = (long long)m * d.Cout + nb;
            if (d.splitk > 1) {                                   // this split's own fp32 slab: plain stores, no atomics
                *(f32x4*)(d.splitk_ws + (long long)blockIdx.y * slab + off) = acc[tn][tm];
                continue;
            }
            const f32x4 v = dc_epi_plain_with(
                acc[tn][tm], flags, d.act, 0.f, 0.f, zero, [&] { return *(const f32x4*)(d.bias + nb); },
                [&] { return *(const f32x4*)(d.row_add + (long long)nimg * d.row_add_stride + nb); }, d.out_scale,
                [&] { return *(const bf16x4*)((const bf16_t*)d.residual + off); });
            if (d.out_f32) *(f32x4*)((float*)d.out + off) = v;
            else *(bf16x4*)((bf16_t*)d.out + off) = dc_pack_bf16x4(v);
        }
    }
}
