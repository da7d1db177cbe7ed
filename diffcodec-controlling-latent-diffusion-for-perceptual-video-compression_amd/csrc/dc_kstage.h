// The ONE K-loop operand stage of the six bf16 matrix kernels (gemm_dma.hip, gemm_wide.hip, gemm_p8.hip, gemm_rowpanel.hip,
// conv3x3_tile.hip, igemm.hip): how a 64-wide K slice of an operand lies in LDS, how LDS-DMA puts it there, how it comes back as
// v_mfma_f32_16x16x32_bf16 fragments, and the MFMA step that consumes them — the counterpart of dc_epilogue.h for everything in front
// of the last MFMA.  The functions own no pipeline: which stage is filled when, the counted waits and the barriers stay in the
// kernels (their hazard descriptions with them); the wait / barrier primitives themselves are in dc_common.h beside dc_ring_sync.
// A piece is used where the kernel's instruction stream stays what it was (tools/kernel_resources.py).  Written out in the kernels for
// that reason: the fragment-read loops (only their swizzle comes from here; a shared row address moved the integer address arithmetic
// of gemm_dma.hip or conv3x3_tile.hip), accumulator zeroing, tile origin and split-K range (branch layout or register allocation
// changed somewhere), gemm_rowpanel.hip's MFMA loop (X fragments indexed [tm][k]; 238 VGPRs) and per-stage wait (as two
// dc_wait_vm_lgkm calls EPI 4 loses an s_nop, EPI 1 is rescheduled), conv3x3_tile.hip's source chunk, and two DMA calls (see dc_dma16).
#pragma once
#include "dc_common.h"

// ---- address spaces and LDS-DMA.  `global_load_lds_dwordx4`: global -> LDS without VGPR staging or ds_write.  The LDS address is
// wave-uniform base + 16 * lane (lane-LINEAR: the instruction cannot scatter), only the per-lane SOURCE address is free — so any
// swizzle of the LDS image is applied by choosing which source chunk each lane fetches.  To the compiler a DMA is an LDS store: it
// does not sink below LDS reads that precede it, but it may be scheduled among the MFMAs that follow it.
// (gemm_dma.hip's issue_stage and gemm_rowpanel.hip's issue_w call the builtin themselves: through dc_dma16 hipcc stops merging the
// pieces of issue_stage's two branches in the prologue — 4-5 more LDS-DMA instructions per instance — and reschedules issue_w.)
typedef const void __attribute__((address_space(1))) * dc_gptr_t;
typedef void __attribute__((address_space(3))) * dc_lptr_t;
__device__ __forceinline__ void dc_dma16(const char* src, char* lds)
{
    __builtin_amdgcn_global_load_lds((dc_gptr_t)src, (dc_lptr_t)lds, 16, 0, 0);
}
// one dword per lane (gemm_rowpanel.hip: the residual "touch")
__device__ __forceinline__ void dc_dma4(const void* src, char* lds)
{
    __builtin_amdgcn_global_load_lds((dc_gptr_t)src, (dc_lptr_t)lds, 4, 0, 0);
}

// ---- layout.  A stage holds operand rows (pixels of X, output channels of W) of DC_KROW = 128 bytes: 64 bf16 of K = 8 chunks of
// 16 bytes.  One DMA wave-instruction lands a PIECE of 8 rows (1024 B): piece g covers rows [8g, 8g + 8), lane s lands in row
// 8g + (s >> 3), chunk slot s & 7.  A fragment read takes, for k-half s (32 of the 64 K values), 16 consecutive rows `fr` at chunk
// 4s + fq: unswizzled, the 16 lanes of a row group would hit the same 4 banks 16 ways.  So chunk c of row r is stored in slot
// c ^ (r & 7): the DMA lane of slot (s & 7) fetches source chunk (s & 7) ^ (row & 7), the fragment read of chunk c looks in slot
// c ^ (fr & 7) (every tile starts on a multiple of 16 rows, so row & 7 == fr & 7), ds_read_b128 is conflict-free and rows stay
// whole 128-byte lines.  gemm_rowpanel.hip keeps all 320 of K per W row (640 B = 40 chunks): the same XOR, which stays inside each
// aligned group of 8 chunks.  The static_asserts below prove that both sides agree.
constexpr int DC_KROW = 128;                                   // bytes of one operand row per K-step
constexpr int DC_KCHUNK = 16;                                  // bytes per lane of a DMA piece / of a fragment read
constexpr int DC_KPIECE = 8 * DC_KROW;                         // bytes one DMA wave-instruction lands: 8 rows
// source chunk the DMA lane `lane` of a piece must fetch for its row
__host__ __device__ __forceinline__ constexpr int dc_kstage_src_chunk(int lane, int row) { return (lane & 7) ^ (row & 7); }
// byte offset inside its row of the fragment a lane (fr = lane & 15, fq = lane >> 4) reads for k-half s
__host__ __device__ __forceinline__ constexpr int dc_kstage_frag_off(int s, int fq, int fr) { return ((4 * s + fq) ^ (fr & 7)) << 4; }
// the 640-byte-row form: source chunk of the lane that lands in chunk position q of row n; fragment offset of 32-wide k-step k
constexpr int DC_RP_KROW = 640;
__host__ __device__ __forceinline__ constexpr int dc_kstage_rp_src_chunk(int q, int n) { return q ^ (n & 7); }
__host__ __device__ __forceinline__ constexpr int dc_kstage_rp_frag_off(int k, int fq, int fr) { return (k >> 1) * DC_KROW + dc_kstage_frag_off(k & 1, fq, fr); }

constexpr bool dc_kstage_layouts_agree()
{
    for (int row = 0; row < 16; ++row) {
        for (int c = 0; c < 8; ++c) {                          // chunk c = 4 s + fq is read from the slot the DMA filled with chunk c
            const int slot = dc_kstage_frag_off(c >> 2, c & 3, row) / DC_KCHUNK;
            if (slot < 0 || slot > 7 || dc_kstage_src_chunk(slot, row) != c) return false;
        }
        for (int c = 0; c < 40; ++c) {                         // row panel: chunk c = 4 k + fq
            const int q = dc_kstage_rp_frag_off(c >> 2, c & 3, row) / DC_KCHUNK;
            if (q < 0 || q > 39 || dc_kstage_rp_src_chunk(q, row) != c) return false;
        }
    }
    return true;
}
static_assert(dc_kstage_layouts_agree(), "the chunk a fragment read expects at a position is the chunk the DMA placed there");

// ---- the MFMA step.  D[n][m] tiles: W fragments are the A operand, X fragments the B operand, so a lane ends up with 4 consecutive
// output channels of one row (dc_epilogue.h).  One k-half = TN x TM MFMAs into the TN x TM block of `acc` at (N0, M0).
template <int TN, int TM, int N0 = 0, int M0 = 0, int AN, int AM>
__device__ __forceinline__ void dc_mfma_khalf(f32x4 (&acc)[AN][AM], const bf16x8 (&wf)[TN], const bf16x8 (&xf)[TM])
{
    static_assert(N0 + TN <= AN && M0 + TM <= AM, "accumulator block");
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
            acc[N0 + tn][M0 + tm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[tn], xf[tm], acc[N0 + tn][M0 + tm], 0, 0, 0);
}
// both k-halves of a 64-wide K-step, ascending in k (the accumulation order every kernel keeps)
template <int TN, int TM, int N0 = 0, int M0 = 0, int AN, int AM>
__device__ __forceinline__ void dc_mfma_kstep(f32x4 (&acc)[AN][AM], const bf16x8 (&wf)[2][TN], const bf16x8 (&xf)[2][TM])
{
#pragma unroll
    for (int s = 0; s < 2; ++s) dc_mfma_khalf<TN, TM, N0, M0>(acc, wf[s], xf[s]);
}

// ---- the interleave recipe of a K-step that reads all its fragments up front and refills the ring under its MFMAs (gemm_dma.hip,
// conv3x3_tile.hip): all NRD fragment reads first (both k-halves, two register sets: the reads of the second half land while the
// MFMAs of the first run; left to itself hipcc keeps one weight fragment live at a time and waits lgkmcnt(0) in front of every group
// of TM MFMAs), then the NDMA LDS-DMA pieces of the next stage spread between the NMF MFMAs, one per few MFMAs — an LDS-DMA
// wave-instruction holds the wave's issue for 60-100 cycles, which a leading block of them would put in front of the first MFMA of
// every K-step.  Placed right after the MFMAs in program order.
template <int NMF, int NRD, int NDMA>
__device__ __forceinline__ void dc_sched_reads_mfma_dma()
{
    constexpr int PER = NMF / (NDMA + 1) > 0 ? NMF / (NDMA + 1) : 1;
    __builtin_amdgcn_sched_group_barrier(0x100, NRD, 0);                        // every fragment read first
#pragma unroll
    for (int i = 0; i < NDMA; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);                    // a few MFMAs ...
        __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);                      // ... then one LDS-DMA piece
    }
    __builtin_amdgcn_sched_group_barrier(0x008, NMF - NDMA * PER, 0);
}
