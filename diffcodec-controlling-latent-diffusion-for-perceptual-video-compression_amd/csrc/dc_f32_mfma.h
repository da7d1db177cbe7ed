// The exact-fp32 core shared by lpips.hip, fid.hip, fvd.hip and cmp.hip: implicit-GEMM convolutions  D[co][pixel] += W[co][k] * X[k][pixel]
// on v_mfma_f32_32x32x2_f32 with the weights packed K-major ([k][CoP], CoP = Cout rounded up to 32), a chunk of k rows and its
// input patch staged in LDS, and 32-channel accumulator tiles per wave.  The pieces here are the ones every such kernel spells the
// same way; what differs between the families stays in their files: the load pipelines (staged in place, or through registers one
// chunk ahead) and the epilogue arithmetic, the ReLU / NaN rule included (cmp.hip keeps NaN, the others use fmaxf).
//
// MFMA operand layout: A = W[co = lane & 31][k = lane >> 5], B = X[k = lane >> 5][pixel = lane & 31]: lane half h = lane >> 5 holds
// k = 2 kp + h of k-pair kp.  Nothing is assumed about the order of the two products inside one MFMA; the order of the MFMAs that
// feed an output element is fixed by the kernel's loops alone, which is what makes the results reproducible.
//
// A helper that contains a multiply whose rounding matters carries its own `#pragma clang fp contract(off)` (see dc_scale_res in
// dc_common.h: a pragma at the call site does not reach into an inlined helper).  None of the helpers below has one.
//
// A kernel uses a helper only where its generated code stayed the same (profiles/f32_mfma_codegen.txt).  The epilogue walks and
// the patch staging loops did not survive that as functor-taking helpers, so they stay written out at their kernels, on
// dc_f32_channel; a new network starts from the pieces here and adds its rows to tests/golden/f32_mfma_bits.json.
#pragma once
#include "dc_common.h"

// ------------------------------------------------------------------------------------------------ device pieces
template <int NQ>
__device__ __forceinline__ void dc_f32_zero(f32x16 (&acc)[NQ])
{
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
}

// C/D layout of the 32x32 MFMA: lane & 31 = pixel, register r of lane half h = channel (r & 3) + 8 (r >> 2) + 4 h of the tile, so
// one store instruction writes 32 consecutive pixels of a channel row.  `base`: the tile's first channel.
__device__ __forceinline__ constexpr int dc_f32_channel(int r, int h, int base = 0) { return base + (r & 3) + 8 * (r >> 2) + 4 * h; }

// One k-pair step: `a` points at this lane's element of the weight row pair in LDS (row 2 kp + h, column = the lane's channel of
// tile 0), tile q reads a[q * 32]; `b` is the lane's patch element.  One B read feeds up to NQ MFMAs; tiles q >= nq (the padded Cout
// ended first) are skipped.  With nq == NQ at the call site the mask folds away.
template <int NQ>
__device__ __forceinline__ void dc_f32_kpair(f32x16 (&acc)[NQ], int nq, const float* a, float b)
{
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        if (q < nq) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q * 32], b, acc[q], 0, 0, 0);
}

// Patch offset of chunk-local k = (slice, ky, kx) of a KS x KS kernel in a patch [slice][py][px] with row pitch PW and slice size PS.
// A chunk holds KC real k, padded to whole pairs with zero weight rows: a padded k reads the tap before it (a finite value times 0).
template <int KS, int PW, int PS, int KC>
__device__ constexpr int dc_f32_patch_off(int k)
{
    const int kk = k < KC ? k : KC - 1;
    return (kk / (KS * KS)) * PS + ((kk % (KS * KS)) / KS) * PW + (kk % KS);
}

// Weight slab global [rows][gpitch] -> LDS [rows][PITCH] in float4 pieces, w4 pieces per row; pieces at columns >= wcols (beyond the
// padded Cout of this channel block; the default folds the compare away) are skipped.  Both sides are 16-byte aligned.
template <int PITCH>
__device__ __forceinline__ void dc_f32_copy_w(float* Wl, const float* wc, long long gpitch, int rows, int w4, int tid,
                                              int wcols = 0x7fffffff)
{
    for (int p = tid; p < rows * w4; p += 256) {
        const int row = p / w4, c4 = (p - row * w4) * 4;
        if (c4 < wcols) *(f32x4*)&Wl[row * PITCH + c4] = *(const f32x4*)&wc[(long long)row * gpitch + c4];
    }
}

// ------------------------------------------------------------------------------------------------ host pieces
struct dc_strides4 {                            // element strides of an image operand
    long long n, c, h, w;
    explicit dc_strides4(const long long* s) : n(s[0]), c(s[1]), h(s[2]), w(s[3]) {}
};

inline int dc_f32_cop(int cout) { return (cout + 31) & ~31; }      // Cout padded to whole 32-channel tiles

// a packed unit: the K-major matrix [rows][CoP], then s [CoP], then t [CoP]
inline void dc_f32_split(const float* packed, long long rows, int cop, const float*& wp, const float*& s, const float*& t)
{
    wp = packed, s = packed + rows * cop, t = s + cop;
}

// grid of a grid-stride launch over `total` elements, 256 per block, at most `cap` blocks
inline int dc_f32_blocks(long long total, long long cap) { return (int)min(cap, (total + 255) / 256); }

// Workspace planner: offsets in elements of UNIT bytes (1: bytes, 4: floats), every block rounded up to 256 bytes
template <int UNIT>
struct dc_f32_bump {
    long long off = 0;
    long long take(long long n)
    {
        const long long at = off;
        off += (n + 256 / UNIT - 1) & ~(long long)(256 / UNIT - 1);
        return at;
    }
};
