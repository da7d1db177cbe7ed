// MFMA implicit-GEMM convolution / linear for gfx950:  out[m][n] = sum_k X(m,k) * W[n][k]
//   m = (sample, oy, ox) pixel row of an NHWC bf16 activation, n = output channel,
//   k = (tap, cin) with cin contiguous -> the A-operand gather is a 128-byte row piece per (pixel, tap).
// Replaces F.conv2d / nn.Linear inside the diffusers blocks the reference calls (flownet.py:83-124,
// pipeline.py:358-367,391) — see include/diffcodec_hip.h.
//
// Structure (per workgroup, 256 threads = 4 waves, one output tile BM x BN, BK = 64):
//   global -> registers (16 B / lane, 8 lanes cover one 128-B row piece) -> [GN affine + SiLU in fp32] ->
//   LDS (chunk-major image, XOR-swizzled so that both the ds_write_b128 and the MFMA-fragment ds_read_b128
//   are bank-conflict-free) -> v_mfma_f32_16x16x32_bf16, fp32 accumulate.  LDS is double-buffered; the next
//   K-tile's global loads are issued before the current tile's MFMAs (one barrier per K-step).
//   The MFMA computes the transposed tile (A-operand = weights, B-operand = pixels) so that each lane ends up
//   with 4 consecutive output channels of one pixel -> 8-byte NHWC stores, float4 bias loads.
#include "dc_epilogue.h"

namespace {

constexpr int BK = 64;

template <int WM, int WN, int TM, int TN, bool KS3, bool GN>
__global__ __launch_bounds__(256, 2) void igemm_kernel(const dc_conv_desc d)
{
    constexpr int BM = WM * TM * 16;
    constexpr int BN = WN * TN * 16;
    constexpr int PA = BM / 32;          // A (pixel) rows per thread per K-step
    constexpr int PB = BN / 32;          // B (weight) rows per thread per K-step
    constexpr int A_BYTES = BM * 128;
    constexpr int B_BYTES = BN * 128;
    constexpr int BUF_BYTES = A_BYTES + B_BYTES;
    static_assert(WM * WN == 4, "4 waves");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave % WM;
    const int wn = wave / WM;
    const int q = tid & 7;               // 16-byte chunk of the 128-byte K piece
    const int r0 = tid >> 3;             // row within a 32-row pass

    const int HoWo = d.Ho * d.Wo;
    const int M = d.N * HoWo;
    const int Cin = d.C1 + d.C2;
    const int nkc = Cin >> 6;
    const int taps = KS3 ? 9 : 1;
    const int KT = taps * nkc;

    // ---- tile coordinates; XCD-aware remap: blocks b and b+8 share an XCD, give each XCD a contiguous range
    const int n_tiles = (d.Cout + BN - 1) / BN;
    const int m_tiles = (M + BM - 1) / BM;
    const int nblk = n_tiles * m_tiles;
    const int bid = dc_xcd_remap(blockIdx.x, nblk);
    const int tile_n = bid % n_tiles;
    const int tile_m = bid / n_tiles;
    const int m0 = tile_m * BM;
    const int n0 = tile_n * BN;

    int kt_begin = 0, kt_end = KT;
    if (d.splitk > 1) {
        const int per = (KT + d.splitk - 1) / d.splitk;
        kt_begin = blockIdx.y * per;
        kt_end = min(KT, kt_begin + per);
        if (kt_begin >= kt_end) return;
    }

    // ---- per-thread A row bookkeeping
    int a_n[PA], a_oy[PA], a_ox[PA];
    bool a_ok[PA];
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        const int m = m0 + r0 + 32 * i;
        a_ok[i] = m < M;
        const int mm = a_ok[i] ? m : 0;
        a_n[i] = mm / HoWo;
        const int rem = mm - a_n[i] * HoWo;
        a_oy[i] = rem / d.Wo;
        a_ox[i] = rem - a_oy[i] * d.Wo;
    }
    const bf16_t* __restrict__ x1 = (const bf16_t*)d.x1;
    const bf16_t* __restrict__ x2 = (const bf16_t*)d.x2;
    const bf16_t* __restrict__ wgt = (const bf16_t*)d.w;

    u32x4 ra[PA], rb[PB];
    unsigned va = 0;                     // validity bits of the staged A rows
    int cur_c = 0;
    int a_nb[PA];                        // gn_ab row of each staged A row's sample
#pragma unroll
    for (int i = 0; i < PA; ++i) a_nb[i] = GN ? a_n[i] % d.gn_batch : 0;

    auto issue_loads = [&](int kt) {
        const int tap = KS3 ? kt / nkc : 0;
        const int cc = KS3 ? kt - tap * nkc : kt;
        const int c = cc * 64 + q * 8;           // channel within cat[x1,x2]
        cur_c = c;
        const bool second = c >= d.C1;
        const bf16_t* __restrict__ src = second ? x2 : x1;
        const int cs = second ? d.C2 : d.C1;
        const int co = second ? c - d.C1 : c;
        const int ky = KS3 ? tap / 3 : 0;
        const int kx = KS3 ? tap - ky * 3 : 0;
        va = 0;
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            bool ok = a_ok[i];
            long long pix;
            if (KS3) {
                int uy = a_oy[i] * d.stride + ky - d.pad;
                int ux = a_ox[i] * d.stride + kx - d.pad;
                if (d.upsample) {
                    ok = ok && uy >= 0 && ux >= 0 && uy < 2 * d.H && ux < 2 * d.W;
                    uy >>= 1;
                    ux >>= 1;
                } else {
                    ok = ok && uy >= 0 && ux >= 0 && uy < d.H && ux < d.W;
                }
                pix = ((long long)a_n[i] * d.H + uy) * d.W + ux;
            } else {
                pix = (long long)(m0 + r0 + 32 * i);
            }
            u32x4 v = {0u, 0u, 0u, 0u};
            if (ok) {
                v = *(const u32x4*)(src + pix * cs + co);
                va |= 1u << i;
            }
            ra[i] = v;
        }
        const long long wk = (long long)tap * Cin + cc * 64 + q * 8;
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            const int n = n0 + r0 + 32 * i;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (n < d.Cout) v = *(const u32x4*)(wgt + (long long)n * taps * Cin + wk);
            rb[i] = v;
        }
    };

    auto store_lds = [&](int buf) {
        char* sA = smem + buf * BUF_BYTES;
        char* sB = sA + A_BYTES;
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            u32x4 v = ra[i];
            if (GN) {
                if (va & (1u << i)) {
                    // (scale, shift) of this row's sample: 64 B, L1-resident (shared by the 32 rows of a pass)
                    const float* __restrict__ abp = d.gn_ab + ((long long)a_nb[i] * Cin + cur_c) * 2;
                    f32x4 g[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) g[j] = *(const f32x4*)(abp + 4 * j);
                    uint32_t o[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t u = v[j];
                        float lo = __uint_as_float(u << 16);
                        float hi = __uint_as_float(u & 0xffff0000u);
                        lo = lo * g[j][0] + g[j][1];
                        hi = hi * g[j][2] + g[j][3];
                        if (d.gn_silu) {
                            lo = dc_silu(lo);
                            hi = dc_silu(hi);
                        }
                        bf16x2 p = {(bf16_t)lo, (bf16_t)hi};
                        o[j] = *(uint32_t*)&p;
                    }
                    v = u32x4{o[0], o[1], o[2], o[3]};
                }
            }
            const int r = r0 + 32 * i;
            *(u32x4*)(sA + q * (BM * 16) + ((r ^ q) << 4)) = v;
        }
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            const int r = r0 + 32 * i;
            *(u32x4*)(sB + q * (BN * 16) + ((r ^ q) << 4)) = rb[i];
        }
    };

    f32x4 acc[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto compute = [&](int buf) {
        const char* sA = smem + buf * BUF_BYTES;
        const char* sB = sA + A_BYTES;
        const int fr = lane & 15;
        const int fq = lane >> 4;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int qq = 4 * s + fq;
            bf16x8 wf[TN], xf[TM];
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const int row = (wn * TN + tn) * 16 + fr;
                wf[tn] = *(const bf16x8*)(sB + qq * (BN * 16) + ((row ^ qq) << 4));
            }
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) {
                const int row = (wm * TM + tm) * 16 + fr;
                xf[tm] = *(const bf16x8*)(sA + qq * (BM * 16) + ((row ^ qq) << 4));
            }
            dc_mfma_khalf(acc, wf, xf);
        }
    };

    // ---- main loop
    issue_loads(kt_begin);
    store_lds(0);
    __syncthreads();
    int buf = 0;
    for (int kt = kt_begin; kt < kt_end; ++kt) {
        const bool more = kt + 1 < kt_end;
        if (more) issue_loads(kt + 1);
        compute(buf);
        if (more) store_lds(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }

    // ---- epilogue: lane holds out[m = .. + (lane&15)][n = .. + 4*(lane>>4) + 0..3]
    dc_epi_direct<TM, TN>(acc, d, m0, n0, wm, wn, lane & 15, lane >> 4);
}

// Second pass of split-K: sum of the per-split slabs -> bias / row_add / scale / residual -> output.
__global__ void splitk_finish_kernel(const dc_conv_desc d, long long total4)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    const long long off = i * 4;
    const int nb = (int)(off % d.Cout);
    const long long m = off / d.Cout;
    const int nimg = (int)(m / (d.Ho * d.Wo));
    // every operand is FETCHED before anything is added (left as `v += load` per split, hipcc emits load - vmcnt(0) - add per split and
    // per epilogue operand: five to twenty dependent memory round trips in a kernel that small launches run latency-bound); the
    // additions keep their fixed order (split 0, 1, 2, ... then bias, row_add): deterministic, and the same bits as before
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 bv = d.bias ? *(const f32x4*)(d.bias + nb) : zero;
    const f32x4 ra = d.row_add ? *(const f32x4*)(d.row_add + (long long)nimg * d.row_add_stride + nb) : zero;
    bf16x4 rr = {(bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
    if (d.residual) rr = *(const bf16x4*)((const bf16_t*)d.residual + off);
    const float* __restrict__ slab = d.splitk_ws + off;
    const long long ss = total4 * 4;                            // elements per split slab
    f32x4 v = *(const f32x4*)slab;
    int k = 1;
    for (; k + 4 <= d.splitk; k += 4) {
        const f32x4 a0 = *(const f32x4*)(slab + k * ss), a1 = *(const f32x4*)(slab + (k + 1) * ss);
        const f32x4 a2 = *(const f32x4*)(slab + (k + 2) * ss), a3 = *(const f32x4*)(slab + (k + 3) * ss);
        v += a0;
        v += a1;
        v += a2;
        v += a3;
    }
    for (; k < d.splitk; ++k) v += *(const f32x4*)(slab + k * ss);
    v = dc_epi_plain(v, (d.bias ? DC_EPI_BIAS : 0) | (d.row_add ? DC_EPI_ROWADD : 0) | (d.residual ? DC_EPI_RES : 0), d.act, 0.f, 0.f, zero, bv, ra,
                     d.out_scale, rr);
    if (d.out_f32) *(f32x4*)((float*)d.out + off) = v;
    else *(bf16x4*)((bf16_t*)d.out + off) = dc_pack_bf16x4(v);
}

template <int WM, int WN, int TM, int TN>
int launch_cfg(const dc_conv_desc& d, const dc_route& r, hipStream_t st)
{
    constexpr int BM = WM * TM * 16, BN = WN * TN * 16;
    const int M = d.N * d.Ho * d.Wo;
    const int nblk = dc_cdiv(M, BM) * dc_cdiv(d.Cout, BN);
    const dim3 grid(nblk, d.splitk > 1 ? d.splitk : 1);
    const size_t lds = 2 * (BM + BN) * 128;
#define DC_IGEMM_LAUNCH(KS3, GN)                                                                              \
    do {                                                                                                      \
        auto kern = igemm_kernel<WM, WN, TM, TN, KS3, GN>;                                                    \
        static std::atomic<unsigned long long> attr_done{0};                                                  \
        dc_set_max_dyn_lds((const void*)kern, (int)lds, attr_done);                                           \
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, d);                                                \
    } while (0)
    if (r.ks3) {
        if (r.gn) DC_IGEMM_LAUNCH(true, true);
        else DC_IGEMM_LAUNCH(true, false);
    } else {
        if (r.gn) DC_IGEMM_LAUNCH(false, true);
        else DC_IGEMM_LAUNCH(false, false);
    }
#undef DC_IGEMM_LAUNCH
    return dc_launch_status();
}

// The gather GEMM takes every launch the other families pass.  Tile choice: wide-N tile (160) when dc_n_tile says so, else 128;
// tall-M tile (128) only when that still yields >= 2 workgroups per CU.
int igemm_route(const dc_conv_desc& d, dc_route& r)
{
    const long long M = (long long)d.N * d.Ho * d.Wo;
    const int bn = dc_n_tile(d);
    const long long big_tiles = ((M + 127) / 128) * ((d.Cout + bn - 1) / bn) * d.splitk;
    r.kernel = DC_ROUTE_IGEMM;
    r.tm = big_tiles >= 512 ? 4 : 2;
    r.tn = bn / 32;
    r.variant = r.tm * 10 + r.tn;
    r.ks3 = d.ksize == 3;
    r.gn = d.gn_ab != nullptr;
    return DC_OK;
}

int igemm_launch(const dc_conv_desc& d, const dc_route& r, hipStream_t st)
{
    switch (r.variant) {
        case 45: return launch_cfg<2, 2, 4, 5>(d, r, st);
        case 44: return launch_cfg<2, 2, 4, 4>(d, r, st);
        case 25: return launch_cfg<2, 2, 2, 5>(d, r, st);
        default: return launch_cfg<2, 2, 2, 4>(d, r, st);
    }
}

// every split must own a non-empty range of the `units` its kernel partitions, or its slab would stay unwritten: shrink to the
// fixpoint of splitk = ceil(units / ceil(units / splitk))
int splitk_fixpoint(int splitk, int units)
{
    for (;;) {
        const int per = (units + splitk - 1) / splitk, s2 = (units + per - 1) / per;
        if (s2 == splitk) return splitk;
        splitk = s2;
    }
}

int conv_route(const dc_conv_desc& in, dc_conv_desc& d, dc_route& r);

// The smallest divisor s of `units` (at most 20, at least 8 of the `kt` K steps per split) with tiles * s >= target workgroups; the
// largest such divisor when none reaches the target.  An even partition is preferred, so the split is a divisor of `units`.
int splitk_smallest_divisor(long long tiles, int units, int kt, int target)
{
    int last = 1;
    for (int s = 1; s <= units && s <= 20; ++s) {
        if (units % s || kt / s < 8) continue;
        if (tiles * s >= target) return s;
        last = s;
    }
    return last;
}

// The split-K the library picks for dc_conv_desc.splitk = DC_SPLITK_AUTO.  Split the K loop over workgroups when the output has
// too few tiles to fill 256 CUs and K is long (the weight-streaming layers at 8x8 / 16x16).  Each split stores its partial tile
// into its own fp32 slab and a finish pass sums the slabs (M*Cout*4 bytes written and read once per split: cheap next to the
// weight stream, and deterministic).
int splitk_pick(const dc_conv_desc& d)
{
    // the folded LayerNorm / row statistics and GEGLU live in the unsplit bf16 epilogue; a Cout that is no multiple of 16 runs on
    // the halo-tile kernel unsplit only (conv_route refuses every other split of it)
    if (d.ln_stats || d.stats_out || d.epilogue == 1 || (d.Cout & 15)) return 1;
    const long long m = (long long)d.N * d.Ho * d.Wo;
    const int nkc = (d.C1 + d.C2) >> 6, kt = (d.ksize == 3 ? 9 : 1) * nkc;
    const int bn = dc_n_tile(d);
    const long long tiles = ((m + 63) / 64) * ((d.Cout + bn - 1) / bn);
    // The stride-2 Downsample2D convs (gather GEMM, 64-row tiles): measured per shape (tools/experiments/bench_down.py, model batches
    // 32 and 2) the best split is the smallest divisor of the K steps that yields ~1024 workgroups with at least 8 steps each —
    // 1 / 2 / 4 at the three levels of a 16-frame step (the general rule gave 1 / 1 / 3: 136 -> 109 us at 32x32x640), 5 at the top
    // level of a one-frame decode (53 -> 25 us), which the general rule leaves unsplit because its K loop is short.
    if (d.ksize == 3 && d.stride == 2) return splitk_smallest_divisor(tiles, kt, kt, 1024);
    // what the launched kernel partitions: 64-channel chunks for the halo-tile 3x3 kernel, 64-wide K steps otherwise
    bool tile3 = false;
    if (d.ksize == 3 && d.stride == 1) {
        dc_conv_desc q = d, n;
        dc_route r;
        q.splitk = 1;
        q.gn_part_out = nullptr;
        tile3 = conv_route(q, n, r) == DC_OK && r.kernel == DC_ROUTE_CONV3X3_TILE;
    }
    // (per-shape sweep of every decode shape at model batches 32 and 2, round 3: short K loops are split only at tiny m, where
    // nothing else fills the chip; a 1x1 launch with >= 2048 rows needs >= 128 K steps before a split pays)
    if (tiles >= 512 || (kt < 64 && (m >= 2048 || kt < 32)) || (!tile3 && m >= 2048 && kt < 128)) return 1;
    int target = m >= 2048 ? 1024 : 256;     // measured (tools/bench_splitk.py): ~1 workgroup per CU at small m, 2+ above
    // 32x32 and 64x64 maps of a one- or two-frame decode (the halo-tile kernel's own pixel tiles already give 64-256 workgroups):
    // one workgroup per CU, not four (38 -> 26 us at 2x32x32x640)
    if (tile3 && (long long)d.Ho * d.Wo >= 1024) target = 256;
    return splitk_smallest_divisor(tiles, tile3 ? nkc : kt, kt, target);
}

// dc_conv_desc.splitk as the caller means it: DC_SPLITK_AUTO is the library's pick, any other value below 1 is 1
int splitk_asked(const dc_conv_desc& d) { return d.splitk == DC_SPLITK_AUTO ? splitk_pick(d) : d.splitk < 1 ? 1 : d.splitk; }

// Descriptor checks, normalisation (split-K pick and fixpoint, row_add_stride) and kernel choice: the one routing function of
// dc_conv_igemm_bf16, dc_conv_route, dc_conv_instance and dc_conv_gn_part_chunks.  `d` receives the normalised descriptor the kernels
// are launched with.  Each family is asked once, in priority order: the 1x1 GEMMs, the halo-tile 3x3 kernel, the gather GEMM.
int conv_route(const dc_conv_desc& in, dc_conv_desc& d, dc_route& r)
{
    d = in;
    r = dc_route{};
    const int Cin = d.C1 + d.C2;
    if (!d.x1 || !d.w || !d.out) return DC_ERR_INVALID;
    if (d.ksize != 1 && d.ksize != 3) return DC_ERR_INVALID;
    if (Cin <= 0 || (Cin & 63) || (d.C1 & 63) || (d.C2 && !d.x2)) return DC_ERR_INVALID;
    if (d.Cout <= 0 || (d.Cout & 3)) return DC_ERR_INVALID;             // (multiples of 4: the halo-tile kernel only, see below)
    if (d.N <= 0 || d.H <= 0 || d.W <= 0 || d.Ho <= 0 || d.Wo <= 0) return DC_ERR_INVALID;
    if (d.ksize == 1 && (d.stride != 1 || d.upsample || d.Ho != d.H || d.Wo != d.W)) return DC_ERR_INVALID;
    if (d.ksize == 3) {
        if (d.stride != 1 && d.stride != 2) return DC_ERR_INVALID;
        const int Hin = d.upsample ? 2 * d.H : d.H, Win = d.upsample ? 2 * d.W : d.W;
        const int ho = d.pad ? (Hin + 2 - 3) / d.stride + 1 : (Hin + 1 - 3) / d.stride + 1;
        const int wo = d.pad ? (Win + 2 - 3) / d.stride + 1 : (Win + 1 - 3) / d.stride + 1;
        if (ho != d.Ho || wo != d.Wo) return DC_ERR_INVALID;
    }
    if (d.gn_ab && d.gn_batch <= 0) return DC_ERR_INVALID;
    if (d.act < 0 || d.act > 2) return DC_ERR_INVALID;
    d.splitk = splitk_asked(d);                                         // from here on an ordinary explicit request
    if (d.row_add_stride == 0) d.row_add_stride = d.Cout;
    if (d.epilogue == 1 && (d.splitk > 1 || (d.Cout & 31) || d.residual || d.row_add || d.out_f32)) return DC_ERR_INVALID;
    const int asked = d.splitk, nkc = Cin >> 6;
    d.splitk = r.splitk = splitk_fixpoint(asked, nkc);                  // the GEMMs and the halo-tile kernel split 64-channel chunks,
    int rc = dc_gemm_dma_route(d, r);
    if (rc == DC_ROUTE_PASS) rc = dc_conv3x3_tile_route(d, r);
    if (rc == DC_ROUTE_PASS) {
        d.splitk = r.splitk = splitk_fixpoint(asked, (d.ksize == 3 ? 9 : 1) * nkc);   // the gather GEMM (tap, chunk) steps
        rc = igemm_route(d, r);
    }
    if (rc != DC_OK) return rc;
    // Cout: multiples of 16 everywhere; the halo-tile 3x3 kernel alone also takes multiples of 4 (clamped weight rows,
    // guarded 4-channel epilogue) — UNet conv_out 320->4 runs there on one mostly empty N-tile instead of on the VALU
    if ((d.Cout & 15) && !(r.kernel == DC_ROUTE_CONV3X3_TILE && asked == 1)) return DC_ERR_INVALID;
    const bool gemm = r.kernel != DC_ROUTE_CONV3X3_TILE && r.kernel != DC_ROUTE_IGEMM;
    if ((d.ln_stats || d.stats_out) && !gemm) return DC_ERR_INVALID;     // LDS-DMA GEMM epilogue only
    if (d.gn_part_out && r.gn_chunks == 0) return DC_ERR_INVALID;       // (the gather GEMM has no statistics epilogue)
    return DC_OK;
}

}  // namespace

extern "C" int dc_conv_gn_part_chunks(const dc_conv_desc* dp)
{
    if (!dp) return 0;
    // the launch decision must be the one dc_conv_igemm_bf16 takes with gn_part_out set (the host sizes the buffer from here)
    dc_conv_desc q = *dp, d;
    q.splitk = splitk_asked(q);
    if (q.splitk > 1) return 0;
    if (!q.gn_part_out) q.gn_part_out = (float*)(uintptr_t)16;
    dc_route r;
    return conv_route(q, d, r) == DC_OK ? r.gn_chunks : 0;
}

extern "C" long long dc_conv_igemm_ws_bytes(const dc_conv_desc* d)
{
    if (!d) return 0;
    const int splitk = splitk_asked(*d);
    return splitk > 1 ? (long long)d->N * d->Ho * d->Wo * d->Cout * 4 * splitk : 0;
}

extern "C" int dc_conv_route(const dc_conv_desc* dp, int* info)
{
    if (!info) return DC_ERR_INVALID;
    for (int i = 0; i < DC_ROUTE_INFO_INTS; ++i) info[i] = 0;
    if (!dp) return DC_ERR_INVALID;
    dc_conv_desc d;
    dc_route r;
    const int rc = conv_route(*dp, d, r);
    if (rc != DC_OK) return rc;
    info[0] = r.kernel;
    info[1] = r.variant;
    info[2] = r.epi;
    info[3] = r.splitk;
    info[4] = r.ln_first;
    return DC_OK;
}

extern "C" int dc_conv_instance(const dc_conv_desc* dp, int* info)
{
    if (!info) return DC_ERR_INVALID;
    for (int i = 0; i < DC_CONV_INSTANCE_INTS; ++i) info[i] = 0;
    if (!dp) return DC_ERR_INVALID;
    dc_conv_desc d;
    dc_route r;
    const int rc = conv_route(*dp, d, r);
    if (rc != DC_OK) return rc;
    info[0] = r.kernel;
    int* a = info + 1;                                      // the template arguments, in the order of the kernel's template
    switch (r.kernel) {
        case DC_ROUTE_GEMM_DMA: a[0] = r.tm, a[1] = r.tn, a[2] = r.nst, a[3] = r.epi; break;
        case DC_ROUTE_GEMM_WIDE: a[0] = r.tn, a[1] = r.epi, a[2] = r.st; break;
        case DC_ROUTE_GEMM_P8: a[0] = r.epi; break;
        case DC_ROUTE_GEMM_ROWPANEL: a[0] = r.epi, a[1] = r.gn; break;
        case DC_ROUTE_CONV3X3_TILE:
            a[0] = r.tm, a[1] = r.tn, a[2] = r.gn, a[3] = r.nst, a[4] = r.epi, a[5] = r.fast, a[6] = r.ups, a[7] = r.sh;
            break;
        default: a[0] = r.tm, a[1] = r.tn, a[2] = r.ks3, a[3] = r.gn; break;
    }
    return DC_OK;
}

extern "C" int dc_conv_igemm_bf16(const dc_conv_desc* dp, void* stream)
{
    if (!dp) return DC_ERR_INVALID;
    dc_conv_desc d;
    dc_route r;
    hipStream_t st = (hipStream_t)stream;
    int rc = conv_route(*dp, d, r);
    if (rc != DC_OK) return rc;
    if (d.splitk > 1 && !d.splitk_ws) return DC_ERR_INVALID;
    if (r.ln_first) {                                       // raw LayerNorm partials -> (mean, rstd) pairs in the caller's scratch
        if (!d.ln_scratch) return DC_ERR_INVALID;
        rc = dc_ln_finalize(d.ln_stats, d.ln_scratch, (long long)d.N * d.Ho * d.Wo, d.ln_parts, d.C1 + d.C2, d.ln_eps, stream);
        if (rc != DC_OK) return rc;
        d.ln_stats = d.ln_scratch;
        d.ln_parts = 0;
    }
    switch (r.kernel) {
        case DC_ROUTE_GEMM_DMA: rc = dc_gemm_dma_launch(d, r, st); break;
        case DC_ROUTE_GEMM_WIDE: rc = dc_gemm_wide_launch(d, r, st); break;
        case DC_ROUTE_GEMM_P8: rc = dc_gemm_p8_launch(d, r, st); break;
        case DC_ROUTE_GEMM_ROWPANEL: rc = dc_gemm_rowpanel_launch(d, r, st); break;
        case DC_ROUTE_CONV3X3_TILE: rc = dc_conv3x3_tile_launch(d, r, st); break;
        default: rc = igemm_launch(d, r, st); break;
    }
    if (rc != DC_OK) return rc;
    if (d.splitk > 1) {
        const long long M = (long long)d.N * d.Ho * d.Wo;
        const long long total4 = M * d.Cout / 4;
        hipLaunchKernelGGL(splitk_finish_kernel, dim3(dc_cdiv(total4, 256)), dim3(256), 0, st, d, total4);
        return dc_launch_status();
    }
    return DC_OK;
}
