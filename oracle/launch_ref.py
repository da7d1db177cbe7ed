"""fp64 references of single HIP launches, and the checker that holds a launch's output against them.

Every reference computes, in fp64, the operation a launch promises, from the exact operands that launch read (bf16 / fp32
tensors on any device: the CPU tests run them on small tensors, tests/launch_shadow.py on the GPU next to the real launch).
Only sampled output rows are computed (`sample_rows`); every column of a sampled row is checked.

Tolerance model (fixed in advance, not fitted to results).  Per checked element
    |y - r| <= e_out * |r| + K_TOL * U * S,        S = sqrt(sum_k (a_k * w_k)^2)  (fp64, over the launch's own gather),
U = 2^-8, K_TOL = 4, e_out = 2^-8 for a bf16 output and 2^-20 for fp32.  The S term covers the bf16 rounding of operands a
kernel transforms on load (GroupNorm affine / SiLU, the nearest upsample is exact) and any fp32 accumulation order; e_out covers
the rounding of the stored result.  Epilogue transforms scale S by their first-order sensitivity: |out_scale| * |act'(z)| for
the plain epilogue, |gelu(g)| S_h + |h gelu'(g)| S_g for GEGLU.  Attention uses a_k = p_k, w_k = v_k.  Because the elementwise
bound admits small systematic errors, each launch must also meet  rms(y - r) / rms(r) <= RMS_MAX = 2^-7  over its checked
elements.

e_out = 2^-8 is exactly bf16's worst-case relative half ulp, so a single correct rounding alone can reach err/tol = 1 where S
is negligible; the S term is what leaves room for a value computed in fp32 to land on the other side of a rounding boundary.

Statistics outputs (GroupNorm scale / shift, LayerNorm mean / rstd, row and GroupNorm partial sums) are fp32 results of fp32
reductions; their bounds are stated next to each reference."""
import math

import numpy as np
import torch

U = 2.0 ** -8
K_TOL = 4.0
E_OUT_BF16 = 2.0 ** -8
E_OUT_F32 = 2.0 ** -20
RMS_MAX = 2.0 ** -7
BLOCK = 256                      # rows per M block of the sampling rule (the tallest row tile of the GEMM family)
F64 = torch.float64


def e_out(dtype):
    return E_OUT_F32 if dtype == torch.float32 else E_OUT_BF16


# ------------------------------------------------------------------------------------------ row sampling
def sample_rows(M, spatial=None, row_bytes=()):
    """The one row-sampling rule.  Output rows 0..M-1 (row m = pixel / token m of a [M, C] output):
      * every row of the first and of the last 256-row block;
      * in every 256-row block t, the four rows t*256 + j*64 + (37*t mod 64), j = 0..3: every M tile of every kernel is touched
        and every residue mod 64 appears;
      * spatial = (N, Ho, Wo): one full output row and one full output column of every sample — row 0 and column Wo-1 of even
        samples, row Ho-1 and column 0 of odd ones — so that the padding borders are checked;
      * row_bytes: bytes per row of each operand indexed by m; for an operand larger than 2^31 or 2^32 bytes, the whole 256-row
        block centred on the first row that reaches past each boundary.
    Returns a sorted int64 tensor (CPU)."""
    nblk = (M + BLOCK - 1) // BLOCK
    parts = [np.arange(0, min(M, BLOCK)), np.arange((nblk - 1) * BLOCK, M)]
    t = np.arange(nblk)
    for j in range(4):
        parts.append(t * BLOCK + j * 64 + (37 * t) % 64)
    if spatial is not None:
        n_, ho, wo = spatial
        for n in range(n_):
            base = n * ho * wo
            oy = 0 if n % 2 == 0 else ho - 1
            ox = wo - 1 if n % 2 == 0 else 0
            parts.append(base + oy * wo + np.arange(wo))
            parts.append(base + np.arange(ho) * wo + ox)
    for rb in row_bytes:
        for lim in (2 ** 31, 2 ** 32):
            if rb and rb * M > lim:
                r = lim // rb                                    # the row that holds byte `lim`
                parts.append(np.arange(max(0, r - BLOCK // 2), r + BLOCK // 2))
    rows = np.unique(np.concatenate(parts))
    return torch.from_numpy(rows[(rows >= 0) & (rows < M)].astype(np.int64))


# ------------------------------------------------------------------------------------------ checker
class Mismatch(AssertionError):
    pass


def check(y, r, s, out_dtype):
    """y: the launch's values at the checked elements (any float dtype), r / s: fp64 reference and S term of the same shape.
    -> dict(ratio = worst err/tol, rms = relative RMS error, worst = index tuple, err, tol, ok)."""
    y = y.to(F64)
    err = (y - r).abs()
    tol = e_out(out_dtype) * r.abs() + K_TOL * U * s
    bad_nan = ~torch.isfinite(y)
    ratio_t = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio_t = torch.where(bad_nan, torch.full_like(err, math.inf), ratio_t)
    idx = int(torch.argmax(ratio_t.reshape(-1)))
    worst = tuple(int(v) for v in np.unravel_index(idx, tuple(r.shape)))
    den = float((r * r).sum())
    num = float((err * err).sum()) if not bool(bad_nan.any()) else math.inf
    rms = math.sqrt(num / den) if den > 0 else (0.0 if num == 0 else math.inf)
    ratio = float(ratio_t.reshape(-1)[idx])
    return dict(ratio=ratio, rms=rms, worst=worst, err=float(err.reshape(-1)[idx]), tol=float(tol.reshape(-1)[idx]),
                ok=ratio <= 1.0 and rms <= RMS_MAX)


# ------------------------------------------------------------------------------------------ weights
def unpack_weight(pc):
    """PackedConv (any layout: igemm incl. GEGLU row interleave and mfma_small_cout, small_cin, small_cout) ->
    (w fp64 [Cout, k*k, Cin] in checkpoint row order, bias fp64 [Cout] or None).  For GEGLU rows [0, Cout/2) are the hidden
    half and [Cout/2, Cout) the gate half, as in the checkpoint's ff.net.0.proj."""
    w = pc.w.to(F64)
    k2 = pc.ksize * pc.ksize
    if pc.kind == "small_cin":
        w = w.reshape(k2, pc.cin, pc.cout).permute(2, 0, 1)
    else:
        w = w.reshape(pc.cout, k2, pc.cin)
    b = None if pc.bias is None else pc.bias.to(F64)
    if pc.geglu:
        f = pc.cout // 2
        idx = torch.arange(pc.cout).reshape(2, f // 16, 16).permute(1, 0, 2).reshape(-1)   # packed row p holds checkpoint row idx[p]
        inv = torch.empty_like(idx)
        inv[idx] = torch.arange(pc.cout)
        inv = inv.to(w.device)
        w = w[inv]
        b = None if b is None else b[inv]
    return w, b


# ------------------------------------------------------------------------------------------ conv / linear
def _act(z, act):
    if act == 0:
        return z, torch.ones_like(z)
    c = 1.0 if act == 1 else 1.702
    sg = torch.sigmoid(c * z)
    return z * sg, (sg + c * z * sg * (1 - sg)).abs()


def _gelu(z):
    cdf = 0.5 * torch.erfc(-z / math.sqrt(2.0))                  # (1 + erf cancels for very negative z, even in fp64)
    pdf = torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    return z * cdf, cdf + z * pdf


def conv_gather(x1, rows, *, x2=None, ksize=1, stride=1, pad=1, upsample=False, Ho=None, Wo=None, gn_ab=None, gn_silu=False):
    """A operand of the sampled output rows: fp64 [R, k*k, C1+C2] — the concat, the GroupNorm affine (+SiLU) on load, the fused
    nearest-2x upsample, stride and padding (1: symmetric; 0: F.pad(x, (0, 1, 0, 1)) then no padding) exactly as
    dc_conv_desc describes them; padding taps are zero after the affine."""
    n_, h, w, c1 = x1.shape
    dev = x1.device
    rows = rows.to(dev)
    xs = [x1.reshape(-1, c1)] + ([] if x2 is None else [x2.reshape(-1, x2.shape[-1])])
    if ksize == 1:
        ho, wo = h, w
    hw = Ho * Wo if ksize == 3 else h * w
    n = rows // hw
    if ksize == 1:
        pix = rows[:, None]
        valid = torch.ones_like(pix, dtype=torch.bool)
    else:
        rem = rows - n * hw
        oy, ox = rem // Wo, rem % Wo
        ky = torch.arange(3, device=dev).repeat_interleave(3)
        kx = torch.arange(3, device=dev).repeat(3)
        p = 1 if pad else 0
        uy = oy[:, None] * stride + ky[None] - p
        ux = ox[:, None] * stride + kx[None] - p
        lh, lw = (2 * h, 2 * w) if upsample else (h, w)
        valid = (uy >= 0) & (ux >= 0) & (uy < lh) & (ux < lw)
        if upsample:
            uy, ux = uy // 2, ux // 2
        pix = (n[:, None] * h + uy.clamp(0, h - 1)) * w + ux.clamp(0, w - 1)
    a = torch.cat([t[pix.reshape(-1)].to(F64) for t in xs], 1).reshape(pix.shape[0], pix.shape[1], -1)
    if gn_ab is not None:
        ab = gn_ab.to(F64)[n % gn_ab.shape[0]]                   # [R, C, 2]
        a = a * ab[:, None, :, 0] + ab[:, None, :, 1]
        if gn_silu:
            a = a * torch.sigmoid(a)
    return a * valid[..., None]


GELU_ABS = 2.0 ** -22
"""The kernels evaluate GELU as 0.5 g (1 + erf(g / sqrt 2)) in fp32 with a polynomial erf of absolute error <= 1.5e-7: the Phi(g)
factor carries an absolute error of at most 2^-22 (with the fp32 rounding of 1 + erf), which first-order propagation through
h * gelu(g) does not see where Phi(g) itself is tiny (g << 0); it enters the bound as |h g| 2^-22."""


def conv_ref(x1, pc, rows, *, x2=None, gn_ab=None, gn_silu=False, row_add=None, residual=None, stride=1, pad=1, upsample=False,
             out_scale=1.0, act=0, chunk_elems=1 << 25):
    """fp64 reference (r, S) [R, Cout_eff] of one `ops.conv` launch at output rows `rows` (a folded LayerNorm is evaluated as
    Linear(LN(x1)) with W', b' and (mean, rstd) computed in fp64 from x1 itself, not from the launch's statistics operand)."""
    n_, h, w, _ = x1.shape
    k = pc.ksize
    if k == 1:
        ho, wo = h, w
    else:
        hin, win = (2 * h, 2 * w) if upsample else (h, w)
        ho = (hin + (2 if pad else 1) - 3) // stride + 1
        wo = (win + (2 if pad else 1) - 3) // stride + 1
    wt, bias = unpack_weight(pc)
    wt = wt.to(x1.device).reshape(wt.shape[0], -1)
    w2 = wt * wt
    rows = rows.to(x1.device)
    step = max(1, chunk_elems // max(1, wt.shape[1]))
    rs, ss = [], []
    for i in range(0, rows.numel(), step):
        rr = rows[i:i + step]
        a = conv_gather(x1, rr, x2=x2, ksize=k, stride=stride, pad=pad, upsample=upsample, Ho=ho, Wo=wo, gn_ab=gn_ab,
                        gn_silu=gn_silu).reshape(rr.numel(), -1)
        if pc.ln_eps is not None:
            mean = a.mean(1, keepdim=True)
            var = ((a - mean) ** 2).mean(1, keepdim=True)
            a = (a - mean) / torch.sqrt(var + pc.ln_eps)
        rs.append(a @ wt.T)
        ss.append(torch.sqrt((a * a) @ w2.T))
    r, s = torch.cat(rs), torch.cat(ss)
    if bias is not None:
        r = r + bias.to(r.device)
    if pc.geglu:
        f = pc.cout // 2
        hh, g = r[:, :f], r[:, f:]
        gg, dg = _gelu(g)
        return hh * gg, gg.abs() * s[:, :f] + (hh * dg).abs() * s[:, f:] + (hh * g).abs() * GELU_ABS / (K_TOL * U)
    if row_add is not None:
        r = r + row_add.to(F64)[rows // (ho * wo)]
    r, d = _act(r, act)
    s = s * d * abs(out_scale)
    r = r * out_scale
    if residual is not None:
        r = r + residual.reshape(-1, pc.cout)[rows].to(F64)
    return r, s


def row_stats_totals_ref(y_rows):
    """Per-row (sum, sum of squares) of the launch's own stored output rows [R, C] -> fp64 [R, 2] and its bound: the partials
    (`stats_out`, any number per row) must add up to these within  U * sum|y| (resp. U * sum y^2) — they may be formed from the
    fp32 values before the bf16 rounding of the output (half an ulp, U / 2, per element)."""
    y = y_rows.to(F64)
    r = torch.stack([y.sum(1), (y * y).sum(1)], 1)
    s = torch.stack([y.abs().sum(1), (y * y).sum(1)], 1)
    return r, s / K_TOL                 # checked with check(..., torch.float32): e_out 2^-20 |r| + U * sum


def gn_part_totals_ref(y):
    """Per-(sample, channel) (sum, sum of squares) over the pixels of a launch's stored output y [N, ..., C] -> fp64 [N, C, 2] and
    the bound of the `.gn_part` slabs' total (same argument as row_stats_totals_ref)."""
    n, c = y.shape[0], y.shape[-1]
    r = torch.zeros((n, c, 2), dtype=F64, device=y.device)
    s = torch.zeros((n, c, 2), dtype=F64, device=y.device)
    for i in range(n):
        v = y[i].reshape(-1, c).to(F64)
        r[i, :, 0], r[i, :, 1] = v.sum(0), (v * v).sum(0)
        s[i, :, 0], s[i, :, 1] = v.abs().sum(0), (v * v).sum(0)
    return r, s / K_TOL


def conv3x3_nchw_f32_ref(x, w, bias, rows, stride=1, silu=False, chunk_elems=1 << 25):
    """fp32 NCHW 3x3 conv, padding 1, stride s (+ SiLU) of the control extractors, at output pixels `rows` (n * Ho * Wo + oy * Wo
    + ox) -> (r, S) [R, Cout].  x may be a channel-slice view.
    The launch is fp32 throughout (an exact k-ordered fmaf chain of K = 9 Cin terms, dc_conv3x3_nchw_f32): there is no bf16 operand
    rounding for U to cover, so S is replaced by the chain's own rounding: each of the K steps rounds its running sum s_j by at
    most 2^-24 |s_j| <= 2^-24 A, A = sum_k |a_k w_k| (+ |bias|); with independent rounding errors the total stays below
    2^-24 sqrt(K) A, which enters the bound as the S-equivalent 2^-24 sqrt(K) A / U.  SiLU scales it by |silu'| and adds its fp32
    evaluation, a relative 2^-20."""
    n_, cin, h, wd = x.shape
    cout = w.shape[0]
    ho, wo = (h + 2 - 3) // stride + 1, (wd + 2 - 3) // stride + 1
    rows = rows.to(x.device)
    wt = w.to(F64).reshape(cout, -1)                                  # [Cout, Cin*9] (ci, ky, kx)
    ky = torch.arange(3, device=x.device).repeat_interleave(3)
    kx = torch.arange(3, device=x.device).repeat(3)
    step = max(1, chunk_elems // (cin * 9))
    rs, ss = [], []
    for i in range(0, rows.numel(), step):
        rr = rows[i:i + step]
        n = rr // (ho * wo)
        rem = rr - n * ho * wo
        uy = (rem // wo)[:, None] * stride + ky[None] - 1
        ux = (rem % wo)[:, None] * stride + kx[None] - 1
        ok = (uy >= 0) & (ux >= 0) & (uy < h) & (ux < wd)
        a = x[n[:, None], :, uy.clamp(0, h - 1), ux.clamp(0, wd - 1)].to(F64)       # [r, 9, Cin]
        a = (a * ok[..., None]).permute(0, 2, 1).reshape(rr.numel(), -1)
        rs.append(a @ wt.T)
        ss.append(a.abs() @ wt.abs().T)
    r, s = torch.cat(rs), torch.cat(ss)
    if bias is not None:
        r = r + bias.to(F64)
        s = s + bias.to(F64).abs()
    s = s * (2.0 ** -24 * math.sqrt(9 * cin) / U)
    if silu:
        z = r
        r, d = _act(z, 1)
        s = s * d + r.abs() * (2.0 ** -20 / (K_TOL * U))
    return r, s


# ------------------------------------------------------------------------------------------ attention
def attention_ref(q, k, v, heads, rows, scale=None, causal=False, q_rounded=None):
    """softmax(q k^T * scale) v in fp64 at rows (b * Nq + i) of the [B * Nq, C] output; q / k / v may be strided views.
    S term: a_k = p_k, w_k = v_k (the bf16 rounding of the probabilities before the PV product).
    q_rounded (default: head dims that are not a multiple of 16, the kernel's offset-in-the-GEMM form): the kernel multiplies
    the queries by scale*log2(e) and rounds them to bf16 before QK^T, which perturbs every logit of a query by
    delta_k = sum_c eps_c q_c k_kc scale with |eps_c| <= 2^-9, one eps per query channel shared by all keys.  To first order
    the output moves by sum_c eps_c q_c scale G_c with G_c = sum_k p_k k_kc (v_k - o); its worst case
    2^-9 scale sum_c |q_c G_c| enters S as the term (U / 2) scale sum_c |q_c G_c| / U."""
    b_, nq, c = q.shape
    d = c // heads
    sc = d ** -0.5 if scale is None else scale
    if q_rounded is None:
        q_rounded = d % 16 != 0
    rows = rows.to(q.device)
    rs, ss = [], []
    for b in torch.unique(rows // nq).tolist():
        sel = rows[(rows // nq) == b] - b * nq
        qq = q[b, sel].to(F64).reshape(-1, heads, d).transpose(0, 1)           # [h, R, d]
        kk = k[b].to(F64).reshape(-1, heads, d).transpose(0, 1)                # [h, Nk, d]
        vv = v[b].to(F64).reshape(-1, heads, d).transpose(0, 1)
        lg = qq @ kk.transpose(1, 2) * sc
        if causal:
            lg = lg.masked_fill(torch.arange(kk.shape[1], device=q.device)[None, None, :] > sel[None, :, None], -math.inf)
        p = torch.softmax(lg, -1)
        o = p @ vv                                                              # [h, R, d]
        s2 = torch.sqrt((p * p) @ (vv * vv))
        if q_rounded:
            step = max(1, (1 << 24) // (heads * kk.shape[1] * d))
            for i in range(0, sel.numel(), step):
                j = slice(i, i + step)
                pk = p[:, j, :, None] * kk[:, None]                             # [h, r, Nk, d]: p_k k_kc
                g = pk.transpose(2, 3) @ vv[:, None] - pk.sum(2)[..., None] * o[:, j, None, :]   # [h, r, c, e]: sum_k p_k k_kc (v_ke - o_e)
                s2[:, j] += 0.5 * sc * (qq[:, j].abs()[..., None] * g.abs()).sum(2)
        rs.append(o.transpose(0, 1).reshape(-1, c))
        ss.append(s2.transpose(0, 1).reshape(-1, c))
    return torch.cat(rs), torch.cat(ss)


# ------------------------------------------------------------------------------------------ normalisation
def group_norm_ab_ref(x, gamma, beta, groups, eps, x2=None):
    """-> fp64 ab [N, C, 2] (scale, shift) of GroupNorm(cat[x, x2]) and per-(sample, channel) group statistics
    dict(mean, std, rms) for check_group_norm_ab."""
    n, c1 = x.shape[0], x.shape[-1]
    xs = x.reshape(n, -1, c1).to(F64)
    if x2 is not None:
        xs = torch.cat([xs, x2.reshape(n, -1, x2.shape[-1]).to(F64)], 2)
    c = xs.shape[2]
    g = xs.reshape(n, xs.shape[1], groups, c // groups)
    mean = g.mean((1, 3))
    var = g.var((1, 3), unbiased=False)
    rms = torch.sqrt((g * g).mean((1, 3)))
    rstd = 1.0 / torch.sqrt(var + eps)
    ga = torch.ones(c, dtype=F64, device=x.device) if gamma is None else gamma.to(F64)
    be = torch.zeros(c, dtype=F64, device=x.device) if beta is None else beta.to(F64)
    a = rstd.repeat_interleave(c // groups, 1) * ga
    b = be - mean.repeat_interleave(c // groups, 1) * a
    rep = lambda t: t.repeat_interleave(c // groups, 1)
    return torch.stack([a, b], 2), dict(mean=rep(mean), std=rep(torch.sqrt(var + eps)), rms=rep(rms))


def check_group_norm_ab(ab, ref, st):
    """The (scale, shift) pair feeds y = x*a + b.  It is held to the error it causes in y over the group's values x = mean +- std:
        |da * mean + db| + |da| * std  <=  |a| * (2^-9 * rms + 2^-20 * rms^2 / std).
    First term: the statistics may be taken from the fp32 values before the producer's bf16 rounding (`.gn_part` epilogues): that
    moves the mean by at most half a bf16 ulp of the group's RMS.  Second term: var = E[x^2] - mean^2 in fp32 loses
    2^-20 E[x^2] (rounding of a sum of up to 2^20 partials), i.e. a relative 2^-20 rms^2 / std^2 of the normalised value."""
    a, b = ab[..., 0].to(F64), ab[..., 1].to(F64)
    da, db = a - ref[..., 0], b - ref[..., 1]
    err = (da * st["mean"] + db).abs() + da.abs() * st["std"]
    tol = ref[..., 0].abs() * (2.0 ** -9 * st["rms"] + 2.0 ** -20 * st["rms"] ** 2 / st["std"])
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), (err > 0).to(F64) * math.inf)
    ratio = torch.where(torch.isfinite(a) & torch.isfinite(b), ratio, torch.full_like(ratio, math.inf))
    idx = int(torch.argmax(ratio.reshape(-1)))
    worst = tuple(int(v) for v in np.unravel_index(idx, tuple(ratio.shape)))
    r = float(ratio.reshape(-1)[idx])
    # systematic error, as for every launch: RMS of the error in y over RMS of the normalised output's scale |a| * std (= |gamma|)
    den = float(((ref[..., 0] * st["std"]) ** 2).sum())
    num = float((err * err).sum()) if math.isfinite(r) else math.inf
    rms = math.sqrt(num / den) if den > 0 else (0.0 if num == 0 else math.inf)
    return dict(ratio=r, rms=rms, worst=worst, err=float(err.reshape(-1)[idx]), tol=float(tol.reshape(-1)[idx]),
                ok=r <= 1.0 and rms <= RMS_MAX)


def gn_apply_ref(x, ab, rows, silu=False, x2=None):
    """y = cat[x, x2] * a + b (+ SiLU) at rows of [N*HW, C]: (r, S)."""
    n = x.shape[0]
    a = conv_gather(x, rows, x2=x2)[:, 0]                       # [R, C] raw input
    hw = x.numel() // (n * x.shape[-1])
    abn = ab.to(F64)[(rows.to(x.device) // hw)]
    z = a * abn[..., 0] + abn[..., 1]
    s = torch.sqrt((a * abn[..., 0]) ** 2 + abn[..., 1] ** 2)
    if silu:
        z, d = _act(z, 1)
        s = s * d
    return z, s


def fdn_modulate_ref(x, ab, gamma, beta, rows):
    """y = (x*a + b) * (1 + gamma) + beta, gamma / beta of sample n % Bp: (r, S)."""
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    rows = rows.to(x.device)
    nn_ = rows // hw
    xx = x.reshape(-1, c)[rows].to(F64)
    abn = ab.to(F64)[nn_]
    bp = gamma.shape[0]
    pix = (nn_ % bp) * hw + rows % hw
    g = gamma.reshape(-1, c)[pix].to(F64)
    b = beta.reshape(-1, c)[pix].to(F64)
    t = xx * abn[..., 0] + abn[..., 1]
    r = t * (1 + g) + b
    s = torch.sqrt(((xx * abn[..., 0]) ** 2 + abn[..., 1] ** 2) * (1 + g) ** 2 + b ** 2)
    return r, s


def layer_norm_ref(x, gamma, beta, eps, rows):
    c = x.shape[-1]
    xx = x.reshape(-1, c)[rows.to(x.device)].to(F64)
    mean = xx.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xx - mean) ** 2).mean(1, keepdim=True) + eps)
    t = (xx - mean) * rstd * gamma.to(F64)
    b = beta.to(F64).expand_as(t)
    return t + b, torch.sqrt(t * t + b * b)


def row_stats_ref(x, rows):
    """(sum, sum of squares) [R, 1, 2] of rows of x [M, C]; S = sqrt(sum x^2) resp. sqrt(sum x^4)."""
    c = x.shape[-1]
    xx = x.reshape(-1, c)[rows.to(x.device)].to(F64)
    r = torch.stack([xx.sum(1), (xx * xx).sum(1)], 1)[:, None]
    s = torch.stack([torch.sqrt((xx * xx).sum(1)), torch.sqrt((xx ** 4).sum(1))], 1)[:, None]
    return r, s


def ln_finalize_ref(partials, c, eps, rows):
    """(mean, rstd) [R, 2] over c channels from partials [M, parts, 2].  S: mean from sqrt(E[x^2]) / sqrt(c)-scaled sums; rstd
    through var = E[x^2] - mean^2, whose fp32 cancellation is bounded by E[x^2] / (var + eps) times the rounding of E[x^2]."""
    p = partials[rows.to(partials.device)].to(F64).sum(1)
    mean = p[:, 0] / c
    ex2 = p[:, 1] / c
    var = (ex2 - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    r = torch.stack([mean, rstd], 1)
    s_mean = torch.sqrt(ex2) / K_TOL * 2.0 ** -12
    s_rstd = rstd * ex2 / (var + eps) / K_TOL * 2.0 ** -12
    return r, torch.stack([s_mean, s_rstd], 1)


def softmax_rows_ref(s, scale, rows):
    """p = softmax(s * scale) per row.  Besides the rounding of the bf16 output (which alone reaches err/tol = 1: e_out = 2^-8 is
    bf16's worst-case half ulp), the fp32 evaluation moves p by a relative 2^-20 (exp, sum, reciprocal) plus 2^-23 |s * scale| (the
    rounding of the exponent's argument), which can push a value across a rounding boundary; S carries both, and an absolute
    floor of 2^-30 for underflowing terms."""
    z = s[rows.to(s.device)].to(F64) * scale
    p = torch.softmax(z, 1)
    return p, (p * (2.0 ** -20 + 2.0 ** -23 * z.abs()) + 2.0 ** -30) / (K_TOL * U)


# ------------------------------------------------------------------------------------------ elementwise
def add_ref(a, b, rows):
    c = a.shape[-1]
    x, y = (t.reshape(-1, c)[rows.to(a.device)].to(F64) for t in (a, b))
    return x + y, torch.sqrt(x * x + y * y)


def f32_to_bf16_ref(x, rows):
    """one rounding: the S term is zero."""
    c = x.shape[-1]
    r = x.reshape(-1, c)[rows.to(x.device)].to(F64)
    return r, torch.zeros_like(r)


def transpose_ref(x, rows):
    """[B, R, C] -> [B, C, R] at rows (b * C + c) of the output: exact (S = 0; the bf16 e_out term is not a licence — check
    with exact=True)."""
    b_, r_, c_ = x.shape
    rows = rows.to(x.device)
    b, c = rows // c_, rows % c_
    return x[b, :, c].to(F64), None


def freeu_backbone_ref(x, b, rows):
    c = x.shape[-1]
    xx = x.reshape(-1, c)[rows.to(x.device)].to(F64)
    scale = torch.ones(c, dtype=F64, device=x.device)
    scale[: c // 2] = b
    r = xx * scale
    return r, torch.zeros_like(r)


def freeu_lowfreq_ref(x, s, rows):
    """diffusers fourier_filter (threshold 1): the 2x2 lowest-frequency block (frequencies -1 and 0 on each axis) scaled by s.
    S = |x| + 2 |s - 1| rms over the map's sums (four DFT terms of HW inputs each)."""
    n, h, w, c = x.shape
    rows = rows.to(x.device)
    out_r, out_s = [], []
    for i in torch.unique(rows // (h * w)).tolist():
        xi = x[i].to(F64).permute(2, 0, 1)
        X = torch.fft.fft2(xi)
        m = torch.ones((h, w), dtype=F64, device=x.device)
        for fy in (0, h - 1):
            for fx in (0, w - 1):
                m[fy, fx] = s
        y = torch.fft.ifft2(X * m).real.permute(1, 2, 0).reshape(-1, c)
        sel = rows[rows // (h * w) == i] - i * h * w
        xx = xi.permute(1, 2, 0).reshape(-1, c)
        out_r.append(y[sel])
        out_s.append(xx[sel].abs() + 4 * abs(s - 1) * torch.sqrt((xx * xx).sum(0) / (h * w))[None])
    return torch.cat(out_r), torch.cat(out_s)


# ------------------------------------------------------------------------------------------ loop-state kernels (fp32)
def _f32_chain(n, a):
    """S-equivalent of an fp32 evaluation of n roundings whose running values stay below A = sum of the absolute terms: as in
    conv3x3_nchw_f32_ref, independent roundings of at most 2^-24 A each stay below 2^-24 sqrt(n) A."""
    return a * (2.0 ** -24 * math.sqrt(n) / U)


def _nhwc_to_nchw(t):
    return t.to(F64).permute(0, 3, 1, 2)


def cfg_ddim_step_ref(eps, lat, coef_row, guidance, cfg, B):
    """dc_cfg_ddim_step's new latents: eps NHWC fp32 [(2 if cfg else 1) * B, H, W, C] (CFG: unconditional half first), lat NCHW
    fp32 [B, C, H, W] (the state BEFORE the launch), coef_row the four fp32 values (sqrt(1-a_t), sqrt(a_t), sqrt(a_prev),
    sqrt(1-a_prev)) of the step's table row as stored, guidance as the launch receives it (fp32) -> (r, S) [B, C, H, W]:
        e = eu + g (et - eu)  (cfg)  |  eps;      r = sap (x - s1mat e) / sat + s1map e.
    The kernel is fp32 throughout.  Its roundings, counted from cfg_ddim_kernel: et - eu, g *, eu + (3, CFG only), s1mat * e,
    x -, / sat, sap *, and the final multiply-add (5): n = 8 with CFG, 5 without (a contracted fma only removes roundings).  Every
    intermediate is bounded by the sum of the absolute terms
        A = |sap / sat| (|x| + |s1mat| Ae) + |s1map| Ae,      Ae = |eu| + |g| (|et| + |eu|)   (|eps| without CFG),
    which also carries the cancellation between sap s1mat / sat and s1map at small steps."""
    s1mat, sat, sap, s1map = (float(v) for v in torch.as_tensor(coef_row, dtype=torch.float32).reshape(4).to(F64).tolist())
    g = float(torch.tensor(float(guidance), dtype=torch.float32).to(F64))
    x = lat.to(F64)
    e_all = _nhwc_to_nchw(eps)
    if cfg:
        eu, et = e_all[:B], e_all[B:2 * B]
        e = eu + g * (et - eu)
        ae = eu.abs() + abs(g) * (et.abs() + eu.abs())
        n = 8
    else:
        e = e_all[:B]
        ae = e.abs()
        n = 5
    r = sap * (x - s1mat * e) / sat + s1map * e
    a = abs(sap / sat) * (x.abs() + abs(s1mat) * ae) + abs(s1map) * ae
    return r, _f32_chain(n, a)


VAE_LOGVAR_MIN, VAE_LOGVAR_MAX = -30.0, 20.0


def vae_sample_latents_ref(moments, noise, scale):
    """dc_vae_sample_latents (diffusers DiagonalGaussianDistribution.sample, times the scaling factor): moments NHWC fp32
    [N, H, W, 2C] = (mean | log-variance), noise NCHW fp32 [N, C, H, W] -> (r, S) [N, C, H, W]:
        r = (mean + exp(0.5 clamp(lv, -30, 20)) z) scale.
    Roundings: 0.5 lv is exact; expf, * z, mean +, * scale: n = 4.  expf evaluates to a couple of ulps and amplifies the rounding
    of its argument by |0.5 lv|, so the noise term t = exp(.) z enters with the weight 2 + |0.5 lv|:
        A = (|mean| + |t| (2 + |0.5 lv|)) |scale|."""
    c = noise.shape[1]
    mean, lv = _nhwc_to_nchw(moments[..., :c]), _nhwc_to_nchw(moments[..., c:])
    sc = float(torch.tensor(float(scale), dtype=torch.float32).to(F64))
    half = 0.5 * lv.clamp(VAE_LOGVAR_MIN, VAE_LOGVAR_MAX)
    t = torch.exp(half) * noise.to(F64)
    r = (mean + t) * sc
    a = (mean.abs() + t.abs() * (2 + half.abs())) * abs(sc)
    return r, _f32_chain(4, a)


def latents_to_model_input_ref(lat, mul, rep=1):
    """dc_latents_to_model_input: lat NCHW fp32 [B, C, H, W] -> (r, S) [rep * B, H, W, C], the bf16 NHWC model input lat * mul
    repeated `rep` times along the batch.  One fp32 product, then the output rounding (e_out): S = |r| 2^-24 / U."""
    m = float(torch.tensor(float(mul), dtype=torch.float32).to(F64))
    r = (lat.to(F64) * m).permute(0, 2, 3, 1).repeat(rep, 1, 1, 1)
    return r, r.abs() * (2.0 ** -24 / U)


def timestep_embedding_ref(t, n, dim):
    """[n, dim] fp32 = [cos(t f_k), sin(t f_k)], f_k = exp(-ln(10^4) k / half).  The kernel forms the argument in fp32: S covers
    4 ulps of the argument (|t f_k| 2^-22) plus the fp32 rounding of f_k itself."""
    half = dim // 2
    k = torch.arange(half, dtype=F64)
    f = torch.exp(-math.log(10000.0) * k / half)
    a = float(t) * f
    r = torch.cat([torch.cos(a), torch.sin(a)])[None].expand(n, dim)
    s = (a.abs() * 2.0 ** -20 / (K_TOL * U)).repeat(2)[None].expand(n, dim)
    return r, s


# ------------------------------------------------------------------------------------------ control stage (fp32 NCHW)
EPS_SPLAT = float(np.float32(0.0000001))           # the constants as the kernels hold them (fp32)
EPS_FUSE = float(np.float32(1e-6))
OCC_THRESHOLD = float(np.float32(0.3))
F32_TINY = 2.0 ** -126                             # smallest normal fp32: below it a reciprocal is flushed to zero


def _splat_accumulate(planes, flow):
    """Forward (summation) splat in fp64 of `planes` [N, C, H, W] (fp64) along flow [N, 2, H, W] (fp32) -> (sum, count k of the
    sources that reach each target [N, 1, H, W]).  The landing point (x + fx, y + fy) is formed in fp32, as the kernel and the
    reference kernel form it (in fp64 its floor could name another cell); everything after it is fp64.  Non-finite landing
    points are skipped; the corner weights are those of softsplat.py:315-318."""
    n, c, h, w = planes.shape
    dev = planes.device
    gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=dev), torch.arange(w, dtype=torch.float32, device=dev),
                            indexing="ij")
    fx = gx[None] + flow[:, 0].to(torch.float32)
    fy = gy[None] + flow[:, 1].to(torch.float32)
    fin = torch.isfinite(fx) & torch.isfinite(fy)
    fx = torch.where(fin, fx, torch.zeros_like(fx)).to(F64)
    fy = torch.where(fin, fy, torch.zeros_like(fy)).to(F64)
    x0, y0 = torch.floor(fx), torch.floor(fy)
    out = torch.zeros((n, c, h * w), dtype=F64, device=dev)
    cnt = torch.zeros((n, 1, h * w), dtype=F64, device=dev)
    src = planes.reshape(n, c, h * w)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        cx, cy = x0 + dx, y0 + dy
        wx = (x0 + 1 - fx) if dx == 0 else (fx - x0)
        wy = (y0 + 1 - fy) if dy == 0 else (fy - y0)
        ok = fin & (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h)
        wgt = torch.where(ok, wx * wy, torch.zeros_like(wx)).reshape(n, 1, h * w)
        idx = torch.where(ok, cy * w + cx, torch.zeros_like(cx)).long().reshape(n, 1, h * w)
        out.scatter_add_(2, idx.expand(n, c, h * w), src * wgt)
        cnt.scatter_add_(2, idx, ok.reshape(n, 1, h * w).to(F64))
    return out.reshape(n, c, h, w), cnt.reshape(n, 1, h, w)


def splat_sum_ref(x, flow):
    """dc_splat_sum_f32: out = sum over sources of in * w -> (r, S, k).  Per target k products in * w (the weight itself carries
    the roundings of its two factors and of their product) and k additions: n = 3 k + 1, A = sum |in * w|."""
    xx = x.to(F64)
    r, k = _splat_accumulate(xx, flow)
    a, _ = _splat_accumulate(xx.abs(), flow)
    return r, a * (2.0 ** -24 / U) * torch.sqrt(3 * k + 1), k


def splat_soft_ref(x, flow, metric, mask=None):
    """dc_splat_soft_f32 (softsplat 'soft' mode + FeatureWarperSoftsplat's mask multiply) -> (r, S, k):
        r = sum in e w / (sum e w + 1e-7) [* (1 - mask)],      e = exp(metric) of the source.
    Roundings per target with k sources, counted from splat_gather_kernel<1>: in * e, * w and the addition per term of the
    numerator (3 k), e * w and the addition per term of the denominator (2 k, they enter through |r| den below), then + 1e-7, the
    divide, 1 - mask and the mask product (4); expf is good to 2 ulp per term, which the factor K_TOL of the check covers.  The
    running values of numerator and denominator stay below their sums of absolute terms, so the error of the quotient stays below
        2^-24 sqrt(3 k + 4) A,      A = (sum |in e w| + |r| den) / (den + 1e-7)."""
    xx, e = x.to(F64), torch.exp(metric.to(F64))
    n, c = xx.shape[:2]
    acc, k = _splat_accumulate(torch.cat([xx * e, e, xx.abs() * e], 1), flow)
    num, den, anum = acc[:, :c], acc[:, c:c + 1], acc[:, c + 1:]
    r = num / (den + EPS_SPLAT)
    a = (anum + r.abs() * den) / (den + EPS_SPLAT)
    if mask is not None:
        keep = 1.0 - mask.to(F64)
        r, a = r * keep, a * keep.abs()
    return r, a * (2.0 ** -24 / U) * torch.sqrt(3 * k + 4), k


def occlusion_mask_ref(flow_a, flow_b):
    """dc_occlusion_mask_f32 (compute_mask, control_utils.py:11-17) -> dict(norm, mask, delta), each [N, 1, H, W]:
        norm = || b + splat_soft(a, b, ones) ||_2 in fp64,   mask = norm > 0.3 (the threshold as fp32 holds it),
    delta = the bound on the fp32 kernel's own norm: the bound of each splat component (the gradient of the norm has length <= 1, so
    they add) plus the five roundings of b + ., the squares, their sum and the root, each below 2^-24 of |b| + |r|.  A device mask
    may differ from `mask` only where |norm - 0.3| <= delta (check_occlusion_mask)."""
    r, s, _ = splat_soft_ref(flow_a, flow_b, torch.ones_like(flow_b[:, :1]))
    b = flow_b.to(F64)
    d = b + r
    norm = torch.sqrt((d * d).sum(1, keepdim=True))
    t = E_OUT_F32 * r.abs() + K_TOL * U * s
    delta = t.sum(1, keepdim=True) + K_TOL * 2.0 ** -24 * math.sqrt(5) * (b.abs() + r.abs()).sum(1, keepdim=True)
    return dict(norm=norm, mask=(norm > OCC_THRESHOLD).to(F64), delta=delta)


def check_occlusion_mask(y, ref):
    """y: the launch's mask [N, 1, H, W].  Every value must be exactly 0.0 or 1.0; outside the band |norm - 0.3| <= delta it must equal
    the reference mask; inside the band either value passes.  -> dict(ok, flips, not_binary, band = share of pixels inside the band,
    ones = share of reference pixels that are 1)."""
    yy = y.to(F64)
    binary = (yy == 0.0) | (yy == 1.0)
    band = (ref["norm"] - OCC_THRESHOLD).abs() <= ref["delta"]
    flips = int(((yy != ref["mask"]) & ~band).sum())
    not_binary = int((~binary).sum())
    return dict(ok=flips == 0 and not_binary == 0, flips=flips, not_binary=not_binary, band=float(band.to(F64).mean()),
                ones=float(ref["mask"].mean()))


def flow_resize_ref(flow2, h, w, div_x, div_y):
    """dc_flow_resize_normalize_f32 (div = ((w - 1) / 2, (h - 1) / 2)) and dc_flow_resize_divide_f32: F.interpolate(bilinear,
    align_corners=False) of flow2 [N, 2, H, W] (any batch stride) to (h, w), the source index clamped at 0, component 0 divided by
    div_x and component 1 by div_y -> (r, S) [N, 2, h, w].
    The kernel forms the source coordinate f = (H / h) (o + 0.5) - 0.5 in fp32 (the ratio, the product and the difference: three
    roundings of at most 2^-24 (|f| + 0.5) each), which moves the interpolation weight; the interpolant is continuous and piecewise
    linear, so that moves the value by at most the coordinate error times the local slope.  The value path has 12 roundings (1 - l
    twice, four products and two sums inside, two products and a sum outside, the divide):
        A = (sum |w_ij s_ij| + 3 (|fy| + 0.5) |slope_y| + 3 (|fx| + 0.5) |slope_x|) / |div|."""
    n, _, hh, ww = flow2.shape
    dev = flow2.device
    s = flow2.to(F64)

    def axis(size_in, size_out):
        f = (size_in / size_out) * (torch.arange(size_out, dtype=F64, device=dev) + 0.5) - 0.5
        f = f.clamp_min(0.0)
        i0 = torch.floor(f).long().clamp_max(size_in - 1)
        i1 = (i0 + 1).clamp_max(size_in - 1)
        return f, i0, i1, f - i0

    fy, y0, y1, ly = axis(hh, h)
    fx, x0, x1, lx = axis(ww, w)
    ly, lx = ly[:, None], lx[None, :]
    hy, hx = 1 - ly, 1 - lx
    s00, s01 = s[:, :, y0][:, :, :, x0], s[:, :, y0][:, :, :, x1]
    s10, s11 = s[:, :, y1][:, :, :, x0], s[:, :, y1][:, :, :, x1]
    div = torch.tensor([float(np.float32(div_x)), float(np.float32(div_y))], dtype=F64, device=dev).reshape(1, 2, 1, 1)
    r = (hy * (hx * s00 + lx * s01) + ly * (hx * s10 + lx * s11)) / div
    a = hy * (hx * s00.abs() + lx * s01.abs()) + ly * (hx * s10.abs() + lx * s11.abs())
    slope_y = hx * (s10 - s00).abs() + lx * (s11 - s01).abs()
    slope_x = hy * (s01 - s00).abs() + ly * (s11 - s10).abs()
    a = a + 3 * (fy[:, None] + 0.5) * slope_y + 3 * (fx[None, :] + 0.5) * slope_x
    return r, _f32_chain(12, a / div.abs())


def flow_hw2_resize_scale_ref(src_hw2, th, tw):
    """dc_flow_hw2_resize_scale_f32: F.interpolate(bilinear, align_corners=True) of a [H, W, 2] flow (the .flo payload layout) to
    [2, th, tw], component 0 multiplied by tw / W and component 1 by th / H -> (r, S).
    The source index follows the kernel and ATen in fp32: scale = (H - 1) / (th - 1) (0 when th = 1) and f = scale * o, each rounded
    to fp32; i0 = floor(f), the weight l = f - i0 is then exact.  The multipliers are the fp32 values of tw / W and th / H.  Values in
    fp64.  The value path has 12 roundings (1 - l twice, four products and two sums inside, two products and a sum outside, the
    multiply) of running values below A = |mul| sum |weight tap|."""
    hh, ww, _ = src_hw2.shape
    dev = src_hw2.device
    s = src_hw2.to(F64)

    def axis(size_in, size_out):
        scale = np.float32(size_in - 1) / np.float32(size_out - 1) if size_out > 1 else np.float32(0)
        f = (scale * np.arange(size_out, dtype=np.float32)).astype(np.float32)
        i0 = np.minimum(f.astype(np.int64), size_in - 1)
        i1 = np.minimum(i0 + 1, size_in - 1)
        lam = (f - i0.astype(np.float32)).astype(np.float64)
        return torch.from_numpy(i0).to(dev), torch.from_numpy(i1).to(dev), torch.from_numpy(lam).to(dev)

    y0, y1, ly = axis(hh, th)
    x0, x1, lx = axis(ww, tw)
    ly, lx = ly[:, None, None], lx[None, :, None]
    hy, hx = 1 - ly, 1 - lx
    s00, s01, s10, s11 = s[y0][:, x0], s[y0][:, x1], s[y1][:, x0], s[y1][:, x1]                 # [th, tw, 2]
    mul = torch.tensor([float(np.float32(tw / ww)), float(np.float32(th / hh))], dtype=F64, device=dev)
    r = (hy * (hx * s00 + lx * s01) + ly * (hx * s10 + lx * s11)) * mul
    a = (hy * (hx * s00.abs() + lx * s01.abs()) + ly * (hx * s10.abs() + lx * s11.abs())) * mul.abs()
    return r.permute(2, 0, 1).contiguous(), _f32_chain(12, a.permute(2, 0, 1).contiguous())


def blend_tiles_ramp_ref(tiles, coords, h, w, feather, scale):
    """dc_blend_tiles_ramp_u8 before its rounding: the weighted mean of the tiles covering each pixel, clipped to [0, 255], in fp64
    -> [h, w, C].  Weight of a tile at a pixel = ramp_y ramp_x, ramp[i] = 0.5 - 0.5 cos(pi (i + 0.5) / feather) over the `feather`
    pixels next to a tile edge that lies inside the frame, 1 elsewhere (the policy of tiling.merge_ramp, restated independently:
    tiles [T, C, th, tw], coords (y1, y2, x1, x2))."""
    t = tiles.detach().cpu().to(F64) * float(np.float32(scale))
    c = t.shape[1]
    acc, wsum = torch.zeros(c, h, w, dtype=F64), torch.zeros(h, w, dtype=F64)
    ramp = torch.tensor([0.5 - 0.5 * math.cos(math.pi * (i + 0.5) / feather) for i in range(feather)], dtype=F64)

    def axis(n, lo_inner, hi_inner):
        v = torch.ones(n, dtype=F64)
        if feather and lo_inner:
            v[:feather] = ramp
        if feather and hi_inner:
            v[n - feather:] = ramp.flip(0)
        return v

    for k, (y1, y2, x1, x2) in enumerate(coords):
        m = axis(y2 - y1, y1 > 0, y2 < h)[:, None] * axis(x2 - x1, x1 > 0, x2 < w)[None, :]
        acc[:, y1:y2, x1:x2] += t[k] * m
        wsum[y1:y2, x1:x2] += m
    return (acc / wsum).clamp(0.0, 255.0).permute(1, 2, 0).contiguous()


def fuse_warped_ref(wf, wl, cf, cb, of=None, ob=None):
    """dc_fuse_warped_f32 (extractors.py:297-310): a = max(cf, 0), b = max(cb, 0), fused = a / (a + b + 1e-6) wf + b / (a + b + 1e-6) wl,
    and 0.5 (wf + wl) where of + ob > 1.5 -> (r, S) [N, C, H, W].  Seven roundings (two sums in the denominator, two divides, two
    products, the sum), A = (a |wf| + b |wl|) / (a + b + 1e-6); in a hole A = 0.5 (|wf| + |wl|)."""
    f, l = wf.to(F64), wl.to(F64)
    a, b = cf.to(F64).clamp_min(0.0), cb.to(F64).clamp_min(0.0)
    ws = a + b + EPS_FUSE
    r = a / ws * f + b / ws * l
    aa = a / ws * f.abs() + b / ws * l.abs()
    if of is not None:
        hole = (of.to(F64) + ob.to(F64)) > 1.5
        r = torch.where(hole, 0.5 * (f + l), r)
        aa = torch.where(hole, 0.5 * (f.abs() + l.abs()), aa)
    return r, _f32_chain(7, aa)


def silu_f32_ref(x):
    """dc_silu_f32: y = x / (1 + exp(-x)) as x * rcp(1 + exp2(-x log2 e)).  Roundings: the argument product, exp2, 1 +, the reciprocal,
    the product: n = 5.  The rounding of the exponent's argument (2^-24 |x|) and the 2 ulp of the exponential move e = exp(-x)
    by a relative (2 + |x|) 2^-24, and the result by e / (1 + e) = 1 - sigmoid(x) of that:
        A = |y| (1 + (1 - sigmoid(x)) (2 + |x|)),
    plus |x| 2^-126 for a reciprocal below the smallest normal number, which the hardware flushes to zero."""
    z = x.to(F64)
    sg = torch.sigmoid(z)
    r = z * sg
    a = r.abs() * (1 + (1 - sg) * (2 + z.abs()))
    return r, _f32_chain(5, a) + z.abs() * (F32_TINY / (K_TOL * U))


def add_f32_ref(a, b):
    """dc_add_f32: one correctly rounded sum, A = |r|."""
    r = a.to(F64) + b.to(F64)
    return r, _f32_chain(1, r.abs())


def lincomb_ref(terms):
    """dc_lincomb4_f32: [(coef, tensor)] of 1 to 4 terms, coefficients as fp32 holds them: v = c0 x0, then one fused multiply-add
    per further term, in term order: one rounding per term, A = sum |c_i x_i|."""
    assert 1 <= len(terms) <= 4
    r, a = 0.0, 0.0
    for c, t in terms:
        c = float(np.float32(c))
        r = r + c * t.to(F64)
        a = a + abs(c) * t.to(F64).abs()
    return r, _f32_chain(len(terms), a)


def postprocess_image_ref(x):
    """dc_postprocess_image's fp32 output: x NHWC fp32 [N, H, W, C] (any pixel stride) -> (r, S) NCHW: clamp(x / 2 + 0.5, 0, 1).  The
    halving is exact; one rounding in the sum, A = |x| / 2 + 0.5.  (The uint8 output is round-half-even(255 o32) of the launch's
    own fp32 output, compared exactly by the tests.)"""
    z = x.to(F64).permute(0, 3, 1, 2)
    return (z / 2 + 0.5).clamp(0.0, 1.0), _f32_chain(1, z.abs() / 2 + 0.5)


def nchw_f32_to_nhwc_bf16_ref(x):
    """exact: the permutation and one round-to-nearest-even to bf16 (compare bit for bit)"""
    return x.permute(0, 2, 3, 1).to(torch.bfloat16)


def nhwc_to_nchw_f32_ref(x):
    """exact: the permutation (bf16 -> fp32 widens exactly)"""
    return x.permute(0, 3, 1, 2).to(torch.float32)


def embed_tokens_ref(ids, tok_emb, pos_emb):
    """exact: the fp32 sum of two bf16 values, rounded once to bf16 (in-range ids only)"""
    t = ids.shape[1]
    return (tok_emb[ids].to(torch.float32) + pos_emb[:t].to(torch.float32)[None]).to(torch.bfloat16)
