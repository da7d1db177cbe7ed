"""CPU restatement of the model blocks the device assembles from launches (blocks.py, vae.py), with the device's rounding points
as a parameter, plus the case table, the input families and the named wiring faults that tests/test_block_ref.py (CPU) and
tests/test_gpu_blocks.py (GPU) share.  Nothing here imports the package: torch only.

Every block function works over a flat diffusers-layout state dict of fp64 tensors and logical NCHW / [B, L, C] fp64 activations.
    q      the rounding applied at the device's rounding points.  `ident` (fp64 throughout) is the REFERENCE: it is pinned to
           oracle/sd15_ref.py cast to fp64 at 1e-12 by tests/test_block_ref.py, so it is that oracle, not a second opinion.
           `bf16` (fp64 -> fp32 -> bf16, widened again) is the EMULATION of the device arithmetic.
    fault  None, or one name of FAULTS: a wiring mistake of the restatement, used only to show what the bars reject.

The bars.  Per case two figures, no element excluded: rel_l2 = |y - r|_2 / |r|_2 and max_rel = max|y - r| / max|r|, r the fp64
reference.  The bar of each figure is MARGIN = 4 times the emulation's own figure on that case (DESIGN.md §12's margin).

Rounding points of the emulation, each with the device code that rounds there (paths under the package directory):
  R1  stored activations are bf16: every conv / linear epilogue rounds its fp32 value once, after bias, the fp32 time-embedding
      row, the activation, out_scale and the residual                               csrc/gemm_dma.hip:279-291, dc_common.h:70-77
  R2  packed weights are bf16                                                       ops.py:104
  R3  a folded LayerNorm rounds W * gamma (the product, once); b' = b + W beta and colsum(W') stay fp32, and the epilogue forms
      rstd * (x W'^T - mean * colsum) + b' in fp32                                  ops.py:77-84,107-108, csrc/dc_common.h:79-86
  R4  GroupNorm affine (+ SiLU) applied on load or by the standalone pass: x * a + b (and SiLU) in fp32, one rounding to bf16
      before the MFMA / the store; the same for the affine without SiLU in front of proj_in, on every route
                                          csrc/conv3x3_tile.hip:199-206, csrc/igemm.hip:158-160, csrc/norm.hip:222-231, dc_common.h:91-98
  R5  attention probabilities are rounded to bf16 in registers before the PV MFMA; the output is O / l rounded once
                                                                                    csrc/attention.hip:335-336,358-359,438,452
  R6  head dims that are not a multiple of 32 take the softmax denominator from the ROUNDED probabilities (the ones column of V inside
      the PV MFMA)                                                                  csrc/attention.hip:97-104
  R7  head dims that are not a multiple of 16, except in the short-context form, multiply the queries by scale * log2(e) and round them
      to bf16 before QK^T                                                           csrc/attention.hip:34-37,102,158
  R8  GEGLU: h * gelu(g) formed in fp32 from the two accumulators (bias and LayerNorm fold applied), rounded once
                                                                                    csrc/gemm_dma.hip:262-269
  R9  the standalone LayerNorm (LN_FOLD = False) reads the stored bf16 rows and stores bf16                ops.py:473-479
  R10 the time embedding: the fp32 sinusoid is rounded to bf16 (ops.f32_to_bf16, blocks.py:57), linear_1 and linear_2 store
      bf16 after their fused SiLU (blocks.py:58-59)
  R11 the VAE attention: q, k, v stored bf16; scores fp32 (out_f32); softmax rows normalised in fp32 and rounded to bf16
      (csrc/attention.hip:740); PV and to_out store bf16                            vae.py:39-48
Kept in fp32 on the device, so NOT rounded here: GroupNorm (scale, shift) pairs and LayerNorm (mean, rstd); biases; accumulators;
the batched time_emb_proj output (`out_f32`, blocks.py:60) and its row add; VAE attention scores.  Statistics that a producer's
epilogue emits (GroupNorm partials `gn_part`, LayerNorm row sums `stats_out`) are sums of the fp32 values BEFORE the output's
rounding (csrc/gemm_dma.hip:293-299): the emulation takes them from the unrounded value (`Act.pre`).  Where a launch cannot
emit the GroupNorm partials the device measures the stored tensor instead; the emulation still uses the unrounded value there:
the two differ by the mean of independent half-ulp roundings over a group, a relative 2^-9 / sqrt(count) of the statistics.

The `timestep_embedding` sinusoid is computed in fp32 exactly as the oracle computes it and widened (it is an fp32 value on the
device too, csrc/elementwise.hip dc_timestep_embedding_f32); all else is fp64.
"""
import collections
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
MARGIN = 4.0
LOG2E = 1.4426950408889634


def ident(x):
    return x


def bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


class Act:
    """A stored activation: `v` as stored (rounded), `pre` the fp32 value before the rounding (what epilogue statistics see)."""
    __slots__ = ("v", "pre")

    def __init__(self, v, pre=None):
        self.v, self.pre = v, v if pre is None else pre


def as_act(x):
    return x if isinstance(x, Act) else Act(x)


def figures(y, r):
    """(rel_l2, max_rel) of y against the reference r, every element."""
    y, r = y.to(F64), r.to(F64)
    d = y - r
    return float(d.norm() / r.norm()), float(d.abs().max() / r.abs().max())


# ------------------------------------------------------------------------------------------ primitives
def _bias(sd, k):
    b = sd.get(k + ".bias")
    return None if b is None else b


def conv(sd, k, x, q, *, stride=1, padding=1, row_add=None, residual=None, act=False, out_scale=1.0, upsample=False, f32_out=False):
    """One `ops.conv` launch on NCHW: R2 on the weight, R1 on the result.  x: the stored input (already rounded)."""
    w = sd[k + ".weight"]
    if w.dim() == 2:
        w = w[:, :, None, None]
    if upsample:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    y = F.conv2d(x, q(w), _bias(sd, k), stride=stride, padding=padding if w.shape[-1] == 3 else 0)
    if row_add is not None:
        y = y + row_add[:, :, None, None]
    if act:
        y = F.silu(y)
    y = y * out_scale
    if residual is not None:
        y = y + residual
    return Act(y if f32_out else q(y), y)


def linear(sd, k, x, q, *, residual=None, act=False, f32_out=False, weight=None, bias=None):
    w = sd[k + ".weight"] if weight is None else weight
    b = _bias(sd, k) if weight is None else bias
    y = x @ q(w).T
    if b is not None:
        y = y + b
    if act:
        y = F.silu(y)
    if residual is not None:
        y = y + residual
    return Act(y if f32_out else q(y), y)


def gn_ab(src, gamma, beta, groups, eps):
    """GroupNorm statistics folded with the affine: (scale, shift) [N, C, 1, 1] (fp32 on the device: unrounded)."""
    n, c = src.shape[:2]
    g = src.reshape(n, groups, -1)
    mean = g.mean(2)
    var = (g * g).mean(2) - mean * mean
    rstd = 1.0 / torch.sqrt(var.clamp_min(0) + eps)
    cg = c // groups
    a = gamma[None] * rstd.repeat_interleave(cg, 1)
    b = beta[None] - mean.repeat_interleave(cg, 1) * a
    return a[:, :, None, None], b[:, :, None, None]


def gn_apply(x, ab, q, silu):
    y = x * ab[0] + ab[1]                                                 # R4
    return q(F.silu(y) if silu else y)


def row_mean_rstd(src, eps):
    mean = src.mean(-1, keepdim=True)
    var = (src * src).mean(-1, keepdim=True) - mean * mean
    return mean, 1.0 / torch.sqrt(var.clamp_min(0) + eps)


def ln_linear(sd, lnk, wk, t, q, fold, eps, *, weight=None, bias=None):
    """Linear(LayerNorm(t)) -> fp32 value before the output rounding.  fold: R3 (statistics of t.pre); else R9 + a plain linear."""
    gamma, beta = sd[lnk + ".weight"], sd[lnk + ".bias"]
    w = sd[wk + ".weight"] if weight is None else weight
    b = _bias(sd, wk) if weight is None else bias
    if fold:
        mean, rstd = row_mean_rstd(t.pre, eps)
        wf = q(w * gamma[None])
        bf = w @ beta if b is None else b + w @ beta
        return rstd * (t.v @ wf.T - mean * wf.sum(1)[None]) + bf
    mean, rstd = row_mean_rstd(t.v, eps)
    n = q((t.v - mean) * rstd * gamma + beta)
    y = n @ q(w).T
    return y if b is None else y + b


def attn_short(b, heads, nq, nk, d):
    """Mirror of the SHORT decision of attn_form (csrc/attention.hip:663-686); tests/test_block_ref.py holds it to
    ops.attention_route on every attention shape of the table."""
    short_ctx = nk <= 128
    if d <= 48:
        wgs2 = b * heads * ((nq + 255) // 256)
        if wgs2 >= 512:
            return short_ctx and (b * heads * ((nq + 127) // 128) // 4 >= 512 or wgs2 // 4 >= 512)
    return short_ctx and b * heads * ((nq + 127) // 128) // 4 >= 512


def attention(qm, km, vm, heads, q, *, scale=None, batch=None, interleaved=False, chunk=1024):
    """softmax(Q K^T scale) V on [B, L, C] with R5-R7.  `batch`: the device launch's batch (the form choice depends on it) when
    only some of its samples are computed here."""
    b, nq, c = qm.shape
    nk = km.shape[1]
    d = c // heads
    sc = d ** -0.5 if scale is None else scale
    short = attn_short(b if batch is None else batch, heads, nq, nk, d)

    def split(t):
        if interleaved:                                                   # fault: channel c belongs to head c % heads
            return t.reshape(t.shape[0], t.shape[1], d, heads).permute(0, 3, 1, 2)
        return t.reshape(t.shape[0], t.shape[1], heads, d).transpose(1, 2)

    qh, kh, vh = split(qm), split(km), split(vm)
    qs = qh * (sc * LOG2E)
    if d % 16 != 0 and not short:
        qs = q(qs)                                                        # R7
    outs = []
    for i in range(0, nq, chunk):
        t = qs[:, :, i:i + chunk] @ kh.transpose(2, 3)
        p = torch.exp2(t - t.amax(-1, keepdim=True))
        pr = q(p)                                                         # R5
        l = (pr if d % 32 != 0 else p).sum(-1, keepdim=True)              # R6
        outs.append(q((pr @ vh) / l))
    o = torch.cat(outs, 2)
    if interleaved:
        return o.permute(0, 2, 3, 1).reshape(b, nq, c)
    return o.transpose(1, 2).reshape(b, nq, c)


def _gelu(g):
    return 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))


# ------------------------------------------------------------------------------------------ time embedding
def timestep_sinusoid(t, n, dim):
    """diffusers Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0), fp32 as in the oracle, widened."""
    t = torch.as_tensor(t, dtype=torch.float32).reshape(-1)
    t = t.expand(n) if t.numel() == 1 else t
    half = dim // 2
    exponent = -math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half
    emb = t[:, None].float() * torch.exp(exponent)[None]
    return torch.cat([torch.cos(emb), torch.sin(emb)], dim=-1).to(F64)


def time_embedding(sd, t, n, ch0, prefixes, q=ident, fault=None):
    """TimeEmbedding: -> {prefix: fp32 row [n, cout]} — the batched time_emb_proj GEMM, sliced per ResnetBlock (R10)."""
    e = q(timestep_sinusoid(t, n, ch0))
    e = linear(sd, "time_embedding.linear_1", e, q, act=True).v
    e = linear(sd, "time_embedding.linear_2", e, q, act=fault != "temb_no_silu").v
    w = torch.cat([sd[p + "time_emb_proj.weight"] for p in prefixes], 0)
    b = torch.cat([sd[p + "time_emb_proj.bias"] for p in prefixes], 0)
    allrows = linear(sd, None, e, q, f32_out=True, weight=w, bias=b).v
    out, off = {}, 0
    spans = []
    for p in prefixes:
        co = sd[p + "time_emb_proj.weight"].shape[0]
        spans.append((off, off + co))
        off += co
    for i, p in enumerate(prefixes):
        a, z = spans[(i + 1) % len(spans)] if fault == "temb_slice_of_next_block" else spans[i]
        out[p] = allrows[:, a:z]
    return out


# ------------------------------------------------------------------------------------------ ResnetBlock
def resnet(sd, p, x, temb_row, groups, eps, q=ident, x2=None, fault=None):
    """ResnetBlock.__call__: x (and the skip x2) stored NCHW; temb_row fp32 [n, cout] or None.  -> Act."""
    if fault in ("gn_eps_1e-6", "vae_gn_eps_1e-5"):
        eps = 1e-6 if fault == "gn_eps_1e-6" else 1e-5
    parts = [as_act(x)] if x2 is None else ([as_act(x2), as_act(x)] if fault == "concat_order" else [as_act(x), as_act(x2)])
    xin, xpre = torch.cat([t.v for t in parts], 1), torch.cat([t.pre for t in parts], 1)
    h0 = gn_apply(xin, gn_ab(xpre, sd[p + "norm1.weight"], sd[p + "norm1.bias"], groups, eps), q, True)
    row = None if (temb_row is None or fault == "no_temb") else temb_row
    h = conv(sd, p + "conv1", h0, q, row_add=row)
    h1 = gn_apply(h.v, gn_ab(h.pre, sd[p + "norm2.weight"], sd[p + "norm2.bias"], groups, eps), q, True)
    if (p + "conv_shortcut.weight") in sd:
        sc = conv(sd, p + "conv_shortcut", h0 if fault == "shortcut_of_normed_input" else xin, q).v
    else:
        sc = h0 if fault == "shortcut_of_normed_input" else xin
    return conv(sd, p + "conv2", h1, q, residual=sc)


# ------------------------------------------------------------------------------------------ TransformerBlock
def transformer(sd, p, x, ctx, heads, groups, q=ident, fold=True, fault=None, batch=None):
    """TransformerBlock.__call__ (cfg_shared or not: the same values).  x stored NCHW [B, C, H, W]; ctx stored [B, T, D].  -> Act."""
    x, xpre = as_act(x).v, as_act(x).pre
    b, c, h, w = x.shape
    ab = gn_ab(xpre, sd[p + "norm.weight"], sd[p + "norm.bias"], groups, 1e-5 if fault == "norm_eps_1e-5" else 1e-6)
    xn = gn_apply(x, ab, q, False)
    t = conv(sd, p + "proj_in", xn, q)
    t = Act(t.v.permute(0, 2, 3, 1).reshape(b, h * w, c), t.pre.permute(0, 2, 3, 1).reshape(b, h * w, c))
    tb = p + "transformer_blocks.0."
    eps = 1e-6 if fault == "ln_eps_1e-6" else 1e-5
    if fault == "cfg_context_halves_swapped":
        ctx = torch.cat([ctx[b // 2:], ctx[:b // 2]], 0)
    kw = dict(scale=(c // heads) ** -1.0 if fault == "attn_scale_1_over_d" else None, batch=batch,
              interleaved=fault == "heads_interleaved")

    def normed(t_, lnk):                                                  # fault only: the LayerNorm output as a tensor
        mean, rstd = row_mean_rstd(t_.v, eps)
        return (t_.v - mean) * rstd * sd[lnk + ".weight"] + sd[lnk + ".bias"]

    # self-attention
    wqkv = torch.cat([sd[tb + f"attn1.to_{n}.weight"] for n in "qkv"], 0)
    qkv = q(ln_linear(sd, tb + "norm1", None, t, q, fold, eps, weight=wqkv, bias=None))
    a = attention(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], heads, q, **kw)
    t = linear(sd, tb + "attn1.to_out.0", a, q, residual=normed(t, tb + "norm1") if fault == "residual_from_normed" else t.v)
    # cross-attention
    q2 = q(ln_linear(sd, tb + "norm2", tb + "attn2.to_q", t, q, fold, eps))
    wkv = torch.cat([sd[tb + "attn2.to_k.weight"], sd[tb + "attn2.to_v.weight"]], 0)
    kv = linear(sd, None, ctx, q, weight=wkv, bias=None).v
    a = attention(q2, kv[..., :c], kv[..., c:], heads, q, **kw)
    t = linear(sd, tb + "attn2.to_out.0", a, q, residual=t.v)
    # GEGLU feed-forward
    hg = ln_linear(sd, tb + "norm3", tb + "ff.net.0.proj", t, q, fold, eps)
    hid, gate = hg.chunk(2, dim=-1)
    if fault == "geglu_halves_swapped":
        hid, gate = gate, hid
    f = q(hid * _gelu(gate))                                              # R8
    t = linear(sd, tb + "ff.net.2", f, q, residual=t.v)
    y = t.v.reshape(b, h, w, c).permute(0, 3, 1, 2)
    return conv(sd, p + "proj_out", y, q, residual=None if fault == "proj_out_residual_dropped" else x)


# ------------------------------------------------------------------------------------------ samplers
def downsample(sd, k, x, q=ident, fault=None):
    """Downsample2D of the UNet: 3x3 stride 2, padding 1."""
    return conv(sd, k, as_act(x).v, q, stride=2)


def upsample_conv(sd, k, x, q=ident, fault=None):
    """Upsample2D: nearest 2x, then the 3x3 conv (the device fuses the upsample into the conv's load: exact)."""
    x = as_act(x).v
    if fault == "upsample_after_conv":
        y = conv(sd, k, x, q)
        return Act(F.interpolate(y.v, scale_factor=2.0, mode="nearest"))
    return conv(sd, k, x, q, upsample=True)


def vae_downsample(sd, k, x, q=ident, fault=None):
    """Downsample2D of the VAE encoder: F.pad(x, (0, 1, 0, 1)), then 3x3 stride 2 without padding."""
    if fault == "vae_symmetric_pad":
        return conv(sd, k, x, q, stride=2, padding=1)
    return conv(sd, k, F.pad(x, (0, 1, 0, 1)), q, stride=2, padding=0)


# ------------------------------------------------------------------------------------------ VAE
def vae_attention(sd, p, x, groups, q=ident, fault=None):
    b, c, h, w = x.shape
    ab = gn_ab(x, sd[p + "group_norm.weight"], sd[p + "group_norm.bias"], groups, 1e-5 if fault == "vae_gn_eps_1e-5" else 1e-6)
    y = gn_apply(x, ab, q, False).reshape(b, c, h * w).transpose(1, 2)
    qm, km, vm = (linear(sd, p + f"to_{n}", y, q).v for n in "qkv")
    s = qm @ km.transpose(1, 2)                                           # fp32 scores
    sc = (c // 8) ** -0.5 if fault == "vae_attn_scale_per_head" else c ** -0.5
    pr = q(torch.softmax(s * sc, -1))                                     # R11
    o = q(pr @ vm)
    xr = x.reshape(b, c, h * w).transpose(1, 2)
    out = linear(sd, p + "to_out.0", o, q, residual=xr)
    return Act(out.v.transpose(1, 2).reshape(b, c, h, w), out.pre.transpose(1, 2).reshape(b, c, h, w))


def vae_mid(sd, p, x, groups, q=ident, fault=None):
    x = resnet(sd, p + "resnets.0.", x, None, groups, 1e-6, q, fault=fault).v
    x = vae_attention(sd, p + "attentions.0.", x, groups, q, fault).v
    return resnet(sd, p + "resnets.1.", x, None, groups, 1e-6, q, fault=fault)


def vae_up_block(sd, p, x, groups, layers, q=ident, fault=None):
    """One decoder up block: layers + 1 resnets and the upsampler."""
    for j in range(layers + 1):
        x = resnet(sd, f"{p}resnets.{j}.", x, None, groups, 1e-6, q, fault=fault).v
    return upsample_conv(sd, p + "upsamplers.0.conv", x, q, fault)


def vae_down_block(sd, p, x, groups, layers, q=ident, fault=None):
    """One encoder down block: `layers` resnets and the asymmetric-pad downsampler."""
    for j in range(layers):
        x = resnet(sd, f"{p}resnets.{j}.", x, None, groups, 1e-6, q, fault=fault).v
    return vae_downsample(sd, p + "downsamplers.0.conv", x, q, fault)


def vae_decode(sd, cfg, z, q=ident, fault=None):
    """HipAutoencoderKL.decode_nhwc: z already divided by the scaling factor -> image (fp32 on the device)."""
    g, nb = cfg["groups"], len(cfg["block_out_channels"])
    x = conv(sd, "post_quant_conv", z, q).v
    x = conv(sd, "decoder.conv_in", x, q).v
    x = vae_mid(sd, "decoder.mid_block.", x, g, q, fault)
    for i in range(nb):
        for j in range(cfg["layers_per_block"] + 1):
            x = resnet(sd, f"decoder.up_blocks.{i}.resnets.{j}.", x, None, g, 1e-6, q, fault=fault)
        if i != nb - 1:
            x = upsample_conv(sd, f"decoder.up_blocks.{i}.upsamplers.0.conv", x, q, fault)
    h = gn_apply(x.v, gn_ab(x.pre, sd["decoder.conv_norm_out.weight"], sd["decoder.conv_norm_out.bias"], g, 1e-6), q, True)
    return conv(sd, "decoder.conv_out", h, q, f32_out=True)


def vae_encode(sd, cfg, x, q=ident, fault=None):
    """HipAutoencoderKL.encode_moments_nhwc -> moments (mean | logvar), stored bf16.  conv_out has 8 output channels: the VALU
    conv applies GroupNorm + SiLU on load in fp32 WITHOUT rounding the operand (csrc/conv_direct.hip:306)."""
    g, nb = cfg["groups"], len(cfg["block_out_channels"])
    x = Act(conv(sd, "encoder.conv_in", x, q).v)
    for i in range(nb):
        for j in range(cfg["layers_per_block"]):
            x = resnet(sd, f"encoder.down_blocks.{i}.resnets.{j}.", x, None, g, 1e-6, q, fault=fault)
        if i != nb - 1:
            x = Act(vae_downsample(sd, f"encoder.down_blocks.{i}.downsamplers.0.conv", x.v, q, fault).v)
    x = vae_mid(sd, "encoder.mid_block.", x, g, q, fault)
    h = gn_apply(x.v, gn_ab(x.pre, sd["encoder.conv_norm_out.weight"], sd["encoder.conv_norm_out.bias"], g, 1e-6), ident, True)
    m = conv(sd, "encoder.conv_out", h, q).v
    return conv(sd, "quant_conv", m, q)


# ------------------------------------------------------------------------------------------ UNet / ControlNet wiring
def _encoder_prefixes(cfg):
    boc = cfg["block_out_channels"]
    return [f"down_blocks.{i}.resnets.{j}." for i in range(len(boc)) for j in range(cfg["layers_per_block"])] + \
        ["mid_block.resnets.0.", "mid_block.resnets.1."]


def run_down(sd, cfg, sample, temb, ctx, q, fold, fault, after_block=None):
    """EncoderHalf.run_down (cfg_shared or not: the same values) -> (sample, skips), all Act."""
    g, boc = cfg["groups"], cfg["block_out_channels"]
    res = [sample]
    for i in range(len(boc)):
        for j in range(cfg["layers_per_block"]):
            p = f"down_blocks.{i}.resnets.{j}."
            sample = resnet(sd, p, sample, temb[p], g, 1e-5, q, fault=fault)
            if cfg["down_cross"][i]:
                sample = transformer(sd, f"down_blocks.{i}.attentions.{j}.", sample, ctx, cfg["num_heads"], g, q, fold, fault)
            res.append(sample)
        if i != len(boc) - 1:
            sample = downsample(sd, f"down_blocks.{i}.downsamplers.0.conv", sample, q)
            res.append(sample)
        if after_block is not None:
            sample = after_block(i, sample)
    return sample, res


def run_mid(sd, cfg, sample, temb, ctx, q, fold, fault):
    g = cfg["groups"]
    sample = resnet(sd, "mid_block.resnets.0.", sample, temb["mid_block.resnets.0."], g, 1e-5, q, fault=fault)
    sample = transformer(sd, "mid_block.attentions.0.", sample, ctx, cfg["num_heads"], g, q, fold, fault)
    return resnet(sd, "mid_block.resnets.1.", sample, temb["mid_block.resnets.1."], g, 1e-5, q, fault=fault)


def fdn(sd, name, sample, level, groups, q):
    """FDN (control_utils.py:24-33): GroupNorm without affine, times (1 + gamma), plus beta; gamma / beta = 3x3 convs of the
    pyramid level, stored bf16 (controlnet.py:133-135); one rounding of the result (csrc/norm.hip:257-258).  Its output has no
    epilogue statistics: the next GroupNorm measures the stored tensor."""
    sample = as_act(sample)
    lv = q(level)                                                         # the fp32 pyramid level stored as bf16
    gamma, beta = conv(sd, name + ".conv_gamma", lv, q).v, conv(sd, name + ".conv_beta", lv, q).v
    c = sample.v.shape[1]
    one, zero = torch.ones(c, dtype=F64), torch.zeros(c, dtype=F64)
    a, b = gn_ab(sample.pre, one, zero, groups, 1e-5)
    return Act(q((sample.v * a + b) * (1.0 + gamma) + beta))


FDN_NAMES = ("fdn64", "fdn32", "fdn16", "fdn08")


def controlnet(sd, cfg, x, t, ctx, pyramid, scale, q=ident, fold=True, fault=None, features_only=False):
    """HipDualFlowControlNet.forward_nhwc with the pyramid given -> (12 residuals, mid), or the features before the zero-convs."""
    g, boc = cfg["groups"], cfg["block_out_channels"]
    temb = time_embedding(sd, t, x.shape[0], boc[0], _encoder_prefixes(cfg), q)
    sample = Act(conv(sd, "conv_in", x, q).v)
    sample = fdn(sd, "fdn64", sample, pyramid[0], g, q)

    def hook(i, s):                                                       # fdn08 twice: after blocks 2 and 3 (flownet.py:98-106)
        if fault == "fdn_applied_once" and i == 3:
            return s
        lvl = min(i + 1, 3)
        return fdn(sd, FDN_NAMES[lvl], s, pyramid[lvl], g, q)

    sample, res = run_down(sd, cfg, sample, temb, ctx, q, fold, fault, after_block=hook)
    sample = run_mid(sd, cfg, sample, temb, ctx, q, fold, fault)
    if features_only:
        return res, sample
    if fault == "control_scale_dropped":
        scale = 1.0
    down = [conv(sd, f"controlnet_down_blocks.{i}", r.v, q, out_scale=scale) for i, r in enumerate(res)]
    return down, conv(sd, "controlnet_mid_block", sample.v, q, out_scale=scale)


def unet(sd, cfg, x, t, ctx, q=ident, fold=True, fault=None, down_res=None, mid_res=None, controls=None, freeu=None):
    """HipUNet2DConditionModel.forward_nhwc.  down_res / mid_res: stored residuals, added by dc_add_bf16 (one rounding);
    controls: [(features, mid feature, the ControlNet's state dict, scale)]: zero_conv(f) * scale + skip in one epilogue."""
    g, boc = cfg["groups"], cfg["block_out_channels"]
    nb = len(boc)
    ups = [f"up_blocks.{i}.resnets.{j}." for i in range(nb) for j in range(cfg["layers_per_block"] + 1)]
    temb = time_embedding(sd, t, x.shape[0], boc[0], _encoder_prefixes(cfg) + ups, q)
    sample = Act(conv(sd, "conv_in", x, q).v)
    sample, res = run_down(sd, cfg, sample, temb, ctx, q, fold, fault)
    controls = list(controls or [])
    if fault == "second_controlnet_dropped":
        controls = controls[:1]
    for feats, _, csd, scale in controls:
        sc = 1.0 if fault == "control_scale_dropped" else scale
        res = [conv(csd, f"controlnet_down_blocks.{i}", as_act(f).v, q, out_scale=sc, residual=r.v) for i, (f, r) in enumerate(zip(feats, res))]
    if not controls and down_res is not None:
        res = [Act(q(r.v + d)) for r, d in zip(res, down_res)]
    sample = run_mid(sd, cfg, sample, temb, ctx, q, fold, fault)
    for _, mid_feat, csd, scale in controls:
        sc = 1.0 if fault == "control_scale_dropped" else scale
        sample = conv(csd, "controlnet_mid_block", as_act(mid_feat).v, q, out_scale=sc, residual=sample.v)
    if not controls and mid_res is not None and fault != "mid_residual_dropped":
        sample = Act(q(sample.v + mid_res))
    if fault == "skip_from_wrong_level":                                  # the two skips popped first change places
        res[-1], res[-2] = res[-2], res[-1]
    for i in range(nb):
        for j in range(cfg["layers_per_block"] + 1):
            skip = res.pop()
            p = f"up_blocks.{i}.resnets.{j}."
            if freeu is not None and (i < 2 or fault == "freeu_on_every_up_block"):
                sample, skip = apply_freeu(min(i, 1), sample, skip, freeu, q, fault)
            sample = resnet(sd, p, sample, temb[p], g, 1e-5, q, x2=skip, fault=fault)
            if cfg["down_cross"][nb - 1 - i]:
                sample = transformer(sd, f"up_blocks.{i}.attentions.{j}.", sample, ctx, cfg["num_heads"], g, q, fold, fault)
        if i != nb - 1:
            sample = upsample_conv(sd, f"up_blocks.{i}.upsamplers.0.conv", sample, q, fault)
    h = gn_apply(sample.v, gn_ab(sample.pre, sd["conv_norm_out.weight"], sd["conv_norm_out.bias"], g, 1e-5), q, True)
    return conv(sd, "conv_out", h, q, f32_out=True)


def fourier_filter(x, scale):
    """diffusers' fourier_filter at threshold 1 (oracle/sd15_ref.fourier_filter, in the input's precision): the centred 2x2 block of
    the shifted 2-D spectrum times `scale`."""
    xf = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    h, w = x.shape[-2:]
    mask = torch.ones_like(xf.real)
    mask[..., h // 2 - 1:h // 2 + 1, w // 2 - 1:w // 2 + 1] = scale
    return torch.fft.ifftn(torch.fft.ifftshift(xf * mask, dim=(-2, -1)), dim=(-2, -1)).real


def apply_freeu(idx, sample, skip, freeu, q=ident, fault=None):
    """apply_freeu of the first two up blocks (unet.py:123-125): the first half of the backbone's channels times b (one rounding,
    csrc/elementwise.hip freeu_backbone_kernel), the skip's four lowest frequency bins times s (x + (s - 1) / HW * low in fp32,
    one rounding, freeu_lowfreq_kernel).  Neither output has epilogue statistics: the next GroupNorm measures the stored tensor."""
    b, s = (freeu["b1"], freeu["s1"]) if idx == 0 else (freeu["b2"], freeu["s2"])
    if fault == "freeu_b_s_exchanged":
        b, s = s, b
    sample, skip = as_act(sample).v, as_act(skip).v
    half = sample.shape[1] // 2
    sample = torch.cat([q(sample[:, :half] * b), sample[:, half:]], 1)
    return Act(sample), Act(q(fourier_filter(skip, s)))


def combine_residuals(a, b, q=ident):
    """rescontrolnet.combine_residuals: the two residual sets add (dc_add_bf16: one rounding)."""
    (d1, m1), (d2, m2) = a, b
    return [Act(q(x.v + y.v)) for x, y in zip(d1, d2)], Act(q(m1.v + m2.v))


# ------------------------------------------------------------------------------------------ weights and inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(gen, *shape, std=1.0):
    # fp32 values widened: exactly what the device's loaders receive
    return (std * torch.randn(*shape, generator=gen, dtype=torch.float32)).to(F64)


def _put_conv(sd, gen, k, cout, cin, ks):
    shape = (cout, cin, ks, ks) if ks else (cout, cin)
    sd[k + ".weight"] = _rand(gen, *shape, std=(cin * max(ks, 1) ** 2) ** -0.5)
    sd[k + ".bias"] = _rand(gen, cout, std=0.1)


def _put_norm(sd, gen, k, c):
    sd[k + ".weight"] = 1.0 + _rand(gen, c, std=0.2)
    sd[k + ".bias"] = _rand(gen, c, std=0.2)


def resnet_weights(sd, gen, p, cin, cout, temb_dim=None):
    _put_norm(sd, gen, p + "norm1", cin)
    _put_conv(sd, gen, p + "conv1", cout, cin, 3)
    if temb_dim:
        _put_conv(sd, gen, p + "time_emb_proj", cout, temb_dim, 0)
    _put_norm(sd, gen, p + "norm2", cout)
    _put_conv(sd, gen, p + "conv2", cout, cout, 3)
    if cin != cout:
        _put_conv(sd, gen, p + "conv_shortcut", cout, cin, 1)


def temb_weights(sd, gen, ch0):
    _put_conv(sd, gen, "time_embedding.linear_1", 4 * ch0, ch0, 0)
    _put_conv(sd, gen, "time_embedding.linear_2", 4 * ch0, 4 * ch0, 0)


def transformer_weights(sd, gen, p, c, ctx_dim, family="unit"):
    _put_norm(sd, gen, p + "norm", c)
    _put_conv(sd, gen, p + "proj_in", c, c, 1)
    tb = p + "transformer_blocks.0."
    for n in ("norm1", "norm2", "norm3"):
        _put_norm(sd, gen, tb + n, c)
    for a, kd in (("attn1", c), ("attn2", ctx_dim)):
        sd[tb + a + ".to_q.weight"] = _rand(gen, c, c, std=c ** -0.5)
        sd[tb + a + ".to_k.weight"] = _rand(gen, c, kd, std=kd ** -0.5)
        sd[tb + a + ".to_v.weight"] = _rand(gen, c, kd, std=kd ** -0.5)
        _put_conv(sd, gen, tb + a + ".to_out.0", c, c, 0)
    _put_conv(sd, gen, tb + "ff.net.0.proj", 8 * c, c, 0)
    _put_conv(sd, gen, tb + "ff.net.2", c, 4 * c, 0)
    _put_conv(sd, gen, p + "proj_out", c, c, 1)
    if family == "quiet":                      # rows of proj_in's output with a standard deviation near 3e-3: LayerNorm's eps matters
        sd[p + "proj_in.weight"] = sd[p + "proj_in.weight"] * QUIET
        sd[p + "proj_in.bias"] = sd[p + "proj_in.bias"] * QUIET
    if family == "peaked":                     # logits with a standard deviation near PEAK after the softmax scale: few keys win
        for a in ("attn1", "attn2"):
            sd[tb + a + ".to_q.weight"] = sd[tb + a + ".to_q.weight"] * PEAK
    return sd


def vae_attention_weights(sd, gen, p, c):
    _put_norm(sd, gen, p + "group_norm", c)
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        _put_conv(sd, gen, p + n, c, c, 0)


QUIET = 3e-3
PEAK = 6.0
LOUD = 8.0                                     # standard deviation of the residuals that enter the UNet's deepest level in the loud case


def stored(x):
    """An input as the device receives it: bf16 values, widened."""
    return bf16(x)


def family_input(gen, family, *shape):
    """unit: N(0, 1).  quiet: N(0, 1) * 3e-3 (zero mean, so bf16 keeps its relative precision): per-group and per-row standard
    deviation 3e-3, where an epsilon of 1e-5 against 1e-6 moves rstd by tens of percent.  peaked: N(0, 1) inputs; the
    attention weights carry the family (to_q scaled by PEAK, as the winner lead of edge_cases' peaked attention family: a few
    keys take the softmax, and its scale matters)."""
    x = _rand(gen, *shape)
    return stored(x * QUIET if family == "quiet" else x)


# ------------------------------------------------------------------------------------------ cases
Case = collections.namedtuple("Case", "name block shape opts family branches")
"""block: the function / device class under test.  shape: dict of sizes.  opts: dict of options.  branches: the BRANCHES this case
declares it reaches (checked against the shape predicates on the CPU and against the recorded launches on the GPU)."""

# Every shape-selected branch of the covered wiring, hand-written from the code (file: what selects it).
BRANCHES = {
    "temb.batched_slices": "blocks.py TimeEmbedding: one GEMM for every time_emb_proj, sliced per block",
    "resnet.temb": "blocks.py ResnetBlock: row_add = temb slice",
    "resnet.no_temb": "blocks.py ResnetBlock: temb None (VAE)",
    "resnet.shortcut_conv": "blocks.py ResnetBlock: 1x1 conv_shortcut",
    "resnet.shortcut_identity": "blocks.py ResnetBlock: identity shortcut",
    "resnet.x2_concat": "blocks.py ResnetBlock: skip concat read in place (x2)",
    "conv_gn_silu.fused_on_load": "ops.conv_gn_silu: cout <= FUSE_GN_MAX_COUT or batch <= FUSE_GN_SMALL_BATCH",
    "conv_gn_silu.standalone_gn_apply": "ops.conv_gn_silu: cout > FUSE_GN_MAX_COUT and batch > FUSE_GN_SMALL_BATCH",
    "gn_ab.direct": "ops.group_norm_ab: input without partials, HW <= GN_DIRECT_MAX_PIXELS: one-launch statistics",
    "gn_ab.stats_pass": "ops.group_norm_ab: input without partials, HW > GN_DIRECT_MAX_PIXELS: statistics pass + finalize",
    "transformer.proj_in.gn_apply_then_gemm": "blocks.py TransformerBlock: standalone gn_apply, then the GEMM",
    "transformer.proj_in.rowpanel_gn_on_load": "blocks.py TransformerBlock: ops.rowpanel_takes -> GroupNorm affine on the row panel",
    "transformer.ln_fold": "blocks.py LN_FOLD = True",
    "transformer.ln_standalone": "blocks.py LN_FOLD = False",
    "transformer.unshared": "blocks.py TransformerBlock(cfg_shared=False)",
    "transformer.cfg_shared": "blocks.py TransformerBlock(cfg_shared=True)",
    "down.stride2": "blocks.py EncoderHalf.run_down downsampler",
    "up.fused_nearest2x": "unet.py decode_nhwc / vae.py decode_nhwc: conv with upsample=True",
    "vae.attention": "vae.py VaeAttention",
    "vae.mid": "vae.py d_mid / e_mid: resnet, attention, resnet",
    "vae.dec_up": "vae.py decode_nhwc: one up block",
    "vae.enc_down.asym_pad": "vae.py encode_moments_nhwc: stride-2 conv with pad=0",
    "vae.decode": "vae.py decode_nhwc, with conv_out padded to four output channels on the MFMA path",
    "vae.encode": "vae.py encode_moments_nhwc, with conv_out on the VALU small-cout path and quant_conv on the small-cin path",
    "unet.plain": "unet.py decode_nhwc: no residuals",
    "unet.residuals_added": "unet.py decode_nhwc: down_res / mid_res added by dc_add_bf16",
    "unet.residuals_loud": "unet.py decode_nhwc: the same adds with mid_res and the three 1x1-map down_res at a standard deviation of 8, "
                           "so that the deepest level carries the output (no other launches: what the bars can see differs)",
    "unet.control_one": "unet.py decode_nhwc: one control tuple, zero-convs fused with the skip add",
    "unet.control_two": "unet.py decode_nhwc: two control tuples, their residuals add",
    "run_down.unshared": "blocks.py EncoderHalf.run_down(cfg_shared=False)",
    "run_down.cfg_shared": "blocks.py EncoderHalf.run_down(cfg_shared=True): first resnet and transformer prefix on one half",
    "controlnet.zero_convs": "controlnet.py forward_nhwc: zero-convs with conditioning_scale, FDN hook",
    "controlnet.features_only": "controlnet.py forward_nhwc(features_only=True)",
    "rescontrolnet.combine_residuals": "rescontrolnet.py combine_residuals: two residual sets add",
}
# Branches of the same files that no case can reach, with the reason.
UNREACHABLE = {
    "transformer.proj_in.igemm_gn_on_load": "blocks.py PROJ_IN_FUSE_MIN_ROWS = 1 << 62: no tensor has that many rows",
}

# predicates restated from ops.py; tests/test_block_ref.py holds the constants to the package's
FUSE_GN_MAX_COUT = 160
FUSE_GN_SMALL_BATCH = 4
GN_DIRECT_MAX_PIXELS = 256


def rowpanel_takes(rows, rows_per_sample, cin, cout):
    return cin == 320 and cout >= 320 and cout % 64 == 0 and rows >= 65536 and rows % 256 == 0 and rows_per_sample % 256 == 0


def predicted_branches(case):
    """The shape-selected branches of a case, from the predicates alone (no table look-up)."""
    s, o = case.shape, case.opts
    out = set()
    if case.block == "resnet":
        n, hw = s["n"], s["h"] * s["w"]
        out.add("resnet.temb" if o.get("temb") else "resnet.no_temb")
        if o.get("temb"):
            out.add("temb.batched_slices")
        out.add("resnet.shortcut_conv" if s["cin"] + s.get("c2", 0) != s["cout"] else "resnet.shortcut_identity")
        if s.get("c2"):
            out.add("resnet.x2_concat")
        out.add("conv_gn_silu.standalone_gn_apply" if s["cout"] > FUSE_GN_MAX_COUT and n > FUSE_GN_SMALL_BATCH
                else "conv_gn_silu.fused_on_load")
        out.add("gn_ab.direct" if hw <= GN_DIRECT_MAX_PIXELS else "gn_ab.stats_pass")
    elif case.block == "transformer":
        n = s["n"] * (s.get("tile", 1))
        hw = s["h"] * s["w"]
        half = n // 2 if o.get("cfg_shared") else n
        out.add("transformer.proj_in.rowpanel_gn_on_load" if rowpanel_takes(half * hw, hw, s["c"], s["c"])
                else "transformer.proj_in.gn_apply_then_gemm")
        out.add("transformer.ln_fold" if o.get("fold", True) else "transformer.ln_standalone")
        out.add("transformer.cfg_shared" if o.get("cfg_shared") else "transformer.unshared")
        out.add("gn_ab.direct" if hw <= GN_DIRECT_MAX_PIXELS else "gn_ab.stats_pass")
    elif case.block == "down":
        out.add("down.stride2")
    elif case.block == "up":
        out.add("up.fused_nearest2x")
    elif case.block == "vae_attention":
        out |= {"vae.attention", "gn_ab.direct" if s["h"] * s["w"] <= GN_DIRECT_MAX_PIXELS else "gn_ab.stats_pass"}
    elif case.block == "vae_mid":
        out |= {"vae.mid", "vae.attention", "resnet.no_temb"}
    elif case.block == "vae_up":
        out |= {"vae.dec_up", "up.fused_nearest2x", "resnet.no_temb"}
    elif case.block == "vae_down":
        out |= {"vae.enc_down.asym_pad", "resnet.no_temb"}
    elif case.block == "vae_decode":
        out |= {"vae.decode", "vae.mid", "vae.attention", "vae.dec_up", "up.fused_nearest2x", "resnet.no_temb"}
    elif case.block == "vae_encode":
        out |= {"vae.encode", "vae.mid", "vae.attention", "vae.enc_down.asym_pad", "resnet.no_temb"}
    elif case.block == "controlnet":
        out |= {"controlnet.zero_convs", "run_down.unshared", "down.stride2", "temb.batched_slices", "resnet.temb"}
    elif case.block == "unet":
        mode = o["mode"]
        out |= {"down.stride2", "up.fused_nearest2x", "temb.batched_slices", "resnet.temb", "resnet.x2_concat",
                "run_down.cfg_shared" if o.get("cfg_shared") else "run_down.unshared"}
        out.add({"plain": "unet.plain", "residuals": "unet.residuals_added", "control1": "unet.control_one",
                 "control2": "unet.control_two", "combined2": "unet.residuals_added"}[mode])
        if mode in ("control1", "control2"):
            out.add("controlnet.features_only")
        if mode == "combined2":
            out |= {"controlnet.zero_convs", "rescontrolnet.combine_residuals"}
        if o.get("loud"):
            out.add("unet.residuals_loud")
    return out


def _mk(name, block, shape, opts, family, branches):
    return Case(name, block, shape, opts, family, frozenset(branches))


SMALL_WIDTHS = (64, 128, 256)        # selftest.SMALL_UNET block widths, 8 heads: d = 8, 16, 32
CTX_DIM, CTX_LEN, HEADS, GROUPS = 128, 77, 8, 32

BLOCK_CASES = [
    # ---- ResnetBlock (UNet: eps 1e-5, with the time embedding)
    _mk("res_64_64_b2_12x12", "resnet", dict(n=2, h=12, w=12, cin=64, cout=64), dict(temb=True), "unit",
        ["resnet.temb", "temb.batched_slices", "resnet.shortcut_identity", "conv_gn_silu.fused_on_load", "gn_ab.direct"]),
    _mk("res_64_64_b2_12x12_quiet", "resnet", dict(n=2, h=12, w=12, cin=64, cout=64), dict(temb=True), "quiet",
        ["resnet.temb", "temb.batched_slices", "resnet.shortcut_identity", "conv_gn_silu.fused_on_load", "gn_ab.direct"]),
    _mk("res_64_128_b2_9x7", "resnet", dict(n=2, h=9, w=7, cin=64, cout=128), dict(temb=True), "unit",
        ["resnet.temb", "temb.batched_slices", "resnet.shortcut_conv", "conv_gn_silu.fused_on_load", "gn_ab.direct"]),
    _mk("res_128+64_64_b2_9x7_skip", "resnet", dict(n=2, h=9, w=7, cin=128, cout=64, c2=64), dict(temb=True), "unit",
        ["resnet.temb", "temb.batched_slices", "resnet.shortcut_conv", "resnet.x2_concat", "conv_gn_silu.fused_on_load",
         "gn_ab.direct"]),
    _mk("res_128+64_256_b5_12x12_skip", "resnet", dict(n=5, h=12, w=12, cin=128, cout=256, c2=64), dict(temb=True), "unit",
        ["resnet.temb", "temb.batched_slices", "resnet.x2_concat", "resnet.shortcut_conv",
         "conv_gn_silu.standalone_gn_apply", "gn_ab.direct"]),
    _mk("res_64_192_b5_9x7", "resnet", dict(n=5, h=9, w=7, cin=64, cout=192), dict(temb=True), "unit",
        ["resnet.temb", "temb.batched_slices", "resnet.shortcut_conv", "conv_gn_silu.standalone_gn_apply", "gn_ab.direct"]),
    _mk("res_64_64_b2_17x17", "resnet", dict(n=2, h=17, w=17, cin=64, cout=64), dict(temb=True), "unit",
        ["resnet.temb", "temb.batched_slices", "resnet.shortcut_identity", "conv_gn_silu.fused_on_load", "gn_ab.stats_pass"]),
    # ---- ResnetBlock as the VAE uses it (eps 1e-6, no time embedding)
    _mk("res_vae_64_128_b2_12x12_quiet", "resnet", dict(n=2, h=12, w=12, cin=64, cout=128), dict(temb=False, eps=1e-6), "quiet",
        ["resnet.no_temb", "resnet.shortcut_conv", "conv_gn_silu.fused_on_load", "gn_ab.direct"]),
    # ---- samplers
    _mk("down_128_b2_12x12", "down", dict(n=2, h=12, w=12, c=128), {}, "unit", ["down.stride2"]),
    _mk("down_64_b2_9x7", "down", dict(n=2, h=9, w=7, c=64), {}, "unit", ["down.stride2"]),
    _mk("up_128_b2_9x7", "up", dict(n=2, h=9, w=7, c=128), {}, "unit", ["up.fused_nearest2x"]),
    # ---- VAE
    _mk("vae_attn_256_b2_8x8", "vae_attention", dict(n=2, h=8, w=8, c=256), {}, "unit", ["vae.attention", "gn_ab.direct"]),
    _mk("vae_attn_256_b1_8x16_quiet", "vae_attention", dict(n=1, h=8, w=16, c=256), {}, "quiet", ["vae.attention", "gn_ab.direct"]),
    _mk("vae_mid_256_b1_8x8", "vae_mid", dict(n=1, h=8, w=8, c=256), {}, "unit", ["vae.mid", "vae.attention", "resnet.no_temb"]),
    _mk("vae_up_128_64_b1_8x8", "vae_up", dict(n=1, h=8, w=8, cin=128, c=64), {}, "unit",
        ["vae.dec_up", "up.fused_nearest2x", "resnet.no_temb"]),
    _mk("vae_down_64_128_b1_12x12", "vae_down", dict(n=1, h=12, w=12, cin=64, c=128), {}, "unit",
        ["vae.enc_down.asym_pad", "resnet.no_temb"]),
    _mk("vae_down_64_64_b1_9x7_quiet", "vae_down", dict(n=1, h=9, w=7, cin=64, c=64), {}, "quiet",
        ["vae.enc_down.asym_pad", "resnet.no_temb"]),
]
_TR = ["transformer.proj_in.gn_apply_then_gemm", "gn_ab.direct"]
for _c in SMALL_WIDTHS:
    for _h, _w in ((8, 8), (12, 20)):
        BLOCK_CASES.append(_mk(f"tr_{_c}_b2_{_h}x{_w}", "transformer", dict(n=2, h=_h, w=_w, c=_c), dict(fold=True, cfg_shared=False),
                               "unit", _TR + ["transformer.ln_fold", "transformer.unshared"]))
    BLOCK_CASES.append(_mk(f"tr_{_c}_b2_8x8_cfg", "transformer", dict(n=2, h=8, w=8, c=_c), dict(fold=True, cfg_shared=True), "unit",
                           _TR + ["transformer.ln_fold", "transformer.cfg_shared"]))
    BLOCK_CASES.append(_mk(f"tr_{_c}_b2_12x20_nofold", "transformer", dict(n=2, h=12, w=20, c=_c), dict(fold=False, cfg_shared=False),
                           "unit", _TR + ["transformer.ln_standalone", "transformer.unshared"]))
    BLOCK_CASES.append(_mk(f"tr_{_c}_b2_8x8_quiet", "transformer", dict(n=2, h=8, w=8, c=_c), dict(fold=True, cfg_shared=False), "quiet",
                           _TR + ["transformer.ln_fold", "transformer.unshared"]))
    BLOCK_CASES.append(_mk(f"tr_{_c}_b2_12x20_peaked", "transformer", dict(n=2, h=12, w=20, c=_c), dict(fold=True, cfg_shared=False),
                           "peaked", _TR + ["transformer.ln_fold", "transformer.unshared"]))
BLOCK_CASES += [
    _mk("tr_128_b2_12x20_cfg_nofold", "transformer", dict(n=2, h=12, w=20, c=128), dict(fold=False, cfg_shared=True), "unit",
        _TR + ["transformer.ln_standalone", "transformer.cfg_shared"]),
    _mk("tr_64_b2_12x20_nofold_quiet", "transformer", dict(n=2, h=12, w=20, c=64), dict(fold=False, cfg_shared=False), "quiet",
        _TR + ["transformer.ln_standalone", "transformer.unshared"]),
    # the production route: K = 320 row panel with the GroupNorm affine on load; two distinct samples tiled eight times on the device
    _mk("tr_320_b16_64x64_rowpanel", "transformer", dict(n=2, tile=8, h=64, w=64, c=320), dict(fold=True, cfg_shared=False), "unit",
        ["transformer.proj_in.rowpanel_gn_on_load", "gn_ab.stats_pass", "transformer.ln_fold", "transformer.unshared"]),
]
del _c, _h, _w
# ---- whole-model wiring: selftest.SMALL_UNET / SMALL_VAE at 64x64 pixels (8x8 latents), weights.synthesize (set_model_weights)
_UB = ["down.stride2", "up.fused_nearest2x", "temb.batched_slices", "resnet.temb", "resnet.x2_concat"]
BLOCK_CASES += [
    _mk("unet_plain_b2_cfg", "unet", dict(n=2, h=8, w=8), dict(mode="plain", cfg_shared=True), "unit",
        _UB + ["unet.plain", "run_down.cfg_shared"]),
    _mk("unet_residuals_b2", "unet", dict(n=2, h=8, w=8), dict(mode="residuals"), "unit",
        _UB + ["unet.residuals_added", "run_down.unshared"]),
    _mk("unet_residuals_loud_b2", "unet", dict(n=2, h=8, w=8), dict(mode="residuals", loud=LOUD), "unit",
        _UB + ["unet.residuals_added", "unet.residuals_loud", "run_down.unshared"]),
    _mk("controlnet_b2", "controlnet", dict(n=2, h=8, w=8), dict(scale=1.7), "unit",
        ["controlnet.zero_convs", "run_down.unshared", "down.stride2", "temb.batched_slices", "resnet.temb"]),
    _mk("unet_control1_b2", "unet", dict(n=2, h=8, w=8), dict(mode="control1", scale=1.7), "unit",
        _UB + ["unet.control_one", "controlnet.features_only", "run_down.unshared"]),
    _mk("unet_control2_b2", "unet", dict(n=2, h=8, w=8), dict(mode="control2", scale=1.7), "unit",
        _UB + ["unet.control_two", "controlnet.features_only", "run_down.unshared"]),
    _mk("unet_combined2_b2", "unet", dict(n=2, h=8, w=8), dict(mode="combined2", scale=1.7), "unit",
        _UB + ["unet.residuals_added", "controlnet.zero_convs", "rescontrolnet.combine_residuals", "run_down.unshared"]),
    _mk("vae_decode_b1_8x8", "vae_decode", dict(n=1, h=8, w=8), {}, "unit",
        ["vae.decode", "vae.mid", "vae.attention", "vae.dec_up", "up.fused_nearest2x", "resnet.no_temb"]),
    _mk("vae_encode_b1_64x64", "vae_encode", dict(n=1, h=64, w=64), {}, "unit",
        ["vae.encode", "vae.mid", "vae.attention", "vae.enc_down.asym_pad", "resnet.no_temb"]),
]
MODEL_BLOCKS = ("unet", "controlnet", "vae_decode", "vae_encode")
CASES = {c.name: c for c in BLOCK_CASES}
HEAVY = {"tr_320_b16_64x64_rowpanel"}              # reference of tens of seconds: no faults are evaluated on it


# fault -> the blocks it applies to
FAULTS = {
    "concat_order": ("resnet",), "no_temb": ("resnet",), "temb_no_silu": ("resnet",), "temb_slice_of_next_block": ("resnet",),
    "shortcut_of_normed_input": ("resnet",), "gn_eps_1e-6": ("resnet",),
    "norm_eps_1e-5": ("transformer",), "ln_eps_1e-6": ("transformer",), "residual_from_normed": ("transformer",),
    "geglu_halves_swapped": ("transformer",), "attn_scale_1_over_d": ("transformer",), "heads_interleaved": ("transformer",),
    "cfg_context_halves_swapped": ("transformer",), "proj_out_residual_dropped": ("transformer",),
    "upsample_after_conv": ("up", "vae_up"),
    "vae_symmetric_pad": ("vae_down",), "vae_attn_scale_per_head": ("vae_attention", "vae_mid"),
    "vae_gn_eps_1e-5": ("vae_attention", "vae_down"),
    "control_scale_dropped": ("controlnet", "unet"), "second_controlnet_dropped": ("unet",), "fdn_applied_once": ("controlnet",),
    "mid_residual_dropped": ("unet",), "skip_from_wrong_level": ("unet",),
}
# (mid_residual_dropped and skip_from_wrong_level act at the 1x1 level: with unit residuals they move the 8x8 output by 0.53 and
# 0.8 of the bar; the case unet_residuals_loud_b2 exists to reject them, DESIGN.md §18 has the figures)
_MODES = {"control_scale_dropped": ("control1", "control2", "combined2"), "second_controlnet_dropped": ("control2", "combined2"),
          "upsample_after_conv": ("plain", "residuals"), "mid_residual_dropped": ("residuals",),
          "skip_from_wrong_level": ("residuals",)}
FAULTS["upsample_after_conv"] = ("up", "vae_up", "unet")


def fault_applies(fault, case):
    if case.block not in FAULTS[fault]:
        return False
    if case.block == "unet":
        return case.opts["mode"] in _MODES[fault]
    if fault == "concat_order":
        return bool(case.shape.get("c2"))
    if fault in ("no_temb", "temb_no_silu", "temb_slice_of_next_block"):
        return bool(case.opts.get("temb"))
    if fault == "vae_symmetric_pad":                       # odd maps: the symmetric pad changes the output's size, not its values
        return case.shape["h"] % 2 == 0 and case.shape["w"] % 2 == 0
    if fault == "gn_eps_1e-6":
        return bool(case.opts.get("temb"))                 # the UNet's resnets (eps 1e-5)
    return True


# ------------------------------------------------------------------------------------------ building and running a case
P_RES, P_NEXT, P_TR = "down_blocks.0.resnets.0.", "down_blocks.0.resnets.1.", "down_blocks.0.attentions.0."
TIMESTEP = 801.0


def build_case(case):
    """-> (state dict, inputs dict).  Deterministic per case name; every tensor holds values the device's formats store exactly
    (weights: fp32 values; activations: bf16 values), widened to fp64."""
    seed = sum((i + 1) * ord(ch) for i, ch in enumerate(case.name)) % (2 ** 31)
    gen = _gen(seed)
    s, o, sd, inp = case.shape, case.opts, {}, {}
    if case.block == "resnet":
        cin = s["cin"] + s.get("c2", 0)
        temb_dim = 4 * 64 if o.get("temb") else None
        resnet_weights(sd, gen, P_RES, cin, s["cout"], temb_dim)
        if temb_dim:
            temb_weights(sd, gen, 64)
            _put_conv(sd, gen, P_NEXT + "time_emb_proj", s["cout"], temb_dim, 0)     # the next block's slice of the batched GEMM
        inp["x"] = family_input(gen, case.family, s["n"], s["cin"], s["h"], s["w"])
        if s.get("c2"):
            inp["x2"] = family_input(gen, case.family, s["n"], s["c2"], s["h"], s["w"])
    elif case.block == "transformer":
        transformer_weights(sd, gen, P_TR, s["c"], CTX_DIM, case.family)
        inp["x"] = family_input(gen, case.family, s["n"], s["c"], s["h"], s["w"])
        inp["ctx"] = stored(_rand(gen, s["n"], CTX_LEN, CTX_DIM))
        if o.get("cfg_shared"):                            # the two halves of the batch are the same sample; the contexts differ
            inp["x"] = torch.cat([inp["x"][: s["n"] // 2]] * 2, 0)
    elif case.block in ("down", "up"):
        _put_conv(sd, gen, "s.conv", s["c"], s["c"], 3)
        inp["x"] = family_input(gen, case.family, s["n"], s["c"], s["h"], s["w"])
    elif case.block == "vae_attention":
        vae_attention_weights(sd, gen, "a.", s["c"])
        inp["x"] = family_input(gen, case.family, s["n"], s["c"], s["h"], s["w"])
    elif case.block == "vae_mid":
        resnet_weights(sd, gen, "m.resnets.0.", s["c"], s["c"])
        vae_attention_weights(sd, gen, "m.attentions.0.", s["c"])
        resnet_weights(sd, gen, "m.resnets.1.", s["c"], s["c"])
        inp["x"] = family_input(gen, case.family, s["n"], s["c"], s["h"], s["w"])
    elif case.block == "vae_up":
        for j in range(3):
            resnet_weights(sd, gen, f"u.resnets.{j}.", s["cin"] if j == 0 else s["c"], s["c"])
        _put_conv(sd, gen, "u.upsamplers.0.conv", s["c"], s["c"], 3)
        inp["x"] = family_input(gen, case.family, s["n"], s["cin"], s["h"], s["w"])
    elif case.block == "vae_down":
        for j in range(2):
            resnet_weights(sd, gen, f"d.resnets.{j}.", s["cin"] if j == 0 else s["c"], s["c"])
        _put_conv(sd, gen, "d.downsamplers.0.conv", s["c"], s["c"], 3)
        inp["x"] = family_input(gen, case.family, s["n"], s["cin"], s["h"], s["w"])
    elif case.block in MODEL_BLOCKS:
        sd = model_weights()
        cfg = sd["unet_cfg"]
        if case.block == "vae_decode":
            inp["x"] = family_input(gen, case.family, s["n"], 4, s["h"], s["w"])
        elif case.block == "vae_encode":
            inp["x"] = stored(2 * torch.rand(s["n"], 3, s["h"], s["w"], generator=gen, dtype=torch.float32).to(F64) - 1)
        else:
            inp["x"] = family_input(gen, case.family, s["n"], 4, s["h"], s["w"])
            if o.get("cfg_shared"):
                inp["x"] = torch.cat([inp["x"][: s["n"] // 2]] * 2, 0)
            inp["ctx"] = stored(_rand(gen, s["n"], CTX_LEN, cfg["cross_attention_dim"]))
            boc = cfg["block_out_channels"]
            inj = (boc[0], boc[0], boc[1], boc[2])
            for name in ("pyr1", "pyr2"):                  # the control pyramid is an INPUT here (its extractors decide discretely)
                inp[name] = [stored(_rand(gen, s["n"], c, s["h"] >> i, s["w"] >> i)) for i, c in enumerate(inj)]
            if o.get("mode") == "residuals":
                chans = [boc[0]] + [c for i, c in enumerate(boc) for _ in range(cfg["layers_per_block"] + (i != len(boc) - 1))]
                sizes, lvl = [0], 0
                for i in range(len(boc)):
                    sizes += [lvl] * cfg["layers_per_block"]
                    if i != len(boc) - 1:
                        lvl += 1
                        sizes.append(lvl)
                loud = o.get("loud")                       # the mid residual and the 1x1-map skips' residuals at that standard deviation
                inp["down_res"] = [stored(_rand(gen, s["n"], c, s["h"] >> l, s["w"] >> l, std=loud if loud and l == lvl else 0.5))
                                   for c, l in zip(chans, sizes)]
                inp["mid_res"] = stored(_rand(gen, s["n"], boc[-1], s["h"] >> lvl, s["w"] >> lvl, std=loud or 1.0))
    else:
        raise KeyError(case.block)
    return sd, inp


_MODEL = {}


def set_model_weights(provider):
    """provider() -> dict(unet, cn1, cn2, vae: diffusers-layout state dicts; unet_cfg, vae_cfg).  The tests hand in
    weights.synthesize of the selftest configurations: this module imports nothing from the package."""
    _MODEL["provider"] = provider


def model_weights():
    if "sd" not in _MODEL:
        raw = _MODEL["provider"]()
        _MODEL["sd"] = {k: ({n: t.to(F64) for n, t in v.items()} if k in ("unet", "cn1", "cn2", "vae") else v) for k, v in raw.items()}
    return _MODEL["sd"]


def run_case(case, sd, inp, q=ident, fault=None):
    """The block of a case on its inputs -> the list of its outputs, fp64 NCHW (the stored values)."""
    if fault is not None and not fault_applies(fault, case):
        raise ValueError(f"{fault} does not apply to {case.name}")
    out = _run_case(case, sd, inp, q, fault)
    return [t.v if isinstance(t, Act) else t for t in (out if isinstance(out, list) else [out])]


def _run_case(case, sd, inp, q, fault):
    s, o = case.shape, case.opts
    if case.block == "resnet":
        row = None
        if o.get("temb"):
            row = time_embedding(sd, TIMESTEP, s["n"], 64, [P_RES, P_NEXT], q, fault)[P_RES]
        return resnet(sd, P_RES, inp["x"], row, GROUPS, o.get("eps", 1e-5), q, inp.get("x2"), fault)
    if case.block == "transformer":
        launch_batch = s["n"] * s.get("tile", 1) // (2 if o.get("cfg_shared") else 1)     # cfg_shared: each half is its own launch
        return transformer(sd, P_TR, inp["x"], inp["ctx"], HEADS, GROUPS, q, o.get("fold", True), fault, batch=launch_batch)
    if case.block == "down":
        return downsample(sd, "s.conv", inp["x"], q, fault)
    if case.block == "up":
        return upsample_conv(sd, "s.conv", inp["x"], q, fault)
    if case.block == "vae_attention":
        return vae_attention(sd, "a.", inp["x"], GROUPS, q, fault)
    if case.block == "vae_mid":
        return vae_mid(sd, "m.", inp["x"], GROUPS, q, fault)
    if case.block == "vae_up":
        return vae_up_block(sd, "u.", inp["x"], GROUPS, 2, q, fault)
    if case.block == "vae_down":
        return vae_down_block(sd, "d.", inp["x"], GROUPS, 2, q, fault)
    if case.block == "vae_decode":
        return vae_decode(sd["vae"], sd["vae_cfg"], inp["x"], q, fault)
    if case.block == "vae_encode":
        return vae_encode(sd["vae"], sd["vae_cfg"], inp["x"], q, fault)
    cfg, x, ctx = sd["unet_cfg"], inp["x"], inp["ctx"]
    if case.block == "controlnet":
        down, mid = controlnet(sd["cn1"], cfg, x, TIMESTEP, ctx, inp["pyr1"], o["scale"], q, True, fault)
        return down + [mid]
    assert case.block == "unet", case.block
    mode = o["mode"]
    if mode == "plain":
        return unet(sd["unet"], cfg, x, TIMESTEP, ctx, q, True, fault)
    if mode == "residuals":
        return unet(sd["unet"], cfg, x, TIMESTEP, ctx, q, True, fault, down_res=inp["down_res"], mid_res=inp["mid_res"])
    nets = [("cn1", "pyr1")] + ([("cn2", "pyr2")] if mode in ("control2", "combined2") else [])
    if mode == "combined2":                                # each ControlNet's scaled residuals, summed, then added to the skips
        outs = [controlnet(sd[k], cfg, x, TIMESTEP, ctx, inp[p], o["scale"], q, True, fault) for k, p in nets]
        if fault == "second_controlnet_dropped":
            down, mid = outs[0]
        else:
            down, mid = combine_residuals(outs[0], outs[1], q)
        return unet(sd["unet"], cfg, x, TIMESTEP, ctx, q, True, None, down_res=[d.v for d in down], mid_res=mid.v)
    controls = []
    for k, p in nets:
        feats, midf = controlnet(sd[k], cfg, x, TIMESTEP, ctx, inp[p], o["scale"], q, True, None, features_only=True)
        controls.append((feats, midf, sd[k], o["scale"]))
    return unet(sd["unet"], cfg, x, TIMESTEP, ctx, q, True, fault, controls=controls)


_CACHE = {}


def reference_and_bars(case):
    """-> dict(sd, inp, ref, emu: lists of outputs; emu_figs, bars: one (rel_l2, max_rel) per output); computed once per process
    and case, never changed."""
    if case.name not in _CACHE:
        sd, inp = build_case(case)
        ref = run_case(case, sd, inp, ident)
        emu = run_case(case, sd, inp, bf16)
        figs = [figures(e, r) for e, r in zip(emu, ref)]
        _CACHE[case.name] = dict(sd=sd, inp=inp, ref=ref, emu=emu, emu_figs=figs, bars=[(MARGIN * f[0], MARGIN * f[1]) for f in figs])
    return _CACHE[case.name]
