"""Yardsticks of the trainable FDN injection (plain module, numpy and torch only, nothing from the package; imported by
tests/test_fdn_grad_ref.py on the CPU and tests/test_gpu_fdn_grad.py on the GPU):

* `fdn`              `FDN.forward` after its convolutions (control_utils.py:28-34) in differentiable torch of a given dtype, and
                     `stats`, the mean and rstd of every (sample, group).  `fdn_module` is the whole module through
                     `oracle.control_ref.fdn`, which tests/golden/control_fdn.npz pins to the reference's own module.
* `closed_form`      y, mean, rstd, g_x, g_gamma by the formulas of include/diffcodec_fdn_hip.h in fp64, with the planted faults of
                     the sharpness test.
* case tables, input builders, the conditions the inputs must meet, and the bars: per tensor 4 x the error of the same arithmetic in
  torch fp32 on the CPU against fp64, never below 2^-23; a reference that is identically zero asks for exact zeros.  The error norm is
  max|value - ref| / max|ref| per tensor, no element excluded.  The fp32 errors are stored (`CPU_FP32`, `MODULE_CPU_FP32`,
  `GOLDEN_DISTANCE`); tests/test_fdn_grad_ref.py holds them to a recomputation."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import pyramid_grad_ref as P

F64 = torch.float64
F32 = torch.float32
GROUPS = 32
EPS = float(np.float32(1e-5))                      # nn.GroupNorm's default as fp32 holds it (the launcher's argument is a float)
FACTOR = 4.0
ULP = 2.0 ** -23
TENSORS = ("y", "mean", "rstd", "g_x", "g_gamma")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the operator, differentiable
def fdn(x, gamma, beta, eps=EPS):
    """control_utils.py:28-34 after the two convolutions, in the operands' dtype.  F.group_norm refuses a tensor with one value per
    group in all ([1, 32, 1, 1]: "expected more than 1 value per channel"); `normalize` is the same function written out, used for
    that shape alone (tests/test_fdn_grad_ref.py holds the two together on every other case)."""
    norm = normalize(x, eps) if x.numel() == GROUPS else F.group_norm(x, GROUPS, None, None, eps)
    return norm * (1 + gamma) + beta


def normalize(x, eps=EPS):
    """GroupNorm(32, C, affine=False) written out"""
    xg = x.reshape(x.shape[0], GROUPS, -1)
    mean = xg.mean(-1, keepdim=True)
    var = ((xg - mean) ** 2).mean(-1, keepdim=True)
    return ((xg - mean) / torch.sqrt(var + eps)).reshape(x.shape)


def stats(x, eps=EPS):
    """(mean, rstd), each [N, 32], in x's dtype: the biased variance, as F.group_norm forms it"""
    xg = x.reshape(x.shape[0], GROUPS, -1)
    mean = xg.mean(-1)
    var = ((xg - mean[..., None]) ** 2).mean(-1)
    return mean, 1 / torch.sqrt(var + eps)


def evaluate(t, dtype=F64):
    """(y, mean, rstd, g_x, g_gamma, g_beta) of loss = (fdn(x, gamma, beta) * g).sum() by autograd with leaves of `dtype`"""
    x, gamma, beta, g = (v.detach().to(dtype) for v in t)
    leaves = [v.requires_grad_(True) for v in (x, gamma, beta)]
    y = fdn(*leaves)
    gx, gg, gb = torch.autograd.grad((y * g).sum(), leaves)
    mean, rstd = stats(x.detach())
    return y.detach(), mean, rstd, gx, gg, gb


# ------------------------------------------------------------------------------------------ the closed forms
FAULTS = ("no_s1", "no_s2", "unbiased_var", "no_eps", "gamma_not_1p", "ggamma_from_x", "m_is_hw", "skip_last_channel")


def closed_form(t, fault=None, eps=EPS):
    """fp64 (y, mean, rstd, g_x, g_gamma, g_beta) by the formulas of include/diffcodec_fdn_hip.h"""
    x, gamma, beta, g = (v.to(F64) for v in t)
    n, c, h, w = x.shape
    cpg = c // GROUPS
    m = cpg * h * w
    div = h * w if fault == "m_is_hw" else m
    keep = (cpg - 1) * h * w if fault == "skip_last_channel" and cpg > 1 else m        # the elements every sum runs over
    xg, gmg, btg, gg = (v.reshape(n, GROUPS, m) for v in (x, gamma, beta, g))
    mean = xg[..., :keep].sum(-1) / div
    var = ((xg - mean[..., None]) ** 2)[..., :keep].sum(-1) / div
    if fault == "unbiased_var":
        var = var * m / (m - 1)
    rstd = 1 / torch.sqrt(var + (0.0 if fault == "no_eps" else eps))
    scale = gmg if fault == "gamma_not_1p" else 1 + gmg
    xh = (xg - mean[..., None]) * rstd[..., None]
    y = xh * scale + btg
    gh = gg * scale
    s1 = torch.zeros_like(mean) if fault == "no_s1" else gh[..., :keep].sum(-1)
    s2 = torch.zeros_like(mean) if fault == "no_s2" else (gh * xh)[..., :keep].sum(-1)
    gx = rstd[..., None] * (gh - s1[..., None] / div - xh * s2[..., None] / div)
    ggam = gg * (xg if fault == "ggamma_from_x" else xh)
    return y.reshape(x.shape), mean, rstd, gx.reshape(x.shape), ggam.reshape(x.shape), g


def one_pass_fp32(x, eps=EPS):
    """(mean, rstd) with the single-pass variance E[x^2] - mean^2, every operation in fp32: what the kernels must not be"""
    xg = x.to(F32).reshape(x.shape[0], GROUPS, -1)
    mean = xg.mean(-1)
    var = ((xg * xg).mean(-1) - mean * mean).clamp(min=0)
    return mean, 1 / torch.sqrt(var + np.float32(eps))


# ------------------------------------------------------------------------------------------ op-level cases
# (N, C, H, W, family).  "plain": a per-group offset of a few sigma; "far": |mean| / sigma = 100 in every group, which is what
# separates two-pass from one-pass statistics.
CASES = [(1, 32, 1, 1, "plain"),          # m = 1: var = 0, xh = 0, g_x and g_gamma exactly 0
         (2, 32, 3, 5, "plain"),          # one channel per group, m = 15 below the workgroup size, 4-byte path
         (3, 64, 7, 9, "plain"),          # two channels per group, odd plane, N = 3
         (2, 96, 16, 16, "plain"),        # m = 768: several elements per thread, 16-byte path
         (2, 96, 16, 16, "far"),
         (1, 320, 32, 32, "plain"),       # m = 10240: a production group
         (2, 1280, 8, 8, "plain")]        # 40 channels per group, the deepest level
CONSTANT_GROUP = (0, 3)                   # (sample, group) that is exactly constant wherever m > 1
BATCH_CASE = (3, 64, 7, 9, "plain")
FAR_CASE = (2, 96, 16, 16, "far")


def label(case):
    return "x".join(map(str, case[:4])) + "-" + case[4]


def group_size(case):
    return case[1] // GROUPS * case[2] * case[3]


def inputs(case):
    """fp32 CPU (x, gamma, beta, g).  x = offset + sigma * z per (sample, group), z seeded normal and standardised over the group,
    sigma log-uniform in [0.004, 0.04] (rstd between 25 and 170, so that eps = 1e-5 is not negligible and the constant group's
    rstd = eps^-1/2 = 316 does not set the scale of g_x alone); one group exactly constant; gamma N(0, 0.5^2) with a quarter of the
    elements around -1 and some exactly -1, so that 1 + gamma takes both signs and zero; g seeded normal."""
    n, c, h, w, family = case
    m = group_size(case)
    gen = torch.Generator().manual_seed(41000 + CASES.index(case))
    sigma = torch.exp(torch.rand(n, GROUPS, 1, generator=gen, dtype=F64) * math.log(10.0) + math.log(0.004))
    z = torch.randn(n, GROUPS, m, generator=gen, dtype=F64)
    if m > 1:
        z = (z - z.mean(-1, keepdim=True)) / z.std(-1, unbiased=False, keepdim=True)
    sign = torch.where(torch.rand(n, GROUPS, 1, generator=gen) < 0.5, -1.0, 1.0).to(F64)
    offset = sign * 100.0 * sigma if family == "far" else 3.0 * sigma * torch.randn(n, GROUPS, 1, generator=gen, dtype=F64)
    x = (offset + sigma * z).to(F32)
    if m > 1:
        x[CONSTANT_GROUP] = x[CONSTANT_GROUP][0]
    gamma = 0.5 * torch.randn(n, c, h, w, generator=gen)
    near = torch.rand(n, c, h, w, generator=gen) < 0.25
    gamma = torch.where(near, -1.0 + 0.2 * torch.randn(n, c, h, w, generator=gen), gamma)
    gamma.reshape(n, -1)[:, ::7] = -1.0
    beta = torch.randn(n, c, h, w, generator=gen)
    g = torch.randn(n, c, h, w, generator=gen)
    return x.reshape(n, c, h, w), gamma, beta, g


def conditions(case):
    """-> the complaints about a case's inputs (conditions, not measurements)"""
    x, gamma, beta, g = inputs(case)
    n, c, h, w, family = case
    m = group_size(case)
    bad = []
    xg = x.to(F64).reshape(n, GROUPS, m)
    if m > 1:
        const = torch.zeros(n, GROUPS, dtype=torch.bool)
        const[CONSTANT_GROUP] = True
        spread = xg.amax(-1) - xg.amin(-1)
        if not bool((spread[const] == 0).all()) or not bool((spread[~const] > 0).all()):
            bad.append("exactly one group is constant: no")
        ratio = (xg.mean(-1).abs() / xg.std(-1, unbiased=False).clamp(min=1e-300))[~const]
        if family == "far" and not (99.0 <= float(ratio.min()) and float(ratio.max()) <= 101.0):
            bad.append(f"|mean| / sigma in [{float(ratio.min()):.1f}, {float(ratio.max()):.1f}], not 100")
        if family == "plain" and float(ratio.max()) > 20.0:
            bad.append(f"|mean| / sigma up to {float(ratio.max()):.1f} in a plain case")
        gg = g.reshape(n, GROUPS, m)
        if not bool((gg.amax(-1) > gg.amin(-1)).all()):
            bad.append("g is constant over a group")
    s = (1 + gamma).reshape(n, -1)
    if not bool(((s > 0).any(1) & (s < 0).any(1) & (s == 0).any(1)).all()):
        bad.append("1 + gamma does not take both signs and zero in every sample")
    ref = evaluate((x, gamma, beta, g))
    for nm, r in zip(TENSORS + ("g_beta",), ref):
        zero = float(r.abs().max()) == 0.0
        if zero != (m == 1 and nm in ("g_x", "g_gamma")):                  # at m = 1, xh = 0: both gradients are exactly 0
            bad.append(f"{nm}: identically zero is {zero}")
    return bad


def norm_error(v, ref):
    """max|v - ref| / max|ref| over the whole tensor; for a reference that is identically zero: 0 when v is too, else inf"""
    v = v.detach().cpu().to(F64)
    ref = ref.detach().cpu().to(F64)
    top = float(ref.abs().max())
    if top == 0.0:
        return 0.0 if float(v.abs().max()) == 0.0 else math.inf
    return float((v - ref).abs().max()) / top


def bar_of(fp32_error):
    return max(FACTOR * fp32_error, ULP)


def fp32_error(case):
    """the norm of torch fp32 on the CPU against fp64, per tensor of TENSORS"""
    t = inputs(case)
    return tuple(norm_error(a, b) for a, b in zip(evaluate(t, F32)[:5], evaluate(t, F64)[:5]))


# `fp32_error(case)` as measured on the CPU: (y, mean, rstd, g_x, g_gamma)
CPU_FP32 = {
    (1, 32, 1, 1, 'plain'): (0, 0, 4.2e-08, 0, 0),
    (2, 32, 3, 5, 'plain'): (2.1e-07, 9e-08, 4.9e-08, 1.2e-07, 4.1e-07),
    (3, 64, 7, 9, 'plain'): (2.5e-07, 7e-08, 6.7e-08, 1.4e-07, 2.6e-07),
    (2, 96, 16, 16, 'plain'): (1.2e-07, 3.6e-08, 5.9e-08, 9.3e-08, 1.1e-07),
    (2, 96, 16, 16, 'far'): (2.9e-06, 6.8e-08, 4.2e-08, 4.7e-07, 4e-06),
    (1, 320, 32, 32, 'plain'): (5.3e-07, 1e-07, 4.2e-08, 1.3e-07, 5.7e-07),
    (2, 1280, 8, 8, 'plain'): (2.5e-07, 8.2e-08, 6.4e-08, 9.6e-08, 3e-07),
}
BARS = {k: tuple(bar_of(v) for v in e) for k, e in CPU_FP32.items()}


# ------------------------------------------------------------------------------------------ the golden
def golden():
    """tests/golden/control_fdn.npz -> (sd, x, local, y): FDN.forward of the reference's own module (oracle/make_goldens.py)"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "control_fdn.npz"))
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")}
    return sd, torch.from_numpy(z["x"]), torch.from_numpy(z["local"]), torch.from_numpy(z["y"])


def fdn_module(sd, p, x, local, dtype=F64):
    """oracle.control_ref.fdn on weights and operands of `dtype`"""
    from oracle import control_ref as C
    return C.fdn({k: v.to(dtype) for k, v in sd.items() if k.startswith(p)}, p, x.to(dtype), local.to(dtype))


def golden_distance():
    sd, x, local, y = golden()
    return norm_error(y, fdn_module(sd, "", x, local, F64))


GOLDEN_DISTANCE = 1.9e-07                           # `golden_distance()` as measured on the CPU


# ------------------------------------------------------------------------------------------ the module end to end
MODULE_CASE = P.MODULE_CASES[0]                   # widths (64, 64, 128, 128) on a 192 x 192 input at batch 2: the pyramid module test's
FDN_NAMES = ("fdn64", "fdn32", "fdn16", "fdn08")
SITES = (("fdn64", 0), ("fdn32", 1), ("fdn16", 2), ("fdn08", 3), ("fdn08", 3))       # flownet.py:84, 98-106


def module_state_dict():
    """a seeded fp32 state dict of the layers DualFlowControlNet adds, in the reference's key layout: the pyramid's recipe (non-zero
    zero convs: at their zero initialisation every level is 0 and every extractor gradient vanishes) under `feature_extractor.`, and
    nn.Conv2d's initialisation scale for the FDN convolutions"""
    inject, _ = MODULE_CASE
    sd = {"feature_extractor." + k: v for k, v in P.module_inputs(MODULE_CASE)[0].items()}
    gen = torch.Generator().manual_seed(42000)
    for name, c in zip(FDN_NAMES, inject):
        bound = 1.0 / math.sqrt(c * 9)
        for conv in ("conv_gamma", "conv_beta"):
            sd[f"{name}.{conv}.weight"] = (torch.rand(c, c, 3, 3, generator=gen) * 2 - 1) * bound
            sd[f"{name}.{conv}.bias"] = (torch.rand(c, generator=gen) * 2 - 1) * bound
    return sd


def module_inputs():
    """(sd, cond, flow, samples per site, G per site): cond and flow by the recipe of pyramid_grad_ref.module_inputs, so no level is
    dead; one seeded sample and one seeded linear functional per injection site"""
    inject, n = MODULE_CASE
    _, cond, flow, _ = P.module_inputs(MODULE_CASE)
    gen = torch.Generator().manual_seed(42001)
    s = P.MODULE_SIZE
    shapes = [(n, inject[lv], s >> (3 + lv), s >> (3 + lv)) for _, lv in SITES]
    samples = [torch.randn(sh, generator=gen) + 0.5 for sh in shapes]
    G = [torch.randn(sh, generator=gen) for sh in shapes]
    return module_state_dict(), cond, flow, samples, G


def module_forward(sd, cond, aux, samples, dtype=F64):
    """the five injections through oracle.control_ref.fdn on the pyramid of pyramid_grad_ref.extractor, given each level's flows and
    occlusion masks (`aux`): the masks are a `> 0.3` test on fp32 arithmetic, so the GPU tests hand in the device's own"""
    from oracle import control_ref as C
    ext = {k[len("feature_extractor."):]: v for k, v in sd.items() if k.startswith("feature_extractor.")}
    levels = P.extractor(ext, cond, aux, dtype)
    return [C.fdn(sd, name + ".", smp, levels[lv]) for (name, lv), smp in zip(SITES, samples)]


def module_grads(sd, cond, aux, samples, G, dtype=F64):
    """{key: d loss / d sd[key]} and {"sample.i": d loss / d samples[i]} of loss = sum_sites (out * G).sum()"""
    keys = sorted(sd)
    leaves = {k: sd[k].detach().to(dtype).requires_grad_(True) for k in keys}
    smp = [s.detach().to(dtype).requires_grad_(True) for s in samples]
    outs = module_forward(leaves, cond, aux, smp, dtype)
    loss = sum((o * g.to(dtype)).sum() for o, g in zip(outs, G))
    grads = torch.autograd.grad(loss, [leaves[k] for k in keys] + smp)
    out = dict(zip(keys, grads[:len(keys)]))
    out.update({f"sample.{i}": gr for i, gr in enumerate(grads[len(keys):])})
    return out


def module_fp32_error():
    sd, cond, flow, samples, G = module_inputs()
    aux = P.cpu_aux(cond, flow)
    g64, g32 = module_grads(sd, cond, aux, samples, G, F64), module_grads(sd, cond, aux, samples, G, F32)
    return {k: norm_error(g32[k], g64[k]) for k in g64}


# fp32 against fp64 at the CPU's masks, one entry per parameter and per sample: `module_fp32_error()` as measured on the CPU
MODULE_CPU_FP32 = {
    'fdn08.conv_beta.bias': 1.2e-07,
    'fdn08.conv_beta.weight': 1.6e-07,
    'fdn08.conv_gamma.bias': 2.3e-07,
    'fdn08.conv_gamma.weight': 2e-07,
    'fdn16.conv_beta.bias': 2.8e-07,
    'fdn16.conv_beta.weight': 3.2e-07,
    'fdn16.conv_gamma.bias': 2.1e-07,
    'fdn16.conv_gamma.weight': 3.2e-07,
    'fdn32.conv_beta.bias': 4.7e-07,
    'fdn32.conv_beta.weight': 5.9e-07,
    'fdn32.conv_gamma.bias': 7.3e-07,
    'fdn32.conv_gamma.weight': 9.1e-07,
    'fdn64.conv_beta.bias': 9.3e-07,
    'fdn64.conv_beta.weight': 2e-06,
    'fdn64.conv_gamma.bias': 4.5e-07,
    'fdn64.conv_gamma.weight': 1.2e-06,
    'feature_extractor.extractors_first.0.0.bias': 1.6e-06,
    'feature_extractor.extractors_first.0.0.weight': 2e-06,
    'feature_extractor.extractors_first.1.0.bias': 3.6e-07,
    'feature_extractor.extractors_first.1.0.weight': 5.2e-07,
    'feature_extractor.extractors_first.2.0.bias': 9.1e-07,
    'feature_extractor.extractors_first.2.0.weight': 1.3e-06,
    'feature_extractor.extractors_first.3.0.bias': 1e-06,
    'feature_extractor.extractors_first.3.0.weight': 1e-06,
    'feature_extractor.extractors_last.0.0.bias': 1.4e-06,
    'feature_extractor.extractors_last.0.0.weight': 1.4e-06,
    'feature_extractor.extractors_last.1.0.bias': 4.7e-07,
    'feature_extractor.extractors_last.1.0.weight': 7.8e-07,
    'feature_extractor.extractors_last.2.0.bias': 2.2e-06,
    'feature_extractor.extractors_last.2.0.weight': 2.3e-06,
    'feature_extractor.extractors_last.3.0.bias': 4.5e-07,
    'feature_extractor.extractors_last.3.0.weight': 5.3e-07,
    'feature_extractor.first_pre_extractor.0.bias': 2.1e-06,
    'feature_extractor.first_pre_extractor.0.weight': 2e-06,
    'feature_extractor.first_pre_extractor.2.bias': 3.1e-06,
    'feature_extractor.first_pre_extractor.2.weight': 1.6e-06,
    'feature_extractor.first_pre_extractor.4.bias': 1.7e-06,
    'feature_extractor.first_pre_extractor.4.weight': 2.4e-06,
    'feature_extractor.first_pre_extractor.6.bias': 1.2e-06,
    'feature_extractor.first_pre_extractor.6.weight': 1.8e-06,
    'feature_extractor.first_pre_extractor.8.bias': 1.7e-06,
    'feature_extractor.first_pre_extractor.8.weight': 2.1e-06,
    'feature_extractor.last_pre_extractor.0.bias': 1.4e-06,
    'feature_extractor.last_pre_extractor.0.weight': 2.2e-06,
    'feature_extractor.last_pre_extractor.2.bias': 2.1e-06,
    'feature_extractor.last_pre_extractor.2.weight': 1.3e-06,
    'feature_extractor.last_pre_extractor.4.bias': 1.6e-06,
    'feature_extractor.last_pre_extractor.4.weight': 1.5e-06,
    'feature_extractor.last_pre_extractor.6.bias': 9.9e-07,
    'feature_extractor.last_pre_extractor.6.weight': 1.3e-06,
    'feature_extractor.last_pre_extractor.8.bias': 1.1e-06,
    'feature_extractor.last_pre_extractor.8.weight': 1.5e-06,
    'feature_extractor.wrapper.0.metric_net.0.bias': 8.5e-06,
    'feature_extractor.wrapper.0.metric_net.0.weight': 4.8e-06,
    'feature_extractor.wrapper.0.metric_net.2.bias': 9.4e-06,
    'feature_extractor.wrapper.0.metric_net.2.weight': 8.3e-06,
    'feature_extractor.wrapper.1.metric_net.0.bias': 3e-06,
    'feature_extractor.wrapper.1.metric_net.0.weight': 1.3e-06,
    'feature_extractor.wrapper.1.metric_net.2.bias': 2.6e-06,
    'feature_extractor.wrapper.1.metric_net.2.weight': 1.5e-06,
    'feature_extractor.wrapper.2.metric_net.0.bias': 9.6e-06,
    'feature_extractor.wrapper.2.metric_net.0.weight': 5e-06,
    'feature_extractor.wrapper.2.metric_net.2.bias': 3.7e-05,
    'feature_extractor.wrapper.2.metric_net.2.weight': 6.4e-06,
    'feature_extractor.wrapper.3.metric_net.0.bias': 2e-05,
    'feature_extractor.wrapper.3.metric_net.0.weight': 2.2e-06,
    'feature_extractor.wrapper.3.metric_net.2.bias': 1.7e-05,
    'feature_extractor.wrapper.3.metric_net.2.weight': 6.5e-06,
    'feature_extractor.zero_convs.0.bias': 7.2e-07,
    'feature_extractor.zero_convs.0.weight': 1.5e-06,
    'feature_extractor.zero_convs.1.bias': 4.2e-07,
    'feature_extractor.zero_convs.1.weight': 8.1e-07,
    'feature_extractor.zero_convs.2.bias': 3.2e-07,
    'feature_extractor.zero_convs.2.weight': 6.9e-07,
    'feature_extractor.zero_convs.3.bias': 1.9e-07,
    'feature_extractor.zero_convs.3.weight': 5.1e-07,
    'sample.0': 2.1e-07,
    'sample.1': 1.2e-07,
    'sample.2': 1.6e-07,
    'sample.3': 1.2e-07,
    'sample.4': 1.2e-07,
}


def module_bar(key):
    return bar_of(MODULE_CPU_FP32[key])
