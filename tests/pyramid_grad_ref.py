"""Yardsticks of the trainable control pyramid (plain module, numpy and torch only, nothing from the package; imported by
tests/test_pyramid_grad_ref.py on the CPU and tests/test_gpu_pyramid_grad.py on the GPU):

* `level`            one pyramid level after its convolutions (extractors.py:293-310 with control_utils.py:49-72 inlined) in
                     differentiable torch of a given dtype, on `splat_grad_ref.softsplat_f64` / `softsplat_f32`.  Flows and masks are
                     constants.
* `extractor`        the whole Bi_Dir_FeatureExtractor forward in differentiable torch of a given dtype, GIVEN each level's resized
                     flows and occlusion masks: `occ` is a `> 0.3` test on fp32 arithmetic, so a reference that recomputed it would
                     linearise at other masks than the device.  The GPU tests hand in the device's own (`return_aux`).
* `closed_form`      the gradients of `level` by the formulas of include/diffcodec_pyramid_hip.h in fp64, with the planted faults
                     of the sharpness test.
* case tables, input builders, the conditions the inputs must meet, and the bars: per gradient tensor 4 x the
  `splat_grad_ref.grad_norm_error` of the fp32 restatement against fp64 on that case (the margin the splat and loss tests give a
  different summation order).  The fp32 errors are stored (`CPU_FP32`, `MODULE_CPU_FP32`); tests/test_pyramid_grad_ref.py holds
  them to a recomputation."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import edge_cases as E
import splat_grad_ref as S

F64 = torch.float64
F32 = torch.float32
EPS_FUSE = float(np.float32(1e-6))                 # extractors.py:298 as fp32 holds it
FACTOR = 4.0
GRAD_NAMES = ("first", "last", "metric_f", "metric_b")


# ------------------------------------------------------------------------------------------ the level, differentiable
def level(first, last, mf, mb, ff, fb, of, ob, dtype=F64):
    splat = S.softsplat_f64 if dtype == F64 else S.softsplat_f32
    first, last, mf, mb, of, ob = (t.to(dtype) for t in (first, last, mf, mb, of, ob))
    wf = splat(first, ff, mf, "soft") * (1 - of)
    wl = splat(last, fb, mb, "soft") * (1 - ob)
    conf = torch.clamp(torch.cat([mf, mb], 1), min=0)
    w = conf / (conf.sum(1, keepdim=True) + EPS_FUSE)
    fused = w[:, :1] * wf + w[:, 1:] * wl
    holes = (of + ob) > 1.5
    return torch.where(holes.expand_as(fused), 0.5 * (wf + wl), fused)


def level_oracle(first, last, mf, mb, ff, fb, of, ob):
    """the same level written as oracle/control_ref.py writes it (feature_warper's tail and bi_dir_feature_extractor's fusion),
    fp64, with this module's splat: what `level` is held to"""
    def warper(feat, flow, metric, mask):
        warped = S.softsplat_f64(feat, flow, metric, "soft")
        if mask is not None:
            warped = warped * (1 - mask)
        return warped, metric
    wf, cf = warper(first.to(F64), ff, mf.to(F64), of.to(F64))
    wl, cb = warper(last.to(F64), fb, mb.to(F64), ob.to(F64))
    conf = torch.clamp(torch.cat([cf, cb], dim=1), min=0)
    w_norm = conf / (conf.sum(dim=1, keepdim=True) + EPS_FUSE)
    fused = w_norm[:, :1] * wf + w_norm[:, 1:] * wl
    holes = (of + ob) > 1.5
    if holes.any():
        fused = torch.where(holes.expand_as(fused), 0.5 * (wf + wl), fused)
    return fused


def level_grads(inputs, G, dtype=F64, fn=level):
    """(d first, d last, d metric_f, d metric_b) of loss = (level(...) * G).sum() by autograd with leaves of `dtype`"""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in inputs[:4]]
    out = fn(*leaves, *inputs[4:]) if fn is not level else level(*leaves, *inputs[4:], dtype=dtype)
    return torch.autograd.grad((out * G.to(out.dtype)).sum(), leaves)


# ------------------------------------------------------------------------------------------ the closed forms
FAULTS = ("gate_gt", "no_occ", "no_gden", "no_gconf", "no_eps6", "no_eps7", "swap_sides", "skip_last_channel", "skip_corner")


def _gather(plane, idx):
    """plane [N, K, HW] read at idx [N, HW] -> [N, K, HW]"""
    n, k, hw = plane.shape
    return torch.gather(plane, 2, idx.reshape(n, 1, hw).expand(n, k, hw))


def closed_form(inputs, G, fault=None):
    """fp64 gradients (first, last, metric_f, metric_b) by the target-side / source-side formulas"""
    first, last, mf, mb, ff, fb, of, ob = inputs
    n, c, h, w = first.shape
    hw = h * w
    x = [first.to(F64), last.to(F64)]
    m = [mf.to(F64), mb.to(F64)]
    occ = [of.to(F64).reshape(n, 1, hw), ob.to(F64).reshape(n, 1, hw)]
    flows = [ff, fb]
    g = G.to(F64).reshape(n, c, hw)
    eps7 = 0.0 if fault == "no_eps7" else S.EPS
    eps6 = 0.0 if fault == "no_eps6" else EPS_FUSE
    e = [t.exp() for t in m]
    corner = [S._corner_terms_f64(fl, h, w) for fl in flows]                # dwx, dwy, weights, ok, idx
    den, y = [], []
    for s in range(2):
        acc = S._splat_sum_torch(torch.cat([x[s] * e[s], e[s]], 1), flows[s], F64).reshape(n, c + 1, hw)
        den.append(acc[:, -1:] + eps7)
        y.append(acc[:, :-1] / den[s])
    wv = [y[s] * (1 - occ[s]) for s in range(2)]
    cc = 1 if fault == "skip_last_channel" and c > 1 else 0
    A = [(g * wv[s])[:, :c - cc].sum(1, keepdim=True) for s in range(2)]
    cf, cb = m[0].reshape(n, 1, hw), m[1].reshape(n, 1, hw)
    p, q = cf.clamp(min=0), cb.clamp(min=0)
    Ssum = p + q + eps6
    hole = (occ[0] + occ[1]) > 1.5
    gate = (lambda v: v > 0) if fault == "gate_gt" else (lambda v: v >= 0)
    zero = torch.zeros_like(cf)
    g_conf = [torch.where(gate(cf) & ~hole, (A[0] * (Ssum - p) - A[1] * q) / Ssum ** 2, zero),
              torch.where(gate(cb) & ~hole, (A[1] * (Ssum - q) - A[0] * p) / Ssum ** 2, zero)]
    half = torch.full_like(cf, 0.5)
    wgt = [torch.where(hole, half, p / Ssum), torch.where(hole, half, q / Ssum)]
    out_x, out_m = [], []
    for s in range(2):
        keep = torch.ones_like(occ[s]) if fault == "no_occ" else 1 - occ[s]
        coef = keep * wgt[s] / den[s]
        gden = torch.zeros_like(coef) if fault == "no_gden" else -wgt[s] * A[s] / den[s]
        _, _, wts, ok, idx = corner[s]
        Ac = torch.zeros((n, c, hw), dtype=F64)
        T = torch.zeros((n, 1, hw), dtype=F64)
        for k in range(4):
            if fault == "skip_corner" and k == 3:
                continue
            b = torch.where(ok[k], wts[k], torch.zeros_like(wts[k])).reshape(n, 1, hw)
            Ac = Ac + b * _gather(coef * g, idx[k])
            T = T + b * _gather(gden, idx[k])
        es = e[s].reshape(n, 1, hw)
        gx = es * Ac
        gm = es * ((x[s].reshape(n, c, hw) * Ac)[:, :c - cc].sum(1, keepdim=True) + T)
        if fault != "no_gconf":
            gm = gm + g_conf[s]
        out_x.append(gx.reshape(n, c, h, w))
        out_m.append(gm.reshape(n, 1, h, w))
    if fault == "swap_sides":
        out_m = out_m[::-1]
    return out_x[0], out_x[1], out_m[0], out_m[1]


# ------------------------------------------------------------------------------------------ op-level cases
# channel slices per pixel of the kernels as built (csrc/pyramid_grad.hip slices()): 1 below 16 channels, else 4 on maps of >= 1024
# pixels and 16 below; a workgroup holds 256 / slices pixels of the N * H * W
def slices(c, hw):
    return 1 if c < 16 else 4 if hw >= 1024 else 16


SHAPES = [(1, 1, 1, 1), (2, 3, 1, 7), (2, 3, 7, 1), (3, 20, 5, 9), (2, 33, 17, 70), (2, 640, 8, 8), (3, 160, 16, 16),
          # one pixel and one channel past every tile edge: 256 pixels x 1 slice, 16 x 16, 64 x 4
          (1, 5, 1, 257), (1, 17, 5, 13), (1, 17, 33, 33)]
TILE_EDGE_SHAPES = SHAPES[-3:]
CASES = [(1, 1, 1, 1, "smooth"), (2, 3, 1, 7, "collapse"), (2, 3, 1, 7, "away"), (2, 3, 7, 1, "border"), (2, 3, 7, 1, "nonfinite")] + \
        [(3, 20, 5, 9, f) for f in E.FLOW_FAMILIES] + \
        [(2, 33, 17, 70, "smooth"), (2, 33, 17, 70, "nonfinite"), (2, 640, 8, 8, "smooth"), (2, 640, 8, 8, "border"),
         (3, 160, 16, 16, "smooth"), (3, 160, 16, 16, "collapse"), (1, 5, 1, 257, "smooth"), (1, 17, 5, 13, "border"),
         (1, 17, 33, 33, "nonfinite")]
assert len(set(CASES)) == len(CASES) and {c[:4] for c in CASES} == set(SHAPES) and {c[4] for c in CASES} == set(E.FLOW_FAMILIES)


# cases whose first seed left a reference gradient identically zero (the border and away families reach a handful of targets, which
# must then be unoccluded and carry a positive confidence): the first multiple of 100 added to the seed that does not
RESEED = {(3, 20, 5, 9, 'border'): 1, (3, 20, 5, 9, 'away'): 6,
          # the single pixel: unoccluded, both confidences positive and the source lands inside, so that no gradient is the 1e-7
          # residue of a cancellation (a quantity fp64 itself holds to 1e-9 only, which the 1e-12 checks cannot use)
          (1, 1, 1, 1, 'smooth'): 68,
          # likewise the one target the away family reaches
          (2, 3, 1, 7, 'away'): 11}


def label(case):
    return "x".join(map(str, case[:4])) + "-" + case[4]


def inputs(case):
    """fp32 CPU (first, last, metric_f, metric_b, flow_f, flow_b, occ_f, occ_b, G) of a case.  Metrics from the signed family
    (multiples of 0.25 in [-2, 2]: both signs and exact zeros, as confidences), with an exact zero planted in each on an unoccluded
    pixel; masks are independent coin flips."""
    n, c, h, w, family = case
    i = CASES.index(case) + 100 * RESEED.get(case, 0)
    gen = torch.Generator().manual_seed(31000 + i)
    first = torch.randn(n, c, h, w, generator=gen) + 0.3
    last = torch.randn(n, c, h, w, generator=gen) - 0.2
    ff = E.splat_flow(family, n, h, w, gen)
    fb = E.splat_flow(family, n, h, w, gen)
    mf = S.metric_family("signed", n, h, w, 2 * i)
    mb = S.metric_family("signed", n, h, w, 2 * i + 1)
    of = (torch.rand(n, 1, h, w, generator=gen) < 0.5).float()
    ob = (torch.rand(n, 1, h, w, generator=gen) < 0.5).float()
    if n * h * w >= 8:
        for t, at in ((mf, 2), (mb, 5)):
            t.reshape(-1)[at] = 0.0
            of.reshape(-1)[at] = 0.0
            ob.reshape(-1)[at] = 0.0
    # An exact zero next to a confidence <= 0 leaves S = 1e-6 and a true derivative of 1e6 A at that pixel: with the end-to-end norm
    # (max error over max reference) a few such pixels would leave every ordinary element unchecked.  The other confidence is
    # positive there, so the gate at exactly 0 is still taken and its gradient is of ordinary size.
    mb[(mf == 0) & (mb <= 0)] = 0.5
    mf[(mb == 0) & (mf <= 0)] = 0.75
    G = torch.randn(n, c, h, w, generator=gen)
    return first, last, mf, mb, ff, fb, of, ob, G


def conditions(case):
    """-> the complaints about a case's inputs (conditions, not measurements); [] for a map of fewer than 32 pixels"""
    first, last, mf, mb, ff, fb, of, ob, G = inputs(case)
    if case[2] * case[3] < 32:
        return []
    bad = []
    for nm, o in (("occ_f", of), ("occ_b", ob)):
        if not 0.2 <= float(o.mean()) <= 0.8:
            bad.append(f"{nm}: {float(o.mean()):.2f} ones")
    both = float((of * ob).mean())
    if not 0.1 <= both <= 0.6:
        bad.append(f"both occluded: {both:.2f}")
    for sf in (True, False):
        for sb in (True, False):
            share = float((((mf > 0) == sf) & ((mb > 0) == sb)).float().mean())
            if share < 0.1:
                bad.append(f"sign class (cf > 0: {sf}, cb > 0: {sb}): {share:.2f}")
    for nm, t in (("metric_f", mf), ("metric_b", mb)):
        if not bool((t == 0).any()):
            bad.append(f"{nm}: no exact zero")
    for nm, g in zip(GRAD_NAMES, level_grads((first, last, mf, mb, ff, fb, of, ob), G, F64)):
        if float(g.abs().max()) == 0.0:
            bad.append(f"d {nm}: identically zero")
    return bad


# fp32 restatement against fp64, per gradient tensor (first, last, metric_f, metric_b): `fp32_error(case)` as measured on the CPU
CPU_FP32 = {
    (1, 1, 1, 1, 'smooth'): (5.9e-08, 2e-08, 1.6e-09, 1.3e-07),
    (2, 3, 1, 7, 'collapse'): (1e-07, 1.1e-07, 1.3e-07, 1.4e-07),
    (2, 3, 1, 7, 'away'): (5e-08, 6.2e-08, 6.5e-07, 9.8e-07),
    (2, 3, 7, 1, 'border'): (0, 0, 0, 0),
    (2, 3, 7, 1, 'nonfinite'): (0, 0, 1.7e-07, 0),
    (3, 20, 5, 9, 'smooth'): (1e-07, 1.1e-07, 1.2e-07, 3.8e-07),
    (3, 20, 5, 9, 'collapse'): (6.9e-08, 1.2e-07, 1.3e-07, 1.8e-07),
    (3, 20, 5, 9, 'border'): (1.1e-07, 5.4e-08, 3.5e-07, 6.1e-08),
    (3, 20, 5, 9, 'away'): (5e-08, 5.6e-08, 2e-07, 8.6e-08),
    (3, 20, 5, 9, 'nonfinite'): (1.1e-07, 1.1e-07, 9.5e-08, 2.6e-07),
    (2, 33, 17, 70, 'smooth'): (1.6e-07, 1.7e-07, 2.1e-07, 1.2e-07),
    (2, 33, 17, 70, 'nonfinite'): (1.4e-07, 1.3e-07, 1.3e-07, 1.3e-07),
    (2, 640, 8, 8, 'smooth'): (1.3e-07, 1.6e-07, 1.7e-07, 3.2e-07),
    (2, 640, 8, 8, 'border'): (8.3e-08, 7.8e-08, 5e-08, 3.6e-08),
    (3, 160, 16, 16, 'smooth'): (1.3e-07, 1.3e-07, 2.7e-07, 6.9e-08),
    (3, 160, 16, 16, 'collapse'): (4e-07, 3.5e-07, 2.8e-07, 4.2e-07),
    (1, 5, 1, 257, 'smooth'): (9.9e-08, 1e-07, 8.8e-08, 1.9e-07),
    (1, 17, 5, 13, 'border'): (1.7e-07, 5.4e-08, 3e-07, 1.6e-07),
    (1, 17, 33, 33, 'nonfinite'): (1e-07, 1.3e-07, 1.5e-07, 1.8e-07),
}
# The bar is FACTOR x the fp32 restatement's error.  On a tensor of one non-zero element that error is a single draw and can be far
# below what the number format can promise (1.6e-9 on metric_f of the single pixel): a result one unit in the last place of its own
# storage away from fp64, 2^-23 of the largest element, cannot be called wrong, so no bar is below that.  With the stored errors
# this moves two bars, both of the single-pixel case (metric_f, and `last` from 8e-8).  A reference that is identically zero keeps
# the bar 0: exact zeros are asked for.
ULP = 2.0 ** -23


def bar_of(fp32_error):
    return 0.0 if fp32_error == 0.0 else max(FACTOR * fp32_error, ULP)


BARS = {k: tuple(bar_of(v) for v in e) for k, e in CPU_FP32.items()}


def norm_error(g, ref):
    """splat_grad_ref.grad_norm_error, and for a reference that is identically zero (a map of a few pixels that are all occluded
    or all leave the map): 0 when g is identically zero too, else inf"""
    if float(ref.abs().max()) == 0.0:
        return 0.0 if float(g.detach().abs().max().cpu()) == 0.0 else math.inf
    return S.grad_norm_error(g, ref)


def fp64_grads(case):
    t = inputs(case)
    return level_grads(t[:8], t[8], F64)


def fp32_error(case):
    t = inputs(case)
    g32 = level_grads(t[:8], t[8], F32)
    return tuple(norm_error(a, b) for a, b in zip(g32, fp64_grads(case)))


# ------------------------------------------------------------------------------------------ the gate where it matters most
# `inputs` keeps a positive confidence next to every exact zero, for the sake of the max-norm.  Where one confidence is exactly 0 and
# the other is <= 0, p = q = 0 and S = 1e-6: the gate `>=` passes g_conf = A / S (about 1e6 A) and a gate `>` passes nothing.  These
# pixels are checked one by one, each against its own reference.  (metric tensor: 2 = metric_f, 3 = metric_b; flat pixel; cf; cb)
GATE_CASE = (3, 20, 5, 9, "smooth")
GATE_PIXELS = ((7, 0.0, -0.5), (11, 0.0, 0.0), (13, -1.0, 0.0), (20, 0.0, 0.0), (45 + 9, 0.0, -2.0), (90 + 30, -0.25, 0.0))
GATE_CHECKS = ((2, 7), (2, 11), (3, 13), (2, 20), (3, 20), (2, 45 + 9), (3, 90 + 30))


def gate_inputs():
    """`inputs(GATE_CASE)` with the GATE_PIXELS planted, unoccluded"""
    t = [x.clone() for x in inputs(GATE_CASE)]
    for at, cf, cb in GATE_PIXELS:
        t[2].reshape(-1)[at], t[3].reshape(-1)[at] = cf, cb
        t[6].reshape(-1)[at] = t[7].reshape(-1)[at] = 0.0
    return tuple(t)


def gate_report(grads, t=None):
    """-> [(metric tensor, pixel, |g - ref|, tol, ref)] over GATE_CHECKS for grads = (d first, d last, d metric_f, d metric_b).
    At such a pixel g_m = A / S + the splat's share, A = sum_c g_c w_c with w the masked warp of that side.  The fp32 chain to A: each
    w_c carries the roundings of its own gather and quotient (at most 16 over the few sources of a smooth flow), then C products and
    C additions, in any order; a worst-case linear bound, since one pixel is one draw:
        tol = (2 C + 16) 2^-24 sum_c |g_c w_c| / S  +  1e-3
    the last term for the splat's share of g_m, a quantity of ordinary size (|.| < 1e2) held to 1e-5 of that."""
    t = gate_inputs() if t is None else t
    first, last, mf, mb, ff, fb, of, ob, G = t
    ref = level_grads(t[:8], G, F64)
    w = (S.softsplat_f64(first, ff, mf, "soft") * (1 - of.to(F64)), S.softsplat_f64(last, fb, mb, "soft") * (1 - ob.to(F64)))
    n, c, h, wd = first.shape
    out = []
    for which, at in GATE_CHECKS:
        img, pix = divmod(at, h * wd)
        mass = float((G.to(F64)[img].reshape(c, -1)[:, pix] * w[which - 2][img].reshape(c, -1)[:, pix]).abs().sum())
        tol = (2 * c + 16) * 2.0 ** -24 * mass / EPS_FUSE + 1e-3
        r = float(ref[which].reshape(-1)[at])
        out.append((which, at, abs(float(grads[which].detach().cpu().to(F64).reshape(-1)[at]) - r), tol, r))
    return out


# ------------------------------------------------------------------------------------------ the whole extractor
def _conv(sd, key, x, stride=1, silu=False):
    y = F.conv2d(x, sd[key + ".weight"].to(x.dtype), sd[key + ".bias"].to(x.dtype), stride=stride, padding=1)
    return F.silu(y) if silu else y


def extractor(sd, cond, aux, dtype=F64):
    """Bi_Dir_FeatureExtractor.forward (oracle/control_ref.py bi_dir_feature_extractor) with every tensor of `dtype` and each level's
    flows and masks taken from `aux` (a list of dict(flow_f, flow_b, occ_f, occ_b)) -> the four levels"""
    cond = cond.to(dtype)

    def pre(p, x):
        for i, st in zip((0, 2, 4, 6, 8), (1, 2, 1, 2, 1)):
            x = _conv(sd, f"{p}_pre_extractor.{i}", x, st, True)
        return x
    f, l = pre("first", cond[:, 3:]), pre("last", cond[:, :3])
    outs = []
    for idx in range(4):
        f = _conv(sd, f"extractors_first.{idx}.0", f, 2, True)
        l = _conv(sd, f"extractors_last.{idx}.0", l, 2, True)
        a = aux[idx]
        mf = _conv(sd, f"wrapper.{idx}.metric_net.2", _conv(sd, f"wrapper.{idx}.metric_net.0", f, 1, True))
        mb = _conv(sd, f"wrapper.{idx}.metric_net.2", _conv(sd, f"wrapper.{idx}.metric_net.0", l, 1, True))
        fused = level(f, l, mf, mb, *(a[k].float().to(cond.device) for k in ("flow_f", "flow_b", "occ_f", "occ_b")), dtype)
        outs.append(_conv(sd, f"zero_convs.{idx}", fused))
    return outs


def state_dict(inject, seed):
    """a seeded fp32 state dict in the reference's key layout: nn.Conv2d's initialisation scale, NON-zero zero convs (a fresh
    module's are zero and every upstream gradient vanishes) and a zero bias on the last metric_net conv (with a random one the
    confidence had one sign over a whole level)"""
    gen = torch.Generator().manual_seed(32000 + seed)
    half = [c // 2 for c in inject]
    sd = {}

    def conv(key, cin, cout, zero_bias=False):
        bound = 1.0 / math.sqrt(cin * 9)
        sd[key + ".weight"] = (torch.rand(cout, cin, 3, 3, generator=gen) * 2 - 1) * bound
        sd[key + ".bias"] = torch.zeros(cout) if zero_bias else (torch.rand(cout, generator=gen) * 2 - 1) * bound
    pre_ch = (3, 16, 32, 32, 64, 64)
    for side in ("first", "last"):
        for j, i in enumerate((0, 2, 4, 6, 8)):
            conv(f"{side}_pre_extractor.{i}", pre_ch[j], pre_ch[j + 1])
        for i in range(4):
            conv(f"extractors_{side}.{i}.0", ([64] + half)[i], half[i])
    for i in range(4):
        conv(f"wrapper.{i}.metric_net.0", half[i], 64)
        conv(f"wrapper.{i}.metric_net.2", 64, 1, zero_bias=True)
        conv(f"zero_convs.{i}", half[i], inject[i])
    return sd


MODULE_SIZE = 192                                   # levels 24, 12, 6, 3
MODULE_CASES = [((64, 64, 128, 128), 2), ((24, 24, 40, 40), 3)]       # (inject_channels, N)
MODULE_SEEDS = (3, 7)                               # other seeds left a level dead (one confidence sign over a whole 3 x 3 level):
#                                                     tests/test_pyramid_grad_ref.py asserts that these do not


def module_label(case):
    return "x".join(map(str, case[0])) + f"-n{case[1]}"


def module_inputs(case):
    """(sd, cond [N,6,S,S], flow [N,4,S,S], G per level): ff = bicubic-upsampled N(0, 0.15^2 px) noise on an S/16 grid,
    fb = -ff + d with |d| log-uniform in [0.02, 4] px per pixel and a uniform angle, so that every level keeps unoccluded pixels (the
    0.3 threshold means 2.25 px at r = 16 and 0.15 px at r = 2: no single residual mixes all four levels)"""
    inject, n = case
    i = MODULE_SEEDS[MODULE_CASES.index(case)]
    sd = state_dict(inject, i)
    gen = torch.Generator().manual_seed(33000 + i)
    s = MODULE_SIZE
    cond = torch.rand(n, 6, s, s, generator=gen) * 2 - 1
    ff = F.interpolate(0.15 * torch.randn(n, 2, s // 16, s // 16, generator=gen), size=(s, s), mode="bicubic", align_corners=False)
    mag = torch.exp(torch.rand(n, 1, s, s, generator=gen) * (math.log(4.0) - math.log(0.02)) + math.log(0.02))
    ang = torch.rand(n, 1, s, s, generator=gen) * (2 * math.pi)
    fb = -ff + torch.cat([mag * ang.cos(), mag * ang.sin()], 1)
    flow = torch.cat([ff, fb], 1).contiguous()
    G = [torch.randn(n, inject[k], s >> (3 + k), s >> (3 + k), generator=gen) for k in range(4)]
    return sd, cond, flow, G


def module_grads(sd, cond, aux, G, dtype=F64):
    """{key: d loss / d sd[key]} of loss = sum_levels (out * G).sum()"""
    keys = sorted(sd)
    leaves = {k: sd[k].detach().to(dtype).requires_grad_(True) for k in keys}
    outs = extractor(leaves, cond, aux, dtype)
    loss = sum((o * g.to(dtype)).sum() for o, g in zip(outs, G))
    return dict(zip(keys, torch.autograd.grad(loss, [leaves[k] for k in keys])))


def cpu_aux(cond, flow):
    """the resized flows and the masks of every level as oracle/control_ref.py forms them in fp32 on the CPU (the GPU tests take
    the device's own instead)"""
    from oracle import control_ref as R
    h = cond.shape[-2]
    aux = []
    for r in (h // 8, h // 16, h // 32, h // 64):
        flow_f, flow_b = R.resize_and_normalize_flow(flow[:, :2], r, r), R.resize_and_normalize_flow(flow[:, 2:], r, r)
        aux.append(dict(flow_f=flow_f, flow_b=flow_b, occ_f=R.compute_mask(flow_f, flow_b), occ_b=R.compute_mask(flow_b, flow_f)))
    return aux


# fp32 restatement against fp64 at the CPU's masks, the largest over a case's parameter tensors per kind of tensor would hide the
# small ones: one entry per parameter
MODULE_CPU_FP32 = {
    '64x64x128x128-n2': {
        'extractors_first.0.0.bias': 1.5e-06,
        'extractors_first.0.0.weight': 1.5e-06,
        'extractors_first.1.0.bias': 5.3e-07,
        'extractors_first.1.0.weight': 5.7e-07,
        'extractors_first.2.0.bias': 9e-07,
        'extractors_first.2.0.weight': 9.9e-07,
        'extractors_first.3.0.bias': 4.4e-07,
        'extractors_first.3.0.weight': 5.4e-07,
        'extractors_last.0.0.bias': 9e-07,
        'extractors_last.0.0.weight': 1.6e-06,
        'extractors_last.1.0.bias': 4.4e-06,
        'extractors_last.1.0.weight': 4.6e-06,
        'extractors_last.2.0.bias': 1.6e-05,
        'extractors_last.2.0.weight': 1.7e-05,
        'extractors_last.3.0.bias': 3.5e-07,
        'extractors_last.3.0.weight': 4.1e-07,
        'first_pre_extractor.0.bias': 3.7e-06,
        'first_pre_extractor.0.weight': 2e-06,
        'first_pre_extractor.2.bias': 1.8e-06,
        'first_pre_extractor.2.weight': 1.8e-06,
        'first_pre_extractor.4.bias': 2.4e-06,
        'first_pre_extractor.4.weight': 1.5e-06,
        'first_pre_extractor.6.bias': 1e-06,
        'first_pre_extractor.6.weight': 1.5e-06,
        'first_pre_extractor.8.bias': 1.4e-06,
        'first_pre_extractor.8.weight': 1.6e-06,
        'last_pre_extractor.0.bias': 3.2e-06,
        'last_pre_extractor.0.weight': 1.8e-06,
        'last_pre_extractor.2.bias': 1.8e-06,
        'last_pre_extractor.2.weight': 1.2e-06,
        'last_pre_extractor.4.bias': 1.4e-06,
        'last_pre_extractor.4.weight': 1.2e-06,
        'last_pre_extractor.6.bias': 1e-06,
        'last_pre_extractor.6.weight': 1.2e-06,
        'last_pre_extractor.8.bias': 2.5e-06,
        'last_pre_extractor.8.weight': 2.8e-06,
        'wrapper.0.metric_net.0.bias': 5.9e-06,
        'wrapper.0.metric_net.0.weight': 3.9e-06,
        'wrapper.0.metric_net.2.bias': 4.8e-06,
        'wrapper.0.metric_net.2.weight': 4.9e-06,
        'wrapper.1.metric_net.0.bias': 1.4e-06,
        'wrapper.1.metric_net.0.weight': 7.7e-07,
        'wrapper.1.metric_net.2.bias': 8e-07,
        'wrapper.1.metric_net.2.weight': 1.4e-06,
        'wrapper.2.metric_net.0.bias': 4.6e-05,
        'wrapper.2.metric_net.0.weight': 1.2e-05,
        'wrapper.2.metric_net.2.bias': 5.9e-05,
        'wrapper.2.metric_net.2.weight': 1.8e-05,
        'wrapper.3.metric_net.0.bias': 1.3e-05,
        'wrapper.3.metric_net.0.weight': 2.2e-06,
        'wrapper.3.metric_net.2.bias': 1.2e-05,
        'wrapper.3.metric_net.2.weight': 6.7e-06,
        'zero_convs.0.bias': 5.7e-07,
        'zero_convs.0.weight': 7e-07,
        'zero_convs.1.bias': 3.9e-07,
        'zero_convs.1.weight': 5.4e-07,
        'zero_convs.2.bias': 2.8e-07,
        'zero_convs.2.weight': 6.4e-07,
        'zero_convs.3.bias': 1.1e-07,
        'zero_convs.3.weight': 4e-07,
    },
    '24x24x40x40-n3': {
        'extractors_first.0.0.bias': 2.7e-06,
        'extractors_first.0.0.weight': 3.4e-06,
        'extractors_first.1.0.bias': 4.3e-07,
        'extractors_first.1.0.weight': 7.5e-07,
        'extractors_first.2.0.bias': 4.6e-07,
        'extractors_first.2.0.weight': 5.2e-07,
        'extractors_first.3.0.bias': 3.2e-07,
        'extractors_first.3.0.weight': 3.7e-07,
        'extractors_last.0.0.bias': 1.1e-06,
        'extractors_last.0.0.weight': 1.4e-06,
        'extractors_last.1.0.bias': 8e-07,
        'extractors_last.1.0.weight': 7.5e-07,
        'extractors_last.2.0.bias': 6.4e-07,
        'extractors_last.2.0.weight': 7.6e-07,
        'extractors_last.3.0.bias': 2.3e-07,
        'extractors_last.3.0.weight': 3.3e-07,
        'first_pre_extractor.0.bias': 3.3e-06,
        'first_pre_extractor.0.weight': 3.6e-06,
        'first_pre_extractor.2.bias': 2.8e-06,
        'first_pre_extractor.2.weight': 2.7e-06,
        'first_pre_extractor.4.bias': 2.8e-06,
        'first_pre_extractor.4.weight': 3.1e-06,
        'first_pre_extractor.6.bias': 2.9e-06,
        'first_pre_extractor.6.weight': 2.8e-06,
        'first_pre_extractor.8.bias': 3.3e-06,
        'first_pre_extractor.8.weight': 3.1e-06,
        'last_pre_extractor.0.bias': 3.7e-06,
        'last_pre_extractor.0.weight': 2.6e-06,
        'last_pre_extractor.2.bias': 2e-06,
        'last_pre_extractor.2.weight': 1.3e-06,
        'last_pre_extractor.4.bias': 9.4e-07,
        'last_pre_extractor.4.weight': 1.8e-06,
        'last_pre_extractor.6.bias': 8e-07,
        'last_pre_extractor.6.weight': 1.2e-06,
        'last_pre_extractor.8.bias': 8.3e-07,
        'last_pre_extractor.8.weight': 1.2e-06,
        'wrapper.0.metric_net.0.bias': 2.8e-06,
        'wrapper.0.metric_net.0.weight': 2.5e-06,
        'wrapper.0.metric_net.2.bias': 2.7e-06,
        'wrapper.0.metric_net.2.weight': 2.7e-06,
        'wrapper.1.metric_net.0.bias': 1.4e-06,
        'wrapper.1.metric_net.0.weight': 2.6e-06,
        'wrapper.1.metric_net.2.bias': 2.9e-07,
        'wrapper.1.metric_net.2.weight': 1.8e-06,
        'wrapper.2.metric_net.0.bias': 7.8e-07,
        'wrapper.2.metric_net.0.weight': 7.5e-07,
        'wrapper.2.metric_net.2.bias': 1.2e-06,
        'wrapper.2.metric_net.2.weight': 7.8e-07,
        'wrapper.3.metric_net.0.bias': 1.6e-06,
        'wrapper.3.metric_net.0.weight': 2.3e-07,
        'wrapper.3.metric_net.2.bias': 2e-06,
        'wrapper.3.metric_net.2.weight': 8e-07,
        'zero_convs.0.bias': 5.3e-07,
        'zero_convs.0.weight': 5e-07,
        'zero_convs.1.bias': 3.8e-07,
        'zero_convs.1.weight': 1.9e-07,
        'zero_convs.2.bias': 2.2e-07,
        'zero_convs.2.weight': 9.7e-07,
        'zero_convs.3.bias': 1.5e-07,
        'zero_convs.3.weight': 1.5e-07,
    },
}


def module_bar(case, key):
    return bar_of(MODULE_CPU_FP32[module_label(case)][key])


def module_fp32_error(case):
    sd, cond, flow, G = module_inputs(case)
    aux = cpu_aux(cond, flow)
    g64, g32 = module_grads(sd, cond, aux, G, F64), module_grads(sd, cond, aux, G, F32)
    return {k: norm_error(g32[k], g64[k]) for k in g64}
