"""Yardsticks of the softsplat drop-in (plain module, numpy and torch only; restated from the semantics of
controlnet/softsplat.py:232-524, imported by tests/test_splat_grad_ref.py on the CPU and tests/test_gpu_softsplat.py on the GPU):

* `softsplat_f64`   the whole wrapper — every mode string, read literally — in differentiable fp64 torch.  The landing point is
                    formed in fp32 and then widened, as launch_ref._splat_accumulate forms it; autograd through it yields the
                    fp64 gradients w.r.t. in, flow and metric.
* `softsplat_f32`   the same arithmetic with every tensor held in fp32: the reference's arithmetic, not the code under test; it
                    measures what fp32 alone costs in the end-to-end gradient norm (`grad_norm_error`).
* `ingrad_f32`, `flowgrad_f32`   the two backward kernels in fp32 numpy, operation for operation: every product and sum rounded
                    on its own, sequential channel loop, corners in the order NW, NE, SW, SE, nothing contracted.
* `flowgrad_ref`    fp64 value and the S term of launch_ref's tolerance model for a flow gradient.
* `normalise_f32`   the fp32 normaliser of softsplat.py:253-270 on a splat_sum(cat[...]) result.
* `metric_family`   positive / signed metrics of the fused-mode tests."""
import math

import numpy as np
import torch

from oracle import launch_ref as L

F64 = torch.float64
EPS = L.EPS_SPLAT                                 # 0.0000001 (softsplat.py:257 / :260 / :266) as fp32 holds it


# ------------------------------------------------------------------------------------------ the wrapper, differentiable
def _splat_sum_torch(planes, flow, dtype):
    """Summation splat of planes [N, C, H, W] (dtype, may require grad) along flow [N, 2, H, W] (may require grad), differentiable
    in both.  The landing point takes the VALUE (x + fx) formed in fp32 (then widened) and the derivative 1 w.r.t. the flow."""
    n, c, h, w = planes.shape
    dev = planes.device
    gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=dev), torch.arange(w, dtype=torch.float32, device=dev),
                            indexing="ij")
    fl = flow.to(dtype)
    land = torch.stack([gx[None] + flow[:, 0].detach().to(torch.float32), gy[None] + flow[:, 1].detach().to(torch.float32)], 1)
    fin = torch.isfinite(land[:, 0]) & torch.isfinite(land[:, 1])
    safe = torch.where(fin[:, None], fl, torch.zeros_like(fl))                        # gradient 0 into a non-finite source
    land = torch.where(fin[:, None], land, torch.zeros_like(land)).to(dtype)
    pt = safe + (land - safe).detach()                                                # value: land, d/dflow: 1
    fx, fy = pt[:, 0], pt[:, 1]
    x0, y0 = torch.floor(fx).detach(), torch.floor(fy).detach()
    out = torch.zeros((n, c, h * w), dtype=dtype, device=dev)
    src = planes.reshape(n, c, h * w)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):                                   # NW, NE, SW, SE
        cx, cy = x0 + dx, y0 + dy
        wx = (x0 + 1 - fx) if dx == 0 else (fx - x0)
        wy = (y0 + 1 - fy) if dy == 0 else (fy - y0)
        ok = fin & (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h)
        wgt = torch.where(ok, wx * wy, torch.zeros_like(wx)).reshape(n, 1, h * w)
        idx = torch.where(ok, cy * w + cx, torch.zeros_like(cx)).long().reshape(n, 1, h * w)
        out = out.scatter_add(2, idx.expand(n, c, h * w), src * wgt)
    return out.reshape(n, c, h, w)


def _wrapper(tenIn, tenFlow, tenMetric, strMode, dtype):
    parts = strMode.split("-")
    base = parts[0]
    if base not in ("sum", "avg", "linear", "soft"):
        raise ValueError(strMode)
    if strMode in ("sum", "avg") and tenMetric is not None:
        raise ValueError("metric given")
    if base in ("linear", "soft") and tenMetric is None:
        raise ValueError("metric missing")
    x = tenIn.to(dtype)
    m = None if tenMetric is None else tenMetric.to(dtype)
    if strMode == "avg":                                                              # the exact test: 'avg-addeps' appends nothing
        x = torch.cat([x, torch.ones_like(x[:, :1])], 1)
    elif base == "linear":
        x = torch.cat([x * m, m], 1)
    elif base == "soft":
        x = torch.cat([x * m.exp(), m.exp()], 1)
    out = _splat_sum_torch(x, tenFlow, dtype)
    if base in ("avg", "linear", "soft"):
        den = out[:, -1:]
        eps = "addeps" if len(parts) == 1 else parts[1]
        if eps == "addeps":
            den = den + EPS
        elif eps == "zeroeps":
            den = torch.where(den == 0.0, torch.ones_like(den), den)
        elif eps == "clipeps":
            den = den.clip(EPS, None)
        out = out[:, :-1] / den
    return out


def softsplat_f64(tenIn, tenFlow, tenMetric, strMode):
    return _wrapper(tenIn, tenFlow, tenMetric, strMode, F64)


def softsplat_f32(tenIn, tenFlow, tenMetric, strMode):
    return _wrapper(tenIn, tenFlow, tenMetric, strMode, torch.float32)


def grads(fn, x, flow, metric, mode, G, dtype):
    """(d loss / d in, d flow, d metric) of loss = (fn(x, flow, metric, mode) * G).sum() with leaves of `dtype`"""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in (x, flow, metric)]
    out = fn(*leaves, mode)
    return torch.autograd.grad((out * G.to(out.dtype)).sum(), leaves)


def grad_norm_error(g, ref):
    """the per-tensor norm of the end-to-end test: max |g - ref| / max |ref| (no element excluded)"""
    g, ref = g.detach().cpu().to(F64), ref.detach().cpu().to(F64)
    if not bool(torch.isfinite(g).all()):
        return math.inf
    return float((g - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------------------------------ the backward kernels, fp32
def _corners_f32(flow, h, w):
    """fp32 corner factors of every source: ax, bx, ay, by [N, H, W], per corner (NW, NE, SW, SE) validity and target index"""
    f = np.ascontiguousarray(flow, dtype=np.float32)
    gy, gx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        fx = (gx[None] + f[:, 0]).astype(np.float32)
        fy = (gy[None] + f[:, 1]).astype(np.float32)
        # no corner of a landing point outside [-1, W) x [-1, H) lies inside the map (and its floor need not fit an int)
        near = np.isfinite(fx) & np.isfinite(fy) & (fx >= -1) & (fx < w) & (fy >= -1) & (fy < h)
        fx, fy = np.where(near, fx, np.float32(0)), np.where(near, fy, np.float32(0))
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, bx = (x0 + np.float32(1)) - fx, fx - x0
        ay, by = (y0 + np.float32(1)) - fy, fy - y0
    ok, idx = [], []
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        cx, cy = x0.astype(np.int64) + dx, y0.astype(np.int64) + dy
        o = near & (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h)
        ok.append(o)
        idx.append(np.where(o, cy * w + cx, 0))
    return tuple(a.astype(np.float32) for a in (ax, bx, ay, by)), ok, idx


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def ingrad_f32(flow, outgrad, bounds_test=True):
    """softsplat_ingrad in fp32 numpy -> torch [N, C, H, W].  bounds_test=False: the mutant that skips the out-of-bounds test
    (out-of-bounds corners read the clamped pixel)."""
    flow, og = _np(flow), np.ascontiguousarray(_np(outgrad), dtype=np.float32)
    n, c, h, w = og.shape
    (ax, bx, ay, by), ok, idx = _corners_f32(flow, h, w)
    wts = [(ax * ay).astype(np.float32), (bx * ay).astype(np.float32), (ax * by).astype(np.float32), (bx * by).astype(np.float32)]
    ogf = og.reshape(n, c, h * w)
    g = np.zeros((n, c, h, w), dtype=np.float32)
    for k in range(4):
        v = np.take_along_axis(ogf, np.broadcast_to(idx[k].reshape(n, 1, h * w), (n, c, h * w)), 2).reshape(n, c, h, w)
        term = (v * wts[k][:, None]).astype(np.float32)
        use = ok[k][:, None] if bounds_test else np.ones_like(ok[k][:, None])
        g = np.where(use, (g + term).astype(np.float32), g)
    return torch.from_numpy(g)


def flowgrad_f32(x, flow, outgrad, drop_last_channel=False, flip_corner=None, swap_weights=False):
    """softsplat_flowgrad in fp32 numpy, sequential channel loop -> torch [N, 2, H, W].  The keyword arguments are the mutants of
    the sharpness test: the last channel dropped, the sign of one corner's term flipped, the x-derivative weights used for y."""
    x, flow, og = np.ascontiguousarray(_np(x), dtype=np.float32), _np(flow), np.ascontiguousarray(_np(outgrad), dtype=np.float32)
    n, c, h, w = x.shape
    (ax, bx, ay, by), ok, idx = _corners_f32(flow, h, w)
    dwx = [-ay, ay, -by, by]
    dwy = [-ax, -bx, ax, bx]
    if swap_weights:
        dwy = dwx
    ogf = og.reshape(n, c, h * w)
    g = np.zeros((n, 2, h, w), dtype=np.float32)
    for ch in range(c - 1 if drop_last_channel else c):
        for k in range(4):
            v = np.take_along_axis(ogf[:, ch], idx[k].reshape(n, h * w), 1).reshape(n, h, w)
            t = (v * x[:, ch]).astype(np.float32)
            sgn = np.float32(-1 if flip_corner == k else 1)
            g[:, 0] = np.where(ok[k], (g[:, 0] + (t * dwx[k]).astype(np.float32) * sgn).astype(np.float32), g[:, 0])
            g[:, 1] = np.where(ok[k], (g[:, 1] + (t * dwy[k]).astype(np.float32) * sgn).astype(np.float32), g[:, 1])
    return torch.from_numpy(g)


# ------------------------------------------------------------------------------------------ fp64 references and bounds
def _corner_terms_f64(flow, h, w):
    """fp64 version of the corner factors (landing point formed in fp32, then widened): dwx, dwy, ok, idx as torch tensors"""
    dev = flow.device
    gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=dev), torch.arange(w, dtype=torch.float32, device=dev),
                            indexing="ij")
    fx = gx[None] + flow[:, 0].to(torch.float32)
    fy = gy[None] + flow[:, 1].to(torch.float32)
    fin = torch.isfinite(fx) & torch.isfinite(fy)
    fx = torch.where(fin, fx, torch.zeros_like(fx)).to(F64)
    fy = torch.where(fin, fy, torch.zeros_like(fy)).to(F64)
    x0, y0 = torch.floor(fx), torch.floor(fy)
    ax, bx, ay, by = x0 + 1 - fx, fx - x0, y0 + 1 - fy, fy - y0
    ok, idx = [], []
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        cx, cy = x0 + dx, y0 + dy
        o = fin & (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h)
        ok.append(o)
        idx.append(torch.where(o, cy * w + cx, torch.zeros_like(cx)).long())
    return [-ay, ay, -by, by], [-ax, -bx, ax, bx], [ax * ay, bx * ay, ax * by, bx * by], ok, idx


def flowgrad_ref(x, flow, outgrad):
    """fp64 flow gradient of the 'sum' splat and its S term -> (r, S) [N, 2, H, W]:
        S = A (2^-24 / U) sqrt(n),   A = sum |outgrad * in * dw|,   n = 12 C + 1
    (two products and one addition per term, four terms per channel, plus the rounding of dw)."""
    n, c, h, w = x.shape
    dwx, dwy, _, ok, idx = _corner_terms_f64(flow, h, w)
    xx = x.to(F64)
    ogf = outgrad.to(F64).reshape(n, c, h * w)
    r = torch.zeros((n, 2, h, w), dtype=F64, device=x.device)
    a = torch.zeros_like(r)
    for k in range(4):
        v = torch.gather(ogf, 2, idx[k].reshape(n, 1, h * w).expand(n, c, h * w)).reshape(n, c, h, w)
        t = torch.where(ok[k][:, None], v * xx, torch.zeros_like(xx))
        for comp, dw in ((0, dwx[k]), (1, dwy[k])):
            r[:, comp] += (t * dw[:, None]).sum(1)
            a[:, comp] += (t * dw[:, None]).abs().sum(1)
    return r, a * (2.0 ** -24 / L.U) * math.sqrt(12 * c + 1)


def ingrad_ref(flow, outgrad):
    """fp64 input gradient and S term -> (r, S): four terms of a product each (the weight carries the roundings of its two factors
    and of their product), n = 3 * 4 + 1, A = sum |outgrad * w|.  Used only to show that the ingrad yardstick is sharp."""
    n, c, h, w = outgrad.shape
    _, _, wts, ok, idx = _corner_terms_f64(flow, h, w)
    ogf = outgrad.to(F64).reshape(n, c, h * w)
    r = torch.zeros((n, c, h, w), dtype=F64, device=outgrad.device)
    a = torch.zeros_like(r)
    for k in range(4):
        v = torch.gather(ogf, 2, idx[k].reshape(n, 1, h * w).expand(n, c, h * w)).reshape(n, c, h, w)
        t = torch.where(ok[k][:, None], v * wts[k][:, None], torch.zeros_like(v))
        r += t
        a += t.abs()
    return r, a * (2.0 ** -24 / L.U) * math.sqrt(13)


# ------------------------------------------------------------------------------------------ fused forward modes
def normalise_f32(acc, eps):
    """fp32 normaliser (softsplat.py:253-270) of acc = splat_sum(cat[numerator planes, denominator plane]) [N, C + 1, H, W]"""
    num, den = acc[:, :-1].float(), acc[:, -1:].float().clone()
    if eps == "addeps":
        den = den + EPS
    elif eps == "zeroeps":
        den[den == 0.0] = 1.0
    else:
        assert eps == "clipeps", eps
        den = den.clip(EPS, None)
    return num / den


def quotient_ref(cat, flow, eps, extra=0):
    """fp64 value and S term of normalise(splat_sum(cat)) for cat = [numerator planes, denominator plane] (fp32 values) -> (r, S).
    The model of launch_ref.splat_soft_ref with the planes taken as given: per target with k sources, 3 k roundings in each sum
    (the weight, the product, the addition) and 4 around the quotient; the sums' errors stay below 2^-24 sqrt(.) of their sums of
    absolute terms and move the quotient, to first order, by
        2^-24 sqrt((3 + extra) k + 4) A,      A = (sum |num terms| + |r| sum |den terms|) / |normalised den|.
    extra: roundings per term inside the planes themselves when the value is compared with one formed from unrounded planes
    (1: the product in * metric of 'linear'; 2: exp and the product of 'soft')."""
    cc = cat.to(F64)
    c = cc.shape[1] - 1
    acc, k = L._splat_accumulate(torch.cat([cc, cc.abs()], 1), flow)
    num, den, anum, aden = acc[:, :c], acc[:, c:c + 1], acc[:, c + 1:2 * c + 1], acc[:, 2 * c + 1:]
    if eps == "addeps":
        dn = den + L.EPS_SPLAT
    elif eps == "zeroeps":
        dn = torch.where(den == 0.0, torch.ones_like(den), den)
    else:
        dn = den.clip(L.EPS_SPLAT, None)
    r = num / dn
    a = (anum + r.abs() * aden) / dn.abs()
    return r, a * (2.0 ** -24 / L.U) * torch.sqrt((3 + extra) * k + 4)


def cat_for(mode, x, metric):
    """the tensor the wrapper hands to the 'sum' primitive (softsplat.py:240-247), fp32 on the CPU"""
    x = x.float()
    if mode == "avg":
        return torch.cat([x, torch.ones_like(x[:, :1])], 1)
    if mode == "linear":
        return torch.cat([x * metric, metric], 1)
    assert mode == "soft", mode
    return torch.cat([x * metric.exp(), metric.exp()], 1)


def metric_family(family, n, h, w, seed):
    """fp32 metric [n, 1, h, w]:
      positive  0.25 + |N(0, 1)|;
      signed    multiples of 0.25 in [-2, 2] (with the exactly representable weights of the `border` flow family the denominator
                reaches exactly 0 and negative values), and exact +-m pairs on neighbouring pixels."""
    gen = torch.Generator().manual_seed(21000 + seed)
    if family == "positive":
        return torch.randn(n, 1, h, w, generator=gen).abs() + 0.25
    assert family == "signed", family
    m = torch.randint(-8, 9, (n, 1, h, w), generator=gen).float() * 0.25
    flat = m.reshape(-1)
    flat[1::2] = -flat[0::2][: flat[1::2].numel()]
    return m


# ------------------------------------------------------------------------------------------ end-to-end gradients
E2E_SHAPES = [(3, 7, 7, 9), (2, 5, 24, 40)]
E2E_FAMILIES = ("smooth", "border", "nonfinite")
E2E_MODES = ("soft", "linear")
E2E_CASES = [(m, s, f) for m in E2E_MODES for s in E2E_SHAPES for f in E2E_FAMILIES]
E2E_FACTOR = 4.0                                  # over the fp32 arithmetic's own error: accumulation order and device exp


def e2e_label(case):
    return f"{case[0]}-" + "x".join(map(str, case[1])) + f"-{case[2]}"


def e2e_inputs(case):
    """(x, flow, metric, G) of an end-to-end case: the edge_cases inputs of (shape, family, 'normal') and a fixed seeded G"""
    import edge_cases as E
    _, shape, family = case
    key = tuple(shape) + (family, "normal")
    i = E.SPLAT_CASES.index(key)
    x, flow, metric, _ = E.splat_inputs(key, E.splat_seed(i))
    G = torch.randn(x.shape, generator=torch.Generator().manual_seed(23000 + i))
    return x, flow, metric, G


def e2e_fp64(case):
    """fp64 autograd gradients (in, flow, metric) of loss = (softsplat_f64(x, flow, metric, mode) * G).sum()"""
    x, flow, metric, G = e2e_inputs(case)
    return grads(softsplat_f64, x, flow, metric, case[0], G, F64)


def e2e_fp32_error(case):
    """max |g32 - g64| / max |g64| per tensor for softsplat_f64's arithmetic run in fp32 on the CPU: what the number format alone
    costs (the reference's arithmetic, not the code under test)"""
    x, flow, metric, G = e2e_inputs(case)
    g32 = grads(softsplat_f32, x, flow, metric, case[0], G, torch.float32)
    return tuple(grad_norm_error(a, b) for a, b in zip(g32, e2e_fp64(case)))
