"""fp64 restatement of PSNR and of pytorch_msssim 1.0's ssim / ms_ssim (the rules in diffcodec_amd/metrics.py's docstring), on the
CPU with torch conv2d in fp64.  The device kernels of csrc/metrics.hip are checked against this (tests/test_gpu_metrics.py); this
file is pinned to an independent scipy evaluation and to avg_pool2d in tests/test_metrics_ref.py.

`ssim_bound` is the bar of the edge tests: a worst-case first-order bound of the kernel's fp32 arithmetic, per (n, c) plane, from
the reference's own fp64 intermediates (no fitted factor).  `expected` / `check_out` hold a launch's whole output vector
[N*C + N + 1] (per plane, per sample, overall) to it; tests/test_metrics_ref.py shows on the CPU that an fp32 restatement passes
and that structural faults fail."""
import math

import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window(ws=11, sigma=1.5):
    c = torch.arange(ws, dtype=torch.float64) - ws // 2
    g = torch.exp(-(c ** 2) / (2.0 * sigma * sigma))
    return g / g.sum()


def as_nchw64(t):
    """uint8 NHWC frames or float NCHW images -> fp64 NCHW on the CPU (dense NCHW either way: a permuted view would let torch sum
    in the order of its strides, and the last bit would depend on where the frames came from)."""
    t = t.detach().cpu()
    return t.permute(0, 3, 1, 2).double().contiguous() if t.dtype == torch.uint8 else t.double()


def gaussian_filter(x, g):
    """valid correlation with g along H, then along W, per channel"""
    c, ws = x.shape[1], g.numel()
    x = F.conv2d(x, g.view(1, 1, ws, 1).repeat(c, 1, 1, 1), groups=c)
    return F.conv2d(x, g.view(1, 1, 1, ws).repeat(c, 1, 1, 1), groups=c)


def ssim_cs(X, Y, data_range, g, K=(0.01, 0.03)):
    """per-(n, c) spatial means of ssim_map and cs_map, [N, C] each"""
    c1, c2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mx, my = gaussian_filter(X, g), gaussian_filter(Y, g)
    sxx = gaussian_filter(X * X, g) - mx * mx
    syy = gaussian_filter(Y * Y, g) - my * my
    sxy = gaussian_filter(X * Y, g) - mx * my
    cs_map = (2 * sxy + c2) / (sxx + syy + c2)
    ssim_map = (2 * mx * my + c1) / (mx * mx + my * my + c1) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def pool(x):
    """avg_pool2d(kernel 2, padding (H % 2, W % 2), count_include_pad) written out: an odd axis gains one zero row / column on both
    sides (the last one is dropped by the floor), every 2x2 window is divided by 4."""
    ph, pw = x.shape[-2] % 2, x.shape[-1] % 2
    x = F.pad(x, (pw, pw, ph, ph))
    h, w = x.shape[-2] // 2 * 2, x.shape[-1] // 2 * 2
    x = x[..., :h, :w]
    return (x[..., 0::2, 0::2] + x[..., 0::2, 1::2] + x[..., 1::2, 0::2] + x[..., 1::2, 1::2]) / 4


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, weights=WEIGHTS, K=(0.01, 0.03), per_channel=False):
    X, Y = as_nchw64(X), as_nchw64(Y)
    g = window(win_size, win_sigma)
    w = torch.tensor(weights, dtype=torch.float64)
    vals = []
    for i in range(len(weights)):
        s, cs = ssim_cs(X, Y, data_range, g, K)
        if i < len(weights) - 1:
            vals.append(torch.relu(cs))
            X, Y = pool(X), pool(Y)
    vals.append(torch.relu(s))
    v = torch.prod(torch.stack(vals, 0) ** w.view(-1, 1, 1), 0)          # [N, C]
    if per_channel:
        return v
    return v.mean() if size_average else v.mean(1)


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, K=(0.01, 0.03), nonnegative_ssim=False,
         per_channel=False):
    X, Y = as_nchw64(X), as_nchw64(Y)
    s, _ = ssim_cs(X, Y, data_range, window(win_size, win_sigma), K)
    if nonnegative_ssim:
        s = torch.relu(s)
    if per_channel:
        return s
    return s.mean() if size_average else s.mean(1)


def psnr(X, Y, data_range=255.0):
    """[N] fp64: 10 log10(L^2 / mse) per image, +inf when mse == 0"""
    X, Y = as_nchw64(X), as_nchw64(Y)
    mse = ((X - Y) ** 2).flatten(1).mean(1)
    return torch.tensor([math.inf if m == 0 else 10 * math.log10(data_range ** 2 / m) for m in mse.tolist()], dtype=torch.float64)


# ------------------------------------------------------------------------------------------ the bound of the edge tests
U32 = 2.0 ** -24                   # fp32 unit roundoff


def ssim_bound(X, Y, data_range, g, K=(0.01, 0.03)):
    """-> (d_ssim, d_cs) [N, C]: worst-case first-order error of the per-plane means of ssim_map and cs_map as csrc/metrics.hip
    computes them (fp32, values shifted by L/2 on load, separable window of ws taps in fma chains, sigma = E[x'^2] - mean'^2).

    u = 2^-24; kappa = (2 ws + 2) u: a product, ws fma steps of the first pass and ws of the second, one subtraction.  Primes:
    shifted values x' = x - L/2.  G* = the window applied to a map.  Per output pixel
        d_xx  = kappa (G*x'^2 + 2 (G*|x'|)^2)             second moment, and the square of the mean it is subtracted from
        d_xy  = kappa (G*|x'y'| + 2 (G*|x'|)(G*|y'|))
        d_cs  = (2 d_xy + |cs| (d_xx + d_yy)) / (s_xx + s_yy + C2) + 4 u |cs|        numerator, denominator, 4 roundings
        d_mu  = kappa G*|x'| + u |mu|                      the mean, and the shift added back
        d_lum = (2 (|mu_y| d_mux + |mu_x| d_muy) + 2 |lum| (|mu_x| d_mux + |mu_y| d_muy)) / D + 6 u |lum|,  D = mu_x^2 + mu_y^2 + C1
        d_ssim = |lum| d_cs + |cs| d_lum + u |lum cs|
    and the plane bound is the mean over the pixels (the sums and the division run in fp64)."""
    ws = g.numel()
    kappa = (2 * ws + 2) * U32
    c1, c2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    xs, ys = X - data_range / 2, Y - data_range / 2
    mx, my = gaussian_filter(X, g), gaussian_filter(Y, g)
    sxx = gaussian_filter(X * X, g) - mx * mx
    syy = gaussian_filter(Y * Y, g) - my * my
    sxy = gaussian_filter(X * Y, g) - mx * my
    cs = (2 * sxy + c2) / (sxx + syy + c2)
    den = mx * mx + my * my + c1
    lum = (2 * mx * my + c1) / den
    ax, ay = gaussian_filter(xs.abs(), g), gaussian_filter(ys.abs(), g)
    d_xx = kappa * (gaussian_filter(xs * xs, g) + 2 * ax * ax)
    d_yy = kappa * (gaussian_filter(ys * ys, g) + 2 * ay * ay)
    d_xy = kappa * (gaussian_filter((xs * ys).abs(), g) + 2 * ax * ay)
    d_cs = (2 * d_xy + cs.abs() * (d_xx + d_yy)) / (sxx + syy + c2) + 4 * U32 * cs.abs()
    d_mx, d_my = kappa * ax + U32 * mx.abs(), kappa * ay + U32 * my.abs()
    d_lum = (2 * (my.abs() * d_mx + mx.abs() * d_my) + 2 * lum.abs() * (mx.abs() * d_mx + my.abs() * d_my)) / den + 6 * U32 * lum.abs()
    d_ssim = lum.abs() * d_cs + cs.abs() * d_lum + U32 * (lum * cs).abs()
    return d_ssim.flatten(2).mean(-1), d_cs.flatten(2).mean(-1)


def scale_means(X, Y, data_range, g, K, levels):
    """per scale s of `levels` (fp64 pooling between them): (ssim, cs, d_ssim, d_cs), [N, C] each"""
    out = []
    for s in range(levels):
        if s:
            X, Y = pool(X), pool(Y)
        out.append(ssim_cs(X, Y, data_range, g, K) + ssim_bound(X, Y, data_range, g, K))
    return out


def expected(X, Y, data_range, g, K, weights=None, nonnegative=False, exact=None):
    """What a launch of dc_ssim (weights None) / dc_ms_ssim must write for fp64 NCHW operands X, Y, window taps g (fp64 tensor), K
    and weights as the launch reads them: dict(v = values [N, C], d = their bounds [N, C], base, delta [S, N, C] = the unclamped
    per-scale means entering the product and their bounds, exact = the value every output element must equal bit for bit, or None).
    MS-SSIM: v = prod_s relu(base_s)^w_s, d = v sum_s w_s delta_s / relu(base_s)."""
    levels = 1 if weights is None else len(weights)
    sc = scale_means(X, Y, data_range, g, K, levels)
    base = torch.stack([sc[s][1] if s < levels - 1 else sc[s][0] for s in range(levels)])
    delta = torch.stack([sc[s][3] if s < levels - 1 else sc[s][2] for s in range(levels)])
    if weights is None:
        v = torch.relu(base[0]) if nonnegative else base[0]
        d = delta[0]
    else:
        w = torch.tensor([float(x) for x in weights], dtype=torch.float64).view(-1, 1, 1)
        b = torch.relu(base)
        v = torch.prod(b ** w, 0)
        d = v * (w * delta / b).sum(0)
    return dict(v=v, d=d, base=base, delta=delta, exact=exact)


def case_expected(c, X, Y, g):
    """`expected` of a tests/edge_cases.py MetricCase on its logical NCHW inputs and fp32 taps: the fp64 reference on the operands
    as the launch reads them (the ABI takes the taps, K and the weights as fp32)."""
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    w = None if c.weights is None else [f32(v) for v in c.weights]
    return expected(X.double(), Y.double(), c.L, g.double(), (f32(c.K[0]), f32(c.K[1])), w, c.nonneg, c.exact)


def check_out(out, exp):
    """out: fp64 [N*C + N + 1] of a launch (any device).  -> dict(ok, ratio = worst err / bound over the three segments, what).
    Planes are held to their bounds, the per-sample and overall means to the mean of the plane bounds plus 2^-50 relative (their
    own fp64 sums); where the reference is NaN (a NaN pixel) the output must be NaN — the plane, its sample's mean and the overall
    mean — and the other planes and samples are held as usual; exp['exact'] demands that value in every element."""
    out = out.detach().cpu().double()
    v, d = exp["v"], exp["d"]
    n, c = v.shape
    assert out.numel() == n * c + n + 1
    if exp["exact"] is not None:
        ok = bool((out == exp["exact"]).all())
        return dict(ok=ok, ratio=0.0 if ok else math.inf, what=f"every element must equal {exp['exact']}: {out.tolist()[:8]}")
    got = [out[:n * c].reshape(n, c), out[n * c:n * c + n], out[n * c + n].reshape(1)]
    want = [v, v.mean(1), v.mean().reshape(1)]
    bound = [d, d.mean(1), d.mean().reshape(1)]
    worst, what, ok = 0.0, "", True
    for name, y, r, b in zip(("plane", "sample", "overall"), got, want, bound):
        nan = torch.isnan(r)
        if not bool(torch.isnan(y[nan]).all()) or bool(torch.isnan(y[~nan]).any()):
            return dict(ok=False, ratio=math.inf, what=f"{name}: NaN pattern {torch.isnan(y).tolist()} != {nan.tolist()}")
        if name != "plane":
            b = b + 2.0 ** -50 * r.abs()
        err, b = (y - r).abs()[~nan], b[~nan]
        if err.numel() == 0:
            continue
        ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
        i = int(torch.argmax(ratio))
        if float(ratio[i]) >= worst:
            worst, what = float(ratio[i]), f"{name} {i}: err {float(err[i]):.3e} bound {float(b[i]):.3e}"
        ok = ok and float(ratio[i]) <= 1.0
    return dict(ok=ok, ratio=worst, what=what)
