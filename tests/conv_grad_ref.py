"""fp64 restatements of the three gradients of the fp32 extractor convolution (csrc/conv_f32_grad.hip), their error bounds, and the
case table shared by tests/test_conv_grad_ref.py (CPU) and tests/test_gpu_conv_grad.py (GPU).  Plain module: imports nothing from
the package or the oracle.

With z = conv3x3(x, w, padding 1, stride s) + b and y = silu ? SiLU(z) : z, each gradient is restated on its own, from the exact
fp32 operands its launch read (dgrad and wgrad are given the device's own gz):

    silu_grad_ref(z, gy)             gz = gy silu'(z),  silu'(z) = s + z s (1 - s),  s = sigmoid(z)
    dgrad_ref(gz, w, h, w_, stride)  dx[n][ci][iy][ix] = sum gz[n][co][oy][ox] w[co][ci][ky][kx] over oy s + ky - 1 = iy, ox s + kx - 1 = ix
    wgrad_ref(x, gz, stride)         dw[co][ci][ky][kx] = sum gz[n][co][oy][ox] x[n][ci][oy s + ky - 1][ox s + kx - 1], db[co] = sum gz

written as nine strided slices of a padded plane (no convolution call, no autograd: tests/test_conv_grad_ref.py holds them to
fp64 autograd of F.conv2d).

Bounds, derived and not fitted.  The convolution gradients follow the model the forward's reference uses (an fp32 chain of K terms
whose roundings are independent): per element

    |y - r| <= 2^-20 |r| + 4 * 2^-24 * sqrt(K) * A,      A = the sum of the terms' magnitudes,

K = the number of (co, tap) terms that reach the element for dgrad (at most 9 Cout; fewer at the border and, with a stride, in
most phases; 0 for a pixel nothing reads, which must then be exactly 0) and K = N Ho Wo for dw and db.  The SiLU gradient is
|gz - r| <= 1.33 * 2^-20 |gy| + 2^-24 |r|: silu' is a sum of two terms, s and z s (1 - s), of total magnitude at most 1.33 (|silu'|
<= 1.1 and |z s (1 - s)| <= 0.23), each evaluated to the forward's accepted relative 2^-20, and the product with gy rounds once.
Systematic error: the relative RMS error of every output is at most 2^-7, as everywhere in the suite."""
import math

import torch

F64 = torch.float64
RMS_MAX = 2.0 ** -7

# (N, Cin, H, W, Cout, stride); every case runs with SiLU on and off and with and without a bias
GENERIC_CASES = [
    (2, 1, 1, 1, 1, 1),
    (3, 3, 7, 9, 5, 1),
    (2, 5, 8, 11, 1, 2),
    (3, 2, 9, 6, 7, 2),
    (2, 3, 13, 10, 4, 4),
    (2, 1, 5, 5, 3, 4),
    (3, 16, 4, 130, 8, 1),
]
MFMA_CASES = [
    (2, 32, 8, 16, 32, 1),
    (3, 40, 12, 36, 96, 1),       # ragged pixel tiles in x, ragged channel tiles (40 of 64, 96 = 64 + 32), a short last K step
    (2, 64, 16, 16, 64, 2),
    (3, 32, 10, 34, 160, 2),
    (2, 160, 8, 8, 320, 1),
    (2, 640, 8, 8, 64, 1),
    (3, 32, 48, 48, 32, 1),       # several K parts with a short last one in wgrad
    (3, 64, 6, 10, 32, 2),        # completes the table: dgrad stride 2 with 64-channel tiles at batch 3
    (2, 32, 12, 8, 32, 2),        # ... and with 32-channel tiles at batch 2
    (2, 40, 6, 20, 40, 1),        # stride 1 with pixel tiles ragged in x and y (8 x 16 tiles on 6 x 20)
]
CASES = GENERIC_CASES + MFMA_CASES
SLICE_CASE = (3, 40, 12, 36, 96, 1)          # run once more with x a channel-slice view of a wider tensor
NONCONTIGUOUS_GY_CASE = (2, 64, 16, 16, 64, 2)

# the convolutions of a 512 x 512 frame with Cin >= 32 and Cout >= 32: (Cin, H, W, Cout, stride)
PRODUCTION_LAYERS = [
    (32, 256, 256, 32, 1), (32, 256, 256, 64, 2), (64, 128, 128, 64, 1), (64, 128, 128, 160, 2), (160, 64, 64, 160, 2),
    (160, 32, 32, 320, 2), (320, 16, 16, 640, 2),
    (160, 64, 64, 64, 1), (320, 32, 32, 64, 1), (640, 16, 16, 64, 1),
    (160, 64, 64, 320, 1), (160, 32, 32, 320, 1), (320, 16, 16, 640, 1), (640, 8, 8, 1280, 1),
]


def out_size(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def case_inputs(case, seed, silu=True, bias=True):
    """-> dict(x, w, b | None, gy) fp32 CPU tensors: values of order one, the weights scaled so that z is of order one too (both
    branches of the SiLU are exercised)."""
    n, cin, h, w, cout, s = case
    g = torch.Generator().manual_seed(1000 + seed)
    ho, wo = out_size(h, w, s)
    x = torch.randn((n, cin, h, w), generator=g)
    wt = torch.randn((cout, cin, 3, 3), generator=g) * (1.5 / math.sqrt(9 * cin))
    b = torch.randn((cout,), generator=g) * 0.5 if bias else None
    gy = torch.randn((n, cout, ho, wo), generator=g)
    return dict(x=x, w=wt, b=b, gy=gy)


# ------------------------------------------------------------------------------------------ bounds
def chain_tol(r, a, k):
    """2^-20 |r| + 4 * 2^-24 * sqrt(K) * A; k: a number or a tensor of r's shape"""
    k = torch.as_tensor(k, dtype=F64)
    return 2.0 ** -20 * r.abs() + 4 * 2.0 ** -24 * torch.sqrt(k) * a


def check(y, r, tol):
    """y: the values under test (any float dtype), r / tol: fp64 reference and bound of the same shape.
    -> dict(ratio = worst err / tol, rms = relative RMS error, worst = flat index, err, tol, ok)"""
    y = y.detach().to("cpu", F64)
    assert y.shape == r.shape, (y.shape, r.shape)
    err = (y - r).abs()
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    finite = torch.isfinite(y)
    ratio = torch.where(finite, ratio, torch.full_like(err, math.inf))
    i = int(torch.argmax(ratio.reshape(-1)))
    den = float((r * r).sum())
    num = float((err * err).sum()) if bool(finite.all()) else math.inf
    rms = math.sqrt(num / den) if den > 0 else (0.0 if num == 0 else math.inf)
    worst = float(ratio.reshape(-1)[i])
    return dict(ratio=worst, rms=rms, worst=i, err=float(err.reshape(-1)[i]), tol=float(tol.reshape(-1)[i]),
                ok=worst <= 1.0 and rms <= RMS_MAX)


# ------------------------------------------------------------------------------------------ restatements
def conv_ref(x, w, b, stride, silu):
    """the forward in fp64 -> (z, y): what the gradients below differentiate"""
    x, w = x.detach().to("cpu", F64), w.detach().to("cpu", F64)
    n, cin, h, wd = x.shape
    ho, wo = out_size(h, wd, stride)
    xp = torch.zeros((n, cin, h + 2, wd + 2), dtype=F64)
    xp[:, :, 1:h + 1, 1:wd + 1] = x
    z = torch.zeros((n, w.shape[0], ho, wo), dtype=F64)
    for ky in range(3):
        for kx in range(3):
            xs = xp[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
            z += torch.einsum("nchw,oc->nohw", xs, w[:, :, ky, kx])
    if b is not None:
        z = z + b.detach().to("cpu", F64).reshape(1, -1, 1, 1)
    return z, (z * torch.sigmoid(z) if silu else z)


def silu_prime(z):
    s = torch.sigmoid(z)
    return s + z * s * (1 - s)


def silu_grad_ref(z, gy):
    """-> (r, tol) from the fp32 z and gy the launch read"""
    z, gy = z.detach().to("cpu", F64), gy.detach().to("cpu", F64)
    r = gy * silu_prime(z)
    return r, 1.33 * 2.0 ** -20 * gy.abs() + 2.0 ** -24 * r.abs()


def dgrad_ref(gz, w, h, wd, stride, taps=None, channels=None, drop_odd_rows=False):
    """-> (r, tol) [N, Cin, H, W].  taps / channels / drop_odd_rows restrict the sum (for the planted faults of the CPU tests):
    the (ky, kx) pairs that contribute, the number of leading output channels, and whether dx rows of odd phase get nothing."""
    gz, w = gz.detach().to("cpu", F64), w.detach().to("cpu", F64)
    n, cout, ho, wo = gz.shape
    assert (ho, wo) == out_size(h, wd, stride)
    if channels is not None:
        gz, w = gz[:, :channels], w[:channels]
    cin = w.shape[1]
    r = torch.zeros((n, cin, h + 2, wd + 2), dtype=F64)          # padded coordinates: row iy + 1 = oy s + ky
    a = torch.zeros_like(r)
    k = torch.zeros((1, 1, h + 2, wd + 2), dtype=F64)
    for ky in range(3):
        for kx in range(3):
            if taps is not None and (ky, kx) not in taps:
                continue
            sl = (slice(None), slice(None), slice(ky, ky + stride * (ho - 1) + 1, stride), slice(kx, kx + stride * (wo - 1) + 1, stride))
            r[sl] += torch.einsum("nohw,oc->nchw", gz, w[:, :, ky, kx])
            a[sl] += torch.einsum("nohw,oc->nchw", gz.abs(), w[:, :, ky, kx].abs())
            k[sl] += gz.shape[1]
    r, a, k = (t[:, :, 1:h + 1, 1:wd + 1] for t in (r, a, k))
    if drop_odd_rows:
        r = r.clone()
        r[:, :, 1::2] = 0
    return r, chain_tol(r, a, k.expand_as(r))


def wgrad_ref(x, gz, stride, taps=None, rows=None, images=None):
    """-> ((dw, tol), (db, tol)).  taps / rows / images restrict the sums (planted faults): the contributing (ky, kx) pairs, the
    number of leading output rows in dw, the number of leading images in db."""
    x, gz = x.detach().to("cpu", F64), gz.detach().to("cpu", F64)
    n, cin, h, wd = x.shape
    _, cout, ho, wo = gz.shape
    assert (ho, wo) == out_size(h, wd, stride)
    xp = torch.zeros((n, cin, h + 2, wd + 2), dtype=F64)
    xp[:, :, 1:h + 1, 1:wd + 1] = x
    gw = gz if rows is None else gz[:, :, :rows]
    hr = gw.shape[2]
    dw = torch.zeros((cout, cin, 3, 3), dtype=F64)
    aw = torch.zeros_like(dw)
    for ky in range(3):
        for kx in range(3):
            if taps is not None and (ky, kx) not in taps:
                continue
            xs = xp[:, :, ky:ky + stride * (hr - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
            dw[:, :, ky, kx] = torch.einsum("nohw,nchw->oc", gw, xs)
            aw[:, :, ky, kx] = torch.einsum("nohw,nchw->oc", gw.abs(), xs.abs())
    gb = gz if images is None else gz[:images]
    db, ab = gb.sum((0, 2, 3)), gb.abs().sum((0, 2, 3))
    k = n * ho * wo
    return (dw, chain_tol(dw, aw, k)), (db, chain_tol(db, ab, k))


# ------------------------------------------------------------------------------------------ a chain of convolutions
def chain_ref(x, params, strides, silus, c):
    """Gradients of the linear functional L = <c, y_last> of a chain of convolutions y_l = conv(y_(l-1); w_l, b_l, stride_l, silu_l)
    w.r.t. the input and every parameter, with the chain's propagated first-order bound.  x: fp32 input; params: [(w, b)] fp32;
    c: fp32 of the last output's shape.  -> (dx, [(dw, db)]), (tol_dx, [(tol_dw, tol_db)]) in fp64.

    The bound.  A device chain differs from this one in two ways, and to first order the two add.  (1) Every launch rounds: the
    forward of layer l within f_l = 2^-20 |z| + 4 * 2^-24 sqrt(9 Cin) A (the forward reference's chain bound) and 2^-20 |y| for
    the SiLU, the backward launches within the bounds above.  (2) Every launch reads operands that carry the errors of the
    launches before it.  The model behind every bound here is that roundings are independent, so the errors that reach a launch
    from different elements and different launches add in quadrature: they are carried as squares through the chain's own linear
    maps with every coefficient squared (S' = silu'(z_l), |silu''| <= 0.5, g_l = the gradient at y_l):
        forward   p_l = conv(e_(l-1); w_l^2) + f_l^2,          e_l = S'^2 p_l + (2^-20 y_l)^2
        backward  d_l = S'^2 q_l + (0.5 g_l)^2 p_l + t_l^2,    q_(l-1) = dgrad(d_l; w_l^2) + (the dgrad bound)^2,   t_l: the SiLU-gradient bound
        tol_dw_l = the wgrad bound + sqrt(wgrad(x_l^2, d_l) + wgrad(e_(l-1), gz_l^2)),  tol_db_l alike,  tol_dx = sqrt(q_0)."""
    xs = [x.detach().to("cpu", F64)]
    zs = []
    for (w, b), s, act in zip(params, strides, silus):
        z, y = conv_ref(xs[-1], w, b, s, act)
        zs.append(z)
        xs.append(y)
    es = [torch.zeros_like(xs[0])]                               # squared forward error of y_l
    ps = []                                                      # squared error of z_l
    for l, ((w, b), s, act) in enumerate(zip(params, strides, silus)):
        w64 = w.detach().to("cpu", F64)
        za, _ = conv_ref(xs[l].abs(), w64.abs(), None if b is None else b.detach().abs(), s, False)
        pz, _ = conv_ref(es[l], w64 ** 2, None, s, False)
        p = pz + chain_tol(zs[l], za, 9 * w64.shape[1]) ** 2
        ps.append(p)
        es.append(silu_prime(zs[l]) ** 2 * p + (2.0 ** -20 * xs[l + 1]) ** 2 if act else p)
    g = c.detach().to("cpu", F64)
    q = torch.zeros_like(g)                                      # squared error of g
    grads, tols = [], []
    for l in reversed(range(len(params))):
        (w, b), s, act = params[l], strides[l], silus[l]
        w64 = w.detach().to("cpu", F64)
        h, wd = xs[l].shape[2:]
        if act:
            gz, tz = silu_grad_ref(zs[l], g)
            d = silu_prime(zs[l]) ** 2 * q + (0.5 * g) ** 2 * ps[l] + tz ** 2
        else:
            gz, d = g, q
        (dw, tw), (db, tb) = wgrad_ref(xs[l], gz, s)
        (ew1, _), (eb1, _) = wgrad_ref(xs[l] ** 2, d, s)
        (ew2, _), _ = wgrad_ref(es[l], gz ** 2, s)
        grads.append((dw, db if b is not None else None))
        tols.append((tw + torch.sqrt(ew1 + ew2), tb + torch.sqrt(eb1)))
        gx, tx = dgrad_ref(gz, w64, h, wd, s)
        ex, _ = dgrad_ref(d, w64 ** 2, h, wd, s)
        g, q = gx, tx ** 2 + ex
    return (g, grads[::-1]), (torch.sqrt(q), tols[::-1])
