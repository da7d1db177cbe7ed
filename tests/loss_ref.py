"""fp64 restatement of the two training losses (diffcodec_amd.losses) and of their backward, on the CPU with torch.nn.functional.
Nothing here comes from the package: the kernels of csrc/lpips_grad.hip and csrc/edge_loss.hip are checked against this
(tests/test_gpu_losses.py), and this file against autograd of the whole function and hand-computed values (tests/test_loss_ref.py).

`lpips_loss` is differentiable by autograd.  `backward_from_maps` is the backward LINEARISED AT GIVEN post-ReLU maps: autograd of
the distance tail on the maps as leaves, the mask map > 0, torch.nn.grad.conv2d_input, autograd of max_pool2d on the given lower
map, and 1 / scale.  The device is held to it fed the device's own maps: one ReLU or argmax decision that differs between an fp32
and an fp64 forward moves a pixel's gradient by percents, which is no arithmetic error.  Fed the fp64 maps it equals fp64 autograd
of the whole loss.

The stage references return (r, S) for oracle.launch_ref.check(y, r, S, torch.float32): S = 2^-24 sqrt(K) A / U, K the length of the
longest chain that feeds an element and A the sum of the absolute values of its terms (launch_ref.conv3x3_nchw_f32_ref's form)."""
import math

import torch
import torch.nn.functional as F

from lpips_ref import CHANNELS, PAD, SCALE, SHIFT, STRIDE, _params, synth_weights, tail, unit_normalize  # noqa: F401

F64 = torch.float64
U = 2.0 ** -8                                    # launch_ref.U
SHAPES = ((2, 31, 31), (3, 67, 95), (2, 70, 146))
FAULTS = ("no_relu", "last_argmax", "unmirrored", "drop_lin", "no_scale", "no_normaliser_term")


# ------------------------------------------------------------------------------------------------ bars
SEED = 100                                         # case i of SHAPES uses loss_inputs(..., SEED + i)

# max |d| / max |ref| of the fp32 CPU run per case (the larger of both sides; tests/test_loss_ref.py recomputes it), and the GPU
# bar = 4 x that.
#   case       fp32 CPU    bar       measured on the MI355X (tests/test_gpu_losses.py: dx, dy)
#   2x31x31    4.8e-7      1.9e-6    4.7e-7, 7.9e-7
#   3x67x95    5.7e-7      2.3e-6    9.4e-7, 1.13e-6
#   2x70x146   5.8e-7      2.3e-6    9.2e-7, 9.0e-7
CPU_FP32 = {(2, 31, 31): 4.8e-7, (3, 67, 95): 5.7e-7, (2, 70, 146): 5.8e-7}
BARS = {k: 4 * v for k, v in CPU_FP32.items()}
SOBEL_SHAPES = ((1, 1, 1, 1), (2, 3, 1, 70), (2, 3, 70, 1), (3, 3, 17, 70), (2, 2, 17, 65))     # the last: one pixel past the 16 x 64 tile
# Sobel gradient ('mean') of the fp32 CPU run against plain fp64 autograd, max |d| / max |ref|; the 1x1 image has a zero gradient
SOBEL_CPU_FP32 = {(2, 3, 1, 70): 1.6e-7, (2, 3, 70, 1): 1.6e-7, (3, 3, 17, 70): 1.1e-6, (2, 2, 17, 65): 9.6e-7}
SOBEL_BARS = {k: 4 * v for k, v in SOBEL_CPU_FP32.items()}
SOBEL_SEED = 7


# ------------------------------------------------------------------------------------------------ inputs
def loss_inputs(n, h, w, seed):
    """(x, y, g) fp32: images uniform in [-1, 1] with a flat 25 x 25 patch at (4, 4) per image and channel (conv1 then gives equal
    values at 3 x 3 neighbouring positions: positive ties inside pool windows, which is where the first-maximum rule shows), and
    the upstream gradient g [n] of the values, of both signs."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, h, w, generator=gen) * 2 - 1
    y = torch.rand(n, 3, h, w, generator=gen) * 2 - 1
    x[:, :, 4:29, 4:29] = (torch.rand(n, 3, 1, 1, generator=gen) * 2 - 1)
    y[:, :, 4:29, 4:29] = (torch.rand(n, 3, 1, 1, generator=gen) * 2 - 1)
    g = torch.rand(n, generator=gen) + 0.5
    g[1::2] *= -1
    return x, y, g


def sobel_inputs(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=gen) * 2 - 1, torch.rand(*shape, generator=gen) * 2 - 1


# ------------------------------------------------------------------------------------------------ LPIPS
def params(sd, dtype=F64, lpips=True):
    convs, lins = _params(sd)
    convs = [(w.to(dtype), b.to(dtype)) for w, b in convs]
    lins = [(v if lpips else torch.ones_like(v)).to(dtype) for v in lins]
    return convs, lins


def features(sd, x, normalize=False, dtype=F64):
    """relu1 .. relu5 of float NCHW images, differentiable (lpips_ref.features without its detach)"""
    convs, _ = params(sd, dtype)
    x = x.to(dtype)
    if normalize:
        x = 2 * x - 1
    x = (x - torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    out = []
    for l, (w, b) in enumerate(convs):
        if l in (1, 2):
            x = F.max_pool2d(x, 3, 2)
        x = torch.relu(F.conv2d(x, w, b, stride=STRIDE[l], padding=PAD[l]))
        out.append(x)
    return out


def lpips_loss(sd, x, y, normalize=False, lpips=True, dtype=F64):
    """(value [N], per-layer [5][N], maps of x, maps of y) of NormFixLPIPS; differentiable by autograd"""
    _, lins = params(sd, dtype, lpips)
    fx, fy = features(sd, x, normalize, dtype), features(sd, y, normalize, dtype)
    layers = [tail(a, b, w, True) for a, b, w in zip(fx, fy, lins)]
    return sum(layers), layers, fx, fy


def tail_grad(fx, fy, lin, g, fault=None):
    """d/d fx of sum_n g_n tail(fx, fy)_n, written out: t_c = 2 g w_c d_c / HW, (t_c - u_c sum_k u_k t_k) / n"""
    n = torch.sqrt((fx * fx + 1e-8).sum(1, keepdim=True))
    u = fx / n
    d = u - unit_normalize(fy, True)
    t = 2 * g.view(-1, 1, 1, 1) * lin.view(1, -1, 1, 1) * d / (fx.shape[2] * fx.shape[3])
    if fault == "no_normaliser_term":
        return t / n
    return (t - u * (u * t).sum(1, keepdim=True)) / n


def pool_grad(m, gp, last=False):
    """gradient of max_pool2d(m, 3, 2) w.r.t. m for the output gradient gp: autograd of F.max_pool2d (first maximum in raster
    order); last=True is the faulty rule that sends it to the last maximum"""
    if not last:
        leaf = m.detach().clone().requires_grad_(True)
        return torch.autograd.grad(F.max_pool2d(leaf, 3, 2), leaf, gp)[0]
    n, c, h, w = m.shape
    win = m.unfold(2, 3, 2).unfold(3, 3, 2).reshape(n, c, gp.shape[2], gp.shape[3], 9)
    arg = 8 - win.flip(-1).argmax(-1)
    oy = torch.arange(gp.shape[2]).view(1, 1, -1, 1)
    ox = torch.arange(gp.shape[3]).view(1, 1, 1, -1)
    idx = (2 * oy + arg // 3) * w + 2 * ox + arg % 3
    return torch.zeros(n, c, h * w, dtype=m.dtype).scatter_add_(2, idx.reshape(n, c, -1), gp.reshape(n, c, -1)).view_as(m)


def backward_from_maps(sd, maps_x, maps_y, g, hw, normalize=False, lpips=True, fault=None):
    """fp64 gradients of sum_{l, n} g[l][n] layer_l(x, y)_n w.r.t. the images, linearised at the given post-ReLU maps.
    g: [5][N] (or [N]: the gradient of the value, the same for every layer); hw = (H, W) of the images.
    -> dict(dx, dy, and per side s in 'xy': tail_s [5] the masked tail gradients, d_s [5] the gradient at relu1..5 (masked),
    pool_s [2] the gradient at the pooled relu1, relu2)"""
    convs, lins = params(sd, F64, lpips)
    if fault == "drop_lin":
        lins[0] = lins[0].clone()
        lins[0][3] = 0
    g = g.to(F64)
    g = g.expand(5, -1) if g.dim() == 1 else g
    mx, my = [m.detach().to(F64) for m in maps_x], [m.detach().to(F64) for m in maps_y]
    n = mx[0].shape[0]
    scale = torch.tensor(SCALE, dtype=F64).view(1, 3, 1, 1)
    out = {}
    for s, (a, b) in (("x", (mx, my)), ("y", (my, mx))):
        mask = [torch.ones_like(m) if fault == "no_relu" else (m > 0).to(F64) for m in a]
        t = []
        for l in range(5):
            if fault == "no_normaliser_term":
                t.append(tail_grad(a[l], b[l], lins[l], g[l], fault) * mask[l])
            else:
                leaf = a[l].clone().requires_grad_(True)
                t.append(torch.autograd.grad((tail(leaf, b[l], lins[l], True) * g[l]).sum(), leaf)[0] * mask[l])
        w = [c[0].flip(2, 3) if fault == "unmirrored" else c[0] for c in convs]
        d = [None] * 5
        d[4] = t[4]
        d[3] = t[3] + F.grad.conv2d_input(a[3].shape, w[4], d[4], padding=1) * mask[3]
        d[2] = t[2] + F.grad.conv2d_input(a[2].shape, w[3], d[3], padding=1) * mask[2]
        p2 = F.grad.conv2d_input((n, 192) + tuple(a[2].shape[2:]), w[2], d[2], padding=1)
        d[1] = t[1] + pool_grad(a[1], p2, fault == "last_argmax") * mask[1]
        p1 = F.grad.conv2d_input((n, 64) + tuple(a[1].shape[2:]), w[1], d[1], padding=2)
        d[0] = t[0] + pool_grad(a[0], p1, fault == "last_argmax") * mask[0]
        di = F.grad.conv2d_input((n, 3) + tuple(hw), w[0], d[0], stride=4, padding=2)
        if fault != "no_scale":
            di = di / scale
        out["d" + s] = 2 * di if normalize else di
        out["tail_" + s], out["d_" + s], out["pool_" + s] = t, d, [p1, p2]
    return out


def autograd_images(sd, x, y, g, normalize=False, lpips=True, dtype=F64):
    """(dx, dy, maps of x, maps of y) by autograd of the whole function in `dtype` (fp64: the reference; fp32: the reference
    implementation's own arithmetic on the CPU)"""
    x = x.detach().to(dtype).requires_grad_(True)
    y = y.detach().to(dtype).requires_grad_(True)
    val, _, fx, fy = lpips_loss(sd, x, y, normalize, lpips, dtype)
    dx, dy = torch.autograd.grad((val * g.to(dtype)).sum(), (x, y))
    return dx, dy, [f.detach() for f in fx], [f.detach() for f in fy]


def relative_to_max(got, ref):
    """max |got - ref| / max |ref|: the norm of the end-to-end bars"""
    return float((got.to(F64) - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------------------------------------ stage references
def _s(k, a):
    return a * (2.0 ** -24 * math.sqrt(k) / U)


def tail_grad_ref(fx, fy, lin, g):
    """(r, S) of dc_lpips_tail_grad for the side whose maps are fx: the written-out gradient, masked by fx > 0.  The launch forms
    n^2 (C squares), u = x / n, d, t and the dot product sum_k u_k t_k in chains of at most C fp32 terms; with ax = |u_x| + |u_y|
    and T_c = 2 |g| w_c ax_c / HW every term of an element is bounded by A_c = (T_c + |u_c| sum_k |u_k| T_k) / n, K = C + 8."""
    fx, fy, lin, g = fx.to(F64), fy.to(F64), lin.to(F64), g.to(F64)
    mask = (fx > 0).to(F64)
    r = tail_grad(fx, fy, lin, g) * mask
    n = torch.sqrt((fx * fx + 1e-8).sum(1, keepdim=True))
    u = (fx / n).abs()
    ax = u + unit_normalize(fy, True).abs()
    t = 2 * g.abs().view(-1, 1, 1, 1) * lin.view(1, -1, 1, 1) * ax / (fx.shape[2] * fx.shape[3])
    a = (t + u * (u * t).sum(1, keepdim=True)) / n
    return r, _s(fx.shape[1] + 8, a * mask)


def conv_dgrad_ref(gin, w, pad, add=None, mapv=None):
    """(r, S) of dc_lpips_conv_dgrad: (add + conv2d_input) * (map > 0); K = Cout k^2 (+ 1 for the add)"""
    gin, w = gin.to(F64), w.to(F64)
    shape = (gin.shape[0], w.shape[1]) + tuple(gin.shape[2:])
    r = F.grad.conv2d_input(shape, w, gin, padding=pad)
    a = F.grad.conv2d_input(shape, w.abs(), gin.abs(), padding=pad)
    if add is not None:
        r, a = r + add.to(F64), a + add.to(F64).abs()
    if mapv is not None:
        m = (mapv > 0).to(F64)
        r, a = r * m, a * m
    return r, _s(w.shape[0] * w.shape[2] * w.shape[3] + 1, a)


def pool_grad_ref(gp, mapv, add=None):
    """(r, S) of dc_lpips_pool_grad: at most four window gradients and the add, K = 5"""
    gp, mapv = gp.to(F64), mapv.to(F64)
    r, a = pool_grad(mapv, gp), pool_grad(mapv, gp.abs())
    if add is not None:
        r, a = r + add.to(F64), a + add.to(F64).abs()
    m = (mapv > 0).to(F64)
    return r * m, _s(5, a * m)


def conv1_dgrad_ref(gin, w1, hw, normalize=False):
    """(r, S) of dc_lpips_conv1_dgrad: at most 3 x 3 taps x 64 channels per element, K = 576 (+ 2: the division and the factor)"""
    gin, w1 = gin.to(F64), w1.to(F64)
    shape = (gin.shape[0], 3) + tuple(hw)
    scale = torch.tensor(SCALE, dtype=F64).view(1, 3, 1, 1) / (2 if normalize else 1)
    r = F.grad.conv2d_input(shape, w1, gin, stride=4, padding=2) / scale
    a = F.grad.conv2d_input(shape, w1.abs(), gin.abs(), stride=4, padding=2) / scale
    return r, _s(578, a)


# ------------------------------------------------------------------------------------------------ Sobel edge loss
SOBEL_X = ((-1.0, 0.0, 1.0), (-2.0, 0.0, 2.0), (-1.0, 0.0, 1.0))
SOBEL_Y = ((-1.0, -2.0, -1.0), (0.0, 0.0, 0.0), (1.0, 2.0, 1.0))


def sobel_edges(img):
    c = img.shape[1]
    kx = torch.tensor(SOBEL_X, dtype=img.dtype, device=img.device).view(1, 1, 3, 3).expand(c, -1, -1, -1)
    ky = torch.tensor(SOBEL_Y, dtype=img.dtype, device=img.device).view(1, 1, 3, 3).expand(c, -1, -1, -1)
    gx = F.conv2d(img, kx, padding=1, groups=c)
    gy = F.conv2d(img, ky, padding=1, groups=c)
    return torch.sqrt(gx ** 2 + gy ** 2 + 1e-6)


def sobel_edge_loss(pred, target, reduction="mean"):
    """controlnet/edge_loss.py:22-38 in the operands' dtype; differentiable by autograd"""
    return F.l1_loss(sobel_edges((pred + 1) / 2), sobel_edges((target + 1) / 2), reduction=reduction)
