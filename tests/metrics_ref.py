"""fp64 restatement of PSNR and of pytorch_msssim 1.0's ssim / ms_ssim (the rules in diffcodec_amd/metrics.py's docstring), on the
CPU with torch conv2d in fp64.  The device kernels of csrc/metrics.hip are checked against this (tests/test_gpu_metrics.py); this
file is pinned to an independent scipy evaluation and to avg_pool2d in tests/test_metrics_ref.py."""
import math

import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window(ws=11, sigma=1.5):
    c = torch.arange(ws, dtype=torch.float64) - ws // 2
    g = torch.exp(-(c ** 2) / (2.0 * sigma * sigma))
    return g / g.sum()


def as_nchw64(t):
    """uint8 NHWC frames or float NCHW images -> fp64 NCHW on the CPU."""
    t = t.detach().cpu()
    return t.permute(0, 3, 1, 2).double() if t.dtype == torch.uint8 else t.double()


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


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, K=(0.01, 0.03), nonnegative_ssim=False):
    X, Y = as_nchw64(X), as_nchw64(Y)
    s, _ = ssim_cs(X, Y, data_range, window(win_size, win_sigma), K)
    if nonnegative_ssim:
        s = torch.relu(s)
    return s.mean() if size_average else s.mean(1)


def psnr(X, Y, data_range=255.0):
    """[N] fp64: 10 log10(L^2 / mse) per image, +inf when mse == 0"""
    X, Y = as_nchw64(X), as_nchw64(Y)
    mse = ((X - Y) ** 2).flatten(1).mean(1)
    return torch.tensor([math.inf if m == 0 else 10 * math.log10(data_range ** 2 / m) for m in mse.tolist()], dtype=torch.float64)
