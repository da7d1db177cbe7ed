"""fp64 restatement of torchmetrics' FrechetInceptionDistance(feature=64) with torch on the CPU (the rules in the docstring of
diffcodec_amd.metrics.FrechetInceptionDistance), plus the seeded synthetic weights the tests use.  Nothing here comes from the
package: the device kernels of csrc/fid.hip are checked against this (tests/test_gpu_fid.py), and this file against hand-written
loops, numpy and scipy in tests/test_fid_ref.py."""
import math

import numpy as np
import torch
import torch.nn.functional as F

BLOCKS = ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3")
CIN = (3, 32, 32)
COUT = (32, 32, 64)
STRIDE = (2, 1, 1)
PAD = (0, 0, 1)
SIZE = 299
BN_EPS = 1e-3


def synth_weights(seed=0):
    """Seeded fp32 weights under the checkpoint's keys, drawn per block in this order from one generator: conv weight
    randn * sqrt(2 / (9 Cin)), BN weight 0.5 + rand, BN bias 0.3 randn, running_mean 0.2 randn, running_var 0.5 + rand; plus one key
    of a later block, which a loader has to ignore."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, ci, co in zip(BLOCKS, CIN, COUT):
        sd[f"{name}.conv.weight"] = torch.randn(co, ci, 3, 3, generator=g) * math.sqrt(2.0 / (9 * ci))
        sd[f"{name}.bn.weight"] = 0.5 + torch.rand(co, generator=g)
        sd[f"{name}.bn.bias"] = 0.3 * torch.randn(co, generator=g)
        sd[f"{name}.bn.running_mean"] = 0.2 * torch.randn(co, generator=g)
        sd[f"{name}.bn.running_var"] = 0.5 + torch.rand(co, generator=g)
    sd["Conv2d_3b_1x1.conv.weight"] = torch.zeros(80, 64, 1, 1)
    return sd


def as_u8_nchw64(x, normalize=False):
    """uint8 NHWC frames, or (normalize) a float NCHW image in [0,1] taken as (x * 255) truncated to uint8 in the image's own
    precision -> the 8-bit values as fp64 NCHW"""
    x = x.detach().cpu()
    if x.dtype == torch.uint8:
        assert not normalize
        return x.permute(0, 3, 1, 2).double()
    assert normalize, "float images are taken with normalize=True only"
    return (x * 255).to(torch.uint8).double()


def _axis(I):
    p = torch.arange(SIZE, dtype=torch.float64) * (I / SIZE)
    i0 = p.floor().long()
    i1 = (i0 + 1).clamp(max=I - 1)
    return i0, i1, p - i0


def resize(x):
    """fp64 [N,C,H,W] -> [N,C,299,299]: TF1-legacy bilinear (no half-pixel offset)"""
    y0, y1, ly = _axis(x.shape[2])
    x0, x1, lx = _axis(x.shape[3])
    ly = ly.view(-1, 1)
    tl, tr = x[:, :, y0][:, :, :, x0], x[:, :, y0][:, :, :, x1]
    bl, br = x[:, :, y1][:, :, :, x0], x[:, :, y1][:, :, :, x1]
    top = tl + (tr - tl) * lx
    bot = bl + (br - bl) * lx
    return top + (bot - top) * ly


def maps(sd, x, normalize=False):
    """[resized and scaled, relu1, relu2, relu3, pooled] in fp64"""
    x = (resize(as_u8_nchw64(x, normalize)) - 128.0) / 128.0
    out = [x]
    for name, s, p in zip(BLOCKS, STRIDE, PAD):
        v = F.conv2d(x, sd[f"{name}.conv.weight"].double(), None, stride=s, padding=p)
        g, b, m, var = (sd[f"{name}.bn.{k}"].double().view(1, -1, 1, 1) for k in ("weight", "bias", "running_mean", "running_var"))
        x = torch.relu((v - m) / torch.sqrt(var + BN_EPS) * g + b)
        out.append(x)
    out.append(F.max_pool2d(x, 3, 2))
    return out


def features(sd, x, normalize=False, chunk=8):
    """fp64 [N,64]"""
    return torch.cat([maps(sd, x[i:i + chunk], normalize)[4].mean((2, 3)) for i in range(0, x.shape[0], chunk)])


def sums(f):
    """(n, sum f [64], sum f f^T [64,64]) of fp64 rows"""
    f = f.double()
    return f.shape[0], f.sum(0), f.t() @ f


def stats(n, s, sq):
    """(mu, cov) from the sums: mu = sum / n, cov = (sumsq - n mu mu^T) / (n - 1)"""
    mu = s / n
    return mu, (sq - n * torch.outer(mu, mu)) / (n - 1)


def fid(f_real, f_fake):
    """the Frechet distance of two sets of feature rows, fp64, in the eigenvalue form"""
    (mu_r, cov_r), (mu_f, cov_f) = stats(*sums(f_real)), stats(*sums(f_fake))
    ev = np.linalg.eigvals((cov_r @ cov_f).numpy())
    c = np.sqrt(ev.astype(np.complex128)).real.sum()
    d = mu_r - mu_f
    return float((d * d).sum() + cov_r.trace() + cov_f.trace() - 2 * c)
