"""fp64 restatement of lpips.LPIPS(net='alex', version='0.1') with torch.nn.functional on the CPU (the rules in the docstring of
diffcodec_amd.metrics.LPIPS), plus the seeded synthetic weights the tests use.  Nothing here comes from the package: the device
kernels of csrc/lpips.hip are checked against this (tests/test_gpu_lpips.py), and this file against hand-computed values in
tests/test_lpips_ref.py."""
import math

import torch
import torch.nn.functional as F

CHANNELS = (64, 192, 384, 256, 256)
CIN = (3, 64, 192, 384, 256)
KERNEL = (11, 5, 3, 3, 3)
STRIDE = (4, 1, 1, 1, 1)
PAD = (2, 2, 1, 1, 1)
POSITION = (0, 3, 6, 8, 10)                    # torchvision alexnet.features indices of the convolutions
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


def synth_weights(seed=0, layout="library"):
    """Seeded fp32 weights as a state dict: convs uniform in +-1.7/sqrt(Cin k^2), biases uniform in +-1/sqrt(Cin k^2), lin weights
    non-negative.  layout "library": the lpips module's keys (with its `lins.*` duplicates and `scaling_layer.*` buffers);
    "torchvision": (AlexNet features dict with a classifier entry, lin dict)."""
    g = torch.Generator().manual_seed(seed)
    convs, lins = {}, {}
    for l, (co, ci, k, pos) in enumerate(zip(CHANNELS, CIN, KERNEL, POSITION)):
        a = 1.0 / math.sqrt(ci * k * k)
        convs[pos] = ((torch.rand(co, ci, k, k, generator=g) * 2 - 1) * (1.7 * a), (torch.rand(co, generator=g) * 2 - 1) * a)
    for l, co in enumerate(CHANNELS):
        lins[l] = torch.rand(1, co, 1, 1, generator=g) * 0.5
    if layout == "library":
        sd = {"scaling_layer.shift": torch.tensor(SHIFT).view(1, 3, 1, 1), "scaling_layer.scale": torch.tensor(SCALE).view(1, 3, 1, 1)}
        for l, pos in enumerate(POSITION):
            sd[f"net.slice{l + 1}.{pos}.weight"], sd[f"net.slice{l + 1}.{pos}.bias"] = convs[pos]
            sd[f"lin{l}.model.1.weight"] = lins[l]
            sd[f"lins.{l}.model.1.weight"] = lins[l]
        return sd
    feats = {"classifier.1.weight": torch.zeros(4, 4), "classifier.1.bias": torch.zeros(4)}
    for pos in POSITION:
        feats[f"features.{pos}.weight"], feats[f"features.{pos}.bias"] = convs[pos]
    return feats, {f"lin{l}.model.1.weight": lins[l] for l in range(5)}


def _params(sd):
    """[(weight, bias)] * 5 and [lin] * 5 in fp64 from the library-layout dict"""
    convs = [(sd[f"net.slice{l + 1}.{p}.weight"].double(), sd[f"net.slice{l + 1}.{p}.bias"].double()) for l, p in enumerate(POSITION)]
    return convs, [sd[f"lin{l}.model.1.weight"].double().view(-1) for l in range(5)]


def as_nchw64(t):
    """uint8 NHWC frames -> x / 255; float NCHW images as they are; fp64 NCHW on the CPU."""
    t = t.detach().cpu()
    return t.permute(0, 3, 1, 2).double() / 255.0 if t.dtype == torch.uint8 else t.double()


def features(sd, x, normalize=False):
    """relu1 .. relu5 in fp64"""
    convs, _ = _params(sd)
    x = as_nchw64(x)
    if normalize:
        x = 2 * x - 1
    x = (x - torch.tensor(SHIFT, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=torch.float64).view(1, 3, 1, 1)
    out = []
    for l, (w, b) in enumerate(convs):
        if l in (1, 2):
            x = F.max_pool2d(x, 3, 2)
        x = torch.relu(F.conv2d(x, w, b, stride=STRIDE[l], padding=PAD[l]))       # conv2d pads the scaled tensor with zeros
        out.append(x)
    return out


def unit_normalize(f, normfix=False):
    if normfix:
        return f / torch.sqrt((f * f + 1e-8).sum(1, keepdim=True))
    return f / (torch.sqrt((f * f).sum(1, keepdim=True)) + 1e-10)


def tail(fx, fy, lin, normfix=False):
    """[N]: spatial mean of sum_c lin_c (x^_c - y^_c)^2"""
    d = (unit_normalize(fx, normfix) - unit_normalize(fy, normfix)) ** 2
    return (d * lin.view(1, -1, 1, 1)).sum(1).flatten(1).mean(1)


def lpips(sd, x, y, normalize=False, normfix=False):
    """(value [N], per-layer [5][N]) in fp64"""
    _, lins = _params(sd)
    fx, fy = features(sd, x, normalize), features(sd, y, normalize)
    layers = [tail(a, b, w, normfix) for a, b, w in zip(fx, fy, lins)]
    return sum(layers), layers
