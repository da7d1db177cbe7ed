"""The project's own restatement of the flow-propagation network (diffcodec_amd.flow_propagation.HipCMP, csrc/cmp.hip) with torch on
the CPU, in fp64 unless another dtype is asked for, and the seeded weights the tests share: the BatchNorm fold, convolutions,
pools, the align_corners upsample, the softmax expectation and the grid sampling.  It keeps its own table of the architecture (it
does not read the package's), and tests/golden/cmp_flow.npz (tools/make_cmp_goldens.py) pins it against the reference's own CMP
module, Fuser.convert_flow and CMP.eval upsample."""
import math

import torch
import torch.nn.functional as F

DATA_MEAN = (123.675, 116.28, 103.53)
DATA_DIV = (58.395, 57.12, 57.375)
EPS = 1e-5
CONFIGS = {
    "skip": dict(arch="CMP", image_encoder="resnet50", sparse_encoder="shallownet8x", flow_decoder="MotionDecoderSkipLayer",
                 skip_layer=True, img_enc_dim=256, sparse_enc_dim=16, output_dim=198, decoder_combo=[1, 2, 4],
                 pretrained_image_encoder=False, flow_criterion="DiscreteLoss", nbins=99, fmax=50),
    "plain": dict(arch="CMP", image_encoder="resnet50", sparse_encoder="shallownet8x", flow_decoder="MotionDecoderPlain",
                  skip_layer=False, img_enc_dim=256, sparse_enc_dim=16, output_dim=198, decoder_combo=[1, 2, 4],
                  pretrained_image_encoder=False, flow_criterion="DiscreteLoss", nbins=99, fmax=50),
}
WEIGHT_SEED = 4321
# the head's weights are multiplied by this so that the logits have a standard deviation near 6 (a default-initialised head gives
# one-hot softmaxes, and the flow would then test nothing but the argmax); measured by tools/make_cmp_goldens.py
HEAD_SCALE = {"skip": 0.125, "plain": 0.105}
LAYERS = (("layer1", 64, 3, 1, 1), ("layer2", 128, 4, 2, 1), ("layer3", 256, 6, 1, 2), ("layer4", 512, 3, 1, 4))
ENDPOINTS = {"skip": ("sparse_enc", "img_enc", "skip2", "skip4", "f8", "f4", "f2", "logits", "flow", "flow_up"),
             "plain": ("sparse_enc", "img_enc", "skip2", "skip4", "cat8", "logits", "flow", "flow_up")}


def units(arch):
    """[(conv key, bn key or None, Cin, Cout, k, bias)] in the reference's state-dict order."""
    u = [("image_encoder.conv1", "image_encoder.bn1", 3, 64, 7, False)]
    cin = 64
    for layer, planes, blocks, _, _ in LAYERS:
        for b in range(blocks):
            p = f"image_encoder.{layer}.{b}"
            u.append((p + ".conv1", p + ".bn1", cin, planes, 1, False))
            u.append((p + ".conv2", p + ".bn2", planes, planes, 3, False))
            u.append((p + ".conv3", p + ".bn3", planes, planes * 4, 1, False))
            if b == 0:
                u.append((p + ".downsample.0", p + ".downsample.1", cin, planes * 4, 1, False))
            cin = planes * 4
    u.append(("image_encoder.conv5", None, 2048, 256, 1, True))
    u.append(("flow_encoder.features.0", "flow_encoder.features.1", 4, 16, 5, True))
    u.append(("flow_encoder.features.4", "flow_encoder.features.5", 16, 16, 3, True))
    depth = 3 if arch == "skip" else 2
    for c in ((1, 2, 4, 8) if arch == "skip" else (1, 2, 4)):
        first = 0 if c == 1 else 1
        for i in range(depth):
            u.append((f"flow_decoder.decoder{c}.{first + 3 * i}", f"flow_decoder.decoder{c}.{first + 3 * i + 1}",
                      272 if i == 0 else 128, 128, 3, True))
    if arch == "skip":
        for name, ci, co in (("fusion8", 512, 256), ("skipconv4", 256, 128), ("fusion4", 384, 128), ("skipconv2", 64, 32),
                             ("fusion2", 160, 64)):
            u.append((f"flow_decoder.{name}.0", f"flow_decoder.{name}.1", ci, co, 3, True))
        u.append(("flow_decoder.head", None, 64, 198, 1, True))
    else:
        u.append(("flow_decoder.head", None, 384, 198, 1, True))
    return u


def synth_weights(arch, seed=WEIGHT_SEED, head_scale=None):
    """A reference-shaped state dict drawn in `units` order from one generator: conv randn * sqrt(2 / fan_in), conv bias
    0.1 randn, bn.weight 0.5 + rand (0.25 + 0.5 rand on a residual branch's last BatchNorm, so sixteen blocks do not explode),
    bn.bias 0.2 randn, running_mean 0.2 randn, running_var 0.5 + rand: every statistic away from (0, 1, 1, 0)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for ck, bk, ci, co, k, bias in units(arch):
        sd[ck + ".weight"] = torch.randn(co, ci, k, k, generator=g) * math.sqrt(2.0 / (ci * k * k))
        if bias:
            sd[ck + ".bias"] = 0.1 * torch.randn(co, generator=g)
        if bk:
            last = bk.endswith(".bn3")
            sd[bk + ".weight"] = (0.25 + 0.5 * torch.rand(co, generator=g)) if last else (0.5 + torch.rand(co, generator=g))
            sd[bk + ".bias"] = 0.2 * torch.randn(co, generator=g)
            sd[bk + ".running_mean"] = 0.2 * torch.randn(co, generator=g)
            sd[bk + ".running_var"] = 0.5 + torch.rand(co, generator=g)
            sd[bk + ".num_batches_tracked"] = torch.tensor(0)
    sd["flow_decoder.head.weight"] = sd["flow_decoder.head.weight"] * (HEAD_SCALE[arch] if head_scale is None else head_scale)
    return sd


def inputs(n, h, w, seed):
    """(uint8 frames [n,h,w,3], sparse [n,4,h,w]): smooth frames, and a smooth +-20 px flow kept at a stride-8 grid."""
    g = torch.Generator().manual_seed(seed)
    img = F.avg_pool2d(torch.rand(n, 3, h, w, generator=g), 5, 1, 2, count_include_pad=False)
    img = ((img - 0.5) * 3 + 0.5).clamp(0, 1)
    u8 = (img * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    lo = torch.randn(n, 2, max(h // 16, 2), max(w // 16, 2), generator=g) * 10.0
    flow = F.interpolate(lo, size=(h, w), mode="bilinear", align_corners=True)
    return u8, sparse_grid(flow.double(), 8).float()


def normalise(u8, dtype=torch.float64):
    """uint8 [N,H,W,3] -> [N,3,H,W], (v - mean_c) / div_c"""
    x = u8.permute(0, 3, 1, 2).to(dtype)
    return (x - torch.tensor(DATA_MEAN, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(DATA_DIV, dtype=dtype).view(1, 3, 1, 1)


# ------------------------------------------------------------------------------------------------ stages
def fold(sd, ck, bk, eps=EPS):
    """(w, s, t) in fp64 with y = s * conv(x, w) + t"""
    w = sd[ck + ".weight"].double()
    b = sd[ck + ".bias"].double() if ck + ".bias" in sd else torch.zeros(w.shape[0], dtype=torch.float64)
    if bk is None:
        return w, torch.ones_like(b), b
    s = sd[bk + ".weight"].double() / torch.sqrt(sd[bk + ".running_var"].double() + eps)
    return w, s, sd[bk + ".bias"].double() - sd[bk + ".running_mean"].double() * s + b * s


def conv(x, w, s, t, stride=1, dilation=1, residual=None, relu=True):
    k = w.shape[-1]
    y = F.conv2d(x, w.to(x.dtype), stride=stride, dilation=dilation, padding=dilation * (k - 1) // 2)
    y = y * s.to(x.dtype).view(1, -1, 1, 1) + t.to(x.dtype).view(1, -1, 1, 1)
    if residual is not None:
        y = y + residual
    return torch.relu(y) if relu else y


def max_pool(x, k, stride, pad=0):
    return F.max_pool2d(x, k, stride, pad)


def avg_pool(x):
    return F.avg_pool2d(x, 2, 2)


def upsample(x, ho, wo):
    """bilinear, align_corners = True, written out: source position o * (in - 1) / (out - 1), 0 when out = 1"""
    n, c, h, w = x.shape
    py = torch.arange(ho, dtype=torch.float64) * ((h - 1) / (ho - 1) if ho > 1 else 0.0)
    px = torch.arange(wo, dtype=torch.float64) * ((w - 1) / (wo - 1) if wo > 1 else 0.0)
    y0, x0 = py.floor().long().clamp(max=h - 1), px.floor().long().clamp(max=w - 1)
    y1, x1 = (y0 + 1).clamp(max=h - 1), (x0 + 1).clamp(max=w - 1)
    ly, lx = (py - y0).to(x.dtype).view(1, 1, ho, 1), (px - x0).to(x.dtype).view(1, 1, 1, wo)
    top = x[:, :, y0][:, :, :, x0] * (1 - lx) + x[:, :, y0][:, :, :, x1] * lx
    bot = x[:, :, y1][:, :, :, x0] * (1 - lx) + x[:, :, y1][:, :, :, x1] * lx
    return top * (1 - ly) + bot * ly


def convert_flow(logits, nbins=99, fmax=50.0):
    """two softmaxes and the expectation over the bin centres (i + 1/2) * 2 fmax / nbins - fmax"""
    centres = ((torch.arange(nbins, dtype=torch.float64) + 0.5) * (2.0 * fmax / nbins) - fmax).to(logits.dtype).view(1, -1, 1, 1)
    out = []
    for half in (logits[:, :nbins], logits[:, nbins:]):
        e = torch.exp(half - half.max(dim=1, keepdim=True).values)
        out.append((e * centres).sum(1, keepdim=True) / e.sum(1, keepdim=True))
    return torch.cat(out, 1)


def grid_points(h, w, stride):
    """flow_sampler's 'grid' strategy: (rows, columns) of the guide points"""
    y0 = int((h - h // stride * stride) / 2)
    x0 = int((w - w // stride * stride) / 2)
    return list(range(y0, h, stride)), list(range(x0, w, stride))


def sparse_grid(flow, stride):
    """[N,2,H,W] -> [N,4,H,W]: the flow at the grid points, zero elsewhere; the mask twice"""
    n, _, h, w = flow.shape
    ys, xs = grid_points(h, w, stride)
    mask = torch.zeros(1, 1, h, w, dtype=flow.dtype)
    for y in ys:
        for x in xs:
            mask[0, 0, y, x] = 1
    return torch.cat([flow * mask, mask.expand(n, 2, h, w)], 1)


# ------------------------------------------------------------------------------------------------ the network
def endpoints(image, sparse, sd, arch, dtype=torch.float64):
    """image: normalised [N,3,H,W]; sparse [N,4,H,W] -> dict of ENDPOINTS[arch]"""
    image, sparse = image.to(dtype), sparse.to(dtype)
    f = lambda ck, bk: fold(sd, ck, bk)
    x = conv(sparse, *f("flow_encoder.features.0", "flow_encoder.features.1"), stride=2)
    x = conv(max_pool(x, 2, 2), *f("flow_encoder.features.4", "flow_encoder.features.5"))
    sparse_enc = avg_pool(x)

    stem = conv(image, *f("image_encoder.conv1", "image_encoder.bn1"), stride=2)
    x = max_pool(stem, 3, 2, 1)
    for layer, _, blocks, stride, dil in LAYERS:
        for b in range(blocks):
            p = f"image_encoder.{layer}.{b}"
            st = stride if b == 0 else 1
            res = conv(x, *f(p + ".downsample.0", p + ".downsample.1"), stride=st, relu=False) if b == 0 else x
            y = conv(x, *f(p + ".conv1", p + ".bn1"))
            y = conv(y, *f(p + ".conv2", p + ".bn2"), stride=st, dilation=dil)
            x = conv(y, *f(p + ".conv3", p + ".bn3"), residual=res)
        if layer == "layer1":
            layer1 = x
    img_enc = conv(x, *f("image_encoder.conv5", None), relu=False)
    if img_enc.shape[2:] != sparse_enc.shape[2:]:
        raise ValueError(f"the encoders disagree: {tuple(img_enc.shape[2:])} against {tuple(sparse_enc.shape[2:])}")
    ep = dict(sparse_enc=sparse_enc, img_enc=img_enc, skip2=stem, skip4=layer1)
    enc = torch.cat([img_enc, sparse_enc], 1)
    h8, w8 = enc.shape[2:]

    depth = 3 if arch == "skip" else 2
    branches = []
    for c in ((1, 2, 4, 8) if arch == "skip" else (1, 2, 4)):
        first = 0 if c == 1 else 1
        x = enc if c == 1 else max_pool(enc, c, c)
        for i in range(depth):
            x = conv(x, *f(f"flow_decoder.decoder{c}.{first + 3 * i}", f"flow_decoder.decoder{c}.{first + 3 * i + 1}"))
        branches.append(x if c == 1 else upsample(x, h8, w8))
    cat = torch.cat(branches, 1)
    g = lambda name: f(f"flow_decoder.{name}.0", f"flow_decoder.{name}.1")
    if arch == "skip":
        ep["f8"] = f8 = conv(cat, *g("fusion8"))
        cat4 = torch.cat([upsample(f8, *layer1.shape[2:]), conv(layer1, *g("skipconv4"))], 1)
        ep["f4"] = f4 = conv(cat4, *g("fusion4"))
        cat2 = torch.cat([upsample(f4, *stem.shape[2:]), conv(stem, *g("skipconv2"))], 1)
        ep["f2"] = f2 = conv(cat2, *g("fusion2"))
        top = f2
    else:
        ep["cat8"] = top = cat
    ep["logits"] = conv(top, *f("flow_decoder.head", None), relu=False)
    ep["flow"] = convert_flow(ep["logits"])
    ep["flow_up"] = upsample(ep["flow"], image.shape[2], image.shape[3])
    return ep


def subsample(t, count=600):
    flat = t.reshape(-1)
    return flat[::max(1, flat.numel() // count)][:count].contiguous()
