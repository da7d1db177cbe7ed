"""The FDN injection (`FDN`, controlnet/control_utils.py:19-34) and everything `DualFlowControlNet` adds to a diffusers
`ControlNetModel` (controlnet/flownet.py:40-47) as trainable modules, forward and backward in HIP:

    from diffcodec_amd.fdn_train import fdn, FDN, DualFlowControlLayers

`fdn(x, gamma, beta)` is `GroupNorm(32, C, affine=False)(x) * (1 + gamma) + beta` in fp32 NCHW as ONE autograd operator
(csrc/fdn_grad.hip, include/diffcodec_fdn_hip.h) with gradients to all three operands; the gradient of beta is the incoming gradient
itself, for which nothing is launched.  gamma and beta may be the two channel halves of one tensor: their planes are read in place.
Exact fp32 with a fixed summation order and no float atomics: bitwise reproducible, a sample's results independent of the batch it
is in, every launch only enqueues on the current stream (graph-capturable).  There is no double backward and no CPU path.

`FDN` is the module on `train.Conv3x3` and `fdn` with the reference's parameter names, so an `fdn64.*` slice of a checkpoint loads
with `load_state_dict`.  `DualFlowControlLayers` holds the trainable pyramid (`pyramid_train.BiDirFeatureExtractor`) and the four
FDNs under the attribute names of flownet.py:40-47, so `load_state_dict(controlnet_state_dict, strict=False)` picks up exactly their
slices.  This is the fp32 training path; the bf16 NHWC inference FDN (`ops.fdn_modulate`, gamma and beta hoisted per frame) is
untouched."""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import lib
from .pyramid_train import INJECT_CHANNELS, BiDirFeatureExtractor
from .train import Conv3x3

F32 = torch.float32
GROUPS = 32                                                                # control_utils.py:25
EPS = 1e-5                                                                 # nn.GroupNorm's default, which the reference keeps


def _need_device(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: the operand is on device '{t.device}'; the FDN kernels run on the GPU only (there is no CPU path)")


def _like(t):
    """An output of x's shape (y, g_x, g_gamma; dense, any contents, every element is written).  One function so that the tests can
    hand out guarded buffers."""
    return torch.empty(t.shape, device=t.device, dtype=F32)


def _stats(n, device):
    """The saved mean or rstd ([N, 32]; every element is written); see _like."""
    return torch.empty((n, GROUPS), device=device, dtype=F32)


def _planes(t):
    """t [N, C, H, W] -> (tensor whose [C, H, W] planes are dense, its batch stride in elements).  A channel-slice view of a contiguous
    tensor is passed as it lies; anything else is made contiguous."""
    n, c, h, w = t.shape
    if not (t.stride(3) == 1 and t.stride(2) == w and t.stride(1) == h * w and (n == 1 or t.stride(0) >= c * h * w)):
        t = t.contiguous()
    return t, (t.stride(0) if n > 1 else c * h * w)


class _FDNFunction(torch.autograd.Function):
    """y = dc_fdn_f32(x, gamma, beta), saving x, gamma and the [N, 32] mean and rstd.  Backward: one dc_fdn_grad_f32 launch for the
    gradients of x and gamma, each only when wanted; the gradient of beta is the incoming gradient."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, gamma, beta, eps):
        for t, what in ((x, "x"), (gamma, "gamma"), (beta, "beta")):
            if t.dtype != F32:
                raise ValueError(f"fdn {what}: expected torch.float32, got {t.dtype}")
        n, c, h, w = x.shape
        x = x.contiguous()
        gamma, gs = _planes(gamma)
        beta, bs = _planes(beta)
        with torch.cuda.device(x.device):
            stream = torch.cuda.current_stream().cuda_stream
            y, mean, rstd = _like(x), _stats(n, x.device), _stats(n, x.device)
            lib.call("dc_fdn_f32", x.data_ptr(), gamma.data_ptr(), gs, beta.data_ptr(), bs, y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                     n, c, h, w, eps, stream)
        ctx.save_for_backward(x, gamma, mean, rstd)
        return y

    @staticmethod
    @once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        x, gamma, mean, rstd = ctx.saved_tensors
        need_x, need_gamma, need_beta = ctx.needs_input_grad[:3]
        gx = gg = None
        if need_x or need_gamma:
            n, c, h, w = x.shape
            gd = g.to(F32).contiguous()
            gamma, gs = _planes(gamma)
            with torch.cuda.device(x.device):
                stream = torch.cuda.current_stream().cuda_stream
                gx = _like(x) if need_x else None
                gg = _like(x) if need_gamma else None
                lib.call("dc_fdn_grad_f32", gd.data_ptr(), x.data_ptr(), gamma.data_ptr(), gs, mean.data_ptr(), rstd.data_ptr(),
                         0 if gx is None else gx.data_ptr(), 0 if gg is None else gg.data_ptr(), c * h * w, n, c, h, w, stream)
        return gx, gg, (g if need_beta else None), None


def fdn(x, gamma, beta, eps=EPS):
    """`F.group_norm(x, 32, eps=eps) * (1 + gamma) + beta` in fp32 with a backward to x, gamma and beta.  x, gamma, beta: [N, C, H, W]
    on the GPU, C a multiple of 32; gamma and beta may be channel-slice views of a contiguous tensor (read in place).  A gamma or beta
    whose spatial size differs from x's is the reference's assertion at control_utils.py:30."""
    if x.dim() != 4:
        raise ValueError(f"fdn: x {tuple(x.shape)} is not [N, C, H, W]")
    if x.shape[1] % GROUPS or x.shape[1] == 0:
        raise ValueError(f"fdn: {x.shape[1]} channels are not a positive multiple of {GROUPS} (GroupNorm(32, C))")
    for t, what in ((gamma, "gamma"), (beta, "beta")):
        if tuple(t.shape) != tuple(x.shape):
            raise ValueError(f"fdn: {what} {tuple(t.shape)}, expected x's {tuple(x.shape)}")
    if not float(eps) > 0.0:
        raise ValueError(f"fdn: eps {eps}")
    for t, what in ((x, "x"), (gamma, "gamma"), (beta, "beta")):
        _need_device(t, "fdn " + what)
    return _FDNFunction.apply(x, gamma, beta, float(eps))


class FDN(nn.Module):
    """`FDN(norm_nc, label_nc)` (control_utils.py:19-34), trainable: `forward(x [N, norm_nc, H, W], local_features [N, label_nc, H, W])`
    = fdn(x, conv_gamma(local_features), conv_beta(local_features)), the two convolutions on `train.Conv3x3` with nn.Conv2d's
    parameter names and initialisation."""

    def __init__(self, norm_nc, label_nc):
        super().__init__()
        if norm_nc <= 0 or norm_nc % GROUPS:
            raise ValueError(f"FDN: norm_nc {norm_nc} is not a positive multiple of {GROUPS} (GroupNorm(32, C))")
        self.norm_nc, self.label_nc = int(norm_nc), int(label_nc)
        self.conv_gamma = Conv3x3(label_nc, norm_nc, 1, False)
        self.conv_beta = Conv3x3(label_nc, norm_nc, 1, False)

    def forward(self, x, local_features):
        if x.dim() != 4 or local_features.dim() != 4 or local_features.shape[2:] != x.shape[2:] or local_features.shape[0] != x.shape[0]:
            raise ValueError(f"FDN: x {tuple(x.shape)} and local_features {tuple(local_features.shape)} differ in batch or spatial size")
        return fdn(x, self.conv_gamma(local_features), self.conv_beta(local_features))

    def extra_repr(self):
        return f"norm_nc={self.norm_nc}, label_nc={self.label_nc}"


class DualFlowControlLayers(nn.Module):
    """What DualFlowControlNet adds to ControlNetModel (flownet.py:40-47), trainable, under the reference's attribute names:
    `feature_extractor` and `fdn64`, `fdn32`, `fdn16`, `fdn08`.

    `pyramid(controlnet_cond [B,6,H,W], flow_cond [B,4,H,W])` returns the four levels P64, P32, P16, P08 (flownet.py:79);
    `inject(i, sample, levels)` is the i-th injection of the encoder (flownet.py:84, 98-106) on those levels: 0 after conv_in
    (fdn64, P64), 1 after down block 0 (fdn32, P32), 2 after down block 1 (fdn16, P16), 3 and 4 after down blocks 2 and 3 (fdn08, P08
    both times).  The module keeps nothing between calls: the caller holds the levels of the step, and with them their graph."""

    SITES = (("fdn64", 0), ("fdn32", 1), ("fdn16", 2), ("fdn08", 3), ("fdn08", 3))

    def __init__(self, inject_channels=INJECT_CHANNELS):
        super().__init__()
        inject = tuple(int(c) for c in inject_channels)
        self.inject_channels = inject
        self.feature_extractor = BiDirFeatureExtractor(inject)
        c64, c32, c16, c08 = inject
        self.fdn64 = FDN(c64, c64)
        self.fdn32 = FDN(c32, c32)
        self.fdn16 = FDN(c16, c16)
        self.fdn08 = FDN(c08, c08)

    def pyramid(self, controlnet_cond, flow_cond, return_aux=False):
        return self.feature_extractor(controlnet_cond, flow_cond, return_aux=return_aux)

    def inject(self, i, sample, levels):
        """sample after the i-th injection; levels: the four levels `pyramid` returned for this step"""
        if not 0 <= i < len(self.SITES):
            raise ValueError(f"DualFlowControlLayers.inject: site {i} (0 .. {len(self.SITES) - 1})")
        if len(levels) != 4:
            raise ValueError(f"DualFlowControlLayers.inject: {len(levels)} levels (the four of `pyramid`)")
        name, level = self.SITES[i]
        return getattr(self, name)(sample, levels[level])
