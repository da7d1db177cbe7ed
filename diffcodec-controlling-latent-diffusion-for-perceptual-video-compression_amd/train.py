"""The fp32 3x3 convolution of the control extractors with a backward, forward and backward in HIP (csrc/conv_direct.hip,
csrc/conv_f32_mfma.hip, csrc/conv_f32_grad.hip):

    from diffcodec_amd.train import Conv3x3, conv3x3_f32

`conv3x3_f32` is `nn.Conv2d(k=3, padding=1, stride 1 | 2 | 4) [+ SiLU]` in fp32, the one operator every convolution of
`Bi_Dir_FeatureExtractor`, `Bi_Dir_ResidueExtractor`, `WarpExtractor`, the metric nets, the flow-refine convs and the zero convs
goes through; its output has the bits of the inference call `ops.conv3x3_nchw_f32`.  Gradients are exact fp32 with a fixed
summation order and no float atomics: bitwise reproducible, the data gradient of an image independent of its position in the
batch, and every launch only enqueues on the current stream (graph-capturable).  The weight is read in checkpoint layout on every
call, so an optimiser step needs no repacking.  There is no double backward and no CPU path."""
from collections import namedtuple

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import lib

F32 = torch.float32
GRAD_FORMS = {1: "mfma", 2: "valu"}
GRAD_KINDS = {"dgrad": 0, "wgrad": 1}
GradRoute = namedtuple("GradRoute", "form stride ch_t cols_t rows_t groups parts_per_group steps_per_part")


def conv3x3_f32_grad_route(kind, n, cin, h, w, cout, stride):
    """The kernel instance the data gradient (kind 'dgrad') or the weight gradient ('wgrad') launches for a shape, without launching
    (host code only: needs the library, not a GPU): form 'mfma' | 'valu', the MFMA form's STRIDE and channels per workgroup, its pixel
    tile, and for wgrad the K partition (dc_conv3x3_f32_grad_route).  Raises HipLaunchError for a shape the launch would refuse."""
    info = lib.query("dc_conv3x3_f32_grad_route", 8, GRAD_KINDS[kind], int(n), int(cin), int(h), int(w), int(cout), int(stride))
    return GradRoute(GRAD_FORMS[info[0]], *info[1:])


def _workspace(nbytes, device):
    """The split-K workspace of one dc_conv3x3_f32_wgrad launch (any contents).  One function so that the tests can hand out a
    guarded buffer."""
    return torch.empty(nbytes // 4, dtype=F32, device=device)


def _need_device(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: the operand is on device '{t.device}'; the convolution kernels run on the GPU only (there is no CPU path)")


class _Conv3x3Function(torch.autograd.Function):
    """z = dc_conv3x3_nchw_f32 without SiLU (kept for the backward), y = dc_silu_f32(z) when asked: the bits of the fused inference
    launch.  Backward: dc_silu_grad_f32, dc_conv3x3_f32_dgrad, dc_conv3x3_f32_wgrad, each only when its gradient is wanted."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, weight, bias, stride, silu):
        for t, what in ((x, "x"), (weight, "weight"), (bias, "bias")):
            if t is not None and t.dtype != F32:
                raise ValueError(f"conv3x3_f32 {what}: expected torch.float32, got {t.dtype}")
        n, c, h, w = x.shape
        cout = weight.shape[0]
        if not (x.stride(3) == 1 and x.stride(2) == w and x.stride(1) == h * w):
            x = x.contiguous()                                   # dense CHW planes; a channel-slice view is read in place
        wt = weight.contiguous()
        b = None if bias is None else bias.contiguous()
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        with torch.cuda.device(x.device):
            stream = torch.cuda.current_stream().cuda_stream
            z = torch.empty((n, cout, ho, wo), device=x.device, dtype=F32)
            lib.call("dc_conv3x3_nchw_f32", x.data_ptr(), x.stride(0), wt.data_ptr(), 0 if b is None else b.data_ptr(), z.data_ptr(),
                     n, c, h, w, cout, stride, 0, stream)
            y = z
            if silu:
                y = torch.empty_like(z)
                lib.call("dc_silu_f32", z.data_ptr(), y.data_ptr(), z.numel(), stream)
        ctx.save_for_backward(x, wt, z if silu else None)
        ctx.stride, ctx.silu, ctx.has_bias = stride, silu, bias is not None
        return y

    @staticmethod
    @once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, gy):
        x, wt, z = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        if not (need_x or need_w or need_b):
            return None, None, None, None, None
        n, c, h, w = x.shape
        cout, stride = wt.shape[0], ctx.stride
        gz = gy.to(F32).contiguous()
        dx = dw = db = None
        with torch.cuda.device(x.device):
            stream = torch.cuda.current_stream().cuda_stream
            if ctx.silu:
                g = torch.empty_like(gz)
                lib.call("dc_silu_grad_f32", z.data_ptr(), gz.data_ptr(), g.data_ptr(), gz.numel(), stream)
                gz = g
            if need_x:
                dx = torch.empty((n, c, h, w), device=x.device, dtype=F32)
                lib.call("dc_conv3x3_f32_dgrad", gz.data_ptr(), wt.data_ptr(), dx.data_ptr(), n, c, h, w, cout, stride, stream)
            if need_w or need_b:
                dw = torch.empty_like(wt)
                db = torch.empty(cout, device=x.device, dtype=F32) if need_b else None
                ws = _workspace(lib.load().dc_conv3x3_f32_wgrad_ws_bytes(n, c, h, w, cout, stride), x.device)
                lib.call("dc_conv3x3_f32_wgrad", x.data_ptr(), x.stride(0), gz.data_ptr(), dw.data_ptr(),
                         0 if db is None else db.data_ptr(), ws.data_ptr(), n, c, h, w, cout, stride, stream)
                if not need_w:
                    dw = None
        return dx, dw, db, None, None


def conv3x3_f32(x, weight, bias=None, stride=1, silu=False):
    """`F.conv2d(x, weight, bias, stride, padding=1)` (+ SiLU) in fp32 with a backward to x, weight and bias.  x: [N, Cin, H, W] on
    the GPU (a channel-slice view of a contiguous tensor is read in place, anything else is made contiguous); weight: OIHW
    [Cout, Cin, 3, 3]; bias: [Cout] or None.  The output has the bits of `ops.conv3x3_nchw_f32` on the same operands."""
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[1:]) != (x.shape[1], 3, 3):
        raise ValueError(f"conv3x3_f32: x {tuple(x.shape)} and weight {tuple(weight.shape)} do not form a 3x3 convolution")
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"conv3x3_f32: bias {tuple(bias.shape)} for {weight.shape[0]} output channels")
    if stride not in (1, 2, 4):
        raise ValueError(f"conv3x3_f32: stride {stride} (1, 2 or 4)")
    for t, what in ((x, "x"), (weight, "weight")) + (((bias, "bias"),) if bias is not None else ()):
        _need_device(t, "conv3x3_f32 " + what)
    return _Conv3x3Function.apply(x, weight, bias, int(stride), bool(silu))


class Conv3x3(nn.Module):
    """`nn.Conv2d(in_ch, out_ch, 3, stride, padding=1)` (+ SiLU) on `conv3x3_f32`, with nn.Conv2d's parameter names (`weight`,
    `bias`) and initialisation, so a slice of a reference checkpoint loads with `load_state_dict`."""

    def __init__(self, in_ch, out_ch, stride=1, silu=False, bias=True):
        super().__init__()
        if in_ch <= 0 or out_ch <= 0:
            raise ValueError(f"Conv3x3: {in_ch} -> {out_ch} channels")
        if stride not in (1, 2, 4):
            raise ValueError(f"Conv3x3: stride {stride} (1, 2 or 4)")
        self.in_ch, self.out_ch, self.stride, self.silu = int(in_ch), int(out_ch), int(stride), bool(silu)
        ref = nn.Conv2d(in_ch, out_ch, 3, stride, 1, bias=bias)          # its initialisation
        self.weight = nn.Parameter(ref.weight.detach().clone())
        self.register_parameter("bias", nn.Parameter(ref.bias.detach().clone()) if bias else None)

    @classmethod
    def from_packed(cls, pc, stride=1, silu=False):
        """Wrap the tensors of an inference `ops.PackedConvF32` as parameters that share its storage: an optimiser step on the
        module is what the inference net reads next."""
        m = cls.__new__(cls)
        nn.Module.__init__(m)
        if stride not in (1, 2, 4):
            raise ValueError(f"Conv3x3: stride {stride} (1, 2 or 4)")
        if pc.w.dim() != 4 or tuple(pc.w.shape[2:]) != (3, 3) or pc.w.dtype != F32 or not pc.w.is_contiguous():
            raise ValueError("Conv3x3.from_packed: expected the contiguous fp32 OIHW weight of a 3x3 PackedConvF32")
        m.in_ch, m.out_ch, m.stride, m.silu = pc.cin, pc.cout, int(stride), bool(silu)
        m.weight = nn.Parameter(pc.w)
        m.register_parameter("bias", nn.Parameter(pc.bias) if pc.bias is not None else None)
        return m

    def forward(self, x):
        return conv3x3_f32(x, self.weight, self.bias, self.stride, self.silu)

    def extra_repr(self):
        return f"{self.in_ch}, {self.out_ch}, stride={self.stride}, silu={self.silu}, bias={self.bias is not None}"
