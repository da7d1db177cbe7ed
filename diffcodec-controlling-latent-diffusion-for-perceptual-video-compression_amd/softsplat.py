"""Drop-in for the reference's controlnet/softsplat.py on gfx950: ``softsplat(tenIn, tenFlow, tenMetric, strMode)`` with every
mode string the reference accepts, and ``softsplat_func``, the differentiable 'sum' primitive (forward + backward in HIP).

    from diffcodec_amd.softsplat import softsplat, softsplat_func

Two paths, same results:
  * composed — the wrapper's cat / exp / divide in torch around ``softsplat_func`` (softsplat.py:240-270): whenever a gradient
    is required, and for any mode string the fused kernel does not cover;
  * fused    — one gather launch (dc_splat_sum_f32 / dc_splat_norm_f32) under no-grad for 'sum', 'avg', 'linear[-*eps]' and
    'soft[-*eps]'.  For 'sum', 'avg' and 'linear' it returns the bits of the composed path.
Forward and backward are deterministic (no float atomics), fp32, and safe to capture into a graph.  There is no CPU path."""
import torch
from torch.autograd.function import once_differentiable

from . import ops

_BASES = ("sum", "avg", "linear", "soft")
_EPS = ("addeps", "zeroeps", "clipeps")
_FUSED = {"avg": ("avg", "addeps")}
_FUSED.update({b: (b, "addeps") for b in ("linear", "soft")})
_FUSED.update({f"{b}-{e}": (b, e) for b in ("linear", "soft") for e in _EPS})


def _f32c(t):
    return t.to(torch.float32).contiguous()


def _need_device(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"softsplat: {name} is on device '{t.device}'; the splat kernels run on the GPU only (there is no CPU path)")


class softsplat_func(torch.autograd.Function):
    """out = splat(tenIn, tenFlow), the 'sum' primitive (softsplat.py:277-530).  Inputs are cast to fp32 and made contiguous, the
    output is fp32; under torch.autocast it runs with autocast off on fp32 inputs, as the reference's
    custom_fwd(cast_inputs=torch.float32) / custom_bwd pair does."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, tenIn, tenFlow):
        _need_device(tenIn, "tenIn")
        _need_device(tenFlow, "tenFlow")
        tenIn, tenFlow = _f32c(tenIn), _f32c(tenFlow)
        ctx.save_for_backward(tenIn, tenFlow)
        return ops.splat_sum(tenIn, tenFlow)

    @staticmethod
    @once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, tenOutgrad):
        tenIn, tenFlow = ctx.saved_tensors
        tenOutgrad = _f32c(tenOutgrad)
        tenIngrad = ops.splat_ingrad(tenFlow, tenOutgrad) if ctx.needs_input_grad[0] else None
        tenFlowgrad = ops.splat_flowgrad(tenIn, tenFlow, tenOutgrad) if ctx.needs_input_grad[1] else None
        return tenIngrad, tenFlowgrad


def softsplat(tenIn: torch.Tensor, tenFlow: torch.Tensor, tenMetric: torch.Tensor, strMode: str):
    """softsplat.py:232-274, read literally: the mode tests on `strMode.split('-')[0]` and the exact tests `strMode == 'sum'` /
    `strMode == 'avg'` are the reference's, so e.g. 'avg-addeps' appends no ones channel and normalises by the last input channel."""
    parts = strMode.split("-")
    base = parts[0]
    if base not in _BASES:
        raise ValueError(f"softsplat: unknown mode {strMode!r} (expected one of {_BASES}, optionally with -addeps / -zeroeps / -clipeps)")
    if strMode in ("sum", "avg") and tenMetric is not None:
        raise ValueError(f"softsplat: mode {strMode!r} takes no metric (tenMetric must be None)")
    if base in ("linear", "soft") and tenMetric is None:
        raise ValueError(f"softsplat: mode {strMode!r} needs a metric (tenMetric is None)")
    for t, nm in ((tenIn, "tenIn"), (tenFlow, "tenFlow"), (tenMetric, "tenMetric")):
        if t is not None:
            _need_device(t, nm)

    wants_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (tenIn, tenFlow, tenMetric))
    # the fused normalised modes form in * metric in fp32: only fp32 operands give the composed path's products
    all_f32 = all(t is None or t.dtype == torch.float32 for t in (tenIn, tenFlow, tenMetric))
    if not wants_grad and (strMode == "sum" or (strMode in _FUSED and all_f32)):
        with torch.autocast(device_type="cuda", enabled=False):
            if strMode == "sum":
                return ops.splat_sum(_f32c(tenIn), _f32c(tenFlow))
            mode, eps = _FUSED[strMode]
            return ops.splat_norm(_f32c(tenIn), _f32c(tenFlow), None if mode == "avg" else _f32c(tenMetric), mode, eps)

    if strMode == "avg":
        tenIn = torch.cat([tenIn, tenIn.new_ones([tenIn.shape[0], 1, tenIn.shape[2], tenIn.shape[3]])], 1)
    elif base == "linear":
        tenIn = torch.cat([tenIn * tenMetric, tenMetric], 1)
    elif base == "soft":
        tenIn = torch.cat([tenIn * tenMetric.exp(), tenMetric.exp()], 1)

    tenOut = softsplat_func.apply(tenIn, tenFlow)

    if base in ("avg", "linear", "soft"):
        tenNormalize = tenOut[:, -1:, :, :]
        eps = "addeps" if len(parts) == 1 else parts[1]
        if eps == "addeps":
            tenNormalize = tenNormalize + 0.0000001
        elif eps == "zeroeps":
            tenNormalize = torch.where(tenNormalize == 0.0, torch.ones_like(tenNormalize), tenNormalize)
        elif eps == "clipeps":
            tenNormalize = tenNormalize.clip(0.0000001, None)
        tenOut = tenOut[:, :-1, :, :] / tenNormalize
    return tenOut
