"""The two image-space losses of the reference's training step (train_controlnet.py:951-955, 1138-1157) on gfx950, forward and
backward in HIP (csrc/lpips_grad.hip, csrc/edge_loss.hip):

    from diffcodec_amd.losses import NormFixLPIPS, SobelEdgeLoss

`NormFixLPIPS` is controlnet/lpips_loss.py's module (AlexNet, version 0.1) and `SobelEdgeLoss` controlnet/edge_loss.py's.  Both are
exact fp32 with a fixed summation order and no float atomics: values and gradients are bitwise reproducible, independent of the
pair's position in the batch, and the launches only enqueue on the current stream (graph-capturable).  The LPIPS weights are
frozen (no weight gradients), neither loss has a double backward, and there is no CPU path."""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import lib
from .metrics import LPIPS, LPIPS_CHANNELS, LPIPS_CIN, LPIPS_FEATURE_INDEX, LPIPS_KERNEL, _check_pair, _nchw, _state_tensor


def pack_lpips_dgrad_weights(state_dict, lin_state_dict=None):
    """One fp32 CPU vector in the layout dc_lpips_conv_dgrad reads: for conv2 .. conv5 the matrix [(co, ky, kx)][Cin] with the taps
    mirrored, element [(co k + ky) k + kx][ci] = w[co][ci][k - 1 - ky][k - 1 - kx]: the data gradient of a stride-1 'same'
    convolution is a convolution of the output gradient with these.  Accepts the layouts of metrics.pack_lpips_weights."""
    sd = dict(state_dict)
    if lin_state_dict is not None:
        sd.update(lin_state_dict)
    library = any(k.startswith("net.slice") for k in sd)
    parts = []
    for l, (co, ci, k, pos) in enumerate(zip(LPIPS_CHANNELS, LPIPS_CIN, LPIPS_KERNEL, LPIPS_FEATURE_INDEX)):
        if l == 0:
            continue                                     # conv1's data gradient reads the forward's K-major matrix
        stem = f"net.slice{l + 1}.{pos}" if library else f"features.{pos}"
        w = _state_tensor("LPIPS", sd, stem + ".weight", (co, ci, k, k))
        parts.append(w.flip(2, 3).permute(0, 2, 3, 1).reshape(-1))
    return torch.cat(parts).contiguous()


def _need_device(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: the operand is on device '{t.device}'; the loss kernels run on the GPU only (there is no CPU path)")


class _LpipsKeepFunction(torch.autograd.Function):
    """[6, N] fp32 (the five layer terms, then the value) of dc_lpips_alex_keep; the backward is dc_lpips_alex_backward on the maps
    that forward kept.  Runs on fp32 operands with autocast off."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, in0, in1, model, normalize):
        n, _, h, w = in0.shape
        dev = in0.device
        wts = model._weights(dev)
        l = lib.load()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            keep = torch.empty(l.dc_lpips_keep_ws_bytes(n, h, w), dtype=torch.uint8, device=dev)
            out = torch.empty(6 * n, dtype=torch.float64, device=dev)
            strides = (ctypes.c_longlong * 8)(*in0.stride(), *in1.stride())
            lib.call("dc_lpips_alex_keep", in0.data_ptr(), in1.data_ptr(), strides, n, h, w, int(normalize), wts.data_ptr(),
                     keep.data_ptr(), out.data_ptr(), stream)
        ctx.keep, ctx.model, ctx.normalize, ctx.size = keep, model, int(normalize), (n, h, w)
        return out.view(6, n).float()

    @staticmethod
    @once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad):
        n, h, w = ctx.size
        keep = ctx.keep
        dev = keep.device
        sides = int(ctx.needs_input_grad[0]) | int(ctx.needs_input_grad[1]) << 1
        if not sides:
            return None, None, None, None
        grad = grad.to(torch.float32)
        g = (grad[:5] + grad[5:6]).contiguous()              # per (layer, pair): the layer term's own gradient + the value's
        wts, dwts = ctx.model._weights(dev), ctx.model._dgrad_weights(dev)
        l = lib.load()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            ws = torch.empty(l.dc_lpips_train_ws_bytes(n, h, w, sides), dtype=torch.uint8, device=dev)
            d0 = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev) if sides & 1 else None
            d1 = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev) if sides & 2 else None
            lib.call("dc_lpips_alex_backward", keep.data_ptr(), g.data_ptr(), n, h, w, ctx.normalize, sides, wts.data_ptr(),
                     dwts.data_ptr(), ws.data_ptr(), d0.data_ptr() if d0 is not None else None,
                     d1.data_ptr() if d1 is not None else None, stream)
        return d0, d1, None, None


class NormFixLPIPS(LPIPS):
    """controlnet/lpips_loss.py's `NormFixLPIPS(net='alex', lpips=True)` as a loss: call surface of the reference module,
    `model(in0, in1, retPerLayer=False, normalize=False)` -> fp32 [N,1,1,1] (and the list of five per-layer [N,1,1,1]), built on
    `metrics.LPIPS(normfix=True)` (its rules, weights and `from_state_dict` / `load_state_dict` / `.to(device)`).

    With grad mode on and an operand that requires grad the call goes through an autograd function: the forward convolutions run
    once and the five post-ReLU maps of that pass stay in a buffer for the backward; gradients are computed only for the operands
    that ask (N images, not 2N, when `in1` is the ground truth).  The value has the bits of the no-grad value.  Operands of the
    gradient path are floating NCHW device tensors with any strides, read in place; other float dtypes are converted inside the
    graph, so the gradient comes back in the operand's dtype and shape.  `normalize=True` contributes its factor 2 to the
    gradient, the scaling layer 1 / scale_c.  Without a gradient to compute (uint8 frames included, which are never
    differentiable) the call is `metrics.LPIPS`'s, unchanged.

    `lpips=False` is the reference's unweighted form (lin weights of one).  `train()` and `eval()` return self: the network is
    always in eval mode and its weights are frozen.  spatial=True, other nets and other versions are not implemented."""

    def __init__(self, net="alex", lpips=True, spatial=False, version="0.1"):
        if spatial:
            raise NotImplementedError("NormFixLPIPS spatial=True is not implemented")
        super().__init__(net=net, version=version, normfix=True)
        self.lpips = bool(lpips)
        self.dgrad_packed = None
        self._dgrad_on_device = {}

    _WHAT, _FROM = "NormFixLPIPS", "NormFixLPIPS.from_state_dict"

    def load_state_dict(self, state_dict, lin_state_dict=None):
        sd = dict(state_dict)
        if lin_state_dict is not None:
            sd.update(lin_state_dict)
        if not self.lpips:
            for l, co in enumerate(LPIPS_CHANNELS):
                sd[f"lin{l}.model.1.weight"] = torch.ones(1, co, 1, 1)
        dgrad = pack_lpips_dgrad_weights(sd)
        want = lib.load().dc_lpips_dgrad_weight_floats()
        if dgrad.numel() != want:
            raise RuntimeError(f"packed NormFixLPIPS data-gradient weights hold {dgrad.numel()} floats, the library expects {want}")
        super().load_state_dict(sd)
        self.dgrad_packed = dgrad
        self._dgrad_on_device = {}
        return self

    def to(self, device):
        super().to(device)
        self._dgrad_weights(torch.device(device))
        return self

    def _dgrad_weights(self, device):
        self._weights(device)                                # raises when nothing is loaded
        device = self._device(device)
        w = self._dgrad_on_device.get(device)
        if w is None:
            w = self._dgrad_on_device[device] = self.dgrad_packed.to(device)
        return w

    def train(self, mode=True):
        return self

    def eval(self):
        return self

    def __call__(self, in0, in1, retPerLayer=False, normalize=False):
        if not (torch.is_grad_enabled() and (in0.requires_grad or in1.requires_grad)):
            return super().__call__(in0, in1, retPerLayer=retPerLayer, normalize=normalize)
        X, Y = _check_pair(in0, in1)
        (n, c, h, w), _ = _nchw(X)
        self._check_image(c, h, w)
        _need_device(X, "NormFixLPIPS")
        _need_device(Y, "NormFixLPIPS")
        if X.device != Y.device:
            raise ValueError("X and Y must live on the same device")
        self._dgrad_weights(X.device)
        res = _LpipsKeepFunction.apply(X.float(), Y.float(), self, bool(normalize))
        val = res[5].reshape(n, 1, 1, 1)
        if retPerLayer:
            return val, [res[l].reshape(n, 1, 1, 1) for l in range(5)]
        return val

    forward = __call__


_REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}


class _SobelFunction(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, pred, target, reduction):
        n, c, h, w = pred.shape
        dev = pred.device
        l = lib.load()
        strides = (ctypes.c_longlong * 8)(*pred.stride(), *target.stride())
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            if reduction == 0:
                out = torch.empty((n, c, h, w), dtype=torch.float32, device=dev)
                lib.call("dc_sobel_edge_loss", pred.data_ptr(), target.data_ptr(), strides, n, c, h, w, 0, None, out.data_ptr(), None,
                         stream)
            else:
                ws = torch.empty(l.dc_sobel_edge_ws_bytes(n, c, h, w), dtype=torch.uint8, device=dev)
                acc = torch.empty(1, dtype=torch.float64, device=dev)
                lib.call("dc_sobel_edge_loss", pred.data_ptr(), target.data_ptr(), strides, n, c, h, w, reduction, ws.data_ptr(), None,
                         acc.data_ptr(), stream)
                out = acc.float().reshape(())
        ctx.save_for_backward(pred, target)
        ctx.reduction = reduction
        return out

    @staticmethod
    @once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, gout):
        pred, target = ctx.saved_tensors
        n, c, h, w = pred.shape
        dev = pred.device
        gout = gout.to(torch.float32).contiguous()
        scale = 1.0 / (n * c * h * w) if ctx.reduction == 1 else 1.0
        strides = (ctypes.c_longlong * 8)(*pred.stride(), *target.stride())
        grads = [None, None]
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            for side in (0, 1):
                if ctx.needs_input_grad[side]:
                    grads[side] = torch.empty((n, c, h, w), dtype=torch.float32, device=dev)
                    lib.call("dc_sobel_edge_grad", pred.data_ptr(), target.data_ptr(), strides, n, c, h, w, side, gout.data_ptr(),
                             int(ctx.reduction == 0), scale, grads[side].data_ptr(), stream)
        return grads[0], grads[1], None


class SobelEdgeLoss:
    """controlnet/edge_loss.py's `SobelEdgeLoss(reduction='mean')`: operands in [-1, 1] are mapped to [0, 1], per-channel Sobel x
    and y with zero padding 1, e = sqrt(gx^2 + gy^2 + 1e-6) and `l1_loss(e(pred), e(target), reduction)` with 'mean' | 'sum' |
    'none'.  Floating [N,C,H,W] device tensors of one shape with any strides (read in place), any C, H and W >= 1; the result is
    fp32.  The forward is one fused launch (plus a fixed-order fp64 sum of the per-workgroup partials), the backward one gather
    launch per operand that requires grad, with sign(0) = 0 as torch's L1 backward has it."""

    def __init__(self, reduction="mean"):
        if reduction not in _REDUCTIONS:
            raise ValueError(f"SobelEdgeLoss: reduction {reduction!r} is not one of {tuple(_REDUCTIONS)}")
        self.reduction = reduction

    def to(self, device):
        return self

    def train(self, mode=True):
        return self

    def eval(self):
        return self

    def __call__(self, pred, target):
        if pred.shape != target.shape or pred.dim() != 4:
            raise ValueError(f"SobelEdgeLoss takes two [N,C,H,W] tensors of one shape, got {tuple(pred.shape)} and {tuple(target.shape)}")
        if not (pred.dtype.is_floating_point and target.dtype.is_floating_point):
            raise ValueError(f"SobelEdgeLoss takes floating point tensors, got {pred.dtype} and {target.dtype}")
        if 0 in pred.shape:
            raise ValueError(f"SobelEdgeLoss: empty operand {tuple(pred.shape)}")
        _need_device(pred, "SobelEdgeLoss")
        _need_device(target, "SobelEdgeLoss")
        if pred.device != target.device:
            raise ValueError("pred and target must live on the same device")
        return _SobelFunction.apply(pred.float(), target.float(), _REDUCTIONS[self.reduction])

    forward = __call__
