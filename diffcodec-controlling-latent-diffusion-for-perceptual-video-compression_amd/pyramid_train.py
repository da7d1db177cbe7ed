"""The flow-warped control pyramid (`Bi_Dir_FeatureExtractor`, controlnet/extractors.py:209-316) as a trainable module, forward and
backward in HIP:

    from diffcodec_amd.pyramid_train import BiDirFeatureExtractor, warp_fuse

`warp_fuse` is one pyramid level after its convolutions (extractors.py:293-310 with control_utils.py:49-72 inlined): two 'soft'
splats, the (1 - occ) multiply, clamp(conf, min=0), conf / (sum + 1e-6), the weighted sum and the hole fill, as ONE autograd
operator.  Its forward is the inference launches unchanged (`ops.splat_soft` twice, `ops.fuse_warped`), so the output has their
bits; its backward is csrc/pyramid_grad.hip (include/diffcodec_pyramid_hip.h): one target-side launch that writes per-pixel planes
only and one source-side launch per warp, no tensor of C channels in between.  Gradients go to the two feature maps and the two
metrics; flows and occlusion masks are data in this extractor (`softsplat.softsplat` differentiates a flow).  Exact fp32 with a
fixed summation order and no float atomics: bitwise reproducible, an image's gradients independent of its position in the batch,
every launch only enqueues on the current stream (graph-capturable).  There is no double backward and no CPU path.

`BiDirFeatureExtractor` is the extractor on `train.Conv3x3` and `warp_fuse`, with the reference's parameter names, so the
`feature_extractor.*` slice of a checkpoint loads with `load_state_dict`; `from_inference` wraps the tensors of a live
`controlnet.BiDirFeatureExtractor`, so an optimiser step is what the next decode reads."""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import lib, ops
from .train import Conv3x3

F32 = torch.float32
INJECT_CHANNELS = (320, 320, 640, 1280)


def _need_device(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: the operand is on device '{t.device}'; the pyramid kernels run on the GPU only (there is no CPU path)")


def _plane(shape, device):
    """One per-pixel intermediate or output of the backward ([N, 1, H, W]; any contents, every element is written).  One function
    so that the tests can hand out guarded buffers."""
    return torch.empty(shape, device=device, dtype=F32)


def _like(t):
    """A feature-map gradient (every element is written); see _plane."""
    return torch.empty_like(t)


class _WarpFuseFunction(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, first, last, metric_f, metric_b, flow_f, flow_b, occ_f, occ_b):
        first, last, metric_f, metric_b, flow_f, flow_b, occ_f, occ_b = (
            t.to(F32).contiguous() for t in (first, last, metric_f, metric_b, flow_f, flow_b, occ_f, occ_b))
        with torch.cuda.device(first.device):
            wf = ops.splat_soft(first, flow_f, metric_f, mask=occ_f)
            wl = ops.splat_soft(last, flow_b, metric_b, mask=occ_b)
            fused = ops.fuse_warped(wf, wl, metric_f, metric_b, occ_f, occ_b)
        ctx.save_for_backward(first, last, metric_f, metric_b, flow_f, flow_b, occ_f, occ_b, wf, wl)
        return fused

    @staticmethod
    @once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        first, last, metric_f, metric_b, flow_f, flow_b, occ_f, occ_b, wf, wl = ctx.saved_tensors
        need_x = (ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        need_m = (ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        out = [None] * 8
        if not (any(need_x) or any(need_m)):
            return tuple(out)
        n, c, h, w = first.shape
        dev = first.device
        g = g.to(F32).contiguous()
        sides = ((first, metric_f, flow_f), (last, metric_b, flow_b))
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            e, den, coef, gden = [None, None], [None, None], [None, None], [None, None]
            for s, (_, metric, flow) in enumerate(sides):
                if not (need_x[s] or need_m[s]):
                    continue                                               # nothing of this side is launched
                e[s], den[s] = _plane(metric.shape, dev), _plane(metric.shape, dev)
                coef[s], gden[s] = _plane(metric.shape, dev), _plane(metric.shape, dev)
                lib.call("dc_pyramid_exp_f32", metric.data_ptr(), e[s].data_ptr(), metric.numel(), stream)
                ws = ops._splat_ws(n, h, w, dev)
                # the normaliser sum_s e b, recomputed: it only linearises, so its bits need not be those inside the forward's gather
                lib.call("dc_splat_sum_f32", e[s].data_ptr(), flow.data_ptr(), den[s].data_ptr(), ws.data_ptr(), n, 1, h, w, stream)
            g_conf = (_plane(metric_f.shape, dev), _plane(metric_b.shape, dev))
            lib.call("dc_pyramid_fuse_grad_f32", g.data_ptr(), wf.data_ptr(), wl.data_ptr(), metric_f.data_ptr(), metric_b.data_ptr(),
                     occ_f.data_ptr(), occ_b.data_ptr(), ops._ptr(den[0]), ops._ptr(den[1]), g_conf[0].data_ptr(), g_conf[1].data_ptr(),
                     ops._ptr(coef[0]), ops._ptr(gden[0]), ops._ptr(coef[1]), ops._ptr(gden[1]), n, c, h, w, stream)
            for s, (x, metric, flow) in enumerate(sides):
                if not (need_x[s] or need_m[s]):
                    continue
                gx = _like(x) if need_x[s] else None
                gm = _plane(metric.shape, dev) if need_m[s] else None
                lib.call("dc_pyramid_warp_grad_f32", x.data_ptr(), e[s].data_ptr(), flow.data_ptr(), g.data_ptr(), coef[s].data_ptr(),
                         gden[s].data_ptr(), g_conf[s].data_ptr(), ops._ptr(gx), ops._ptr(gm), n, c, h, w, stream)
                out[s], out[2 + s] = gx, gm
        return tuple(out)


def warp_fuse(first, last, metric_f, metric_b, flow_f, flow_b, occ_f, occ_b):
    """One level of the pyramid after its convolutions -> fused [N, C, H, W] fp32, with a backward to first, last, metric_f and
    metric_b.  first, last: [N, C, H, W]; metric_*: [N, 1, H, W] (the splat's exponent and the fusion's confidence); flow_*:
    [N, 2, H, W]; occ_*: [N, 1, H, W] of zeros and ones.  The output has the bits of `ops.splat_soft` twice and `ops.fuse_warped`."""
    names = ("first", "last", "metric_f", "metric_b", "flow_f", "flow_b", "occ_f", "occ_b")
    ts = (first, last, metric_f, metric_b, flow_f, flow_b, occ_f, occ_b)
    if first.dim() != 4 or last.shape != first.shape:
        raise ValueError(f"warp_fuse: first {tuple(first.shape)} and last {tuple(last.shape)} are not two [N, C, H, W] maps of one shape")
    n, _, h, w = first.shape
    for t, nm in zip(ts[2:], names[2:]):
        want = (n, 2 if nm.startswith("flow") else 1, h, w)
        if tuple(t.shape) != want:
            raise ValueError(f"warp_fuse: {nm} {tuple(t.shape)}, expected {want}")
    if torch.is_grad_enabled():
        for t, nm in zip(ts[4:], names[4:]):
            if t.requires_grad:
                raise ValueError(f"warp_fuse: {nm} requires grad, but flows and occlusion masks are data in this extractor; "
                                 "differentiate a flow with diffcodec_amd.softsplat.softsplat")
    for t, nm in zip(ts, names):
        _need_device(t, "warp_fuse " + nm)
    return _WarpFuseFunction.apply(*ts)


class _Warper(nn.Module):
    """FeatureWarperSoftsplat's parameters (control_utils.py:41-47): metric_net.0 (C -> 64, SiLU) and metric_net.2 (64 -> 1)"""

    def __init__(self, conv0, conv2):
        super().__init__()
        self.metric_net = nn.Sequential(conv0, nn.Identity(), conv2)

    def forward(self, feat):
        return self.metric_net(feat)


def _pre(convs):
    """[conv] * 5 -> Sequential with the convolutions at 0, 2, 4, 6, 8 (the reference's SiLU slots hold nothing: SiLU is fused)"""
    mods = []
    for cv in convs:
        mods += [cv, nn.Identity()]
    return nn.Sequential(*mods[:-1])


class BiDirFeatureExtractor(nn.Module):
    """Bi_Dir_FeatureExtractor (extractors.py:209-316), trainable.  `forward(cond [B,6,H,W], flow [B,4,H,W])` returns the four levels
    with the bits of `controlnet.BiDirFeatureExtractor` on the same weights (levels H/8 ... H/64, the slot swap of :266-267 kept)."""

    PRE_STRIDES = (1, 2, 1, 2, 1)

    def __init__(self, inject_channels=INJECT_CHANNELS):
        super().__init__()
        inject = tuple(int(c) for c in inject_channels)
        if len(inject) != 4 or any(c < 2 for c in inject):
            raise ValueError(f"BiDirFeatureExtractor: inject_channels {inject_channels} (four widths of at least 2)")
        half = [c // 2 for c in inject]
        pre_ch = (3, 16, 32, 32, 64, 64)
        convs = {}
        for side in ("first", "last"):
            convs["pre_" + side] = [Conv3x3(pre_ch[i], pre_ch[i + 1], self.PRE_STRIDES[i], True) for i in range(5)]
            convs["ext_" + side] = [Conv3x3(([64] + half)[i], half[i], 2, True) for i in range(4)]
        convs["metric"] = [(Conv3x3(half[i], 64, 1, True), Conv3x3(64, 1, 1, False)) for i in range(4)]
        convs["zero"] = [Conv3x3(half[i], inject[i], 1, False) for i in range(4)]
        for z in convs["zero"]:                                            # zero_module (control_utils.py:6-9)
            nn.init.zeros_(z.weight)
            nn.init.zeros_(z.bias)
        self._assemble(convs)

    def _assemble(self, convs):
        self.first_pre_extractor = _pre(convs["pre_first"])
        self.last_pre_extractor = _pre(convs["pre_last"])
        self.wrapper = nn.ModuleList([_Warper(a, b) for a, b in convs["metric"]])
        self.extractors_first = nn.ModuleList([nn.Sequential(cv) for cv in convs["ext_first"]])
        self.extractors_last = nn.ModuleList([nn.Sequential(cv) for cv in convs["ext_last"]])
        self.zero_convs = nn.ModuleList(convs["zero"])

    @classmethod
    def from_inference(cls, ext):
        """Wrap the `PackedConvF32` tensors of a live `controlnet.BiDirFeatureExtractor` as parameters that share their storage."""
        m = cls.__new__(cls)
        nn.Module.__init__(m)
        convs = {}
        for side in ("first", "last"):
            convs["pre_" + side] = [Conv3x3.from_packed(pc, cls.PRE_STRIDES[i], True) for i, pc in enumerate(ext.pre[side])]
            convs["ext_" + side] = [Conv3x3.from_packed(pc, 2, True) for pc in ext.ext[side]]
        convs["metric"] = [(Conv3x3.from_packed(a, 1, True), Conv3x3.from_packed(b, 1, False)) for a, b in ext.metric]
        convs["zero"] = [Conv3x3.from_packed(pc, 1, False) for pc in ext.zero]
        m._assemble(convs)
        return m

    def forward(self, cond, flow, return_aux=False):
        """cond [B,6,H,W], flow [B,4,H,W] on the GPU -> the 4 levels, NCHW fp32; with return_aux also a list of
        dict(flow_f, flow_b, occ_f, occ_b) per level."""
        if cond.dim() != 4 or cond.shape[1] != 6 or flow.dim() != 4 or flow.shape[1] != 4 or flow.shape[0] != cond.shape[0] or \
                flow.shape[2:] != cond.shape[2:]:
            raise ValueError(f"BiDirFeatureExtractor: cond {tuple(cond.shape)} and flow {tuple(flow.shape)} are not [B,6,H,W] and [B,4,H,W]")
        if torch.is_grad_enabled() and flow.requires_grad:
            raise ValueError("BiDirFeatureExtractor: flow requires grad, but flows are data in this extractor; differentiate a flow "
                             "with diffcodec_amd.softsplat.softsplat")
        _need_device(cond, "BiDirFeatureExtractor cond")
        _need_device(flow, "BiDirFeatureExtractor flow")
        cond = cond.to(F32).contiguous()
        flow = flow.detach().to(F32).contiguous()
        h = cond.shape[-2]
        f = self.first_pre_extractor(cond[:, 3:])                          # extractors.py:266-267 (slot swap kept)
        l = self.last_pre_extractor(cond[:, :3])
        outs, aux = [], []
        for idx, r in enumerate((h // 8, h // 16, h // 32, h // 64)):
            f = self.extractors_first[idx](f)
            l = self.extractors_last[idx](l)
            with torch.no_grad(), torch.autocast(device_type="cuda", enabled=False), torch.cuda.device(cond.device):
                flow_f = ops.flow_resize_normalize(flow[:, :2], r, r)      # :286-287
                flow_b = ops.flow_resize_normalize(flow[:, 2:], r, r)
                occ_f = ops.occlusion_mask(flow_f, flow_b)                 # :290-291
                occ_b = ops.occlusion_mask(flow_b, flow_f)
            fused = warp_fuse(f, l, self.wrapper[idx](f), self.wrapper[idx](l), flow_f, flow_b, occ_f, occ_b)
            outs.append(self.zero_convs[idx](fused))
            aux.append(dict(flow_f=flow_f, flow_b=flow_b, occ_f=occ_f, occ_b=occ_b))
        return (outs, aux) if return_aux else outs
