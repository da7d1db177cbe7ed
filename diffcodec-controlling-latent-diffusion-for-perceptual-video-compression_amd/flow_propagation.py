"""Sparse guide flow -> dense flow on the GPU: the reference's Conditional Motion Propagation network (cmp/models/modules/cmp.py
`CMP.forward`, cmp/utils/visualize_utils.py `Fuser.convert_flow`, cmp/models/cmp.py `CMP.eval`'s upsample) on csrc/cmp.hip.

    model = HipCMP.from_state_dict(torch.load(checkpoint), config["model"]["module"])
    logits = model(image, sparse)            # [N, 2 nbins, h, w]                      CMP.forward
    flow = model.flow(image, sparse)         # [N, 2, H, W] in pixels                  CMP.eval without its loss
    source = PropagatedFlowSource(DirectorySource(...), model, stride=32)                  # 'grid' guide points
    source = PropagatedFlowSource(DirectorySource(...), model, stride=80, nms_ks=15)      # 'grid' and 'watershed'
    decode_clip(pipe, source, ..., score=True)

Inference only, eval mode, exact fp32: BatchNorm is folded on the host in fp64 to one fma per channel.  No weights ship with the
package and nothing is downloaded: the caller brings the checkpoint.  There is no CPU path: without the built library or a GPU
the calls raise."""
import ctypes

import torch

from . import lib
from .guide_points import sample_watershed, stride_from_bg_ratio, watershed_points  # noqa: F401  (the other guide samplers)
from .metrics import fold_bn

DATA_MEAN = (123.675, 116.28, 103.53)       # data_mean / data_div of every reference config (RGB, 0..255 scale)
DATA_DIV = (58.395, 57.12, 57.375)
BN_EPS = 1e-5
_RESNET50 = (("layer1", 64, 3, 1, 1), ("layer2", 128, 4, 2, 1), ("layer3", 256, 6, 1, 2), ("layer4", 512, 3, 1, 4))
_DECODERS = {"MotionDecoderSkipLayer": 3, "MotionDecoderPlain": 2}          # convolutions per decoder branch


def conv_table(config):
    """[(name, conv key prefix, BatchNorm key prefix or None, Cin, Cout, k)] of the architecture `config` names, in forward
    order.  Raises NotImplementedError naming an architecture this package does not build."""
    enc, sp, dec = config.get("image_encoder"), config.get("sparse_encoder"), config.get("flow_decoder")
    if enc != "resnet50":
        raise NotImplementedError(f"image_encoder {enc!r}: only 'resnet50' is built")
    if sp != "shallownet8x":
        raise NotImplementedError(f"sparse_encoder {sp!r}: only 'shallownet8x' is built")
    if dec not in _DECODERS:
        raise NotImplementedError(f"flow_decoder {dec!r}: only {sorted(_DECODERS)} are built")
    if bool(config.get("skip_layer", dec == "MotionDecoderSkipLayer")) != (dec == "MotionDecoderSkipLayer"):
        raise ValueError("skip_layer goes with flow_decoder MotionDecoderSkipLayer and with no other")
    e_dim, s_dim, out = int(config.get("img_enc_dim", 256)), int(config.get("sparse_enc_dim", 16)), int(config["output_dim"])
    if out != 2 * int(config["nbins"]):
        raise ValueError(f"output_dim {out} is not 2 * nbins: only the discrete (DiscreteLoss) head is built")
    t = [("stem", "image_encoder.conv1", "image_encoder.bn1", 3, 64, 7)]
    cin = 64
    for layer, planes, blocks, _, _ in _RESNET50:
        for b in range(blocks):
            p = f"image_encoder.{layer}.{b}"
            if b == 0:
                t.append((p + ".downsample", p + ".downsample.0", p + ".downsample.1", cin, planes * 4, 1))
            t.append((p + ".conv1", p + ".conv1", p + ".bn1", cin, planes, 1))
            t.append((p + ".conv2", p + ".conv2", p + ".bn2", planes, planes, 3))
            t.append((p + ".conv3", p + ".conv3", p + ".bn3", planes, planes * 4, 1))
            cin = planes * 4
    t.append(("conv5", "image_encoder.conv5", None, 2048, e_dim, 1))
    t.append(("sparse1", "flow_encoder.features.0", "flow_encoder.features.1", 4, 16, 5))
    t.append(("sparse2", "flow_encoder.features.4", "flow_encoder.features.5", 16, s_dim, 3))
    d_in = e_dim + s_dim
    depth = _DECODERS[dec]
    combo = [1, 2, 4, 8] if dec == "MotionDecoderSkipLayer" else [int(c) for c in config.get("decoder_combo", [1, 2, 4])]
    if any(c not in (1, 2, 4, 8) for c in combo) or not combo:
        raise ValueError(f"invalid decoder_combo {combo}")
    for c in combo:
        first = 0 if c == 1 else 1                                        # the pooled branches start with their MaxPool2d
        for i in range(depth):
            p = f"flow_decoder.decoder{c}"
            t.append((f"decoder{c}.{i}", f"{p}.{first + 3 * i}", f"{p}.{first + 3 * i + 1}", d_in if i == 0 else 128, 128, 3))
    if dec == "MotionDecoderSkipLayer":
        for name, ci, co in (("fusion8", 512, 256), ("skipconv4", 256, 128), ("fusion4", 384, 128), ("skipconv2", 64, 32),
                             ("fusion2", 160, 64)):
            t.append((name, f"flow_decoder.{name}.0", f"flow_decoder.{name}.1", ci, co, 3))
        t.append(("head", "flow_decoder.head", None, 64, out, 1))
    else:
        t.append(("head", "flow_decoder.head", None, 128 * len(combo), out, 1))
    return t


def _strip(state_dict):
    if "state_dict" in state_dict and not torch.is_tensor(state_dict["state_dict"]):
        state_dict = state_dict["state_dict"]
    out = {}
    for k, v in state_dict.items():
        while k.startswith("module."):                                    # FixModule / DistModule wrap the network once or twice
            k = k[len("module."):]
        if not k.endswith("num_batches_tracked"):
            out[k] = v
    return out


def fold_and_pack(weight, bias, bn, eps=BN_EPS):
    """One convolution as dc_cmp_conv's `packed` (fp32, [rows + 2][CoP]), the fold done in fp64:
    s = gamma / sqrt(var + eps), t = beta - mean s + bias s; without BatchNorm s = 1, t = bias."""
    w = weight.detach().double().cpu()
    co, ci, k, _ = w.shape
    b = torch.zeros(co, dtype=torch.float64) if bias is None else bias.detach().double().cpu()
    if bn is None:
        s, t = torch.ones(co, dtype=torch.float64), b
    else:
        s, t = fold_bn(*bn, eps)
        t = t + b * s
    K = ci * k * k
    rows, cop = (K + 31) // 32 * 32, (co + 31) // 32 * 32
    m = torch.zeros(rows + 2, cop, dtype=torch.float64)
    m[:K, :co] = w.reshape(co, K).t()
    m[rows, :co] = s
    m[rows + 1, :co] = t
    return m.float().contiguous()


def stage_sizes(config, H, W):
    """((h2, w2), (h4, w4), (h8, w8)) of an H x W image, after the checks the reference's own torch.cat and max-pools make."""
    def enc(v):
        a = (v - 1) // 2 + 1
        b = (a - 1) // 2 + 1
        return a, b, (b - 1) // 2 + 1

    def sparse(v):
        return ((v - 1) // 2 + 1) // 2 // 2

    hs, ws = enc(int(H)), enc(int(W))
    for axis, v, e in (("H", H, hs[2]), ("W", W, ws[2])):
        if v < 1 or sparse(v) != e:
            raise ValueError(f"{axis} = {v}: the image encoder gives {e} rows at 1/8 and the sparse encoder {sparse(v) if v > 0 else 0}; "
                             "their concatenation fails (only sizes 8 m and 8 m - 1 agree)")
    pool = 8 if config["flow_decoder"] == "MotionDecoderSkipLayer" else max(int(c) for c in config.get("decoder_combo", [1, 2, 4]))
    if hs[2] < pool or ws[2] < pool:
        raise ValueError(f"{H} x {W}: the 1/8 map is {hs[2]} x {ws[2]}, smaller than the decoder's {pool} x {pool} max-pool")
    return tuple(zip(hs, ws))


def _i64(vals):
    return (ctypes.c_longlong * len(vals))(*[int(v) for v in vals])


def _stream():
    return torch.cuda.current_stream().cuda_stream


class HipCMP:
    """The CMP network on the device.  `image`: uint8 [N,H,W,3] (any strides: a cropped view is an operand; normalised on load
    with the configs' data_mean / data_div) or already normalised fp32 [N,3,H,W]; `sparse`: fp32 [N,4,H,W] (guide flow at the
    guide points and zero elsewhere; the mask twice)."""

    def __init__(self, packed, config, device):
        self.config = dict(config)
        table = conv_table(config)
        self.table = {name: (cin, cout, k) for name, _, _, cin, cout, k in table}
        self.device = torch.device(device)
        # dc_cmp_forward's `weights`: every block back to back in forward order; `packed` holds views of it
        self.weights = torch.cat([packed[name].reshape(-1) for name, *_ in table]).to(self.device)
        self.packed, at = {}, 0
        for name, *_ in table:
            n = packed[name].numel()
            self.packed[name] = self.weights[at:at + n].view(packed[name].shape)
            at += n
        self.arch = 0 if config["flow_decoder"] == "MotionDecoderSkipLayer" else 1
        self.skip = config["flow_decoder"] == "MotionDecoderSkipLayer"
        self.combo = [1, 2, 4, 8] if self.skip else [int(c) for c in config.get("decoder_combo", [1, 2, 4])]
        self.depth = _DECODERS[config["flow_decoder"]]
        self.nbins, self.fmax = int(config["nbins"]), float(config["fmax"])
        self.e_dim, self.s_dim = int(config.get("img_enc_dim", 256)), int(config.get("sparse_enc_dim", 16))
        self.mean_div = (ctypes.c_float * 6)(*DATA_MEAN, *DATA_DIV)
        self._ws_key, self._ws, self._weights_checked = None, None, False
        if (self.e_dim, self.s_dim) != (256, 16) or (not self.skip and self.combo != [1, 2, 4]):
            raise NotImplementedError(f"img_enc_dim {self.e_dim}, sparse_enc_dim {self.s_dim}, decoder_combo {self.combo}: the device "
                                      "network is built for 256, 16 and [1, 2, 4]")
        if 2 * self.nbins > 224:
            raise NotImplementedError(f"nbins {self.nbins}: the fused head holds at most 112 bins per axis")

    @classmethod
    def from_state_dict(cls, state_dict, config, device="cuda"):
        sd = _strip(state_dict)
        packed = {}
        for name, ck, bk, cin, cout, k in conv_table(config):
            keys = [ck + ".weight"] + ([bk + s for s in (".weight", ".bias", ".running_mean", ".running_var")] if bk else [])
            has_bias = bk is None or name.startswith(("sparse", "decoder", "fusion", "skipconv"))
            if has_bias:
                keys.append(ck + ".bias")
            for key in keys:
                if key not in sd:
                    raise KeyError(f"state dict has no {key!r}")
            w = sd[ck + ".weight"]
            if tuple(w.shape) != (cout, cin, k, k):
                raise ValueError(f"{ck}.weight has shape {tuple(w.shape)}, the architecture needs {(cout, cin, k, k)}")
            for key in keys[1:]:
                if tuple(sd[key].shape) != (cout,):
                    raise ValueError(f"{key} has shape {tuple(sd[key].shape)}, the architecture needs {(cout,)}")
            bn = tuple(sd[bk + s] for s in (".weight", ".bias", ".running_mean", ".running_var")) if bk else None
            packed[name] = fold_and_pack(w, sd[ck + ".bias"] if has_bias else None, bn)
        return cls(packed, config, device)

    # ------------------------------------------------------------------------------------------ stages
    def _conv(self, name, x, stride=1, dilation=1, relu=True, residual=None, out=None, c_off=0):
        cin, cout, k = self.table[name]
        u8 = x.dtype == torch.uint8
        if u8:                                                            # [N,H,W,3] -> strides in (n, c, h, w) order
            N, H, W, _ = x.shape
            strides = (x.stride(0), x.stride(3), x.stride(1), x.stride(2))
        else:
            N, _, H, W = x.shape
            strides = x.stride()
        pad = dilation * (k - 1) // 2
        Ho = (H + 2 * pad - dilation * (k - 1) - 1) // stride + 1
        Wo = (W + 2 * pad - dilation * (k - 1) - 1) // stride + 1
        if out is None:
            out = torch.empty(N, cout, Ho, Wo, dtype=torch.float32, device=x.device)
        assert out.shape[2:] == (Ho, Wo) and out.is_contiguous()
        family = ("stem" if name == "stem" else "sparse" if name.startswith("sparse") else
                  "decoder" if name.startswith(("decoder", "fusion", "skipconv", "head")) else
                  "1x1" if k == 1 else "dilated 3x3" if dilation > 1 else "3x3")
        meta = (family, f"{cin}->{cout} k{k} s{stride} d{dilation} {N}x{H}x{W}", 2.0 * N * cout * Ho * Wo * cin * k * k,
                4.0 * (N * cin * H * W + N * cout * Ho * Wo + cin * cout * k * k))
        lib.call("dc_cmp_conv", x.data_ptr(), int(u8), _i64(strides), self.mean_div, N, cin, H, W, k, stride, dilation,
                 self.packed[name].data_ptr(), cout, None if residual is None else residual.data_ptr(), int(relu), out.data_ptr(),
                 out.shape[1], c_off, _stream(), meta=meta)
        return out

    @staticmethod
    def _maxpool(x, k, stride, pad=0):
        N, C, H, W = x.shape
        out = torch.empty(N, C, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1, dtype=torch.float32, device=x.device)
        lib.call("dc_cmp_maxpool", x.data_ptr(), N * C, H, W, k, stride, pad, out.data_ptr(), _stream())
        return out

    @staticmethod
    def _avgpool(x, out, c_off):
        N, C, H, W = x.shape
        lib.call("dc_cmp_avgpool", x.data_ptr(), N, C, H, W, out.data_ptr(), out.shape[1], c_off, _stream())

    @staticmethod
    def _upsample(x, out, c_off=0):
        N, C, H, W = x.shape
        lib.call("dc_cmp_upsample", x.data_ptr(), N, C, H, W, out.shape[2], out.shape[3], out.data_ptr(), out.shape[1], c_off, _stream())
        return out

    def _convert(self, logits):
        N, _, h, w = logits.shape
        flow = torch.empty(N, 2, h, w, dtype=torch.float32, device=logits.device)
        lib.call("dc_cmp_convert_flow", logits.data_ptr(), N, self.nbins, h, w, self.fmax, flow.data_ptr(), _stream())
        return flow

    # ------------------------------------------------------------------------------------------ the network
    def _check(self, image, sparse):
        if image.dtype == torch.uint8:
            if image.dim() != 4 or image.shape[3] != 3:
                raise ValueError(f"a uint8 image is [N,H,W,3], got {tuple(image.shape)}")
            N, H, W = image.shape[:3]
        elif image.dtype == torch.float32:
            if image.dim() != 4 or image.shape[1] != 3:
                raise ValueError(f"an fp32 image is normalised [N,3,H,W], got {tuple(image.shape)}")
            N, H, W = image.shape[0], image.shape[2], image.shape[3]
        else:
            raise ValueError(f"image is uint8 [N,H,W,3] or fp32 [N,3,H,W], got {image.dtype}")
        if sparse.dtype != torch.float32 or tuple(sparse.shape) != (N, 4, H, W):
            raise ValueError(f"sparse is fp32 {(N, 4, H, W)}, got {sparse.dtype} {tuple(sparse.shape)}")
        if image.device.type != "cuda" or sparse.device != image.device:
            raise RuntimeError("HipCMP runs on the GPU only: image and sparse must be on one cuda device")
        return N, H, W, stage_sizes(self.config, H, W)

    def staged_endpoints(self, image, sparse, upsampled=True):
        """`endpoints` with the chain driven from here, one stage launcher per call and one tensor per stage: the same kernels in
        the same order, so the same bits.  For per-launch timing (tools/bench_cmp.py) and as a cross-check of the C chain."""
        N, H, W, ((h2, w2), (h4, w4), (h8, w8)) = self._check(image, sparse)
        dev = image.device
        sparse = sparse.contiguous()
        new = lambda c, h, w: torch.empty(N, c, h, w, dtype=torch.float32, device=dev)
        ep = {}
        d_in = self.e_dim + self.s_dim
        enc = new(d_in, h8, w8)                                          # torch.cat((img_enc, sparse_enc), 1), never copied

        x = self._conv("sparse1", sparse, stride=2)
        x = self._conv("sparse2", self._maxpool(x, 2, 2))
        self._avgpool(x, enc, self.e_dim)

        stem = self._conv("stem", image, stride=2)
        x = self._maxpool(stem, 3, 2, 1)
        for layer, _, blocks, stride, dil in _RESNET50:
            for b in range(blocks):
                p = f"image_encoder.{layer}.{b}"
                res = self._conv(p + ".downsample", x, stride=stride, relu=False) if b == 0 else x
                y = self._conv(p + ".conv1", x)
                y = self._conv(p + ".conv2", y, stride=stride if b == 0 else 1, dilation=dil)
                x = self._conv(p + ".conv3", y, residual=res)
            if layer == "layer1":
                layer1 = x
        self._conv("conv5", x, relu=False, out=enc, c_off=0)
        ep["sparse_enc"], ep["img_enc"], ep["skip2"], ep["skip4"] = enc[:, self.e_dim:], enc[:, :self.e_dim], stem, layer1

        cat = new(128 * len(self.combo), h8, w8)
        for i, c in enumerate(self.combo):
            x = enc if c == 1 else self._maxpool(enc, c, c)
            for d in range(self.depth):
                last = d == self.depth - 1
                x = self._conv(f"decoder{c}.{d}", x, out=cat if (last and c == 1) else None, c_off=128 * i if (last and c == 1) else 0)
            if c != 1:
                self._upsample(x, cat, 128 * i)
        if self.skip:
            ep["f8"] = f8 = self._conv("fusion8", cat)
            cat4 = new(384, h4, w4)
            self._upsample(f8, cat4, 0)
            self._conv("skipconv4", layer1, out=cat4, c_off=256)
            ep["f4"] = f4 = self._conv("fusion4", cat4)
            cat2 = new(160, h2, w2)
            self._upsample(f4, cat2, 0)
            self._conv("skipconv2", stem, out=cat2, c_off=128)
            ep["f2"] = f2 = self._conv("fusion2", cat2)
            top = f2
        else:
            ep["cat8"] = top = cat
        ep["logits"] = logits = new(2 * self.nbins, *top.shape[2:])
        ep["flow"] = flow = new(2, *top.shape[2:])
        lib.call("dc_cmp_head", top.data_ptr(), N, top.shape[1], top.shape[2], top.shape[3], self.packed["head"].data_ptr(), self.nbins,
                 self.fmax, logits.data_ptr(), flow.data_ptr(), _stream(),
                 meta=("decoder", f"head {top.shape[1]}->{2 * self.nbins} {N}x{top.shape[2]}x{top.shape[3]}",
                       2.0 * N * top.shape[1] * 2 * self.nbins * top.shape[2] * top.shape[3], 0.0))
        if upsampled:
            ep["flow_up"] = flow if flow.shape[2:] == (H, W) else self._upsample(flow, new(2, H, W))
        return ep

    def convert_flow(self, logits):
        """Fuser.convert_flow on logits [N, 2 nbins, h, w] from elsewhere (the network itself fuses it into the head)."""
        return self._convert(logits.contiguous())

    # ------------------------------------------------------------------------------------------ the C chain
    def _workspace(self, device, N, H, W):
        """dc_cmp_forward's workspace for (device, N, H, W): kept from call to call (a clip asks for one size throughout; one buffer
        is held, so calls on one model are for one stream at a time), allocated afresh while a graph is being captured so that the
        graph owns what it replays into."""
        key = (device, N, H, W)
        if not torch.cuda.is_current_stream_capturing() and self._ws_key == key:
            return self._ws
        nbytes = lib.load().dc_cmp_ws_bytes(self.arch, N, H, W)
        if nbytes < 0:
            raise ValueError(f"dc_cmp_ws_bytes refuses {N} x {H} x {W}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        if not torch.cuda.is_current_stream_capturing():
            self._ws_key, self._ws = key, ws
        return ws

    def _operands(self, image, sparse):
        N, H, W, sizes = self._check(image, sparse)
        if not self._weights_checked:
            if self.weights.numel() != lib.load().dc_cmp_weight_floats(self.arch, self.nbins):
                raise RuntimeError("the packed weights do not have dc_cmp_weight_floats elements")
            self._weights_checked = True
        ws = self._workspace(image.device, N, H, W)
        u8 = image.dtype == torch.uint8
        strides = (image.stride(0), image.stride(3), image.stride(1), image.stride(2)) if u8 else image.stride()
        head = (self.arch, image.data_ptr(), int(u8), _i64(strides), sparse.data_ptr(), N, H, W, self.nbins, self.fmax,
                self.weights.data_ptr(), ws.data_ptr())
        new = lambda c, hw: torch.empty(N, c, hw[0], hw[1], dtype=torch.float32, device=image.device)
        return head, new, (H, W), sizes, (image, sparse, ws)             # the last keeps the operands alive past the enqueue

    def endpoints(self, image, sparse):
        """Every named intermediate as a dict of fp32 tensors: sparse_enc, img_enc, skip2 (the stem map), skip4 (layer1), then
        f8, f4, f2 (SkipLayer) or cat8 (Plain), logits, flow and flow_up [N,2,H,W]."""
        sparse = sparse.contiguous()
        head, new, full, (s2, s4, s8), keep = self._operands(image, sparse)
        ep = dict(sparse_enc=new(16, s8), img_enc=new(256, s8), skip2=new(64, s2), skip4=new(256, s4))
        if self.skip:
            ep.update(f8=new(256, s8), f4=new(128, s4), f2=new(64, s2))
        else:
            ep.update(cat8=new(384, s8))
        maps = (ctypes.c_void_p * len(ep))(*[t.data_ptr() for t in ep.values()])
        top = s2 if self.skip else s8
        ep.update(logits=new(2 * self.nbins, top), flow=new(2, top), flow_up=new(2, full))
        lib.call("dc_cmp_endpoints", *head, maps, ep["logits"].data_ptr(), ep["flow"].data_ptr(), ep["flow_up"].data_ptr(), _stream())
        return ep

    def __call__(self, image, sparse):
        """CMP.forward: the logits [N, 2 nbins, h, w] (h = H/2 for the SkipLayer decoder, H/8 for the Plain one)."""
        sparse = sparse.contiguous()
        head, new, _, (s2, _, s8), keep = self._operands(image, sparse)
        logits = new(2 * self.nbins, s2 if self.skip else s8)
        lib.call("dc_cmp_forward", *head, logits.data_ptr(), None, _stream())
        return logits

    def flow(self, image, sparse):
        """CMP.eval without its loss: the expectation of the two softmaxes, upsampled (align_corners = True) to [N,2,H,W].  The
        logits are never stored."""
        sparse = sparse.contiguous()
        head, new, full, _, keep = self._operands(image, sparse)
        out = new(2, full)
        lib.call("dc_cmp_flow", *head, out.data_ptr(), _stream())
        return out


def sparse_from_points(points, vectors, H, W, device="cuda"):
    """The sparse operand [1,4,H,W] of guide `points` [K,2] (integer (y, x), distinct) carrying `vectors` [K,2] ((u, v) in
    pixels): plain indexing, the seam for whatever on-disk format carries the guide points."""
    points = torch.as_tensor(points, dtype=torch.long, device=device).reshape(-1, 2)
    vectors = torch.as_tensor(vectors, dtype=torch.float32, device=device).reshape(-1, 2)
    if points.shape[0] != vectors.shape[0]:
        raise ValueError(f"{points.shape[0]} points and {vectors.shape[0]} vectors")
    y, x = points[:, 0], points[:, 1]
    if points.numel() and (int(y.min()) < 0 or int(y.max()) >= H or int(x.min()) < 0 or int(x.max()) >= W):
        raise ValueError(f"a guide point lies outside {H} x {W}")
    if torch.unique(y * W + x).numel() != y.numel():
        raise ValueError("guide points must be distinct")
    out = torch.zeros(1, 4, H, W, dtype=torch.float32, device=device)
    out[0, 0, y, x] = vectors[:, 0]
    out[0, 1, y, x] = vectors[:, 1]
    out[0, 2, y, x] = 1.0
    out[0, 3, y, x] = 1.0
    return out


def grid_points(H, W, stride):
    """(ys, xs) of the reference's flow_sampler 'grid' strategy (cmp/utils/data_utils.py) for an H x W flow."""
    y0, x0 = int((H - H // stride * stride) / 2), int((W - W // stride * stride) / 2)
    return list(range(y0, H, stride)), list(range(x0, W, stride))


def sample_grid(flow, stride):
    """Dense flow [N,2,H,W] (fp32, on the GPU) -> the sparse operand [N,4,H,W] holding it at the 'grid' guide points."""
    if flow.dim() != 4 or flow.shape[1] != 2 or flow.dtype != torch.float32:
        raise ValueError(f"flow is fp32 [N,2,H,W], got {flow.dtype} {tuple(flow.shape)}")
    if int(stride) < 1:
        raise ValueError(f"stride {stride}")
    flow = flow.contiguous()
    N, _, H, W = flow.shape
    out = torch.empty(N, 4, H, W, dtype=torch.float32, device=flow.device)
    lib.call("dc_cmp_sparse_grid", flow.data_ptr(), N, H, W, int(stride), out.data_ptr(), _stream())
    return out


def anchors_u8(cond):
    """[B,6,H,W] anchors in [0,1] -> (previous, next) as uint8 [B,H,W,3] views: cond * 255 rounded to nearest and clamped."""
    q = (cond.float() * 255.0).round().clamp(0, 255).to(torch.uint8)
    return q[:, :3].permute(0, 2, 3, 1), q[:, 3:].permute(0, 2, 3, 1)


class PropagatedFlowSource:
    """A clip source whose dense flow is what the decoder can rebuild from the sparse rate point: wraps any source with
    `controls(frame, prev, nxt) -> (cond [B,6,H,W], flow [B,4,H,W])`, keeps `cond`, and replaces flow[:, :2] by the propagation
    of its 'grid' samples (one every `stride` pixels) conditioned on the previous anchor cond[:, :3], and flow[:, 2:] by the
    propagation of its samples conditioned on the next anchor cond[:, 3:].  The model is fed the anchors as uint8 frames
    re-quantised from `cond` (`anchors_u8`: cond * 255, rounded, clamped), which for a source that loaded 8-bit frames are the
    frames' own bytes.  With `nms_ks` the samples are the reference configs' ['grid', 'watershed'] pair (`sample_watershed` with
    that NMS window) instead of the grid alone.  Everything else of the inner source (ground_truth, warp, with_warp, noise, ...)
    passes through."""

    def __init__(self, source, model, stride=32, nms_ks=None):
        self.source, self.model, self.stride = source, model, int(stride)
        self.nms_ks = None if nms_ks is None else int(nms_ks)

    def __getattr__(self, name):                                          # only reached for what this class does not define
        return getattr(self.source, name)

    def controls(self, frame, prev, nxt):
        cond, flow = self.source.controls(frame, prev, nxt)
        a_prev, a_next = anchors_u8(cond)
        B = cond.shape[0]
        flow = flow.float()
        both = torch.cat([flow[:, :2], flow[:, 2:]], 0)
        sparse = sample_grid(both, self.stride) if self.nms_ks is None else sample_watershed(both, self.nms_ks, stride=self.stride)
        dense = self.model.flow(torch.cat([a_prev, a_next], 0), sparse)  # one batch: the result does not depend on the batching
        return cond, torch.cat([dense[:B], dense[B:]], 1).to(flow.dtype)
