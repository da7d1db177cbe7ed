"""Frame quality metrics on the device: PSNR, SSIM and MS-SSIM (csrc/metrics.hip), LPIPS (csrc/lpips.hip, `class LPIPS` below),
FID (csrc/fid.hip, `class FrechetInceptionDistance` below) and FVD (csrc/fvd.hip, `class FrechetVideoDistance` below).

The reference harness scores every decoded frame against its ground truth: validation.py:120-155 (`ms_ssim(pred, gt,
data_range=1.0)`, `10*log10(1/mse)`) and test_utils.py:23-55 (`psnr`, `ms_ssim(..., data_range=255)`), both through
`pytorch_msssim`.  `ms_ssim` and `ssim` here take the arguments of pytorch_msssim 1.0 and restate its semantics:

    window   g[i] = exp(-(i - ws//2)^2 / (2 sigma^2)), normalised to sum 1, applied per channel as a valid (unpadded)
             correlation along H, then along W
    maps     cs = (2 s_xy + C2) / (s_xx + s_yy + C2),  ssim = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1) * cs,
             C1 = (K1 L)^2, C2 = (K2 L)^2, L = data_range; per (image, channel) the spatial means of both maps
    MS-SSIM  relu(cs) at every scale but the last, relu(ssim) at the last; between scales avg_pool2d(2, padding=(H%2, W%2))
             with count_include_pad; the value is prod_s v_s^w_s per (n, c); size_average=True -> mean over (n, c),
             otherwise the mean over c ([N])
    NaN      relu is v < 0 ? 0 : v, as torch.relu: a NaN pixel of a float operand makes the value of its (image, channel) plane NaN,
             and with it the mean of that image and the overall mean, in ms_ssim and in ssim (nonnegative_ssim or not); the other
             images are unaffected

Parity with the library itself is unpinned (pytorch_msssim is not a dependency); tests/metrics_ref.py restates the rules above in
fp64 and the device results are checked against that.  Deliberate differences from the library:
  - every float dtype is computed in fp32 (window sums in fp32, per-workgroup and final sums in fp64) and the result is fp32;
  - uint8 operands are taken as NHWC frames ([N,H,W,C], what `units_to_u8`, `blend_frames` and `postprocess_image` produce),
    float operands as NCHW with any strides (a permuted view is read in place);
  - `ssim` raises ValueError when H or W is smaller than the window (the library warns and skips that axis);
  - the window is limited to odd sizes up to 15, MS-SSIM to 8 scales, and only 4-D inputs are taken (no 5-D video form);
  - `win`, when given, must hold the same taps for every channel.

Placement: device tensors give device results on the current stream, with no host synchronisation (the calls can be captured in
a graph).  CPU tensors are copied to the current GPU and the result comes back on the CPU.  There is no CPU compute path.

`psnr(X, Y, data_range)` returns one fp64 value per image: 10 log10(L^2 / mse) over its C*H*W elements, +inf when mse == 0.  With
L = 255 on uint8 frames it equals validation.py's `10*log10(1/mse)` on x / 255."""
import ctypes
import math

import torch

from . import lib

MAX_WIN = 15
MAX_LEVELS = 8
DEFAULT_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def gaussian_window(size, sigma):
    """The library's `_fspecial_gauss_1d`: exp(-(i - size//2)^2 / (2 sigma^2)) normalised to sum 1 (computed in fp64)."""
    g = [math.exp(-((i - size // 2) ** 2) / (2.0 * sigma * sigma)) for i in range(size)]
    s = sum(g)
    return [v / s for v in g]


def _squeeze_like_library(t):
    for d in range(t.dim() - 1, 1, -1):
        t = t.squeeze(dim=d)
    return t


def _check_pair(X, Y):
    if not X.shape == Y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {X.shape} and {Y.shape}.")
    if X.dtype != Y.dtype:
        raise ValueError(f"Input images should have the same dtype, but got {X.dtype} and {Y.dtype}.")
    if X.dtype != torch.uint8:                      # the library drops size-1 dims after the channel axis of NCHW operands
        X, Y = _squeeze_like_library(X), _squeeze_like_library(Y)
    if X.dim() != 4:
        raise ValueError(f"Input images should be 4-d tensors, but got {tuple(X.shape)}")
    if X.dtype != torch.uint8 and not X.dtype.is_floating_point:
        raise ValueError(f"Input images should be uint8 (NHWC) or floating point (NCHW), got {X.dtype}")
    return X, Y


def _nchw(t):
    """(logical N, C, H, W, element strides (n, c, h, w)) of a uint8 NHWC or float NCHW operand."""
    if t.dtype == torch.uint8:
        n, h, w, c = t.shape
        sn, sh, sw, sc = t.stride()
    else:
        n, c, h, w = t.shape
        sn, sc, sh, sw = t.stride()
    return (n, c, h, w), (sn, sc, sh, sw)


def _window(win, win_size, win_sigma):
    if win is not None:
        win_size = int(win.shape[-1])
    if not (win_size % 2 == 1):
        raise ValueError("Window size should be odd.")
    if win is None:
        taps = gaussian_window(win_size, win_sigma)
    else:
        rows = win.detach().double().cpu().reshape(-1, win_size)
        if not bool((rows == rows[0]).all()):
            raise ValueError("win must hold the same taps for every channel")
        taps = rows[0].tolist()
    return taps, win_size


def _to_device(X, Y):
    """(X, Y on the GPU, whether the caller passed host tensors)."""
    if X.is_cuda and Y.is_cuda:
        return X, Y, False
    if X.is_cuda != Y.is_cuda:
        raise ValueError("X and Y must live on the same device")
    if not torch.cuda.is_available():
        raise RuntimeError("diffcodec_amd.metrics computes on the GPU and none is available (there is no CPU path)")
    dev = torch.device("cuda", torch.cuda.current_device())
    return X.to(dev), Y.to(dev), True


def _prepare(X, Y):
    """fp32 (or uint8) operands on the device + the shape / stride arguments of the C-ABI."""
    if X.dtype != torch.uint8 and X.dtype != torch.float32:
        X, Y = X.float(), Y.float()
    if X.device != Y.device:
        raise ValueError("X and Y must live on the same device")
    (n, c, h, w), sx = _nchw(X)
    _, sy = _nchw(Y)
    strides = (ctypes.c_longlong * 8)(*sx, *sy)
    return X, Y, (n, c, h, w), strides, int(X.dtype == torch.uint8)


def _run_ssim(X, Y, data_range, win, win_size, win_sigma, K, weights, mode):
    """mode 0: MS-SSIM with `weights`; 1: SSIM; 2: SSIM with relu.  Returns the fp64 device vector [N*C + N + 1]."""
    X, Y, host = _to_device(X, Y)
    X, Y, (n, c, h, w), strides, u8 = _prepare(X, Y)
    taps, ws = _window(win, win_size, win_sigma)
    levels = len(weights) if mode == 0 else 1
    nbytes = lib.load().dc_ssim_ws_bytes(n, c, h, w, ws, levels)
    if nbytes < 0:
        raise ValueError(f"shape {(n, c, h, w)} / window {ws} / {levels} scales: every scale must keep H, W >= the window "
                         f"(window <= {MAX_WIN}, <= {MAX_LEVELS} scales)")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=X.device)
    out = torch.empty(n * c + n + 1, dtype=torch.float64, device=X.device)
    k1, k2 = (float(v) for v in K)
    win_c = (ctypes.c_float * ws)(*taps)
    with torch.cuda.device(X.device):
        stream = torch.cuda.current_stream().cuda_stream
        if mode == 0:
            w_c = (ctypes.c_float * levels)(*[float(v) for v in weights])
            lib.call("dc_ms_ssim", X.data_ptr(), Y.data_ptr(), u8, strides, n, c, h, w, win_c, ws, w_c, levels, k1, k2,
                     float(data_range), scratch.data_ptr(), out.data_ptr(), stream)
        else:
            lib.call("dc_ssim", X.data_ptr(), Y.data_ptr(), u8, strides, n, c, h, w, win_c, ws, k1, k2, float(data_range),
                     int(mode == 2), scratch.data_ptr(), out.data_ptr(), stream)
    return out, n, c, host


def _result(out, n, c, size_average, host):
    r = (out[n * c + n] if size_average else out[n * c:n * c + n]).float()
    return r.cpu() if host else r


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, K=(0.01, 0.03), nonnegative_ssim=False):
    """pytorch_msssim.ssim: a scalar (size_average) or [N] (mean over channels)."""
    X, Y = _check_pair(X, Y)
    _, ws = _window(win, win_size, win_sigma)
    (_, _, h, w), _ = _nchw(X)
    if ws > MAX_WIN or h < ws or w < ws:
        raise ValueError(f"image {h}x{w} / window {ws}: H and W must be >= the window, and the window <= {MAX_WIN}")
    out, n, c, host = _run_ssim(X, Y, data_range, win, win_size, win_sigma, K, None, 2 if nonnegative_ssim else 1)
    return _result(out, n, c, size_average, host)


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, weights=None, K=(0.01, 0.03)):
    """pytorch_msssim.ms_ssim: a scalar (size_average) or [N] (mean over channels)."""
    X, Y = _check_pair(X, Y)
    _, ws = _window(win, win_size, win_sigma)
    (_, _, h, w), _ = _nchw(X)
    smaller_side = min(h, w)
    assert smaller_side > (ws - 1) * (2 ** 4), \
        "Image size should be larger than %d due to the 4 downsamplings in ms-ssim" % ((ws - 1) * (2 ** 4))
    if weights is None:
        weights = DEFAULT_WEIGHTS
    weights = [float(v) for v in (weights.tolist() if torch.is_tensor(weights) else weights)]
    if ws > MAX_WIN or not 1 <= len(weights) <= MAX_LEVELS:
        raise ValueError(f"window {ws} / {len(weights)} weights: the window must be <= {MAX_WIN}, 1 to {MAX_LEVELS} scales")
    out, n, c, host = _run_ssim(X, Y, data_range, win, win_size, win_sigma, K, weights, 0)
    return _result(out, n, c, size_average, host)


def psnr(X, Y, data_range=255.0):
    """fp64 [N]: 10 log10(L^2 / mse) per image over its C*H*W elements, +inf for identical images."""
    X, Y = _check_pair(X, Y)
    X, Y, host = _to_device(X, Y)
    X, Y, (n, c, h, w), strides, u8 = _prepare(X, Y)
    scratch = torch.empty(lib.load().dc_psnr_ws_bytes(n), dtype=torch.uint8, device=X.device)
    out = torch.empty(n, dtype=torch.float64, device=X.device)
    with torch.cuda.device(X.device):
        lib.call("dc_psnr", X.data_ptr(), Y.data_ptr(), u8, strides, n, c, h, w, float(data_range), scratch.data_ptr(),
                 out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out.cpu() if host else out


def summarize(scores, fid=None, fvd=None):
    """Means over frames of {frame: {"psnr": dB, "ms_ssim": value[, "lpips": value]}} (decode_clip(score=True)), following
    test_utils.py:49-55: a frame whose PSNR exceeds 1000 dB (identical images) is left out of the means.  Returns dict(psnr,
    ms_ssim, frames = the number averaged, identical = the number left out) and, when the scores carry it, lpips; the means are
    NaN when no frame is left.  `fid` (decode_clip's out["fid"], a statistic of the clip and not a mean over frames) is passed
    through as "fid" when given, and `fvd` (out["fvd"]) as "fvd"."""
    kept = [s for _, s in sorted(scores.items()) if not s["psnr"] > 1000]
    m = len(kept)
    out = dict(psnr=sum(s["psnr"] for s in kept) / m if m else float("nan"),
               ms_ssim=sum(s["ms_ssim"] for s in kept) / m if m else float("nan"),
               frames=m, identical=len(scores) - m)
    if any("lpips" in s for s in scores.values()):
        out["lpips"] = sum(s["lpips"] for s in kept) / m if m else float("nan")
    if fid is not None:
        out["fid"] = float(fid)
    if fvd is not None:
        out["fvd"] = float(fvd)
    return out


class _TruthFrames:
    """`source.ground_truth(frame)` over a batch of original frames"""

    def __init__(self, frames):
        self.frames = frames

    def ground_truth(self, frame):
        return self.frames[frame]


def calculate_metrics_batch(original, pred, lpips=None, fid=None, fvd=None, size=(512, 512)):
    """test_utils.py:27-82 on uint8 frames: `original` and `pred` are [N,H,W,3] tensors or lists of [H,W,3] (PIL images as arrays),
    on the device or on the host.  Both frames of a pair are resized to `size` as the reference's `transforms.Resize` does
    (`resample.resize_u8`, "bilinear"; None scores them as they are), then scored.  Returns {"PSNR", "MS-SSIM"} and, for every
    model given (`LPIPS`, `FrechetInceptionDistance`, `FrechetVideoDistance` with weights loaded), "LPIPS", "FID", "FVD": the means
    over the pairs whose PSNR does not exceed 1000 dB (test_utils.py:51-52), the FID of those pairs (the model is reset first) and
    the FVD of the two videos they form, each stacked twice (`clip_decode.fvd_of_frames`).  The scoring is `clip_decode`'s: the
    same calls on the same bytes as `decode_clip(score=True, score_size=size)`."""
    from . import clip_decode
    if len(original) != len(pred):
        raise ValueError(f"calculate_metrics_batch takes as many original as predicted frames, got {len(original)} and {len(pred)}")
    if not len(pred):
        raise ValueError("calculate_metrics_batch needs at least one pair of frames")
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    up = lambda t: t if t.is_cuda or dev is None else t.to(dev)
    frames = {i: up(pred[i]) for i in range(len(pred))}
    truth_src = _TruthFrames([up(original[i]) for i in range(len(original))])
    scores, rows, truth = clip_decode._score_frames(frames, truth_src, lpips, fid, size)
    mean = summarize(scores)
    out = {"PSNR": mean["psnr"], "MS-SSIM": mean["ms_ssim"]}
    if lpips is not None:
        out["LPIPS"] = mean["lpips"]
    if fid is not None:
        fid.reset()
        clip_decode.fid_update_rows(fid, rows)
        out["FID"] = clip_decode._fid_value(fid)
    if fvd is not None:
        out["FVD"] = clip_decode.fvd_of_frames(fvd, frames, truth, scores, size)
    return out


# ------------------------------------------------------------------------------------------------- packed networks
def _state_tensor(what, sd, key, shape):
    if key not in sd:
        raise ValueError(f"{what} state dict: missing key {key!r}")
    t = sd[key]
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} state dict: {key!r} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.detach().to("cpu", torch.float32)


def fold_bn(weight, bias, mean, var, eps):
    """Eval BatchNorm as y = s x + t, formed in fp64: s = weight / sqrt(var + eps), t = bias - mean s."""
    g, b, m, v = (x.detach().double().cpu() for x in (weight, bias, mean, var))
    s = g / torch.sqrt(v + eps)
    return s, b - m * s


class _PackedNet:
    """What LPIPS, FrechetInceptionDistance and FrechetVideoDistance share: the packed fp32 weight vector on the CPU (`packed`), its
    per-device copies, loading from a state dict, and running a batch in chunks that bound the scratch.  A subclass sets `_WHAT`
    (the name in its messages), `_FLOATS` (the library's dc_*_weight_floats), `_pack` and `_chunk_bytes`."""
    _FROM = "from_state_dict"

    def _init_weights(self):
        self.packed = None              # fp32 CPU vector (the subclass's pack_*_weights)
        self._on_device = {}

    @classmethod
    def from_state_dict(cls, state_dict, **kwargs):
        return cls(**kwargs).load_state_dict(state_dict)

    def load_state_dict(self, state_dict, *more):
        packed = self._pack(state_dict, *more)
        want = getattr(lib.load(), self._FLOATS)()
        if packed.numel() != want:
            raise RuntimeError(f"packed {self._WHAT} weights hold {packed.numel()} floats, the library expects {want}")
        self.packed = packed
        self._on_device = {}
        return self

    def to(self, device):
        self._weights(torch.device(device))
        return self

    @staticmethod
    def _device(device):
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        return device

    def _weights(self, device):
        if self.packed is None:
            raise RuntimeError(f"{type(self).__name__} has no weights: call load_state_dict / {self._FROM} (nothing is downloaded)")
        device = self._device(device)
        w = self._on_device.get(device)
        if w is None:
            w = self._on_device[device] = self.packed.to(device)
        return w

    @staticmethod
    def _stage(x, y=None):
        """(x, y as uint8 or fp32 on the GPU, whether the caller passed host tensors)"""
        X, Y, host = _to_device(x, x if y is None else y)
        if X.dtype != torch.uint8 and X.dtype != torch.float32:
            X, Y = X.float(), Y.float()
        return X, Y, host

    def _step(self, n, ws_bytes):
        """items per launch sequence: as many as keep `ws_bytes(items)` of scratch under the class's chunk bound"""
        return max(1, min(n, self._chunk_bytes() // max(1, ws_bytes(1))))

    def _slices(self, n, device, ws_bytes):
        """(slice of the batch, its scratch) chunk by chunk"""
        step = self._step(n, ws_bytes)
        for i in range(0, n, step):
            sl = slice(i, min(i + step, n))
            yield sl, torch.empty(ws_bytes(sl.stop - sl.start), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------------------------------------- LPIPS
LPIPS_CHANNELS = (64, 192, 384, 256, 256)
LPIPS_CIN = (3, 64, 192, 384, 256)
LPIPS_KERNEL = (11, 5, 3, 3, 3)
LPIPS_FEATURE_INDEX = (0, 3, 6, 8, 10)               # torchvision alexnet.features positions of the five convolutions
LPIPS_MIN_SIZE = 31
LPIPS_CHUNK_BYTES = 1 << 30                          # scratch bound of one launch sequence (12.4 MB of maps per 512x512 image)


def lpips_map_sizes(h, w):
    """(H, W) of relu1 .. relu5 for an h x w image: conv 11/4/2, max_pool 3/2, conv 5/1/2, max_pool 3/2, three conv 3/1/1."""
    def down(v):
        return (v - 3) // 2 + 1
    s1 = ((h - 7) // 4 + 1, (w - 7) // 4 + 1)
    s2 = (down(s1[0]), down(s1[1]))
    s3 = (down(s2[0]), down(s2[1]))
    return [s1, s2, s3, s3, s3]


def pack_lpips_weights(state_dict, lin_state_dict=None):
    """One fp32 CPU vector in the layout dc_lpips_alex reads: per conv the K-major matrix [(ci, ky, kx)][Cout] (conv1 followed by
    one zero row, 363 -> 364) and its bias, then the five lin vectors.  Accepts the two layouts of LPIPS.load_state_dict."""
    sd = dict(state_dict)
    if lin_state_dict is not None:
        sd.update(lin_state_dict)
    library = any(k.startswith("net.slice") for k in sd)
    parts = []
    for l, (co, ci, k, pos) in enumerate(zip(LPIPS_CHANNELS, LPIPS_CIN, LPIPS_KERNEL, LPIPS_FEATURE_INDEX)):
        stem = f"net.slice{l + 1}.{pos}" if library else f"features.{pos}"
        w = _state_tensor("LPIPS", sd, stem + ".weight", (co, ci, k, k))
        b = _state_tensor("LPIPS", sd, stem + ".bias", (co,))
        wk = w.reshape(co, ci * k * k).t().contiguous()
        if l == 0:
            wk = torch.cat([wk, torch.zeros(1, co)], 0)
        parts += [wk.reshape(-1), b]
    for l, co in enumerate(LPIPS_CHANNELS):
        parts.append(_state_tensor("LPIPS", sd, f"lin{l}.model.1.weight", (1, co, 1, 1)).reshape(-1))
    return torch.cat(parts).contiguous()


class LPIPS(_PackedNet):
    """`lpips.LPIPS(net='alex')` (version 0.1) on the device in exact fp32 (csrc/lpips.hip): call surface of the library's module,
    `model(in0, in1, retPerLayer=False, normalize=False)` -> fp32 [N,1,1,1] (and the list of five per-layer [N,1,1,1]).

        scaling   (x - shift) / scale, shift = (-.030, -.088, -.188), scale = (.458, .448, .450); normalize=True maps [0,1] to
                  [-1,1] first (2x - 1); uint8 operands are x / 255
        features  relu1 .. relu5 of torchvision's AlexNet: conv 3->64 11/4/2, max_pool 3/2, conv 64->192 5/1/2, max_pool 3/2,
                  conv 192->384, 384->256, 256->256 3/1/1, a ReLU after each conv
        distance  per layer, per pixel: sum_c w_c (x_c / (|x| + 1e-10) - y_c / (|y| + 1e-10))^2 with |x| = sqrt(sum_c x_c^2), its
                  spatial mean; the value is the sum over the five layers.  normfix=True normalises by sqrt(sum_c (x_c^2 + 1e-8)),
                  the form of the reference's training loss (controlnet/lpips_loss.py:27-29)

    No weights ship with the package and none are downloaded: load the published checkpoint with `load_state_dict` /
    `LPIPS.from_state_dict`, which take either
      - the library module's own state dict: `net.slice{1..5}.{0,3,6,8,10}.weight|bias` and `lin{0..4}.model.1.weight` of shape
        [1,C,1,1] (its `lins.*` duplicates and `scaling_layer.*` buffers are ignored), or
      - a torchvision AlexNet state dict (`features.{0,3,6,8,10}.weight|bias`; `classifier.*` ignored) together with the lin
        dict of the library's weights/v0.1/alex.pth (`lin{0..4}.model.1.weight`), as a second argument or merged into the first.
    These key names are recalled from the published packages and are unpinned (neither lpips nor torchvision is a dependency);
    tests/lpips_ref.py restates the rules above in fp64 and the device results are checked against that with seeded weights.

    Operands and placement as for `ms_ssim`: uint8 NHWC or floating NCHW (any strides, read in place; float dtypes other than
    fp32 are converted), C = 3, H and W >= 31.  Device tensors give device results on the current stream with no host
    synchronisation (graph-capturable once the weights are on the device: `model.to(device)` or a first call); CPU tensors are
    copied to the current GPU and the result comes back on the CPU.  Large batches run in chunks that bound the scratch; every
    pair's result is independent of its position and of the batch size, bit for bit."""

    def __init__(self, net="alex", version="0.1", normfix=False):
        if net != "alex":
            raise NotImplementedError(f"LPIPS net {net!r}: only 'alex' is implemented")
        if str(version) != "0.1":
            raise NotImplementedError(f"LPIPS version {version!r}: only '0.1' is implemented")
        self.normfix = bool(normfix)
        self._init_weights()

    _WHAT, _FLOATS, _FROM = "LPIPS", "dc_lpips_weight_floats", "LPIPS.from_state_dict"
    _pack = staticmethod(pack_lpips_weights)
    _chunk_bytes = staticmethod(lambda: LPIPS_CHUNK_BYTES)

    @classmethod
    def from_state_dict(cls, state_dict, lin_state_dict=None, **kwargs):
        return cls(**kwargs).load_state_dict(state_dict, lin_state_dict)

    def load_state_dict(self, state_dict, lin_state_dict=None):
        return super().load_state_dict(state_dict, lin_state_dict)

    @staticmethod
    def _check_image(c, h, w):
        if c != 3:
            raise ValueError(f"LPIPS takes 3-channel images, got {c} channels")
        if h < LPIPS_MIN_SIZE or w < LPIPS_MIN_SIZE:
            raise ValueError(f"LPIPS needs H, W >= {LPIPS_MIN_SIZE}, got {h}x{w}")

    def __call__(self, in0, in1, retPerLayer=False, normalize=False):
        X, Y = _check_pair(in0, in1)
        (n, c, h, w), _ = _nchw(X)
        self._check_image(c, h, w)
        X, Y, host = self._stage(X, Y)
        wts = self._weights(X.device)
        outs = []
        with torch.cuda.device(X.device):
            stream = torch.cuda.current_stream().cuda_stream
            for sl, scratch in self._slices(n, X.device, lambda m: lib.load().dc_lpips_ws_bytes(m, h, w)):
                xs, ys, (m, _, _, _), strides, u8 = _prepare(X[sl], Y[sl])
                out = torch.empty(6 * m, dtype=torch.float64, device=X.device)
                lib.call("dc_lpips_alex", xs.data_ptr(), ys.data_ptr(), u8, strides, m, h, w, int(bool(normalize)), int(self.normfix),
                         wts.data_ptr(), scratch.data_ptr(), out.data_ptr(), stream)
                outs.append(out.view(6, m))
        res = (outs[0] if len(outs) == 1 else torch.cat(outs, 1)).float()
        if host:
            res = res.cpu()
        val = res[5].reshape(n, 1, 1, 1)
        if retPerLayer:
            return val, [res[l].reshape(n, 1, 1, 1) for l in range(5)]
        return val

    forward = __call__

    def features(self, x, normalize=False):
        """The five post-ReLU maps [relu1 .. relu5] of `x` (uint8 NHWC or float NCHW), contiguous fp32 NCHW."""
        X, _ = _check_pair(x, x)
        (n, c, h, w), _ = _nchw(X)
        self._check_image(c, h, w)
        X, _, host = self._stage(X)
        wts = self._weights(X.device)
        sizes = lpips_map_sizes(h, w)
        feats = [torch.empty((n, co) + s, dtype=torch.float32, device=X.device) for co, s in zip(LPIPS_CHANNELS, sizes)]
        with torch.cuda.device(X.device):
            stream = torch.cuda.current_stream().cuda_stream
            for sl, scratch in self._slices(n, X.device, lambda m: lib.load().dc_lpips_features_ws_bytes(m, h, w)):
                xs = X[sl]
                lib.call("dc_lpips_alex_features", xs.data_ptr(), int(xs.dtype == torch.uint8), (ctypes.c_longlong * 4)(*_nchw(xs)[1]),
                         xs.shape[0], h, w, int(bool(normalize)), wts.data_ptr(), scratch.data_ptr(), *[f[sl].data_ptr() for f in feats],
                         stream)
        return [f.cpu() for f in feats] if host else feats


# ------------------------------------------------------------------------------------------------------------- FID
FID_BLOCKS = ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3")
FID_CIN = (3, 32, 32)
FID_COUT = (32, 32, 64)
FID_FEATURES = 64
FID_STATE = 1 + FID_FEATURES + FID_FEATURES * FID_FEATURES       # n, sum f, sum f f^T
FID_SIZE = 299
FID_MAP_SHAPES = ((3, 299, 299), (32, 149, 149), (32, 147, 147), (64, 147, 147), (64, 73, 73))
FID_BN_EPS = 1e-3
FID_CHUNK_BYTES = 1 << 30                            # scratch bound of one launch sequence (12.2 MB of maps per image)


def pack_fid_weights(state_dict):
    """One fp32 CPU vector in the layout dc_fid_features reads: per block the K-major matrix [(ci, ky, kx)][Cout] (block 1 followed
    by one zero row, 27 -> 28), then s = bn.weight / sqrt(running_var + 1e-3) and t = bn.bias - running_mean * s, both formed in
    fp64 and rounded to fp32."""
    parts = []
    for l, (name, ci, co) in enumerate(zip(FID_BLOCKS, FID_CIN, FID_COUT)):
        w = _state_tensor("FID", state_dict, f"{name}.conv.weight", (co, ci, 3, 3))
        s, t = fold_bn(*(_state_tensor("FID", state_dict, f"{name}.bn.{k}", (co,)) for k in ("weight", "bias", "running_mean", "running_var")),
                       FID_BN_EPS)
        wk = w.reshape(co, ci * 9).t().contiguous()
        if l == 0:
            wk = torch.cat([wk, torch.zeros(1, co)], 0)
        parts += [wk.reshape(-1), s.float(), t.float()]
    return torch.cat(parts).contiguous()


def _frechet_value(mu_r, cov_r, mu_f, cov_f):
    """|mu_r - mu_f|^2 + tr cov_r + tr cov_f - 2 tr (cov_r cov_f)^(1/2) from fp64 means [d] and covariances [d,d] of any dimension
    (FID: 64, FVD: 400), the last term as the singular values of cov_r^(1/2) cov_f^(1/2) (see `frechet_distance`)."""
    d = mu_r - mu_f
    (a_r, u_r), (a_f, u_f) = torch.linalg.eigh(cov_r), torch.linalg.eigh(cov_f)
    c = torch.linalg.svdvals((u_r * a_r.clamp_min(0).sqrt()).t() @ (u_f * a_f.clamp_min(0).sqrt())).sum()
    return float((d * d).sum() + cov_r.trace() + cov_f.trace() - 2 * c)


def frechet_distance(state_real, state_fake):
    """The value from two fp64 state vectors [1 + 64 + 4096] (n, sum f, sum f f^T), on the host in fp64:
    mu = sum / n, cov = (sumsq - n mu mu^T) / (n - 1), |mu_r - mu_f|^2 + tr cov_r + tr cov_f - 2 sum sqrt(eigvals(cov_r cov_f)).real.

    The last term is evaluated as the sum of the singular values of cov_r^(1/2) cov_f^(1/2): with cov = U diag(a) U^T (eigh) the
    eigenvalues of cov_r cov_f are the squared singular values of diag(sqrt a_r) U_r^T U_f diag(sqrt a_f).  The value is the same;
    the error is not.  A general eigen-solver returns the zero eigenvalues of a rank-deficient product (fewer than 65 images on a
    side) as +-1e-17 |cov|^2, whose square roots add 1e-8 each, so a set against itself came out at -2.5e-8; singular values carry
    an absolute error of 1e-16 |cov| and the same case gives 1e-14."""
    stats = []
    for st in (state_real, state_fake):
        st = st.detach().to("cpu", torch.float64)
        n = float(st[0])
        if n < 2:
            raise RuntimeError("More than one sample is required for both the real and fake distributed to compute FID")
        mu = st[1:1 + FID_FEATURES] / n
        sq = st[1 + FID_FEATURES:].view(FID_FEATURES, FID_FEATURES)
        stats.append((mu, (sq - n * torch.outer(mu, mu)) / (n - 1)))
    (mu_r, cov_r), (mu_f, cov_f) = stats
    return _frechet_value(mu_r, cov_r, mu_f, cov_f)


class FrechetInceptionDistance(_PackedNet):
    """`torchmetrics.image.fid.FrechetInceptionDistance(feature=64)` on the device in exact fp32 (csrc/fid.hip): `update(imgs, real)`
    accumulates, `compute()` returns the value as a Python float.

        input     3-channel images of any H, W >= 1; with normalize=True a float image in [0,1], taken as (x * 255) truncated to uint8
        resize    to 299 x 299, TF1-legacy bilinear (align_corners=False without the half-pixel offset): for output index o on an
                  axis of input size I, p = o * (I / 299), i0 = floor(p), i1 = min(i0 + 1, I - 1), l = p - i0;
                  top = tl + (tr - tl) lx, bot = bl + (br - bl) lx, out = top + (bot - top) ly; then (x - 128) / 128
        stem      Conv2d_1a_3x3 (3 -> 32, stride 2), Conv2d_2a_3x3 (32 -> 32), Conv2d_2b_3x3 (32 -> 64, pad 1): conv without bias,
                  eval BatchNorm with eps 1e-3 (applied as one fma per channel), ReLU; maps 149 / 147 / 147
        pooling   max-pool 3 x 3 stride 2 (73 x 73), then the spatial mean: 64 features per image
        state     per side (real, fake) n, sum f and sum f f^T in fp64, added image by image in batch order
        value     mu = sum / n, cov = (sumsq - n mu mu^T) / (n - 1),
                  |mu_r - mu_f|^2 + tr cov_r + tr cov_f - 2 sum sqrt(eigvals(cov_r cov_f)).real, the last term evaluated as
                  the singular values of cov_r^(1/2) cov_f^(1/2) (`frechet_distance`): a set against itself gives 0 to 1e-14

    No weights ship with the package and none are downloaded: load the `pt_inception-2015-12-05` FID network's checkpoint with
    `load_state_dict` / `from_state_dict`; the keys `Conv2d_{1a,2a,2b}_3x3.conv.weight` and
    `Conv2d_{1a,2a,2b}_3x3.bn.{weight,bias,running_mean,running_var}` are read by name, every other key is ignored.  These rules and
    key names are recalled from the published packages and are unpinned (neither torchmetrics nor torch-fidelity is a dependency);
    tests/fid_ref.py restates the rules above in fp64 and the device results are checked against that with seeded weights.

    Deliberate differences from the library: uint8 images are NHWC frames ([N,H,W,3], the package's convention; the library takes
    uint8 NCHW); float images are NCHW with any strides (read in place) and are taken only with normalize=True; only feature=64.

    Placement: device tensors are read on the current stream and `update` does not synchronise with the host (graph-capturable once
    the model is on the device: `model.to(device)` or a first call); CPU tensors are copied to the current GPU.  Large batches run
    in chunks that bound the scratch; an image's features do not depend on its position or on the batch size, and
    `update(a); update(b)` leaves the bits of `update(cat(a, b))`.  `compute()` copies the 2 x 4161 doubles of the state to the host
    and runs the 64 x 64 eigenvalue step there in fp64: the one host synchronisation, at the end of a clip."""

    def __init__(self, feature=64, normalize=False):
        if feature != 64:
            raise NotImplementedError(f"FrechetInceptionDistance feature {feature!r}: only 64 is implemented")
        self.normalize = bool(normalize)
        self._init_weights()
        self._state = {True: torch.zeros(FID_STATE, dtype=torch.float64), False: torch.zeros(FID_STATE, dtype=torch.float64)}

    _WHAT, _FLOATS = "FID", "dc_fid_weight_floats"
    _pack = staticmethod(pack_fid_weights)
    _chunk_bytes = staticmethod(lambda: FID_CHUNK_BYTES)

    def to(self, device):
        super().to(device)
        device = self._device(torch.device(device))
        self._state = {k: v.to(device) for k, v in self._state.items()}
        return self

    def _images(self, imgs):
        """(operand on the GPU, whether the caller passed a host tensor, (n, h, w))"""
        if imgs.dim() != 4:
            raise ValueError(f"FID takes 4-d image batches, got {tuple(imgs.shape)}")
        if imgs.dtype == torch.uint8:
            if self.normalize:
                raise ValueError("normalize=True takes float NCHW images in [0,1], got uint8")
        elif not imgs.dtype.is_floating_point:
            raise ValueError(f"FID images should be uint8 (NHWC) or floating point (NCHW, normalize=True), got {imgs.dtype}")
        elif not self.normalize:
            raise ValueError("float images are taken only with normalize=True (values in [0,1]); pass uint8 NHWC frames otherwise")
        (n, c, h, w), _ = _nchw(imgs)
        if c != 3:
            raise ValueError(f"FID takes 3-channel images, got {c} channels")
        if h < 1 or w < 1:
            raise ValueError(f"FID needs H, W >= 1, got {h}x{w}")
        X, _, host = self._stage(imgs)
        return X, host, (n, h, w)

    def _chunks(self, n, h, w):
        return self._step(n, lambda m: lib.load().dc_fid_ws_bytes(m, h, w))

    def features(self, imgs):
        """fp32 [N,64]: the pooled features of `imgs` (uint8 NHWC, or float NCHW with normalize=True)."""
        X, host, (n, h, w) = self._images(imgs)
        wts = self._weights(X.device)
        out = torch.empty((n, FID_FEATURES), dtype=torch.float32, device=X.device)
        with torch.cuda.device(X.device):
            stream = torch.cuda.current_stream().cuda_stream
            for sl, scratch in self._slices(n, X.device, lambda m: lib.load().dc_fid_ws_bytes(m, h, w)):
                xs = X[sl]
                lib.call("dc_fid_features", xs.data_ptr(), int(xs.dtype == torch.uint8), (ctypes.c_longlong * 4)(*_nchw(xs)[1]), xs.shape[0],
                         h, w, wts.data_ptr(), scratch.data_ptr(), out[sl].data_ptr(), stream)
        return out.cpu() if host else out

    def maps(self, imgs):
        """[resized [N,3,299,299], relu1 [N,32,149,149], relu2 [N,32,147,147], relu3 [N,64,147,147], pooled [N,64,73,73]],
        contiguous fp32 NCHW (the test seam; `features` keeps them in scratch)."""
        X, host, (n, h, w) = self._images(imgs)
        wts = self._weights(X.device)
        outs = [torch.empty((n,) + s, dtype=torch.float32, device=X.device) for s in FID_MAP_SHAPES]
        feat = torch.empty((n, FID_FEATURES), dtype=torch.float32, device=X.device)
        step = self._chunks(n, h, w)
        with torch.cuda.device(X.device):
            stream = torch.cuda.current_stream().cuda_stream
            for i in range(0, n, step):
                xs = X[i:i + step]
                lib.call("dc_fid_maps", xs.data_ptr(), int(xs.dtype == torch.uint8), (ctypes.c_longlong * 4)(*_nchw(xs)[1]), xs.shape[0],
                         h, w, wts.data_ptr(), *[t[i:i + step].data_ptr() for t in outs], feat[i:i + step].data_ptr(), stream)
        return [t.cpu() for t in outs] if host else outs

    def update_features(self, f, real):
        """Add feature rows [N,64] (computed by `features`, here or on another rank) to the real or the fake side, in row order."""
        if f.dim() != 2 or f.shape[1] != FID_FEATURES:
            raise ValueError(f"FID feature rows should be [N,{FID_FEATURES}], got {tuple(f.shape)}")
        if f.shape[0] == 0:
            return
        if not f.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError("diffcodec_amd.metrics computes on the GPU and none is available (there is no CPU path)")
            f = f.to(torch.device("cuda", torch.cuda.current_device()))
        f = f.float().contiguous()
        real = bool(real)
        if self._state[real].device != f.device:
            self._state = {k: v.to(f.device) for k, v in self._state.items()}
        with torch.cuda.device(f.device):
            lib.call("dc_fid_accumulate", f.data_ptr(), f.shape[0], self._state[real].data_ptr(), torch.cuda.current_stream().cuda_stream)

    def update(self, imgs, real):
        """Add the images' features to the real (real=True) or the fake side."""
        f = self.features(imgs)
        self.update_features(f, real)

    def state(self):
        """(real, fake): copies of the two fp64 state vectors [1 + 64 + 4096] = n, sum f, sum f f^T (row-major)."""
        return self._state[True].clone(), self._state[False].clone()

    def merge_state(self, real, fake):
        """Add two state vectors (another model's `state()`) to this one's sums."""
        for side, st in ((True, real), (False, fake)):
            if tuple(st.shape) != (FID_STATE,):
                raise ValueError(f"FID state vectors hold {FID_STATE} doubles, got {tuple(st.shape)}")
            self._state[side].add_(st.detach().to(self._state[side].device, torch.float64))

    def reset(self):
        for v in self._state.values():
            v.zero_()

    def compute(self):
        """The Frechet distance of the two accumulated sets as a Python float (synchronises: the state is copied to the host)."""
        return frechet_distance(self._state[True], self._state[False])


# ------------------------------------------------------------------------------------------------------------- FVD
FVD_FEATURES = 400
FVD_SIZE = 224
FVD_MIN_FRAMES = 9                                   # the head's [2,7,7] mean needs two time slices of Mixed_5c
FVD_CHUNK_BYTES = 1 << 30                            # scratch bound of one launch sequence (about 100 MB of maps per 16-frame video)
FVD_BN_EPS = 1e-5
FVD_MAX_FRAMES, FVD_MAX_SIDE = 4096, 16384           # the limits of dc_fvd_ws_bytes
# The network in endpoint order.  ("conv", Cin, Cout, kernel, stride): a Unit3D (conv3d without bias, eval BatchNorm, ReLU), kernel
# and stride the same on (t, h, w); ("pool", kernel (t, h, w), stride (t, h, w)): a SAME-padded max-pool whose padding is zeros
# that enter the max; ("mixed", Cin, (b0, b1a, b1b, b2a, b2b, b3b)): the six-unit module of FVD_BRANCHES.
FVD_NET = (
    ("Conv3d_1a_7x7", "conv", 3, 64, 7, 2),
    ("MaxPool3d_2a_3x3", "pool", (1, 3, 3), (1, 2, 2)),
    ("Conv3d_2b_1x1", "conv", 64, 64, 1, 1),
    ("Conv3d_2c_3x3", "conv", 64, 192, 3, 1),
    ("MaxPool3d_3a_3x3", "pool", (1, 3, 3), (1, 2, 2)),
    ("Mixed_3b", "mixed", 192, (64, 96, 128, 16, 32, 32)),
    ("Mixed_3c", "mixed", 256, (128, 128, 192, 32, 96, 64)),
    ("MaxPool3d_4a_3x3", "pool", (3, 3, 3), (2, 2, 2)),
    ("Mixed_4b", "mixed", 480, (192, 96, 208, 16, 48, 64)),
    ("Mixed_4c", "mixed", 512, (160, 112, 224, 24, 64, 64)),
    ("Mixed_4d", "mixed", 512, (128, 128, 256, 24, 64, 64)),
    ("Mixed_4e", "mixed", 512, (112, 144, 288, 32, 64, 64)),
    ("Mixed_4f", "mixed", 528, (256, 160, 320, 32, 128, 128)),
    ("MaxPool3d_5a_2x2", "pool", (2, 2, 2), (2, 2, 2)),
    ("Mixed_5b", "mixed", 832, (256, 160, 320, 32, 128, 128)),
    ("Mixed_5c", "mixed", 832, (384, 192, 384, 48, 128, 128)),
)
# A module's units in state-dict order: (name, kernel, input = "x" the module's input / the unit it follows / "pool" = the 3x3x3
# stride-1 max-pool of the input).  The output is cat(b0, b1b, b2b, b3b) along the channels.
FVD_BRANCHES = (("b0", 1, "x"), ("b1a", 1, "x"), ("b1b", 3, "b1a"), ("b2a", 1, "x"), ("b2b", 3, "b2a"), ("b3b", 1, "pool"))
FVD_ENDPOINTS = tuple(row[0] for row in FVD_NET)


def fvd_units():
    """[(state-dict prefix, Cin, Cout, kernel, stride)] of the 57 Unit3D with BatchNorm, in state-dict order (the logits conv,
    1024 -> 400 with a bias and no BatchNorm, follows them)."""
    units = []
    for name, kind, *rest in FVD_NET:
        if kind == "conv":
            units.append((name,) + tuple(rest))
        elif kind == "mixed":
            cin, ch = rest
            src = {"x": cin, "pool": cin}
            for (b, k, inp), co in zip(FVD_BRANCHES, ch):
                units.append((f"{name}.{b}", src[inp], co, k, 1))
                src[b] = co
    return units


def fvd_same_pad(size, k, s):
    """TF "SAME" on one axis: (output size, front padding, back padding)."""
    pad = max(k - s, 0) if size % s == 0 else max(k - size % s, 0)
    return -(-size // s), pad // 2, pad - pad // 2


def fvd_endpoint_shapes(t):
    """[(C, T', S, S)] of the 16 endpoint maps for a t-frame video (after the 224 x 224 preprocess)."""
    shapes, c, s = [], 3, FVD_SIZE
    for name, kind, *rest in FVD_NET:
        if kind == "conv":
            _, c, k, st = rest
            t, s = fvd_same_pad(t, k, st)[0], fvd_same_pad(s, k, st)[0]
        elif kind == "pool":
            k, st = rest
            t, s = fvd_same_pad(t, k[0], st[0])[0], fvd_same_pad(s, k[1], st[1])[0]
        else:
            ch = rest[1]
            c = ch[0] + ch[2] + ch[4] + ch[5]
        shapes.append((c, t, s, s))
    return shapes


def fvd_resized_size(h, w):
    """(RH, RW) of fvd.py:176-180: the shorter side becomes 224, the other ceil(side * scale) with scale = 224 / min(h, w) as
    Python floats (the same expression, so the same integer)."""
    scale = FVD_SIZE / min(h, w)
    return (FVD_SIZE, math.ceil(w * scale)) if h < w else (math.ceil(h * scale), FVD_SIZE)


def pack_fvd_unit(w, s, t):
    """One Unit3D in the layout dc_fvd_conv reads: the K-major matrix [(ci, kt, kh, kw)][Cout rounded up to 32] with the zero rows
    of its kernel class (7: one after the 49 taps of every (ci, kt); 3: up to a multiple of 4 input channels; 1: up to a multiple of
    32 input channels), then s and t (y = s * conv + t), zero in the padded columns."""
    co, ci, k = w.shape[0], w.shape[1], w.shape[2]
    if tuple(w.shape[2:]) != (k, k, k) or k not in (1, 3, 7):
        raise ValueError(f"FVD conv kernels are 1x1x1, 3x3x3 or 7x7x7, got {tuple(w.shape[2:])}")
    w = w.detach().to("cpu", torch.float32)
    if k == 7:
        m = w.reshape(co, ci * 7, 49).permute(1, 2, 0)
        m = torch.cat([m, torch.zeros(ci * 7, 1, co)], 1).reshape(ci * 7 * 50, co)
        rows = ci * 7 * 50
    else:
        m = w.reshape(co, ci * k ** 3).t()
        rows = -(-ci // 4) * 108 if k == 3 else -(-ci // 32) * 32
    out = torch.zeros(rows + 2, -(-co // 32) * 32)
    out[:m.shape[0], :co] = m
    out[rows, :co] = s.float()
    out[rows + 1, :co] = t.float()
    return out.reshape(-1)


def pack_fvd_weights(state_dict, bn_eps=FVD_BN_EPS):
    """One fp32 CPU vector in the layout dc_fvd_features reads: `pack_fvd_unit` of the 57 units of `fvd_units()` with
    s = bn.weight / sqrt(running_var + bn_eps), t = bn.bias - running_mean * s (fp64, rounded to fp32), then of the logits conv
    with s = 1, t = its bias."""
    parts = []
    for name, ci, co, k, _ in fvd_units():
        w = _state_tensor("FVD", state_dict, f"{name}.conv3d.weight", (co, ci, k, k, k))
        s, t = fold_bn(*(_state_tensor("FVD", state_dict, f"{name}.bn.{q}", (co,)) for q in ("weight", "bias", "running_mean", "running_var")),
                       bn_eps)
        parts.append(pack_fvd_unit(w, s, t))
    w = _state_tensor("FVD", state_dict, "logits.conv3d.weight", (FVD_FEATURES, 1024, 1, 1, 1))
    b = _state_tensor("FVD", state_dict, "logits.conv3d.bias", (FVD_FEATURES,))
    parts.append(pack_fvd_unit(w, torch.ones(FVD_FEATURES), b))
    return torch.cat(parts).contiguous()


def _fvd_stats(rows):
    rows = rows.detach().to("cpu", torch.float64)
    n = rows.shape[0]
    mu = rows.mean(0)
    c = rows - mu
    return mu, c.t() @ c / (n - 1)


class FrechetVideoDistance(_PackedNet):
    """The FVD of the reference's clip scoring (test_utils.py:45-70, fvd_utils/models/fvd) on the device in exact fp32
    (csrc/fvd.hip): the Inception-v1 I3D network of pytorch_i3d.py, 400 logits per video, and the Frechet distance of two sets of
    such rows.

        input       videos of T >= 9 frames: uint8 [N,T,H,W,3] (taken as x / 255, the documented [0,1] contract of fvd.py; with
                    byte_range=True the raw 0..255 values, which is what test_utils.py:45-70 actually feeds, kept for comparable
                    numbers as the LPIPS [0,1] quirk is) or floating [N,T,3,H,W] with any strides, taken as they are
        preprocess  fvd.py:166-192 per frame: bilinear resize (align_corners=False, no antialias) of the shorter side to 224, the
                    other to ceil(side * 224 / min(h, w)); centre crop to 224 x 224 from (size - 224) // 2; (v - 0.5) * 2; no clamping
        network     FVD_NET / FVD_BRANCHES: Unit3D = conv3d + eval BatchNorm (eps = bn_eps; pytorch_i3d.py:69 says 1e-5, the TF
                    original 1e-3; folded at pack time to one fma per channel) + ReLU, TF "SAME" padding (`fvd_same_pad`); the
                    max-pools pad by the same rule with zeros that enter the max
        head        mean over [2,7,7] windows of Mixed_5c, logits conv 1024 -> 400 with bias, mean over the remaining time positions
        value       mu and cov (n - 1) of the rows of each side on the host in fp64, then `_frechet_value`

    No weights ship with the package and none are downloaded: `load_state_dict` / `from_state_dict` take the InceptionI3d state
    dict of pytorch_i3d.py (`<endpoint>.conv3d.weight`, `<endpoint>.bn.{weight,bias,running_mean,running_var}`,
    `Mixed_xx.{b0,b1a,b1b,b2a,b2b,b3b}.conv3d|bn...`, `logits.conv3d.{weight,bias}`; `num_batches_tracked` and unknown keys are
    ignored), the layout the reference's commented-out loader reads (fvd.py:15-26).  The reference loads a TorchScript detector
    (`i3d_torchscript.pt`) at run time instead; equivalence of this class with that file is unpinned (the file is not available to
    the tests).  tests/fvd_ref.py restates the rules above in fp64; tests/golden/fvd_i3d.npz pins that restatement against
    pytorch_i3d.py and fvd.py with seeded weights, and the device results are checked against the restatement.

    Placement: device tensors give device rows on the current stream with no host synchronisation (graph-capturable once the
    weights are on the device: `model.to(device)` or a first call); CPU tensors are copied to the current GPU and the rows come
    back on the CPU.  Batches run in chunks that bound the scratch; a video's row does not depend on its position or on the batch
    size, bit for bit.  The rows are kept as a list (one per video) and the statistics are formed at `compute()`."""

    def __init__(self, bn_eps=FVD_BN_EPS, byte_range=False):
        self.bn_eps = float(bn_eps)
        self.byte_range = bool(byte_range)
        self._init_weights()
        self._rows = {True: [], False: []}

    _WHAT, _FLOATS = "FVD", "dc_fvd_weight_floats"
    _chunk_bytes = staticmethod(lambda: FVD_CHUNK_BYTES)

    def _pack(self, state_dict):
        return pack_fvd_weights(state_dict, self.bn_eps)

    @staticmethod
    def _check(videos, min_frames=FVD_MIN_FRAMES):
        """(n, t, h, w), element strides (n, t, c, h, w) of a uint8 NTHWC or floating NTCHW batch"""
        if videos.dim() != 5:
            raise ValueError(f"FVD takes 5-d video batches, got {tuple(videos.shape)}")
        if videos.dtype == torch.uint8:
            n, t, h, w, c = videos.shape
            sn, st, sh, sw, sc = videos.stride()
        elif videos.dtype.is_floating_point:
            n, t, c, h, w = videos.shape
            sn, st, sc, sh, sw = videos.stride()
        else:
            raise ValueError(f"FVD videos should be uint8 (NTHWC) or floating point (NTCHW), got {videos.dtype}")
        if c != 3:
            raise ValueError(f"FVD takes 3-channel videos, got {c} channels")
        if t < min_frames:
            raise ValueError(f"FVD needs at least {min_frames} frames per video, got {t}")
        if n < 1 or h < 1 or w < 1:
            raise ValueError(f"FVD needs N, H, W >= 1, got {tuple(videos.shape)}")
        return (n, t, h, w), (sn, st, sc, sh, sw)

    def _operand(self, videos, min_frames=FVD_MIN_FRAMES):
        dims, _ = self._check(videos, min_frames)
        X, _, host = self._stage(videos)
        return X, host, dims

    @staticmethod
    def _ws_bytes(t, h, w):
        """m -> dc_fvd_ws_bytes(m, t, h, w); a size the library refuses is a ValueError"""
        def ws_bytes(m):
            nbytes = lib.load().dc_fvd_ws_bytes(m, t, h, w)
            if nbytes < 0:
                raise ValueError(f"FVD takes videos of at most {FVD_MAX_FRAMES} frames of at most {FVD_MAX_SIDE} x {FVD_MAX_SIDE}, got {t} x {h} x {w}")
            return nbytes
        return ws_bytes

    def _chunks(self, n, t, h, w):
        return self._step(n, self._ws_bytes(t, h, w))

    def _call_args(self, xs, t, h, w):
        (m, _, _, _), strides = self._check(xs, 1)
        rh, rw = fvd_resized_size(h, w)
        u8 = xs.dtype == torch.uint8
        return (xs.data_ptr(), int(u8), int(u8 and not self.byte_range), (ctypes.c_longlong * 5)(*strides), m, t, h, w, rh, rw)

    def features(self, videos):
        """fp32 [N,400]: the logits of `videos` (uint8 [N,T,H,W,3] or floating [N,T,3,H,W])."""
        X, host, (n, t, h, w) = self._operand(videos)
        wts = self._weights(X.device)
        out = torch.empty((n, FVD_FEATURES), dtype=torch.float32, device=X.device)
        with torch.cuda.device(X.device):
            stream = torch.cuda.current_stream().cuda_stream
            for sl, scratch in self._slices(n, X.device, self._ws_bytes(t, h, w)):
                lib.call("dc_fvd_features", *self._call_args(X[sl], t, h, w), wts.data_ptr(), scratch.data_ptr(), out[sl].data_ptr(), stream)
        return out.cpu() if host else out

    def endpoints(self, videos):
        """The 16 endpoint maps (FVD_ENDPOINTS order), contiguous fp32 [N,C,T',S,S] (the test seam; `features` keeps them in scratch)."""
        X, host, (n, t, h, w) = self._operand(videos)
        wts = self._weights(X.device)
        outs = [torch.empty((n,) + s, dtype=torch.float32, device=X.device) for s in fvd_endpoint_shapes(t)]
        feat = torch.empty((n, FVD_FEATURES), dtype=torch.float32, device=X.device)
        with torch.cuda.device(X.device):
            stream = torch.cuda.current_stream().cuda_stream
            for sl, scratch in self._slices(n, X.device, self._ws_bytes(t, h, w)):
                maps = (ctypes.c_void_p * len(outs))(*[o[sl].data_ptr() for o in outs])
                lib.call("dc_fvd_endpoints", *self._call_args(X[sl], t, h, w), wts.data_ptr(), scratch.data_ptr(), maps,
                         feat[sl].data_ptr(), stream)
        return [o.cpu() for o in outs] if host else outs

    def preprocess(self, videos):
        """fp32 [N,3,T,224,224]: the network's input for `videos` (the test seam; any T >= 1)."""
        X, host, (n, t, h, w) = self._operand(videos, 1)
        out = torch.empty((n, 3, t, FVD_SIZE, FVD_SIZE), dtype=torch.float32, device=X.device)
        with torch.cuda.device(X.device):
            lib.call("dc_fvd_preprocess", *self._call_args(X, t, h, w), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        return out.cpu() if host else out

    def update_features(self, rows, real):
        """Add feature rows [N,400] (computed by `features`, here or on another rank) to the real or the fake side, in row order."""
        if rows.dim() != 2 or rows.shape[1] != FVD_FEATURES:
            raise ValueError(f"FVD feature rows should be [N,{FVD_FEATURES}], got {tuple(rows.shape)}")
        if rows.shape[0]:
            self._rows[bool(real)].append(rows.detach().float())

    def update(self, videos, real):
        """Add the videos' rows to the real (real=True) or the fake side."""
        self.update_features(self.features(videos), real)

    def reset(self):
        self._rows = {True: [], False: []}

    def count(self, real):
        return sum(r.shape[0] for r in self._rows[bool(real)])

    def compute(self):
        """The Frechet distance of the two sets as a Python float (synchronises: the rows are copied to the host)."""
        stats = []
        for side in (True, False):
            if self.count(side) < 2:
                raise RuntimeError("More than one sample is required for both the real and fake distributed to compute FID")
            stats.append(_fvd_stats(torch.cat([r.to("cpu", torch.float64) for r in self._rows[side]])))
        (mu_r, cov_r), (mu_f, cov_f) = stats
        return _frechet_value(mu_r, cov_r, mu_f, cov_f)


def calculate_fvd(videos1, videos2, model):
    """fvd_utils/my_utils.py:10-29 with `model` (a `FrechetVideoDistance` with weights loaded) in place of the detector it loads:
    two floating batches [B,T,C,H,W] of the same shape, grey (C = 1) repeated to 3 channels; videos1 is the generated side.  The
    model's accumulated rows are reset."""
    if videos1.shape != videos2.shape:
        raise ValueError(f"the two batches should have the same shape, got {tuple(videos1.shape)} and {tuple(videos2.shape)}")
    if videos1.dim() != 5 or not videos1.dtype.is_floating_point or not videos2.dtype.is_floating_point:
        raise ValueError(f"calculate_fvd takes floating [B,T,C,H,W] batches, got {tuple(videos1.shape)} {videos1.dtype}")
    if videos1.shape[2] == 1:
        videos1, videos2 = videos1.expand(-1, -1, 3, -1, -1), videos2.expand(-1, -1, 3, -1, -1)
    model.reset()
    model.update(videos1, real=False)
    model.update(videos2, real=True)
    return model.compute()
