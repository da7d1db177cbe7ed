"""Frame quality metrics on the device: PSNR, SSIM and MS-SSIM (csrc/metrics.hip).

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


def summarize(scores):
    """Means over frames of {frame: {"psnr": dB, "ms_ssim": value}} (decode_clip(score=True)), following test_utils.py:49-55: a
    frame whose PSNR exceeds 1000 dB (identical images) is left out of both means.  Returns dict(psnr, ms_ssim, frames = the
    number averaged, identical = the number left out); the means are NaN when no frame is left."""
    kept = [s for _, s in sorted(scores.items()) if not s["psnr"] > 1000]
    m = len(kept)
    return dict(psnr=sum(s["psnr"] for s in kept) / m if m else float("nan"),
                ms_ssim=sum(s["ms_ssim"] for s in kept) / m if m else float("nan"),
                frames=m, identical=len(scores) - m)
