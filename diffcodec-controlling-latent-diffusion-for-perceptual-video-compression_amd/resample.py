"""Pillow's 8-bit antialiased resize on the device, bit for bit (csrc/resample.hip): `Image.resize(size, BILINEAR | BICUBIC |
LANCZOS)` of uint8 frames without the device -> host -> device round trip.

Where the reference resizes 8-bit images with Pillow around the decode path:

    test_utils.py:17-21     transforms.Resize((512, 512)) on both PIL frames before the five scores  -> "bilinear"
    utils.py:30-39          img.resize(size, Image.BICUBIC) of the anchors (and the ground truth)    -> "bicubic"
    uvc_codec_eval.py:37    img_b.resize((1920, 1080), Image.Resampling.LANCZOS), `resize=True`      -> "lanczos"

    # the classical-codec frames of uvc_codec_eval.py's resize=True path, x uint8 [N,h,w,3] on the device:
    up = resize_u8(x, (1080, 1920), "lanczos")          # Pillow's size is (w, h) = (1920, 1080); here it is (h, w)

What Pillow computes (Resample.c), per channel: a horizontal pass if the widths differ, then a vertical pass on its uint8 result
if the heights differ; a pass whose sizes agree is skipped.  The table of one axis (`coeffs`) is float64, the samples are integer:

    scale = in / out;  fs = max(scale, 1);  support = S * fs;  ksize = ceil(support) * 2 + 1
    per output xx:  c = (xx + 0.5) * scale;  xmin = max(int(c - support + 0.5), 0);  xmax = min(int(c + support + 0.5), in) - xmin
                    k[x] = filter((x + xmin - c + 0.5) * (1 / fs)), divided by their sum (in index order) when it is not zero
                    K[x] = int(k * 2^22 -+ 0.5)                                  (rounded half away from zero; int truncates)
    sample = clip(((1 << 21) + sum_x K[x] * in[xmin + x]) >> 22, 0, 255)          (int32, arithmetic shift)

Not covered: `box=`, `reducing_gap=`, modes other than 8 bits per channel, the NEAREST / BOX / HAMMING filters.

Placement as in `metrics`: device tensors give device results on the current stream; host tensors are copied to the current GPU
and the result comes back on the host.  There is no CPU compute path (`coeffs` alone needs neither the library nor a GPU)."""
import math

import torch

PRECISION_BITS = 22
FILTERS = ("bilinear", "bicubic", "lanczos")


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5                                            # Keys kernel, in Pillow's Horner form
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


_FILTER = {"bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0)}


def coeffs(in_size, out_size, filter):
    """The table of one axis: (bounds int32 [out, 2] = (xmin, xmax), K int32 [out, ksize], ksize), host tensors.  Python floats
    are C doubles and the expressions keep Pillow's operation order, so the integers are Pillow's."""
    if filter not in _FILTER:
        raise ValueError(f"resample filter should be one of {FILTERS}, got {filter!r}")
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"sizes should be >= 1, got {in_size} -> {out_size}")
    fn, s = _FILTER[filter]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = s * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    one = float(1 << PRECISION_BITS)
    bounds, rows = [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        row = [int(v * one - 0.5) if v < 0 else int(v * one + 0.5) for v in k]
        bounds.append((xmin, xmax))
        rows.append(row + [0] * (ksize - xmax))
    return torch.tensor(bounds, dtype=torch.int32), torch.tensor(rows, dtype=torch.int32).reshape(out_size, ksize), ksize


_TABLES = {}          # (device, in, out, filter) -> (bounds, K, ksize) on that device


def _table(device, in_size, out_size, filter):
    key = (device, in_size, out_size, filter)
    t = _TABLES.get(key)
    if t is None:
        b, k, ksize = coeffs(in_size, out_size, filter)
        t = _TABLES[key] = (b.to(device), k.to(device), ksize)
    return t


def resize_u8(frames, size, resample="bilinear"):
    """uint8 [N,H,W,C] or [H,W,C] (C in 1..4, any strides) -> contiguous uint8 [N,h,w,C] or [h,w,C] with size = (h, w): the bytes of
    Pillow's `Image.resize((w, h), resample)` per frame.  Tables are cached per (device, in, out, filter); a call whose tables are
    cached does no host synchronisation and allocates only the output and the intermediate through torch, so it can be captured in
    a graph.  Equal sizes on both axes return a copy."""
    from . import ops
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4):
        raise ValueError(f"resize_u8 takes uint8 [N,H,W,C] or [H,W,C] frames, got {frames.dtype} {tuple(frames.shape)}")
    if resample not in _FILTER:
        raise ValueError(f"resample should be one of {FILTERS}, got {resample!r}")
    h, w = (int(v) for v in size)
    x = frames if frames.dim() == 4 else frames.unsqueeze(0)
    n, hi, wi, c = x.shape
    if not 1 <= c <= 4 or min(n, hi, wi, h, w) < 1:
        raise ValueError(f"resize_u8 takes 1 to 4 channels and sizes >= 1, got {tuple(frames.shape)} -> {(h, w)}")
    host = not x.is_cuda
    if host:
        if not torch.cuda.is_available():
            raise RuntimeError("diffcodec_amd.resample computes on the GPU and none is available (there is no CPU path)")
        x = x.to(torch.device("cuda", torch.cuda.current_device()))
    if (h, w) == (hi, wi):
        out = x.clone(memory_format=torch.contiguous_format)
    else:
        out = ops.resample_u8(x, h, w, _table(x.device, wi, w, resample) if w != wi else None,
                              _table(x.device, hi, h, resample) if h != hi else None)
    if host:
        out = out.cpu()
    return out if frames.dim() == 4 else out[0]
