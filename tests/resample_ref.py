"""Integer numpy restatement of Pillow's 8-bit antialiased resize (Resample.c), written from its contract and independent of
diffcodec_amd.resample, plus the generator of tests/golden/pil_resample.npz (Pillow's own bytes for the small cases, so the result is
pinned whatever Pillow a machine carries).

    table of one axis (in -> out), float64 throughout:
        scale = in / out;  fs = max(scale, 1);  support = S * fs;  ksize = ceil(support) * 2 + 1;  ss = 1 / fs
        for xx in [0, out):  c = (xx + 0.5) * scale
                             xmin = max((int)(c - support + 0.5), 0);  xmax = min((int)(c + support + 0.5), in) - xmin
                             k[x] = filter((x + xmin - c + 0.5) * ss) for x in [0, xmax);  ww = sum k (index order);  k /= ww if ww != 0
                             K[x] = (int)(k * 2^22 - 0.5) if k < 0 else (int)(k * 2^22 + 0.5)               ((int) truncates)
    one sample:  clip(((1 << 21) + sum_x K[x] * in[xmin + x]) >> 22, 0, 255), int32, arithmetic shift
    passes:      horizontal if the widths differ, then vertical on its uint8 result if the heights differ; equal sizes: skipped

    python tests/resample_ref.py        regenerates the fixture (needs Pillow)"""
import math
import os

import numpy as np

FILTERS = ("bilinear", "bicubic", "lanczos")
SUPPORT = {"bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}
BITS = 22
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pil_resample.npz")

# (H, W) -> (h, w): the small cases of the fixture and of the device tests
SMALL_CASES = (((37, 53), (64, 41)), ((48, 90), (48, 48)), ((90, 48), (48, 48)), ((5, 3), (2, 7)), ((1, 1), (3, 2)), ((9, 9), (1, 1)),
               ((7, 200), (7, 3)), ((20, 300), (10, 600)), ((7, 200), (7, 5)))


def filter_value(name, x):
    if name == "bilinear":
        x = -x if x < 0.0 else x
        return 1.0 - x if x < 1.0 else 0.0
    if name == "bicubic":
        a = -0.5
        x = -x if x < 0.0 else x
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    if name == "lanczos":
        def sinc(v):
            if v == 0.0:
                return 1.0
            v = v * math.pi
            return math.sin(v) / v
        return sinc(x) * sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    raise ValueError(name)


def table(in_size, out_size, name):
    """(bounds int32 [out, 2], K int32 [out, ksize], ksize)"""
    scale = float(in_size) / float(out_size)
    fs = scale if scale > 1.0 else 1.0
    support = SUPPORT[name] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), np.int32)
    K = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        c = (xx + 0.5) * scale
        xmin = int(c - support + 0.5)                   # Python's int() truncates toward zero, as the C cast does
        xmin = 0 if xmin < 0 else xmin
        xmax = int(c + support + 0.5)
        xmax = (in_size if xmax > in_size else xmax) - xmin
        k = np.zeros(xmax, np.float64)
        ww = 0.0
        for x in range(xmax):
            k[x] = filter_value(name, (x + xmin - c + 0.5) * ss)
            ww += float(k[x])
        for x in range(xmax):
            v = float(k[x]) / ww if ww != 0.0 else float(k[x])
            K[xx, x] = int(v * (1 << BITS) - 0.5) if v < 0 else int(v * (1 << BITS) + 0.5)
        bounds[xx] = (xmin, xmax)
    return bounds, K, ksize


def _pass(a, axis, out_size, name, clip):
    """one pass of int64 sums along `axis` of a [..., H, W, C] array (axis = -3 or -2); clip=False returns the shifted sums"""
    bounds, K, _ = table(a.shape[axis], out_size, name)
    src = np.moveaxis(a, axis, -1).astype(np.int64)
    out = np.empty(src.shape[:-1] + (out_size,), np.int64)
    for o in range(out_size):
        lo, n = int(bounds[o, 0]), int(bounds[o, 1])
        acc = (1 << (BITS - 1)) + src[..., lo:lo + n] @ K[o, :n].astype(np.int64)
        assert np.all(np.abs(acc) < 2 ** 31)             # the device (and Pillow) sum in int32
        out[..., o] = acc >> BITS
    out = np.moveaxis(out, -1, axis)
    return np.clip(out, 0, 255).astype(np.uint8) if clip else out


def resize(a, size, name="bilinear"):
    """uint8 [..., H, W, C] -> uint8 [..., h, w, C], size = (h, w)"""
    h, w = size
    a = np.ascontiguousarray(a)
    if w != a.shape[-2]:
        a = _pass(a, -2, w, name, True)
    if h != a.shape[-3]:
        a = _pass(a, -3, h, name, True)
    return a.copy()


def first_pass_unclipped(a, size, name):
    """the shifted sums of the first pass that runs, before the clip to [0, 255] (int64): shows whether an input overshoots"""
    h, w = size
    if w != a.shape[-2]:
        return _pass(a, -2, w, name, False)
    return _pass(a, -3, h, name, False)


def random_bytes(shape, seed):
    """random bytes with saturated 0 / 255 regions"""
    g = np.random.default_rng(seed)
    a = g.integers(0, 256, shape, dtype=np.uint8)
    m = g.integers(0, 8, shape[:-1] + (1,))
    a = np.where(m == 0, 0, a)
    return np.where(m == 1, 255, a).astype(np.uint8)


def small_input(case, c=3):
    (h, w), _ = SMALL_CASES[case]
    return random_bytes((h, w, c), 1000 + case)


def checkerboard(h, w, c=3, period=3):
    """saturated 0 / 255 squares of `period` px"""
    y, x = np.mgrid[0:h, 0:w]
    a = np.where(((y // period) + (x // period)) % 2 == 0, 0, 255).astype(np.uint8)
    return np.repeat(a[:, :, None], c, axis=2)


def pillow_resize(a, size, name):
    """Pillow's own result for one [H,W,C] image, C = 1 (L), 3 (RGB) or 4 (CMYK: four independent channels; Pillow resizes RGBA
    through premultiplied alpha, which is a conversion around the resample and not part of it)"""
    from PIL import Image
    flt = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[name]
    mode = {1: "L", 3: "RGB", 4: "CMYK"}[a.shape[2]]
    img = Image.frombytes(mode, (a.shape[1], a.shape[0]), np.ascontiguousarray(a).tobytes())
    out = np.array(img.resize((size[1], size[0]), flt), dtype=np.uint8)
    return out.reshape(size[0], size[1], a.shape[2])


def make_golden(path=GOLDEN):
    """Pillow's bytes for the small cases, all three filters (inputs are regenerated from their seeds and stored too)"""
    import PIL
    data = {"pillow_version": np.array(PIL.__version__)}
    for i, (_, size) in enumerate(SMALL_CASES):
        a = small_input(i)
        data[f"in_{i}"] = a
        for name in FILTERS:
            data[f"out_{i}_{name}"] = pillow_resize(a, size, name)
    np.savez_compressed(path, **data)
    return path


if __name__ == "__main__":
    print(make_golden(), os.path.getsize(GOLDEN), "bytes")
