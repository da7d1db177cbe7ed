"""Record the bits of the fp32 MFMA networks (csrc/lpips.hip, fid.hip, fvd.hip, cmp.hip) into tests/golden/f32_mfma_bits.json:
case name -> sha256 of the output bytes (`t.cpu().numpy().tobytes()`, contiguous little-endian), or, for the host-side planners,
the list of values they return.

    python tools/record_f32_bits.py [--lib PATH] [--cpu-only] [--out FILE]

`--lib` points diffcodec_amd.lib at another build of the same ABI (one process per library: `lib.load()` caches).  `--cpu-only`
records the rows that need no GPU (`CPU_CASES`: the weight packers and the planners) and keeps the GPU rows already in FILE.

The golden was recorded from the build that preceded the shared header csrc/dc_f32_mfma.h, twice, with identical files.  It pins
the order of the MFMAs and of every rounding in the epilogues: a change that reorders a sum fails tests/test_gpu_f32_bits.py even
though it would pass the fp64 comparisons of tests/test_gpu_{lpips,fid,fvd,cmp}.py.  A mismatch after a refactor means the
arithmetic changed: fix the code, do not record again.  A new network adds its rows here and records only those.

Inputs and seam weights come from numpy.random.RandomState (a frozen stream) seeded by the case name; conv weights are scaled
sqrt(2 / K).  The CPU rows of the packers use the seeded state dicts of tests/*_ref.py as they are."""
import argparse
import ctypes
import hashlib
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "f32_mfma_bits.json")
DEV = "cuda"


def rng(name):
    return np.random.RandomState(int(hashlib.sha256(name.encode()).hexdigest()[:8], 16))


FINITE = {}        # case name -> whether every hashed output element was finite (filled by `run`)
_finite = True


def sha(*tensors):
    global _finite
    h = hashlib.sha256()
    for t in tensors:
        _finite = _finite and bool(torch.isfinite(t).all())
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def run(name):
    """The row of case `name`.  A GPU case's output must be finite unless the case feeds a NaN and an inf on purpose: a golden of
    NaNs would pin nothing."""
    global _finite
    _finite = True
    row = (GPU_CASES.get(name) or CPU_CASES[name])(name)
    FINITE[name] = _finite
    assert _finite or name.endswith("_nonfinite"), f"{name}: a non-finite output"
    return row


def randn(r, *shape, scale=1.0):
    return torch.from_numpy((r.standard_normal(shape) * scale).astype(np.float32))


def rand_u8(r, *shape):
    return torch.from_numpy(r.randint(0, 256, shape).astype(np.uint8))


def numpy_state_dict(template, name):
    """`template`'s keys and shapes with values from the frozen stream: conv weights N(0, 2 / K), BatchNorm weight and running_var in
    [0.5, 1.5), biases and running_mean small."""
    r, sd = rng(name), {}
    for key in sorted(template):
        shape = tuple(template[key].shape)
        if key.endswith("num_batches_tracked"):
            sd[key] = template[key]
        elif len(shape) >= 4:
            sd[key] = randn(r, *shape, scale=math.sqrt(2.0 / max(1, int(np.prod(shape[1:])))))
        elif key.endswith(("running_var", ".weight")):
            sd[key] = torch.from_numpy((0.5 + r.random_sample(shape)).astype(np.float32))
        else:
            sd[key] = randn(r, *shape, scale=0.1)
    return sd


def unit(r, co, ci, *k):
    """(weight, bias, (gamma, beta, mean, var)) of one convolution with BatchNorm"""
    w = randn(r, co, ci, *k, scale=math.sqrt(2.0 / (ci * int(np.prod(k)))))
    bn = (torch.from_numpy((0.5 + r.random_sample(co)).astype(np.float32)), randn(r, co, scale=0.2), randn(r, co, scale=0.2),
          torch.from_numpy((0.5 + r.random_sample(co)).astype(np.float32)))
    return w, randn(r, co, scale=0.1), bn


def poison(x):
    """one NaN and one +inf, away from each other and from the borders' padding"""
    flat = x.view(-1)
    flat[flat.numel() // 3] = float("nan")
    flat[2 * flat.numel() // 3] = float("inf")
    return x


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _i64(v):
    return (ctypes.c_longlong * len(v))(*[int(a) for a in v])


def _cache(fn):
    memo = {}

    def get(*a):
        if a not in memo:
            memo[a] = fn(*a)
        return memo[a]
    return get


# ------------------------------------------------------------------------------------------------------------- LPIPS
@_cache
def lpips_weights():
    import lpips_ref
    from diffcodec_amd import metrics
    return metrics.pack_lpips_weights(numpy_state_dict(lpips_ref.synth_weights(), "lpips_weights")).to(DEV)


def u8_view(r, n, h, w):
    """a cropped window of a larger NHWC frame and its (n, c, h, w) element strides"""
    base = rand_u8(r, n, h + 4, w + 5, 3).to(DEV)
    x = base[:, 2:2 + h, 3:3 + w, :]
    return x, (x.stride(0), x.stride(3), x.stride(1), x.stride(2))


def lpips_conv(name, layer, h, w, form="f32", bad=False):
    from diffcodec_amd import lib, metrics
    r, M = rng(name), 2
    if layer == 0 and form == "u8":
        x, strides = u8_view(r, M, h, w)
        args = (x.data_ptr(), 1, _i64(strides), M, h, w, 0)
    elif layer == 0:
        x = torch.from_numpy(r.random_sample((M, 3, h, w)).astype(np.float32)).to(DEV)
        args = (x.data_ptr(), 0, _i64(x.stride()), M, h, w, 1)
    else:
        x = randn(r, M, metrics.LPIPS_CIN[layer], h, w)
        x = (poison(x) if bad else x).to(DEV)
        args = (x.data_ptr(), 0, None, M, h, w, 0)
    ho, wo = metrics.lpips_map_sizes(h, w)[0] if layer == 0 else (h, w)
    y = torch.full((M, metrics.LPIPS_CHANNELS[layer], ho, wo), 7.5, device=DEV)
    lib.call("dc_lpips_conv", layer, *args, lpips_weights().data_ptr(), y.data_ptr(), _stream())
    return sha(y)


def lpips_alex(name):
    from diffcodec_amd import lib
    r, n, h, w = rng(name), 2, 31, 47
    x, y = rand_u8(r, n, h, w, 3).to(DEV), rand_u8(r, n, h, w, 3).to(DEV)
    s = (x.stride(0), x.stride(3), x.stride(1), x.stride(2))
    ws = torch.empty(lib.load().dc_lpips_ws_bytes(n, h, w), dtype=torch.uint8, device=DEV)
    out = torch.zeros(6 * n, dtype=torch.float64, device=DEV)
    lib.call("dc_lpips_alex", x.data_ptr(), y.data_ptr(), 1, _i64(s + s), n, h, w, 0, 0, lpips_weights().data_ptr(), ws.data_ptr(),
             out.data_ptr(), _stream())
    return sha(out)


# ------------------------------------------------------------------------------------------------------------- FID
FID_IN = ((3, 299), (32, 149), (32, 147))
FID_OUT = ((32, 149), (32, 147), (64, 147))


@_cache
def fid_weights():
    import fid_ref
    from diffcodec_amd import metrics
    return metrics.pack_fid_weights(numpy_state_dict(fid_ref.synth_weights(), "fid_weights")).to(DEV)


def fid_conv(name, layer, bad=False):
    from diffcodec_amd import lib
    x = randn(rng(name), 1, FID_IN[layer][0], FID_IN[layer][1], FID_IN[layer][1])
    x = (poison(x) if bad else x).to(DEV)
    y = torch.full((1, FID_OUT[layer][0], FID_OUT[layer][1], FID_OUT[layer][1]), 7.5, device=DEV)
    lib.call("dc_fid_conv", layer, x.data_ptr(), 1, fid_weights().data_ptr(), y.data_ptr(), _stream())
    return sha(y)


def fid_features(name):
    from diffcodec_amd import lib
    n, h, w = 2, 17, 23
    x = rand_u8(rng(name), n, h, w, 3).to(DEV)
    ws = torch.empty(lib.load().dc_fid_ws_bytes(n, h, w), dtype=torch.uint8, device=DEV)
    out = torch.zeros(n, 64, device=DEV)
    lib.call("dc_fid_features", x.data_ptr(), 1, _i64((x.stride(0), x.stride(3), x.stride(1), x.stride(2))), n, h, w,
             fid_weights().data_ptr(), ws.data_ptr(), out.data_ptr(), _stream())
    return sha(out)


# ------------------------------------------------------------------------------------------------------------- FVD
def fvd_conv(name, k, stride, ci, co, dims, relu=1, bn=True, ctot=None, coff=0, bad=False, seed=None):
    from diffcodec_amd import lib, metrics
    r = rng(seed or name)
    x = randn(r, 1, ci, *dims)
    x = (poison(x) if bad else x).to(DEV)
    w, bias, (g, beta, mean, var) = unit(r, co, ci, k, k, k)
    s = g.double() / torch.sqrt(var.double() + 1e-5) if bn else torch.ones(co, dtype=torch.float64)
    t = beta.double() - mean.double() * s if bn else bias.double()
    packed = metrics.pack_fvd_unit(w, s, t).to(DEV)
    osz = [metrics.fvd_same_pad(v, k, stride)[0] for v in dims]
    ctot = co if ctot is None else ctot
    y = torch.full([1, ctot] + osz, 7.5, device=DEV)
    lib.call("dc_fvd_conv", x.data_ptr(), 1, ci, *dims, k, stride, packed.data_ptr(), co, relu, y.data_ptr(), ctot, coff, _stream())
    return sha(y)


def fvd_features(name):
    import fvd_ref
    from diffcodec_amd import metrics
    model = metrics.FrechetVideoDistance.from_state_dict(numpy_state_dict(fvd_ref.synth_weights(1234), "fvd_weights")).to(DEV)
    return sha(model.features(rand_u8(rng(name), 1, 9, 16, 24, 3).to(DEV)))


# ------------------------------------------------------------------------------------------------------------- CMP
def cmp_conv(name, shape, res=0, relu=1, sl=0, bad=False):
    """`shape`: the entry of tests/test_gpu_cmp.py's CONV_CASES of that name"""
    import cmp_ref
    from test_gpu_cmp import CONV_CASES
    from diffcodec_amd import flow_propagation as FP, lib
    N, ci, H, W, co, k, stride, dil, kind = CONV_CASES[shape]
    r = rng(name)
    if kind == "u8":
        x, strides = u8_view(r, N, H, W)
    else:
        x = randn(r, N, ci, H, W)
        x = (poison(x) if bad else x).to(DEV)
        strides = x.stride()
    w, bias, bn = unit(r, co, ci, k, k)
    packed = FP.fold_and_pack(w, bias, bn).to(DEV)
    pad = dil * (k - 1) // 2
    Ho, Wo = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    rd = randn(r, N, co, Ho, Wo).to(DEV) if res else None
    ctot, coff = (co + 7, 3) if sl else (co, 0)
    y = torch.full((N, ctot, Ho, Wo), 7.5, device=DEV)
    mean_div = (ctypes.c_float * 6)(*cmp_ref.DATA_MEAN, *cmp_ref.DATA_DIV)
    lib.call("dc_cmp_conv", x.data_ptr(), int(kind == "u8"), _i64(strides), mean_div, N, ci, H, W, k, stride, dil, packed.data_ptr(), co,
             None if rd is None else rd.data_ptr(), relu, y.data_ptr(), ctot, coff, _stream())
    return sha(y)


def cmp_head(name, ci, nbins, h, w, logits):
    from diffcodec_amd import flow_propagation as FP, lib
    r, N = rng(name), 2
    x = randn(r, N, ci, h, w).to(DEV)
    packed = FP.fold_and_pack(randn(r, 2 * nbins, ci, 1, 1, scale=6.0 / math.sqrt(ci)), randn(r, 2 * nbins), None).to(DEV)
    fl = torch.full((N, 2, h, w), 7.5, device=DEV)
    lg = torch.full((N, 2 * nbins, h, w), 7.5, device=DEV)
    lib.call("dc_cmp_head", x.data_ptr(), N, ci, h, w, packed.data_ptr(), nbins, 50.0, lg.data_ptr() if logits else None, fl.data_ptr(),
             _stream())
    return sha(fl, lg)


def cmp_flow(name, arch):
    import cmp_ref
    from diffcodec_amd.flow_propagation import HipCMP
    sd = numpy_state_dict(cmp_ref.synth_weights(arch), "cmp_weights_" + arch)
    model = HipCMP.from_state_dict(sd, cmp_ref.CONFIGS[arch], DEV)
    r = rng(name)
    image = rand_u8(r, 1, 64, 64, 3).to(DEV)
    sparse = torch.zeros(1, 4, 64, 64)
    sparse[:, :2, 4::8, 4::8] = randn(r, 1, 2, 8, 8, scale=5.0)
    sparse[:, 2:, 4::8, 4::8] = 1.0
    return sha(model.flow(image, sparse.to(DEV)))


GPU_CASES = {
    "lpips_conv0_u8_view_31x47": lambda n: lpips_conv(n, 0, 31, 47, "u8"),
    "lpips_conv0_f32_35x31_normalize": lambda n: lpips_conv(n, 0, 35, 31),
    "lpips_conv1_7x33": lambda n: lpips_conv(n, 1, 7, 33),
    "lpips_conv2_3x33": lambda n: lpips_conv(n, 2, 3, 33),
    "lpips_conv3_3x33": lambda n: lpips_conv(n, 3, 3, 33),
    "lpips_conv4_3x33": lambda n: lpips_conv(n, 4, 3, 33),
    "lpips_conv2_3x33_nonfinite": lambda n: lpips_conv(n, 2, 3, 33, bad=True),
    "lpips_alex_n2_u8_31x47": lpips_alex,
    "fid_conv0_n1": lambda n: fid_conv(n, 0),
    "fid_conv1_n1": lambda n: fid_conv(n, 1),
    "fid_conv2_n1": lambda n: fid_conv(n, 2),
    "fid_conv1_n1_nonfinite": lambda n: fid_conv(n, 1, bad=True),
    "fid_features_n2_u8_17x23": fid_features,
    "fvd_k7s2_3to64_3x9x35": lambda n: fvd_conv(n, 7, 2, 3, 64, (3, 9, 35)),
    "fvd_k3_6to40_2x5x33": lambda n: fvd_conv(n, 3, 1, 6, 40, (2, 5, 33)),
    "fvd_k3_16to96_3x7x7": lambda n: fvd_conv(n, 3, 1, 16, 96, (3, 7, 7)),
    "fvd_k1_40to33_1x3x43": lambda n: fvd_conv(n, 1, 1, 40, 33, (1, 3, 43)),
    "fvd_k1_64to400_logits_2x1x1": lambda n: fvd_conv(n, 1, 1, 64, 400, (2, 1, 1), relu=0, bn=False),
    "fvd_k3_6to40_2x5x33_slice45_off3": lambda n: fvd_conv(n, 3, 1, 6, 40, (2, 5, 33), ctot=45, coff=3, seed="fvd_k3_6to40_2x5x33"),
    "fvd_k3_6to40_2x5x33_nonfinite": lambda n: fvd_conv(n, 3, 1, 6, 40, (2, 5, 33), bad=True),
    "fvd_features_n1_t9_u8_16x24": fvd_features,
    "cmp_conv_stem_u8_view": lambda n: cmp_conv(n, "stem_u8_view"),
    "cmp_conv_sparse_5x5s2": lambda n: cmp_conv(n, "sparse_5x5s2"),
    "cmp_conv_c3_d2_9x11_res_relu": lambda n: cmp_conv(n, "c3_d2_9x11", res=1),
    "cmp_conv_c3_two_tiles": lambda n: cmp_conv(n, "c3_two_tiles"),
    "cmp_conv_pw_64to198_norelu_slice": lambda n: cmp_conv(n, "pw_64to198", relu=0, sl=1),
    "cmp_conv_c3_two_tiles_nonfinite": lambda n: cmp_conv(n, "c3_two_tiles", bad=True),
    "cmp_head_40_nbins40_9x15_logits": lambda n: cmp_head(n, 40, 40, 9, 15, True),
    "cmp_head_64_nbins112_8x8": lambda n: cmp_head(n, 64, 112, 8, 8, False),
    "cmp_flow_skip_64x64": lambda n: cmp_flow(n, "skip"),
    "cmp_flow_plain_64x64": lambda n: cmp_flow(n, "plain"),
}


# ------------------------------------------------------------------------------------------------------------- CPU rows
def _pack(which):
    import fid_ref
    import fvd_ref
    import lpips_ref
    from diffcodec_amd import metrics
    if which == "lpips":
        return sha(metrics.pack_lpips_weights(lpips_ref.synth_weights()))
    if which == "fid":
        return sha(metrics.pack_fid_weights(fid_ref.synth_weights()))
    return sha(metrics.pack_fvd_weights(fvd_ref.synth_weights(1234)))


def _fold_and_pack(name, bn):
    from diffcodec_amd import flow_propagation as FP
    w, bias, stats = unit(rng(name), 40, 6, 3, 3)
    return sha(FP.fold_and_pack(w, bias, stats if bn else None))


SIZES = ((0, 64, 64), (1, 0, 64), (1, 30, 31), (1, 31, 31), (1, 31, 47), (2, 64, 88), (3, 270, 480), (16, 512, 512), (1, 16384, 16384),
         (1, 16385, 64), (32767, 31, 31), (32768, 31, 31), (65535, 31, 31), (65536, 64, 64))


def _ws(fn, args):
    from diffcodec_amd import lib
    return [int(getattr(lib.load(), fn)(*a)) for a in args]


def _weight_floats(name):
    from diffcodec_amd import lib
    L = lib.load()
    return [L.dc_lpips_weight_floats(), L.dc_fid_weight_floats(), L.dc_fvd_weight_floats()] + \
        [L.dc_cmp_weight_floats(a, b) for a, b in ((0, 99), (1, 99), (0, 40), (1, 112), (0, 113), (2, 99), (0, 0))]


CPU_CASES = {
    "pack_lpips_weights": lambda n: _pack("lpips"),
    "pack_fid_weights": lambda n: _pack("fid"),
    "pack_fvd_weights": lambda n: _pack("fvd"),
    "fold_and_pack_bn": lambda n: _fold_and_pack(n, True),
    "fold_and_pack_plain": lambda n: _fold_and_pack(n, False),
    "dc_lpips_ws_bytes": lambda n: _ws(n, SIZES),
    "dc_lpips_features_ws_bytes": lambda n: _ws(n, SIZES),
    "dc_fid_ws_bytes": lambda n: _ws(n, SIZES),
    "dc_fvd_ws_bytes": lambda n: _ws(n, [(a, t, h, w) for a, h, w in SIZES[:8] + SIZES[-1:] for t in (8, 9, 16, 4096, 4097)]),
    "dc_cmp_ws_bytes": lambda n: _ws(n, [(arch, a, h, w) for arch in (0, 1, 2) for a, h, w in SIZES + ((1, 63, 64), (2, 56, 64), (1, 24, 64))]),
    "weight_floats": _weight_floats,
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libdiffcodec_hip.so (same ABI)")
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    if a.lib:
        from diffcodec_amd import lib
        lib.LIB_PATH = os.path.abspath(a.lib)
    rows = {}
    if a.cpu_only and os.path.exists(a.out):
        with open(a.out) as fh:
            rows = {k: v for k, v in json.load(fh).items() if k in GPU_CASES}
    for name in CPU_CASES:
        rows[name] = run(name)
    if not a.cpu_only:
        assert torch.cuda.is_available(), "the GPU rows need the GPU (--cpu-only records the rest)"
        for name in GPU_CASES:
            rows[name] = run(name)
            print(name, rows[name], "" if FINITE[name] else "(non-finite)", flush=True)
    with open(a.out, "w") as fh:
        json.dump(rows, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"wrote {len(rows)} rows to {a.out}")


if __name__ == "__main__":
    main()
