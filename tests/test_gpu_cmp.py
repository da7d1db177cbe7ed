"""GPU: the flow-propagation network of csrc/cmp.hip (diffcodec_amd.flow_propagation) against the fp64 restatement tests/cmp_ref.py
with seeded synthetic weights: every stage launcher on the smallest shapes that hit its masks, into guarded buffers, every output
element compared; then both decoders end to end at three sizes, exactness properties, graph capture and the clip source.

Bars.
  conv       max |dev - ref| / max |ref| <= (4 sqrt(K) + 4) 2^-24 with K = Cin k^2: an fp32 k-chain of K sequential additions, each
             rounding by at most 2^-24 of a partial sum no larger than about max |ref|, walks sqrt(K) 2^-24 away (one sigma; four
             sigma taken), plus one rounding each for s, t, the fma and the residual add.  A uint8 operand adds another
             4 sqrt(K) 2^-24: (v - mean) / div carries the roundings of the subtraction, the division and the two constants on
             every term.  A wrong tap, pad side, stride or mask is off by 1e-2 or more where it hits.
  pools      max-pool exact (no arithmetic); avg-pool 3 roundings of 2^-24 relative to the peak.
  upsample   4 x 2^-24 of the peak: two weights formed from an fp64 position rounded once, three nested fp32 blends.
  convert    2e-5 px: 99 fp32 exponentials at 1 ulp (2^-23 relative each, summed in fp64) move an expectation whose terms are
             bounded by fmax = 50 by at most 50 x 2 x 2^-23 = 1.2e-5 px, plus the final rounding of a value below 50 (3.8e-6).
  head       the fused head: logits at the conv bar, flow at the convert bar against the expectation of the device's own logits.
  grid       exact.
  network    per endpoint 4 x the reference's own fp32-minus-fp64 error from tests/golden/cmp_flow.npz (64 x 88, relative to
             the endpoint's peak; for the flow in pixels), the margin DESIGN.md section 9 gives "the same arithmetic in another
             order".  Reference fp32 error / peak at 64 x 88 (units of 1e-6), SkipLayer | Plain:
               sparse_enc 0.17 | 0.24   img_enc 1.80 | 2.12   skip2 0.39 | 0.32   skip4 0.47 | 0.52
               f8 1.49   f4 1.48   f2 1.92 | cat8 1.32          logits 1.24 | 1.67
               flow 3.75e-4 px | 3.78e-4 px                     flow_up 3.73e-4 px | 3.63e-4 px
Measured on an MI355X (worst of the three sizes, N = 2; the same units), SkipLayer | Plain, next to the reference's figures above:
               sparse_enc 0.20 | 0.20   img_enc 2.24 | 2.24   skip2 0.39 | 0.39   skip4 0.51 | 0.51
               f8 3.75   f4 3.61   f2 3.87 | cat8 2.33          logits 3.34 | 2.32
               flow 6.3e-4 px | 4.3e-4 px                       flow_up 6.2e-4 px | 4.3e-4 px
             i.e. 0.8 to 2.7 times the reference's own fp32 error; the 4 x bar holds.  Stage seams, worst case: conv 2.2e-6
             (Cin 384), avg-pool 7.7e-8, upsample 1.2e-7, convert 2.0e-6 px.  All figures go through `record`; DESIGN.md section 10."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

import cmp_ref as R
from edge_cases import Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cmp_flow.npz")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _i64(v):
    return (ctypes.c_longlong * len(v))(*[int(a) for a in v])


MEAN_DIV = (ctypes.c_float * 6)(*R.DATA_MEAN, *R.DATA_DIV)


def rel_err(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


# ------------------------------------------------------------------------------------------- dc_cmp_conv
# name: (N, Cin, H, W, Cout, k, stride, dilation, operand)
CONV_CASES = {
    "stem_f32": (2, 3, 13, 18, 64, 7, 2, 1, "f32"),
    "stem_u8_view": (2, 3, 13, 18, 64, 7, 2, 1, "u8"),
    "sparse_5x5s2": (3, 4, 13, 18, 16, 5, 2, 1, "f32"),
    "pw_64to256": (3, 64, 9, 11, 256, 1, 1, 1, "f32"),
    "pw_2048to256": (2, 2048, 8, 8, 256, 1, 1, 1, "f32"),
    "pw_64to198": (2, 64, 12, 13, 198, 1, 1, 1, "f32"),
    "pw_s2_96to64": (3, 96, 9, 11, 64, 1, 2, 1, "f32"),
    "c3_s1": (3, 64, 9, 11, 64, 3, 1, 1, "f32"),
    "c3_s2_odd": (3, 64, 9, 11, 64, 3, 2, 1, "f32"),
    "c3_s2_even": (2, 64, 8, 12, 64, 3, 2, 1, "f32"),
    "c3_d2_8x8": (2, 64, 8, 8, 64, 3, 1, 2, "f32"),
    "c3_d2_9x11": (3, 64, 9, 11, 64, 3, 1, 2, "f32"),
    "c3_d4_8x8": (2, 64, 8, 8, 64, 3, 1, 4, "f32"),
    "c3_d4_9x11": (3, 64, 9, 11, 64, 3, 1, 4, "f32"),
    "c3_cin272": (2, 272, 9, 11, 128, 3, 1, 1, "f32"),
    "c3_cin384": (2, 384, 9, 11, 128, 3, 1, 1, "f32"),
    "c3_cin160": (2, 160, 9, 11, 64, 3, 1, 1, "f32"),
    "c3_two_tiles": (2, 16, 12, 13, 16, 3, 1, 1, "f32"),
}
VARIANTS = [(res, relu, sl) for res in (0, 1) for relu in (0, 1) for sl in (0, 1)]
CONV_PARAMS = [(name, VARIANTS[(3 * i + j) % 8]) for i, name in enumerate(CONV_CASES) for j in (0, 5)]
CONV_PARAMS += [("c3_s1", v) for v in VARIANTS if ("c3_s1", v) not in CONV_PARAMS]


def conv_operands(name):
    N, ci, H, W, co, k, stride, dil, kind = CONV_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    sd = {"c.weight": torch.randn(co, ci, k, k, generator=g) * math.sqrt(2.0 / (ci * k * k)), "c.bias": 0.1 * torch.randn(co, generator=g),
          "b.weight": 0.5 + torch.rand(co, generator=g), "b.bias": 0.2 * torch.randn(co, generator=g),
          "b.running_mean": 0.2 * torch.randn(co, generator=g), "b.running_var": 0.5 + torch.rand(co, generator=g)}
    if kind == "u8":                                                                       # a cropped window of a larger NHWC frame
        base = torch.randint(0, 256, (N, H + 4, W + 5, 3), generator=g, dtype=torch.uint8)
        x = base[:, 2:2 + H, 3:3 + W, :]
        x64 = R.normalise(x)
    else:
        base = x = torch.randn(N, ci, H, W, generator=g)
        x64 = x.double()
    return sd, base, x, x64, g


@pytest.mark.parametrize("name,variant", CONV_PARAMS, ids=[f"{n}-res{v[0]}relu{v[1]}slice{v[2]}" for n, v in CONV_PARAMS])
def test_conv(record, name, variant):
    from diffcodec_amd import flow_propagation as FP, lib
    N, ci, H, W, co, k, stride, dil, kind = CONV_CASES[name]
    res, relu, sl = variant
    sd, base, x, x64, g = conv_operands(name)
    w, s, t = R.fold(sd, "c", "b")
    pad = dil * (k - 1) // 2
    Ho, Wo = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    r = torch.randn(N, co, Ho, Wo, generator=g) if res else None
    want = R.conv(x64, w, s, t, stride, dil, None if r is None else r.double(), bool(relu))
    assert want.shape == (N, co, Ho, Wo)
    packed = FP.fold_and_pack(sd["c.weight"], sd["c.bias"], tuple(sd["b." + q] for q in ("weight", "bias", "running_mean", "running_var"))).to(DEV)
    ctot, coff = (co + 7, 3) if sl else (co, 0)
    out = Guarded((N, ctot, Ho, Wo), torch.float32, DEV)
    bdev = base.to(DEV)
    if kind == "u8":
        xd = bdev[:, 2:2 + H, 3:3 + W, :]
        strides = (xd.stride(0), xd.stride(3), xd.stride(1), xd.stride(2))
    else:
        xd = bdev
        strides = xd.stride()
    rd = None if r is None else r.to(DEV)
    lib.call("dc_cmp_conv", xd.data_ptr(), int(kind == "u8"), _i64(strides), MEAN_DIV, N, ci, H, W, k, stride, dil, packed.data_ptr(), co,
             None if rd is None else rd.data_ptr(), relu, out.view.data_ptr(), ctot, coff, _stream())
    torch.cuda.synchronize()
    out.assert_intact(name)
    assert out.unwritten() == N * (ctot - co) * Ho * Wo                                    # the neighbours hold the pattern, the slice none
    got = out.view[:, coff:coff + co]
    assert torch.isfinite(got).all()
    K = ci * k * k
    bar = ((8 if kind == "u8" else 4) * math.sqrt(K) + 4) * U
    e = rel_err(got, want)
    record(f"cmp_conv_{name}_res{res}relu{relu}slice{sl}", e)
    assert e <= bar, (e, bar)


def test_conv_refusals():
    from diffcodec_amd import lib
    x = torch.zeros(1, 4, 8, 8, device=DEV)
    p = torch.zeros(66 * 32, device=DEV)                                                    # 64 rows + s + t of 32 columns
    y = torch.zeros(1, 4, 8, 8, device=DEV)
    ok = dict(k=3, stride=1, dil=1, cout=4, ctot=4, coff=0, u8=0)
    for bad in (dict(k=2), dict(k=9), dict(stride=3), dict(dil=3), dict(coff=1), dict(ctot=3), dict(u8=1)):
        a = {**ok, **bad}
        with pytest.raises(lib.HipLaunchError):
            lib.call("dc_cmp_conv", x.data_ptr(), a["u8"], _i64(x.stride()), MEAN_DIV, 1, 4, 8, 8, a["k"], a["stride"], a["dil"], p.data_ptr(),
                     a["cout"], None, 0, y.data_ptr(), a["ctot"], a["coff"], _stream())


# ------------------------------------------------------------------------------------------- pools
@pytest.mark.parametrize("k,stride,pad,H,W", [(3, 2, 1, 9, 11), (3, 2, 1, 8, 12), (8, 8, 0, 9, 11), (2, 2, 0, 9, 11), (4, 4, 0, 9, 11),
                                               (2, 2, 0, 16, 22)])
def test_maxpool_is_exact_on_negative_maps(k, stride, pad, H, W):
    from diffcodec_amd import lib
    g = torch.Generator().manual_seed(k * 100 + H)
    x = -1.0 - torch.rand(3, 5, H, W, generator=g)                                         # a zero padding would win every border max
    want = R.max_pool(x.double(), k, stride, pad)
    out = Guarded(tuple(want.shape), torch.float32, DEV)
    lib.call("dc_cmp_maxpool", x.to(DEV).data_ptr(), 15, H, W, k, stride, pad, out.view.data_ptr(), _stream())
    torch.cuda.synchronize()
    out.assert_intact("maxpool")
    assert out.unwritten() == 0
    assert torch.equal(out.view.cpu().double(), want)
    if (k, H, W) == (8, 9, 11):
        assert want.shape[2:] == (1, 1)
    if (k, H, W) == (2, 9, 11):
        assert want.shape[2:] == (4, 5)


def test_maxpool_refuses_an_empty_map_and_keeps_nan():
    from diffcodec_amd import lib
    x = torch.zeros(1, 1, 7, 9, device=DEV)
    y = torch.zeros(16, device=DEV)
    with pytest.raises(lib.HipLaunchError):
        lib.call("dc_cmp_maxpool", x.data_ptr(), 1, 7, 9, 8, 8, 0, y.data_ptr(), _stream())
    x = torch.zeros(1, 1, 4, 4, device=DEV)
    x[0, 0, 1, 1] = float("nan")
    y = torch.zeros(1, 1, 2, 2, device=DEV)
    lib.call("dc_cmp_maxpool", x.data_ptr(), 1, 4, 4, 2, 2, 0, y.data_ptr(), _stream())
    assert torch.isnan(y[0, 0, 0, 0]) and torch.equal(y.flatten()[1:].cpu(), torch.zeros(3))


@pytest.mark.parametrize("H,W,sl", [(9, 11, 0), (8, 12, 1), (17, 22, 1), (2, 3, 0)])
def test_avgpool(record, H, W, sl):
    from diffcodec_amd import lib
    g = torch.Generator().manual_seed(H * 31 + W)
    x = torch.randn(3, 5, H, W, generator=g) - 1.0
    want = R.avg_pool(x.double())
    ctot, coff = (9, 2) if sl else (5, 0)
    out = Guarded((3, ctot, H // 2, W // 2), torch.float32, DEV)
    lib.call("dc_cmp_avgpool", x.to(DEV).data_ptr(), 3, 5, H, W, out.view.data_ptr(), ctot, coff, _stream())
    torch.cuda.synchronize()
    out.assert_intact("avgpool")
    assert out.unwritten() == 3 * (ctot - 5) * (H // 2) * (W // 2)
    e = rel_err(out.view[:, coff:coff + 5], want)
    record(f"cmp_avgpool_{H}x{W}", e)
    assert e <= 3 * U


# ------------------------------------------------------------------------------------------- upsample
@pytest.mark.parametrize("H,W,Ho,Wo", [(1, 1, 9, 11), (1, 5, 9, 11), (9, 11, 9, 11), (4, 5, 9, 11), (8, 11, 16, 22), (32, 44, 64, 88),
                                       (3, 4, 1, 1)])
def test_upsample_into_a_channel_slice(record, H, W, Ho, Wo):
    from diffcodec_amd import lib
    g = torch.Generator().manual_seed(H * 131 + Wo)
    x = torch.randn(2, 3, H, W, generator=g)
    want = R.upsample(x.double(), Ho, Wo)
    torch_says = torch.nn.functional.interpolate(x.double(), size=(Ho, Wo), mode="bilinear", align_corners=True)
    assert float((want - torch_says).abs().max()) < 1e-12                                   # the restatement is torch's rule
    out = Guarded((2, 7, Ho, Wo), torch.float32, DEV)
    lib.call("dc_cmp_upsample", x.to(DEV).data_ptr(), 2, 3, H, W, Ho, Wo, out.view.data_ptr(), 7, 2, _stream())
    torch.cuda.synchronize()
    out.assert_intact("upsample")
    assert out.unwritten() == 2 * 4 * Ho * Wo
    got = out.view[:, 2:5]
    e = rel_err(got, want)
    record(f"cmp_upsample_{H}x{W}_to_{Ho}x{Wo}", e)
    assert e <= 4 * U
    if (H, W) == (1, 1):
        assert torch.equal(got.cpu(), x.expand(2, 3, Ho, Wo))                              # a constant
    if (H, W) == (Ho, Wo):
        assert torch.equal(got.cpu(), x)                                                    # the identity


# ------------------------------------------------------------------------------------------- logits -> flow
def _convert(lg, nbins=99, fmax=50.0):
    from diffcodec_amd import lib
    N, _, h, w = lg.shape
    out = Guarded((N, 2, h, w), torch.float32, DEV)
    lib.call("dc_cmp_convert_flow", lg.to(DEV).data_ptr(), N, nbins, h, w, fmax, out.view.data_ptr(), _stream())
    torch.cuda.synchronize()
    out.assert_intact("convert_flow")
    assert out.unwritten() == 0
    return out.view.cpu()


def test_convert_flow(record):
    g = torch.Generator().manual_seed(5)
    lg = 6.0 * torch.randn(3, 198, 5, 7, generator=g)
    got = _convert(lg)
    want = R.convert_flow(lg.double())
    e = float((got.double() - want).abs().max())
    record("cmp_convert_flow_abs_err_px", e)
    assert e <= 2e-5 and float(want.std()) > 5.0


def test_convert_flow_edges():
    big = torch.where(torch.rand(2, 198, 3, 4, generator=torch.Generator().manual_seed(6)) > 0.5, 1e3, -1e3)
    big[:, 0], big[:, 99] = 1e3, 1e3                                                        # at least one maximum per half
    got = _convert(big)
    assert torch.isfinite(got).all()
    assert float((got.double() - R.convert_flow(big.double())).abs().max()) <= 2e-5
    flat = torch.full((1, 198, 2, 3), 7.25)
    assert float(_convert(flat).abs().max()) < 1e-5                                         # the centres are symmetric about zero
    step = 100.0 / 99
    for b, centre in ((0, -50 + step / 2), (98, 50 - step / 2)):
        hot = torch.full((1, 198, 2, 2), -1e3)
        hot[:, b], hot[:, 99 + b] = 1e3, 1e3
        assert float((_convert(hot).double() - centre).abs().max()) <= 4e-6                 # one rounding of a value below 50


# ------------------------------------------------------------------------------------------- the fused head
@pytest.mark.parametrize("N,ci,h,w,want_logits", [(3, 64, 9, 11, 1), (2, 64, 12, 13, 0), (2, 384, 8, 11, 1), (2, 384, 1, 1, 0)])
def test_fused_head(record, N, ci, h, w, want_logits):
    """logits: the conv bar; flow against the expectation of the device's own logits: the convert bar (2e-5 px); flow against the
    fp64 chain: 2e-5 + 2 fmax eps, eps the logits' bar in absolute terms (d flow / d logit_i = p_i (c_i - flow), sum_i p_i |c_i - flow|
    <= 2 fmax)."""
    from diffcodec_amd import flow_propagation as FP, lib
    g = torch.Generator().manual_seed(ci + h)
    wgt = torch.randn(198, ci, 1, 1, generator=g) * (6.0 / math.sqrt(ci))
    bias = torch.randn(198, generator=g)
    x = torch.randn(N, ci, h, w, generator=g)
    want_lg = R.conv(x.double(), wgt.double(), torch.ones(198, dtype=torch.float64), bias.double(), relu=False)
    want_fl = R.convert_flow(want_lg)
    packed = FP.fold_and_pack(wgt, bias, None).to(DEV)
    fl = Guarded((N, 2, h, w), torch.float32, DEV)
    lg = Guarded((N, 198, h, w), torch.float32, DEV)
    lib.call("dc_cmp_head", x.to(DEV).data_ptr(), N, ci, h, w, packed.data_ptr(), 99, 50.0, lg.view.data_ptr() if want_logits else None,
             fl.view.data_ptr(), _stream())
    torch.cuda.synchronize()
    fl.assert_intact("head flow")
    lg.assert_intact("head logits")
    assert fl.unwritten() == 0 and lg.unwritten() == (0 if want_logits else N * 198 * h * w)   # logits only on request
    eps = (4 * math.sqrt(ci) + 4) * U * float(want_lg.abs().max())
    e = float((fl.view.double().cpu() - want_fl).abs().max())
    record(f"cmp_head_{ci}_{h}x{w}_flow_abs_err_px", e)
    assert e <= 2e-5 + 100.0 * eps, (e, eps)
    assert float(want_fl.std()) > 5.0 or h * w == 1
    if want_logits:
        el = float((lg.view.double().cpu() - want_lg).abs().max())
        record(f"cmp_head_{ci}_{h}x{w}_logits_abs_err", el)
        assert el <= eps, (el, eps)
        assert float((fl.view.double().cpu() - R.convert_flow(lg.view.double().cpu())).abs().max()) <= 2e-5
        ref = Guarded((N, 198, h, w), torch.float32, DEV)                                   # the unfused pair gives the same logits
        xd = x.to(DEV)
        lib.call("dc_cmp_conv", xd.data_ptr(), 0, _i64(xd.stride()), MEAN_DIV, N, ci, h, w, 1, 1, 1, packed.data_ptr(), 198, None, 0,
                 ref.view.data_ptr(), 198, 0, _stream())
        torch.cuda.synchronize()
        assert torch.equal(ref.view, lg.view)


def test_network_launchers_refuse():
    from diffcodec_amd import lib
    model = model_of("plain")
    with pytest.raises(ValueError):
        model.flow(torch.zeros(1, 24, 64, 3, dtype=torch.uint8, device=DEV), torch.zeros(1, 4, 24, 64, device=DEV))
    x = torch.zeros(1, 4, 8, 8, device=DEV)
    with pytest.raises(lib.HipLaunchError):                                                 # nbins beyond the head's seven tiles
        lib.call("dc_cmp_head", x.data_ptr(), 1, 4, 8, 8, x.data_ptr(), 113, 50.0, None, x.data_ptr(), _stream())


# ------------------------------------------------------------------------------------------- grid sampling
@pytest.mark.parametrize("H,W,stride", [(9, 11, 1), (9, 11, 16), (64, 88, 8), (13, 18, 5), (16, 24, 8)])
def test_sample_grid(H, W, stride):
    from diffcodec_amd import lib
    g = torch.Generator().manual_seed(H + stride)
    flow = torch.randn(2, 2, H, W, generator=g)
    want = R.sparse_grid(flow.double(), stride)
    out = Guarded((2, 4, H, W), torch.float32, DEV)
    lib.call("dc_cmp_sparse_grid", flow.to(DEV).data_ptr(), 2, H, W, stride, out.view.data_ptr(), _stream())
    torch.cuda.synchronize()
    out.assert_intact("sparse_grid")
    assert out.unwritten() == 0
    assert torch.equal(out.view.cpu().double(), want)
    ys, xs = R.grid_points(H, W, stride)
    assert int(want[0, 2].sum()) == len(ys) * len(xs)
    if stride == 16:
        assert (len(ys), len(xs)) == (1, 1)                                                 # a stride larger than the map: one point
    if stride == 1:
        assert torch.equal(out.view[:, :2].cpu(), flow)


# ------------------------------------------------------------------------------------------- the whole network
SIZES = [(64, 64), (64, 88), (72, 64)]


@functools.lru_cache(maxsize=None)
def weights(arch):
    return R.synth_weights(arch)


@functools.lru_cache(maxsize=None)
def model_of(arch):
    from diffcodec_amd.flow_propagation import HipCMP
    return HipCMP.from_state_dict({"state_dict": {"module." + k: v for k, v in weights(arch).items()}}, R.CONFIGS[arch], DEV)


@functools.lru_cache(maxsize=None)
def case(arch, size):
    """(uint8 frames, sparse, fp64 endpoints of the restatement); computed once and left unchanged"""
    u8, sparse = R.inputs(2, size[0], size[1], 900 + size[0] + size[1])
    with torch.no_grad():
        return u8, sparse, R.endpoints(R.normalise(u8), sparse, weights(arch), arch)


@functools.lru_cache(maxsize=None)
def bars(arch):
    """name -> (bar, absolute?): 4 x the reference's own fp32 error (relative to the peak; in pixels for the flow)"""
    z = np.load(GOLDEN)
    return {n: ((4 * float(z[f"{arch}_{n}_err32"]), True) if n.startswith("flow") else
                (4 * float(z[f"{arch}_{n}_err32"]) / float(z[f"{arch}_{n}_peak"]), False)) for n in R.ENDPOINTS[arch]}


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("arch", ["skip", "plain"])
def test_network(record, arch, size):
    """Measured device errors: the table in this file's docstring and in DESIGN.md section 10 (SkipLayer logits 3.3e-6 of the peak
    against a bar of 5.0e-6, flow 6.3e-4 px against 1.5e-3); each figure is printed and recorded before the assertion."""
    model = model_of(arch)
    u8, sparse, want = case(arch, size)
    ud, sd_ = u8.to(DEV), sparse.to(DEV)
    got = model.endpoints(ud, sd_)
    torch.cuda.synchronize()
    assert set(got) == set(R.ENDPOINTS[arch])
    failures = []
    for name in R.ENDPOINTS[arch]:
        assert got[name].shape == want[name].shape, name
        bar, absolute = bars(arch)[name]
        d = float((got[name].double().cpu() - want[name]).abs().max())
        e = d if absolute else d / float(want[name].abs().max())
        record(f"cmp_{arch}_{size[0]}x{size[1]}_{name}", e)
        print(f"{arch} {size} {name}: {e:.3e} (bar {bar:.3e})")
        if not e <= bar:
            failures.append((name, e, bar))
    assert not failures, failures
    if size == (64, 88):                                                                    # the condition measures something, on the device's own numbers
        lg = got["logits"].double().cpu()
        pk = torch.maximum(torch.softmax(lg[:, :99], 1).max(1).values, torch.softmax(lg[:, 99:], 1).max(1).values)
        assert float((pk > 0.99).double().mean()) < 0.25 and float(got["flow"].std()) > 5.0
    # the C chain and the chain driven stage by stage from Python run the same launches: the same bits
    staged = model.staged_endpoints(ud, sd_)
    for name in R.ENDPOINTS[arch]:
        assert torch.equal(staged[name], got[name]), name
    # the interface's three calls are the same numbers
    lg = model(ud, sd_)
    fl = model.flow(ud, sd_)
    assert torch.equal(lg, got["logits"]) and torch.equal(fl, got["flow_up"])              # run to run, bitwise
    assert lg.shape[1] == 198 and fl.shape == (2, 2, size[0], size[1])
    # an already normalised fp32 operand: fp32 division on the host, so the same bar, not the same bits
    f32 = model(R.normalise(u8, torch.float32).to(DEV), sd_)
    bar, _ = bars(arch)["logits"]
    assert rel_err(f32, want["logits"]) <= bar
    # sample 0 of N = 2 is the N = 1 result, bit for bit; so is sample 1 moved to position 0
    one = model.endpoints(ud[:1], sd_[:1])
    for name in ("logits", "flow_up"):
        assert torch.equal(one[name], got[name][:1]), name
    assert torch.equal(model(ud.flip(0), sd_.flip(0)), lg.flip(0))
    # the sparse operand matters
    z = model(ud, torch.zeros_like(sd_))
    change = float((z - lg).abs().max() / lg.abs().max())
    record(f"cmp_{arch}_{size[0]}x{size[1]}_zero_sparse_change", change)
    assert change > 20 * bar, (change, bar)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("arch", ["skip", "plain"])
def test_flow_is_graph_capturable(arch, size):
    model = model_of(arch)
    u8, sparse, _ = case(arch, size)
    x, sp = u8.to(DEV), sparse.to(DEV)
    y = x.flip(0).contiguous()
    fx, fy = model.flow(x, sp), model.flow(y, sp)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.flow(x, sp)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = model.flow(x, sp)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, fx)
    x.copy_(y)                                                                              # replay reads the captured operand
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, fy) and not torch.equal(fx, fy)


# ------------------------------------------------------------------------------------------- the caller-owned workspace
# (N, H, W, image form): an odd batch at the size whose 1/8 map (8 x 11) is ragged, as normalised fp32 NCHW; H / 8 = 9 odd (the
# decoder pools 9 -> 4 -> 2 leave a remainder), as a uint8 NHWC window cropped from a larger frame
WS_CASES = [(3, 64, 88, "f32"), (2, 72, 64, "u8_view")]


def _ws_inputs(N, H, W, form, seed):
    """(what keeps the storage alive, image operand on the device, its element strides (n, c, h, w), sparse on the device)"""
    u8, sparse = R.inputs(N, H, W, seed)
    if form == "f32":
        img = R.normalise(u8, torch.float32).contiguous().to(DEV)
        return img, img, img.stride(), sparse.to(DEV)
    base = torch.full((N, H + 4, W + 5, 3), 77, dtype=torch.uint8)
    base[:, 2:2 + H, 3:3 + W] = u8
    bdev = base.to(DEV)
    img = bdev[:, 2:2 + H, 3:3 + W, :]
    return bdev, img, (img.stride(0), img.stride(3), img.stride(1), img.stride(2)), sparse.to(DEV)


@pytest.mark.parametrize("N,H,W,form", WS_CASES, ids=[f"n{c[0]}_{c[1]}x{c[2]}_{c[3]}" for c in WS_CASES])
@pytest.mark.parametrize("arch", ["skip", "plain"])
def test_chain_on_a_guarded_workspace_of_any_contents(record, arch, N, H, W, form):
    """dc_cmp_forward, dc_cmp_flow and dc_cmp_endpoints on a guarded workspace of exactly dc_cmp_ws_bytes under the NaN, zero and
    stale fills, every map pointer a guarded output: the bits HipCMP's __call__ / flow / endpoints return (the wrapper keeps one
    torch.empty workspace from call to call)"""
    import edge_cases as E
    from diffcodec_amd import lib
    from diffcodec_amd.flow_propagation import stage_sizes
    model = model_of(arch)
    sets = [_ws_inputs(N, H, W, form, seed) for seed in (900 + H + W + N, 977)]
    s2, s4, s8 = stage_sizes(model.config, H, W)
    top = s2 if model.skip else s8
    f32 = torch.float32
    maps = [(16, s8), (256, s8), (64, s2), (256, s4)] + ([(256, s8), (128, s4), (64, s2)] if model.skip else [(384, s8)])
    shape = lambda c, hw: ((N, c, hw[0], hw[1]), f32)
    names = R.ENDPOINTS[arch]
    nbytes = lib.load().dc_cmp_ws_bytes(model.arch, N, H, W)

    def head(ws, prime):
        _, img, strides, sparse = sets[int(prime)]
        return (model.arch, img.data_ptr(), int(form != "f32"), _i64(strides), sparse.data_ptr(), N, H, W, model.nbins, model.fmax,
                model.weights.data_ptr(), ws.data_ptr())

    def forward(ws, outs, prime):
        lib.call("dc_cmp_forward", *head(ws, prime), outs[0].data_ptr(), outs[1].data_ptr(), _stream())

    def flow(ws, outs, prime):
        lib.call("dc_cmp_flow", *head(ws, prime), outs[0].data_ptr(), _stream())

    def endpoints(ws, outs, prime):
        ptrs = (ctypes.c_void_p * len(maps))(*[o.data_ptr() for o in outs[:len(maps)]])
        lib.call("dc_cmp_endpoints", *head(ws, prime), ptrs, *[o.data_ptr() for o in outs[len(maps):]], _stream())

    tag = f"{arch} {N}x{H}x{W} {form}"
    _, img, _, sparse = sets[0]
    want = model.endpoints(img, sparse)
    assert list(want) == list(names)
    (lg, fl), share = E.run_on_fills(forward, nbytes, [shape(2 * model.nbins, top), shape(2, top)], f"dc_cmp_forward {tag}", device=DEV)
    record(f"ws_unwritten_share[dc_cmp_forward {tag}]", share)
    assert torch.equal(E.ws_bits(lg), E.ws_bits(model(img, sparse))) and torch.equal(E.ws_bits(fl), E.ws_bits(want["flow"]))
    (up,), share = E.run_on_fills(flow, nbytes, [shape(2, (H, W))], f"dc_cmp_flow {tag}", device=DEV)
    record(f"ws_unwritten_share[dc_cmp_flow {tag}]", share)
    assert torch.equal(E.ws_bits(up), E.ws_bits(model.flow(img, sparse)))
    outputs = [shape(c, hw) for c, hw in maps] + [shape(2 * model.nbins, top), shape(2, top), shape(2, (H, W))]
    outs, share = E.run_on_fills(endpoints, nbytes, outputs, f"dc_cmp_endpoints {tag}", device=DEV)
    record(f"ws_unwritten_share[dc_cmp_endpoints {tag}]", share)
    assert len(outs) == len(names)
    for name, o in zip(names, outs):
        assert torch.equal(E.ws_bits(o), E.ws_bits(want[name])), (tag, name)


def test_sizes_are_refused_on_the_device_too():
    model = model_of("skip")
    for h in (68, 56):
        with pytest.raises(ValueError):
            model(torch.zeros(1, h, 64, 3, dtype=torch.uint8, device=DEV), torch.zeros(1, 4, h, 64, device=DEV))
    with pytest.raises(ValueError):
        model(torch.zeros(1, 64, 64, 3, dtype=torch.uint8, device=DEV), torch.zeros(1, 4, 64, 72, device=DEV))


# ------------------------------------------------------------------------------------------- clip source
def test_propagated_flow_source_is_two_direct_calls():
    from diffcodec_amd.clip_decode import SyntheticSource
    from diffcodec_amd.flow_propagation import PropagatedFlowSource, anchors_u8, sample_grid
    model = model_of("skip")
    inner = SyntheticSource(64, 64, device=DEV)
    src = PropagatedFlowSource(inner, model, stride=8)
    cond, flow = src.controls(3, 0, 8)
    cond0, flow0 = inner.controls(3, 0, 8)
    assert torch.equal(cond, cond0) and flow.shape == flow0.shape == (1, 4, 64, 64) and flow.dtype == flow0.dtype
    prev, nxt = anchors_u8(cond0)
    fwd = model.flow(prev, sample_grid(flow0[:, :2].contiguous(), 8))
    bwd = model.flow(nxt, sample_grid(flow0[:, 2:].contiguous(), 8))
    assert torch.equal(flow[:, :2], fwd) and torch.equal(flow[:, 2:], bwd)
    assert not torch.equal(flow, flow0)
    assert src.with_warp is False and torch.equal(src.warp(3), inner.warp(3))
