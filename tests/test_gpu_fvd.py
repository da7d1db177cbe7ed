"""GPU: FVD of csrc/fvd.hip (diffcodec_amd.metrics.FrechetVideoDistance) against the fp64 restatement tests/fvd_ref.py with seeded
synthetic weights: the Unit3D and max-pool seams on the smallest shapes that hit every mask, the preprocess, the 16 endpoint maps
and the 400 features at T = 10 and T = 11, the value, exactness properties, graph capture and decode_clip(score=True, fvd=model).

Bars.
  conv seam  max |dev - ref| / max |ref| <= 4 sqrt(K) 2^-24 with K = Cin k^3: an fp32 k-chain of K sequential additions, each
             rounding by at most 2^-24 of a partial sum no larger than about max |ref|, walks sqrt(K) 2^-24 away (one sigma); four
             sigma, never above 1e-4.  A wrong tap, pad side or mask is off by 1e-2 or more where it hits.
  pool seam  exact equality (max involves no arithmetic).
  preprocess 1e-6 absolute on the [-1,1] scale against the restatement for unit-range input.  Against the reference's golden (torch
             in fp32, which forms the source position in fp32): the measured |torch fp32 - fp64 restatement| plus the same again,
             wide 6.6e-6 -> 1.32e-5, tall 1.3e-5 -> 2.6e-5.
  endpoints  per endpoint 16 x the error of the fp32 CPU run of the same restatement against its fp64 run on the same videos
             (FP32_CPU below; 16 x because an MFMA k-chain sums K <= 5184 sequentially where torch blocks it), never above 1e-4.
             Measured on the CPU (max |fp32 - fp64| / max |fp64|, units of 1e-6), T = 10 (two uint8 videos) and T = 11 (one
             float video):
               endpoint            T=10   T=11      endpoint            T=10   T=11
               Conv3d_1a_7x7       1.40   1.10      Mixed_4b            1.17   0.98
               MaxPool3d_2a_3x3    1.40   1.10      Mixed_4c            1.22   1.08
               Conv3d_2b_1x1       0.88   0.82      Mixed_4d            1.20   1.20
               Conv3d_2c_3x3       0.70   0.68      Mixed_4e            1.04   0.95
               MaxPool3d_3a_3x3    0.70   0.64      Mixed_4f            1.21   1.37
               Mixed_3b            0.73   0.74      MaxPool3d_5a_2x2    1.13   1.20
               Mixed_3c            0.99   1.05      Mixed_5b            0.97   1.09
               MaxPool3d_4a_3x3    0.99   0.88      Mixed_5c            1.01   0.99
                                                    features (logits)   0.35   0.34
  value      1e-4 relative against the restatement's |f_decoded - f_truth|^2.
Device figures (recorded through `record`): DESIGN.md section 8."""
import math
import os

import pytest
import torch

import fvd_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 1234
CEILING = 1e-4
# max |fp32 CPU restatement - fp64 restatement| / max |fp64| per endpoint (FVD_ENDPOINTS order), then of the features
FP32_CPU = {
    10: (1.40e-6, 1.40e-6, 0.88e-6, 0.70e-6, 0.70e-6, 0.73e-6, 0.99e-6, 0.99e-6, 1.17e-6,
         1.22e-6, 1.20e-6, 1.04e-6, 1.21e-6, 1.13e-6, 0.97e-6, 1.01e-6, 0.35e-6),
    11: (1.10e-6, 1.10e-6, 0.82e-6, 0.68e-6, 0.64e-6, 0.74e-6, 1.05e-6, 0.88e-6, 0.98e-6,
         1.08e-6, 1.20e-6, 0.95e-6, 1.37e-6, 1.20e-6, 1.09e-6, 0.99e-6, 0.34e-6),
}
PREP_GOLDEN_BAR = {"wide": 2 * 6.6e-6, "tall": 2 * 1.3e-5}


def videos(t):
    """The operands of the endpoint tests.  T = 10: two uint8 [2,10,224,224,3] videos, the second the first at half contrast plus
    noise (the decoded / truth pair of the value test); T = 11: one float [1,11,3,224,224] video in [0,1]."""
    g = torch.Generator().manual_seed(700 + t)
    if t == 10:
        a = torch.randint(0, 256, (10, 224, 224, 3), generator=g, dtype=torch.uint8)
        b = (a.float() * 0.5 + 64 + 8 * torch.randn(a.shape, generator=g)).round().clamp(0, 255).to(torch.uint8)
        return torch.stack([a, b])
    return torch.rand(1, t, 3, 224, 224, generator=g)


def as_float(v):
    """[N,T,3,H,W] fp64 values the network sees before the preprocess"""
    return v.double().permute(0, 1, 4, 2, 3) / 255 if v.dtype == torch.uint8 else v.double()


@pytest.fixture(scope="module")
def sd():
    return R.synth_weights(SEED)


@pytest.fixture(scope="module")
def model(sd):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd import metrics
    return metrics.FrechetVideoDistance.from_state_dict(sd).to(DEV)


_REF = {}


def _case(t, sd):
    """the operand and its fp64 restatement, computed once and shared (never modified)"""
    if t not in _REF:
        v = videos(t)
        with torch.no_grad():
            eps = R.endpoints(R.preprocess(as_float(v)), sd)
            _REF[t] = dict(v=v, eps=eps, f=R.head(eps[-1], sd))
    return _REF[t]


def _err(dev, ref):
    return float((dev.double().cpu() - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------------------------------- conv seam
CONV_CASES = (
    [("k7", 7, 2, 3, 64, dims, True, True) for dims in ((10, 18, 37), (11, 17, 36))]
    + [("k3", 3, 1, ci, co, dims, True, True) for dims in ((2, 7, 7), (3, 14, 14)) for ci, co in ((16, 32), (24, 64), (112, 224), (160, 320))]
    + [("k1", 1, 1, ci, co, dims, bn, bn) for dims in ((2, 7, 7), (5, 28, 28))
       for ci, co, bn in ((832, 48, True), (528, 112, True), (192, 16, True), (1024, 400, False))]
)


def _run_conv(x, w, s, t, k, stride, relu, ctot, coff, fill):
    from diffcodec_amd import lib, metrics
    n, ci, T, H, W = x.shape
    co = w.shape[0]
    packed = metrics.pack_fvd_unit(w, s, t).to(DEV)
    osz = [metrics.fvd_same_pad(v, k, stride)[0] for v in (T, H, W)]
    y = torch.full([n, ctot] + osz, fill, dtype=torch.float32, device=DEV)
    xd = x.to(DEV)
    lib.call("dc_fvd_conv", xd.data_ptr(), n, ci, T, H, W, k, stride, packed.data_ptr(), co, int(relu), y.data_ptr(), ctot, coff,
             torch.cuda.current_stream().cuda_stream)
    return y.cpu()


@pytest.mark.parametrize("case", CONV_CASES, ids=[f"{c[0]}_{c[3]}to{c[4]}_{'x'.join(map(str, c[5]))}" for c in CONV_CASES])
def test_conv_seam(model, record, case):
    import torch.nn.functional as F
    tag, k, stride, ci, co, dims, bn, relu = case
    g = torch.Generator().manual_seed(ci * 1000 + co + dims[0])
    x = torch.randn(2, ci, *dims, generator=g)
    w = torch.randn(co, ci, k, k, k, generator=g) * math.sqrt(2.0 / (ci * k ** 3))
    s = (0.5 + torch.rand(co, generator=g)).double() if bn else torch.ones(co, dtype=torch.float64)
    t = 0.2 * torch.randn(co, generator=g).double()
    ref = F.conv3d(R.same_pad(x.double(), (k,) * 3, (stride,) * 3), w.double(), stride=stride) * s.float().double().view(1, -1, 1, 1, 1) \
        + t.float().double().view(1, -1, 1, 1, 1)
    if relu:
        ref = torch.relu(ref)
    bar = min(CEILING, 4 * math.sqrt(ci * k ** 3) * 2.0 ** -24)
    y = _run_conv(x, w, s, t, k, stride, relu, co, 0, float("nan"))
    e = _err(y, ref)
    record(f"fvd_conv_{tag}_{ci}to{co}_{'x'.join(map(str, dims))}", e)
    assert y.shape == ref.shape and e <= bar, (e, bar)
    # at a channel offset of a wider map: the same bits, the neighbour channels untouched
    wide = _run_conv(x, w, s, t, k, stride, relu, co + 5, 3, 7.5)
    assert torch.equal(wide[:, 3:3 + co], y)
    assert bool((wide[:, :3] == 7.5).all()) and bool((wide[:, 3 + co:] == 7.5).all())


def test_conv_seam_refuses_other_kernels(model):
    from diffcodec_amd import lib
    x = torch.zeros(1, 4, 2, 4, 4, device=DEV)
    w = torch.zeros(4096, device=DEV)
    y = torch.zeros(1, 4, 2, 4, 4, device=DEV)
    for k, stride, ctot, coff in ((5, 1, 4, 0), (3, 2, 4, 0), (1, 1, 4, 1)):
        with pytest.raises(lib.HipLaunchError, match="invalid argument"):
            lib.call("dc_fvd_conv", x.data_ptr(), 1, 4, 2, 4, 4, k, stride, w.data_ptr(), 4, 1, y.data_ptr(), ctot, coff, None)


# ------------------------------------------------------------------------------------------- pool seam
POOLS = (((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (1, 1, 1)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 2), (2, 2, 2)))


@pytest.mark.parametrize("k,s", POOLS, ids=["1x3x3s122", "3x3x3s1", "3x3x3s2", "2x2x2s2"])
@pytest.mark.parametrize("dims", [(3, 7, 9), (4, 8, 6)], ids=["odd", "even"])
def test_pool_seam_is_exact(model, k, s, dims):
    from diffcodec_amd import lib, metrics
    g = torch.Generator().manual_seed(sum(dims) + sum(k))
    x = torch.randn(2, 5, *dims, generator=g) - 0.5
    x[0, 0] = -1 - torch.rand(dims, generator=g)                          # an all-negative plane: the zero padding wins at its border
    ref = R.max_pool(x, k, s)
    osz = [metrics.fvd_same_pad(v, kk, ss)[0] for v, kk, ss in zip(dims, k, s)]
    y = torch.full([2, 5] + osz, float("nan"), device=DEV)
    lib.call("dc_fvd_maxpool", x.to(DEV).data_ptr(), 2, 5, *dims, *k, *s, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert tuple(ref.shape) == tuple(y.shape) and torch.equal(y.cpu(), ref)
    padded = any(metrics.fvd_same_pad(v, kk, ss)[1:] != (0, 0) for v, kk, ss in zip(dims, k, s))
    assert bool((ref[0, 0] == 0).any()) == padded and bool((ref[0, 0] <= 0).all())


# ------------------------------------------------------------------------------------------- preprocess
@pytest.mark.parametrize("name,h,w", [("wide", 40, 56), ("tall", 96, 64)])
def test_preprocess(model, sd, golden_dir, record, name, h, w):
    import sys
    import numpy as np
    from diffcodec_amd import metrics
    sys.path.insert(0, os.path.join(os.path.dirname(golden_dir), os.pardir, "tools"))
    import make_fvd_goldens as G
    g = torch.Generator().manual_seed(h)
    u = torch.randint(0, 256, (2, 9, h, w, 3), generator=g, dtype=torch.uint8)
    y = model.preprocess(u.to(DEV))
    e = float((y.double().cpu() - R.preprocess(as_float(u))).abs().max())
    record(f"fvd_prep_{name}_u8_abs_err", e)
    assert y.shape == (2, 3, 9, 224, 224) and e <= 1e-6
    # the same values as fp32 stored NTHWC, passed as a permuted (non-contiguous) NTCHW view: read in place
    f = (u.float() / 255).to(DEV).permute(0, 1, 4, 2, 3)
    assert not f.is_contiguous()
    yf = model.preprocess(f)
    ef = float((yf.double().cpu() - R.preprocess(f.double().cpu())).abs().max())
    record(f"fvd_prep_{name}_view_abs_err", ef)
    assert ef <= 1e-6
    # raw byte range: the same taps not divided by 255, no clamping
    raw = metrics.FrechetVideoDistance.from_state_dict(sd, byte_range=True).preprocess(u[:1].to(DEV))
    want = R.preprocess(u[:1].double().permute(0, 1, 4, 2, 3))
    assert float((raw.double().cpu() - want).abs().max()) <= 1e-6 * 255 and float(raw.max()) > 100
    # against the reference's own preprocess_single (torch fp32) through the golden
    gold = np.load(os.path.join(golden_dir, "fvd_i3d.npz"))
    v = G.source_video(h, w, int(gold[f"prep_{name}_seed"]))
    yg = model.preprocess(v.float().to(DEV))[0]
    eg = float((G.subsample(yg.cpu(), 8000).double() - torch.from_numpy(gold[f"prep_{name}_f32"]).double()).abs().max())
    record(f"fvd_prep_{name}_vs_reference_fp32", eg)
    assert eg <= PREP_GOLDEN_BAR[name]


# ------------------------------------------------------------------------------------------- endpoints, features
@pytest.mark.parametrize("t", [10, 11])
def test_endpoints_and_features(model, sd, record, t):
    from diffcodec_amd import metrics
    c = _case(t, sd)
    x = c["v"].to(DEV)
    eps = model.endpoints(x)
    f = model.features(x)
    assert [tuple(e.shape[1:]) for e in eps] == metrics.fvd_endpoint_shapes(t) and f.shape == (x.shape[0], 400) and f.is_cuda
    errs = {}
    for e, name in enumerate(metrics.FVD_ENDPOINTS):
        errs[name] = _err(eps[e], c["eps"][e])
        record(f"fvd_t{t}_{name}", errs[name])
    errs["features"] = _err(f, c["f"])
    record(f"fvd_t{t}_features", errs["features"])
    for (name, e), cpu in zip(errs.items(), FP32_CPU[t]):
        assert e <= min(CEILING, 16 * cpu), (name, e, 16 * cpu)
    assert float(c["f"].std()) > 1


def test_value_of_the_clip_protocol(model, sd, record):
    """decode_clip's protocol: one decoded and one truth video, each row added twice -> |f_decoded - f_truth|^2"""
    from diffcodec_amd import clip_decode as CD
    c = _case(10, sd)
    v = c["v"].to(DEV)
    frames = {i + 1: v[0, i] for i in range(10)}
    truth = {i + 1: v[1, i] for i in range(10)}
    scores = {i + 1: dict(psnr=30.0) for i in range(10)}
    got = CD.fvd_of_frames(model, frames, truth, scores)
    want = float(((c["f"][0] - c["f"][1]) ** 2).sum())
    record("fvd_clip_value", got)
    record("fvd_clip_value_rel_err", abs(got - want) / want)
    assert isinstance(got, float) and want > 1 and abs(got - want) <= 1e-4 * want, (got, want)
    assert model.count(True) == 2 and model.count(False) == 2
    f = model.features(v)
    assert abs(got - float(((f[0].double() - f[1].double()) ** 2).sum())) <= 1e-9 * got     # the covariance terms vanish
    # an identical frame (PSNR > 1000 dB) is left out: the same ten frames, the same bits
    frames[11], truth[11], scores[11] = v[0, 3], v[0, 3], dict(psnr=float("inf"))
    assert CD.fvd_of_frames(model, frames, truth, scores) == got
    # fewer than nine scored frames: NaN
    scores[1]["psnr"] = scores[2]["psnr"] = float("inf")
    assert math.isnan(CD.fvd_of_frames(model, frames, truth, scores)) and model.count(True) == 0


def test_calculate_fvd(model, record):
    """4 + 4 float videos [B,T,C,H,W], one side grey: the grey expansion, the two updates and the statistics against the same
    Frechet core on the device's own rows.  It does not check the value independently: the rows are checked by the endpoint and
    feature tests, the core by the golden from the reference's `frechet_distance` (tests/test_fvd_ref.py)."""
    from diffcodec_amd import metrics
    g = torch.Generator().manual_seed(5)
    v1 = torch.rand(4, 9, 1, 48, 64, generator=g).to(DEV)
    v2 = (0.5 * v1 + 0.25 * torch.rand(4, 9, 1, 48, 64, generator=g).to(DEV))
    got = metrics.calculate_fvd(v1, v2, model)
    f1, f2 = model.features(v1.repeat(1, 1, 3, 1, 1)), model.features(v2.expand(-1, -1, 3, -1, -1))
    want = R.frechet(f1.cpu(), f2.cpu())
    record("fvd_calculate_fvd_4x4", got)
    assert isinstance(got, float) and got > 0 and got == want
    with pytest.raises(ValueError, match="floating"):
        metrics.calculate_fvd(torch.zeros(2, 9, 3, 8, 8, dtype=torch.uint8), torch.zeros(2, 9, 3, 8, 8, dtype=torch.uint8), model)


# ------------------------------------------------------------------------------------------- exactness
def test_rows_are_reproducible_and_independent_of_the_batch(model, monkeypatch):
    from diffcodec_amd import metrics
    g = torch.Generator().manual_seed(9)
    v = torch.randint(0, 256, (3, 9, 36, 52, 3), generator=g, dtype=torch.uint8).to(DEV)
    f = model.features(v)
    last = model.endpoints(v)[-1]
    assert torch.equal(model.features(v), f)                                              # run to run
    assert torch.equal(model.features(v[1:2]), f[1:2])                                    # batch size
    assert torch.equal(model.features(v.flip(0)), f.flip(0))                              # batch position
    monkeypatch.setattr(metrics, "FVD_CHUNK_BYTES", 1)                                    # one video per launch sequence
    assert model._chunks(3, 9, 36, 52) == 1
    assert torch.equal(model.features(v), f)
    assert torch.equal(model.endpoints(v)[-1], last)
    monkeypatch.undo()
    h = model.features(v.cpu())                                                           # host in, host out
    assert not h.is_cuda and torch.equal(h, f.cpu())
    with pytest.raises(ValueError, match="at least 9 frames"):
        model.features(v[:, :8])


def test_features_are_graph_capturable(model):
    g0 = torch.Generator().manual_seed(11)
    x = torch.randint(0, 256, (1, 9, 32, 32, 3), generator=g0, dtype=torch.uint8).to(DEV)
    y = torch.randint(0, 256, (1, 9, 32, 32, 3), generator=g0, dtype=torch.uint8).to(DEV)
    fx, fy = model.features(x), model.features(y)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.features(x)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = model.features(x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, fx)
    x.copy_(y)                                                                            # replay reads the captured operand
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, fy) and not torch.equal(fx, fy)


# ------------------------------------------------------------------------------------------- the caller-owned workspace
# (N, T, H, W): T = 9, the shortest video (T1 = 5, T4 = 3, T5 = 2), two of them; T = 11 makes T1 = 6 even and T4 = 3 odd
WS_CASES = [(2, 9, 64, 48), (1, 11, 32, 32)]


@pytest.mark.parametrize("entry", ["dc_fvd_features", "dc_fvd_endpoints"])
@pytest.mark.parametrize("n,t,h,w", WS_CASES, ids=[f"n{c[0]}_t{c[1]}_{c[2]}x{c[3]}" for c in WS_CASES])
def test_on_a_guarded_workspace_of_any_contents(model, record, n, t, h, w, entry):
    """dc_fvd_features / dc_fvd_endpoints on a guarded workspace of exactly dc_fvd_ws_bytes under the NaN, zero and stale fills
    (the sixteen maps guarded outputs too): the bits FrechetVideoDistance.features / .endpoints return"""
    import ctypes
    import edge_cases as E
    from diffcodec_amd import lib, metrics
    wts = model._weights(torch.device(DEV))
    sets = []
    for seed in (t * 7 + h + n, 977):
        u = torch.randint(0, 256, (n, t, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
        g = E.Guarded((n, t, h, w, 3), torch.uint8, DEV)
        sets.append((g, g.fill(u.to(DEV))))
    strides = (ctypes.c_longlong * 5)(t * h * w * 3, h * w * 3, 1, w * 3, 3)            # (n, t, c, h, w)
    rh, rw = metrics.fvd_resized_size(h, w)
    st = torch.cuda.current_stream().cuda_stream
    feat = ((n, metrics.FVD_FEATURES), torch.float32)
    if entry == "dc_fvd_features":
        outputs = [feat]

        def launch(ws, outs, prime):
            lib.call("dc_fvd_features", sets[int(prime)][1].data_ptr(), 1, 1, strides, n, t, h, w, rh, rw, wts.data_ptr(), ws.data_ptr(),
                     outs[0].data_ptr(), st)
    else:
        outputs = [((n,) + s, torch.float32) for s in metrics.fvd_endpoint_shapes(t)] + [feat]

        def launch(ws, outs, prime):
            maps = (ctypes.c_void_p * 16)(*[o.data_ptr() for o in outs[:16]])
            lib.call("dc_fvd_endpoints", sets[int(prime)][1].data_ptr(), 1, 1, strides, n, t, h, w, rh, rw, wts.data_ptr(), ws.data_ptr(),
                     maps, outs[16].data_ptr(), st)

    what = f"{entry} {n}x{t}x{h}x{w}"
    outs, share = E.run_on_fills(launch, lib.load().dc_fvd_ws_bytes(n, t, h, w), outputs, what, operands=[s[0] for s in sets], device=DEV)
    record(f"ws_unwritten_share[{what}]", share)
    assert torch.equal(E.ws_bits(outs[-1]), E.ws_bits(model.features(sets[0][1]))), what
    if entry == "dc_fvd_endpoints":
        for k, (o, e) in enumerate(zip(outs[:16], model.endpoints(sets[0][1]))):
            assert torch.equal(E.ws_bits(o), E.ws_bits(e)), (what, metrics.FVD_ENDPOINTS[k])


# ------------------------------------------------------------------------------------------- clip scoring
from test_gpu_metrics import KW, _write_clip, small  # noqa: E402,F401  (the clip fixtures of the PSNR / MS-SSIM tests)


def test_decode_clip_adds_fvd(small, model, tmp_path, record):
    from diffcodec_amd import clip_decode as CD, metrics
    from diffcodec_amd.io_utils import _load_rgb_u8
    pipe, pe, npe = small
    root = str(tmp_path)
    _write_clip(root, "v256", (256, 256), frames=12, gop=11, seed=1)
    src = CD.DirectorySource(root, "v256", 11, (256, 256), device=DEV)
    kw = dict(tile=256, batch=4, seed=5, rank=0, world=1, score=True, **dict(KW, num_inference_steps=1))
    out = CD.decode_clip(pipe, src, 12, 11, 256, 256, pe, npe, fvd=model, **kw)
    plain = CD.decode_clip(pipe, src, 12, 11, 256, 256, pe, npe, **kw)
    order = list(range(1, 11))
    assert "fvd" not in plain and sorted(out["scores"]) == order and out["scores"] == plain["scores"]
    dec = torch.stack([torch.from_numpy(out["frames"][f]) for f in order])
    gt = torch.stack([torch.from_numpy(_load_rgb_u8(os.path.join(root, "v256", "images", f"frame_{f:04d}.png"), (256, 256))) for f in order])
    f = model.features(torch.stack([dec, gt]).to(DEV)).double().cpu()
    want = float(((f[0] - f[1]) ** 2).sum())
    record("clip_256_fvd", out["fvd"])
    assert isinstance(out["fvd"], float) and want > 1e-3 and abs(out["fvd"] - want) <= 1e-9 * want, (out["fvd"], want)
    assert metrics.summarize(out["scores"], fvd=out["fvd"])["fvd"] == out["fvd"]
    # five frames of a gop of four: three scored frames, fewer than nine -> NaN
    _write_clip(root, "v5", (256, 256), seed=2)
    src5 = CD.DirectorySource(root, "v5", 4, (256, 256), device=DEV)
    out5 = CD.decode_clip(pipe, src5, 5, 4, 256, 256, pe, npe, fvd=model, **kw)
    assert math.isnan(out5["fvd"]) and sorted(out5["scores"]) == [1, 2, 3]
