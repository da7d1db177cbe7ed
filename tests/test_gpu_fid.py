"""GPU: FID (feature = 64) of csrc/fid.hip (diffcodec_amd.metrics.FrechetInceptionDistance) against the fp64 restatement
tests/fid_ref.py with seeded synthetic weights: the resized image, the three post-ReLU maps and the pooled map element by element,
the 64 features, the value, exactness properties, graph capture, and decode_clip(score=True, fid=model) on one and two ranks.

Bars.  Measured against the fp64 restatement on an MI355X; each bar is four times the largest measured
value rounded up to one digit, and may not exceed its ceiling:
  maps      ceiling 1e-4: an fp32 chain over K <= 288 perturbs a value by about sqrt(288) 2^-24 = 1e-6 per layer, over three layers,
            while a wrong tap, stride, pad or edge mask is off by >= 1e-2 where it hits.
  features  ceiling 1e-5: a mean over 5,329 pooled values.
  value     ceiling 1e-3 relative: a 1e-6 relative perturbation of the features moves the value by up to 2.4e-5 relative (the
            rank-deficient covariances of fewer than 65 images are the sensitive ones).
Not yet measured on an MI355X: until the figures are recorded here the bars stand at their ceilings."""
import os

import pytest
import torch
import torch.multiprocessing as mp

import fid_ref as R
from test_gpu_lpips import _pair_u8

pytestmark = pytest.mark.gpu

DEV = "cuda"
BAR_M = 1e-4          # max |dev - ref| / max |ref| per map
BAR_F = 1e-5          # max |dev - ref| / max |ref| of the features
BAR_V = 1e-3          # relative error of the value
SEED = 20

# id -> (N, H, W, operand form): "u8" NHWC frames; "view" the same values / 255 as fp32 stored NHWC, passed as a permuted
# (non-contiguous) NCHW view to a model with normalize=True
CASES = {
    "n8_64x48_u8": (8, 64, 48, "u8"),
    "n4_299x299_u8": (4, 299, 299, "u8"),
    "n3_512x512_u8": (3, 512, 512, "u8"),
    "n2_270x480_view": (2, 270, 480, "view"),
    "n2_5x7_u8": (2, 5, 7, "u8"),
}
MAP_NAMES = ("resized", "relu1", "relu2", "relu3", "pooled")


@pytest.fixture(scope="module")
def sd():
    return R.synth_weights(seed=SEED)


@pytest.fixture(scope="module")
def models(sd):
    """{operand form: model}"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd import metrics
    return {"u8": metrics.FrechetInceptionDistance.from_state_dict(sd).to(DEV),
            "view": metrics.FrechetInceptionDistance.from_state_dict(sd, normalize=True).to(DEV)}


_REF = {}


def _operand(u, form):
    return u if form == "u8" else (u.float() / 255.0).permute(0, 3, 1, 2)


def _case(name, sd):
    """operands and the fp64 restatement of one case, computed once and shared (never modified)"""
    if name not in _REF:
        n, h, w, form = CASES[name] if name in CASES else (72, 96, 96, "u8")
        xu, yu = _pair_u8(n, h, w, seed=h * 7 + w + n)
        c = dict(xu=xu, yu=yu, x=_operand(xu, form), y=_operand(yu, form), form=form)
        if name in CASES:
            c["mx"], c["my"] = R.maps(sd, c["x"], form == "view"), R.maps(sd, c["y"], form == "view")
            c["fx"], c["fy"] = c["mx"][4].mean((2, 3)), c["my"][4].mean((2, 3))
        else:
            c["fx"], c["fy"] = R.features(sd, c["x"]), R.features(sd, c["y"])
        c["value"] = R.fid(c["fx"], c["fy"])
        _REF[name] = c
    return _REF[name]


def _err(dev, ref):
    return (dev.double().cpu() - ref).abs().max().item() / ref.abs().max().item()


@pytest.mark.parametrize("name", list(CASES))
def test_maps_match_fp64_restatement(models, sd, record, name):
    c = _case(name, sd)
    model = models[c["form"]]
    if c["form"] == "view":
        assert not c["x"].to(DEV).is_contiguous()                         # read in place through its strides
    worst = [0.0] * 5
    border = 0.0
    for side in ("x", "y"):
        ref = c["m" + side]
        dev = model.maps(c[side].to(DEV))
        assert len(dev) == 5
        assert [tuple(t.shape[1:]) for t in dev] == [(3, 299, 299), (32, 149, 149), (32, 147, 147), (64, 147, 147), (64, 73, 73)]
        for l, (d, r) in enumerate(zip(dev, ref)):
            assert d.is_cuda and d.dtype == torch.float32 and d.shape == r.shape and d.is_contiguous()
            if 1 <= l <= 3:
                zeros = (r == 0).double().mean().item()
                assert 0.2 < zeros < 0.8, (name, l, zeros)                # the ReLU is exercised on both of its sides
            worst[l] = max(worst[l], _err(d, r))
        # the ragged last tiles (149 = 4 * 37 + 1 = 4 * 32 + 21, 147 = 4 * 36 + 3 = 4 * 32 + 19) and conv3's pad-1 border on their own
        for l in (1, 2, 3):
            d, r = dev[l].double().cpu(), ref[l]
            assert r[:, :, -1].abs().max() > 0 and r[:, :, :, 128:].abs().max() > 0
            assert (d[:, :, -1] - r[:, :, -1]).abs().max().item() <= BAR_M * r.abs().max().item()
            assert (d[:, :, :, 128:] - r[:, :, :, 128:]).abs().max().item() <= BAR_M * r.abs().max().item()
        d, r = dev[3].double().cpu(), ref[3]
        for sl in ((slice(None), slice(None), 0), (slice(None), slice(None), 146), (slice(None), slice(None), slice(None), 0),
                   (slice(None), slice(None), slice(None), 146)):
            assert r[sl].abs().max() > 0
            border = max(border, (d[sl] - r[sl]).abs().max().item() / r.abs().max().item())
        if name == "n4_299x299_u8":                                       # passes through the resize unchanged: exact
            want = ((c[side + "u"].permute(0, 3, 1, 2).float() - 128) / 128)
            assert torch.equal(dev[0].cpu(), want)
    for l, e in enumerate(worst):
        record(f"fid_{name}_{MAP_NAMES[l]}_rel_err", e)
    record(f"fid_{name}_relu3_border_rel_err", border)
    assert max(worst) <= BAR_M and border <= BAR_M, (name, worst, border)
    if c["form"] == "view":                                               # the truncation to 8 bits is exact: the uint8 form's bits
        assert torch.equal(model.features(c["x"].to(DEV)), models["u8"].features(c["xu"].to(DEV)))


def test_single_block_entry_on_guarded_maps(models, sd, record):
    """dc_fid_conv (the one-block entry point) on guarded operands and outputs: each block from the device's own input map, twice;
    each output within BAR_M of the fp64 restatement's map"""
    import edge_cases as E
    from diffcodec_amd import lib
    c = _case("n2_5x7_u8", sd)
    model = models["u8"]
    maps = model.maps(c["x"].to(DEV))
    wts = model._weights(torch.device(DEV, torch.cuda.current_device()))
    st = torch.cuda.current_stream().cuda_stream
    n = maps[0].shape[0]
    for layer in range(3):
        gin = E.Guarded(tuple(maps[layer].shape), torch.float32, DEV)
        gin.fill(maps[layer])
        outs = []
        for rep in range(2):
            go = E.Guarded(tuple(maps[layer + 1].shape), torch.float32, DEV)
            lib.call("dc_fid_conv", layer, gin.view.data_ptr(), n, wts.data_ptr(), go.view.data_ptr(), st)
            torch.cuda.synchronize()
            gin.assert_intact(f"fid_conv layer {layer} input")
            go.assert_intact(f"fid_conv layer {layer} output")
            assert go.unwritten() == 0
            outs.append(go.view)
        assert torch.equal(outs[0], outs[1])
        e = _err(outs[0], c["mx"][layer + 1])
        record(f"fid_conv_layer{layer}_rel_err", e)
        assert e <= BAR_M, (layer, e)


@pytest.mark.parametrize("name", list(CASES))
def test_features_match_fp64_restatement(models, sd, record, name):
    c = _case(name, sd)
    model = models[c["form"]]
    worst = 0.0
    for side in ("x", "y"):
        f = model.features(c[side].to(DEV))
        assert f.is_cuda and f.dtype == torch.float32 and f.shape == (CASES[name][0], 64)
        worst = max(worst, _err(f, c["f" + side]))
    record(f"fid_{name}_features_rel_err", worst)
    assert worst <= BAR_F, (name, worst)


@pytest.mark.parametrize("name", ["n8_64x48_u8", "n72_96x96_u8"])
def test_value_matches_fp64_restatement(models, sd, record, name):
    c = _case(name, sd)
    model = models["u8"]
    model.reset()
    model.update(c["x"].to(DEV), real=True)
    model.update(c["y"].to(DEV), real=False)
    v = model.compute()
    assert isinstance(v, float) and c["value"] > 1e-3                     # a non-trivial value
    e = abs(v - c["value"]) / c["value"]
    record(f"fid_{name}_value_rel_err", e)
    record(f"fid_{name}_value", v)
    assert e <= BAR_V, (name, v, c["value"])
    real, fake = model.state()
    n = c["x"].shape[0]
    assert real.is_cuda and real.dtype == torch.float64 and real[0].item() == n and fake[0].item() == n
    fx = model.features(c["x"].to(DEV)).double()                          # the sums are exact fp64 sums of the fp32 rows
    assert (real[1:65] - fx.sum(0)).abs().max().item() <= 1e-12 * fx.sum(0).abs().max().item()
    assert (real[65:].view(64, 64) - fx.t() @ fx).abs().max().item() <= 1e-12 * (fx.t() @ fx).abs().max().item()
    model.reset()


def test_exactness(models, sd, record, monkeypatch):
    from diffcodec_amd import metrics
    c = _case("n8_64x48_u8", sd)
    model = models["u8"]
    x, y = c["x"].to(DEV), c["y"].to(DEV)
    f = model.features(x)
    assert torch.equal(model.features(x), f)                              # two runs
    for i in range(8):                                                    # alone == at position i of the batch of 8
        assert torch.equal(model.features(x[i:i + 1])[0], f[i]), i
    perm = torch.randperm(8, generator=torch.Generator().manual_seed(1)).to(DEV)
    assert torch.equal(model.features(x[perm]), f[perm])
    with monkeypatch.context() as mc:                                     # chunks of three images
        mc.setattr(metrics, "FID_CHUNK_BYTES", 3 * metrics.lib.load().dc_fid_ws_bytes(1, 64, 48) + 1)
        assert model._chunks(8, 64, 48) == 3 and torch.equal(model.features(x), f)
    # update(a); update(b) leaves the bits of update(cat(a, b)); the two sides run the same code
    model.reset()
    assert not model.state()[0].any() and not model.state()[1].any()
    model.update(x, real=True)
    model.update(y, real=True)
    model.update(torch.cat([x, y]), real=False)
    real, fake = model.state()
    assert torch.equal(real, fake) and real[0].item() == 16
    same = model.compute()
    record("fid_self_value", same)
    assert abs(same) < 1e-9
    again = metrics.FrechetInceptionDistance.from_state_dict(sd).to(DEV)
    again.update(torch.cat([x, y]), real=True)
    again.update_features(torch.cat([model.features(x), model.features(y)]), real=False)
    assert torch.equal(again.state()[0], real) and torch.equal(again.state()[1], real)
    model.reset()
    assert not model.state()[0].any() and not model.state()[1].any()
    # host tensors give host results equal to the device ones
    fh = model.features(c["x"])
    assert not fh.is_cuda and torch.equal(fh, f.cpu())
    assert all(not t.is_cuda and torch.equal(t, d.cpu()) for t, d in zip(model.maps(c["x"][:2]), model.maps(x[:2])))
    model.update(c["x"], real=True)
    again.reset()
    again.update(x, real=True)
    assert torch.equal(model.state()[0], again.state()[0])
    model.reset()
    # uint8 NHWC frames and the same values as float NCHW / 255 with normalize=True: the truncation restores the 8-bit value
    ff = models["view"].features((c["x"].permute(0, 3, 1, 2).float() / 255).contiguous().to(DEV))
    equal = torch.equal(ff, f)
    record("fid_u8_vs_float_equal", float(equal))
    assert equal or _err(ff, f.double().cpu()) <= BAR_F
    with pytest.raises(ValueError, match="normalize=True"):
        model.features(x.permute(0, 3, 1, 2).float() / 255)


def test_update_is_graph_capturable(models, sd):
    from diffcodec_amd import metrics
    c = _case("n8_64x48_u8", sd)
    model = models["u8"]
    x, y = c["x"].to(DEV).clone(), c["y"].to(DEV)
    eager = metrics.FrechetInceptionDistance.from_state_dict(sd).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.update(x, real=True)
    torch.cuda.current_stream().wait_stream(s)
    model.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        model.update(x, real=True)
    for _ in range(2):
        g.replay()
        eager.update(x, real=True)
        torch.cuda.synchronize()
        assert torch.equal(model.state()[0], eager.state()[0]) and eager.state()[0][0].item() > 0
    x.copy_(y)                                                            # replay reads the captured operand
    g.replay()
    eager.update(y, real=True)
    torch.cuda.synchronize()
    assert torch.equal(model.state()[0], eager.state()[0]) and model.state()[0][0].item() == 24
    assert not model.state()[1].any()
    model.reset()


# ------------------------------------------------------------------------------------------- clip scoring
from test_gpu_metrics import KW, _free_port, _write_clip, small  # noqa: E402,F401  (the clip fixtures of the PSNR / MS-SSIM tests)


class _TruthIsDecoded:
    """a source whose ground truth of one frame is the decoded frame itself"""

    def __init__(self, source, frame, decoded):
        self._s, self._f, self._d = source, frame, decoded

    def __getattr__(self, name):
        return getattr(self._s, name)

    def ground_truth(self, frame):
        return torch.from_numpy(self._d).to(DEV) if frame == self._f else self._s.ground_truth(frame)


def test_decode_clip_adds_fid(small, models, sd, tmp_path, record):
    from diffcodec_amd import clip_decode as CD, metrics
    from diffcodec_amd.io_utils import _load_rgb_u8
    pipe, pe, npe = small
    model = models["u8"]
    root = str(tmp_path)
    _write_clip(root, "v256", (256, 256), seed=1)
    src = CD.DirectorySource(root, "v256", 4, (256, 256), device=DEV)
    kw = dict(tile=256, batch=4, seed=5, rank=0, world=1, score=True, **KW)
    model.update(_case("n2_5x7_u8", sd)["x"].to(DEV), real=True)         # decode_clip resets the model
    out = CD.decode_clip(pipe, src, 5, 4, 256, 256, pe, npe, fid=model, **kw)
    plain = CD.decode_clip(pipe, src, 5, 4, 256, 256, pe, npe, **kw)
    assert "fid" not in plain and "fid_features" not in plain
    assert sorted(out["scores"]) == sorted(out["fid_features"]) == [1, 2, 3]
    for f, s in out["scores"].items():
        assert sorted(s) == sorted(plain["scores"][f]) == ["ms_ssim", "psnr"]
        assert s["psnr"] == plain["scores"][f]["psnr"] and s["ms_ssim"] == plain["scores"][f]["ms_ssim"]     # the same bits
    dec = torch.stack([torch.from_numpy(out["frames"][f]) for f in (1, 2, 3)])
    gt = torch.stack([torch.from_numpy(_load_rgb_u8(os.path.join(root, "v256", "images", f"frame_{f:04d}.png"), (256, 256))) for f in (1, 2, 3)])
    fd, fg = R.features(sd, dec), R.features(sd, gt)
    for i, f in enumerate((1, 2, 3)):
        d, t = out["fid_features"][f]
        assert d.shape == (64,) and d.dtype == torch.float32 and not d.is_cuda
        assert _err(d, fd[i]) <= BAR_F and _err(t, fg[i]) <= BAR_F
    ref = R.fid(fg, fd)
    e = abs(out["fid"] - ref) / ref
    record("clip_256_fid_rel_err", e)
    record("clip_256_fid", out["fid"])
    assert isinstance(out["fid"], float) and ref > 1e-3 and e <= BAR_V, (out["fid"], ref)
    assert model.state()[0][0].item() == 3 and model.state()[1][0].item() == 3
    assert metrics.summarize(out["scores"], fid=out["fid"])["fid"] == out["fid"]
    # frame 2 against itself: identical, left out of the FID (and of summarize's means)
    wrapped = _TruthIsDecoded(src, 2, out["frames"][2])
    out2 = CD.decode_clip(pipe, wrapped, 5, 4, 256, 256, pe, npe, fid=model, **kw)
    assert out2["scores"][2]["psnr"] > 1000 and sorted(out2["scores"]) == [1, 2, 3] and sorted(out2["fid_features"]) == [1, 3]
    two = metrics.FrechetInceptionDistance.from_state_dict(sd)
    two.update_features(torch.stack([out["fid_features"][f][0] for f in (1, 3)]), real=False)
    two.update_features(torch.stack([out["fid_features"][f][1] for f in (1, 3)]), real=True)
    assert out2["fid"] == two.compute() and out2["fid"] != out["fid"]
    assert model.state()[0][0].item() == 2
    # score_frames on its own updates the model without resetting it
    frames = {f: torch.from_numpy(a).to(DEV) for f, a in out["frames"].items()}
    sc = CD.score_frames(frames, src, fid=model)
    assert model.state()[0][0].item() == 5 and sc == plain["scores"]
    model.reset()


def _world2_worker(rank, world, port, root, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    from diffcodec_amd import clip_decode as CD, metrics, selftest as T, sharding
    sharding.init_from_env(backend="gloo")
    pipe, _ = T.build_small_pipeline()
    pe, npe = T.synth_text(1, dim=T.SMALL_UNET["cross_attention_dim"])
    src = CD.DirectorySource(root, "v256", 4, (256, 256), device=DEV)
    model = metrics.FrechetInceptionDistance.from_state_dict(R.synth_weights(seed=SEED))
    out = CD.decode_clip(pipe, src, 5, 4, 256, 256, pe.to(DEV), npe.to(DEV), tile=256, batch=1, seed=5, gather=False, score=True,
                         fid=model, **KW)
    q.put((rank, [u.frame for u in out["mine"]], out["scores"], out.get("fid"), sorted(out["fid_features"])))
    dist.barrier()
    dist.destroy_process_group()


def test_world2_gloo_gathers_feature_rows_on_rank0(small, models, tmp_path):
    """two ranks share the GPU over gloo, gather=False: the feature rows of every frame reach rank 0 through one more gather, rank 0
    accumulates them in frame order; the value has the bits of a single-rank run."""
    from diffcodec_amd import clip_decode as CD
    pipe, pe, npe = small
    root = str(tmp_path)
    _write_clip(root, "v256", (256, 256), seed=1)
    src = CD.DirectorySource(root, "v256", 4, (256, 256), device=DEV)
    ref = CD.decode_clip(pipe, src, 5, 4, 256, 256, pe, npe, tile=256, batch=1, seed=5, rank=0, world=1, score=True, fid=models["u8"],
                         **KW)
    models["u8"].reset()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_world2_worker, args=(r, 2, port, root, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in range(2)), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert res[0][1] == [1, 3] and res[1][1] == [2]
    assert res[0][2] == ref["scores"] and all(sorted(s) == ["ms_ssim", "psnr"] for s in ref["scores"].values())
    assert res[0][3] == ref["fid"] and ref["fid"] > 1e-3                  # the same bits
    assert res[1][3] is None and res[1][4] == [2] and res[0][4] == [1, 2, 3]


# ------------------------------------------------------------------------------------------- the caller-owned workspace
# (N, H, W): a one-pixel image (every bilinear tap clamps) and an odd batch; the maps are 299 -> 149 -> 147 -> 73 whatever the input
WS_CASES = [(1, 1, 1), (3, 64, 48)]


@pytest.mark.parametrize("n,h,w", WS_CASES, ids=[f"n{c[0]}_{c[1]}x{c[2]}" for c in WS_CASES])
def test_features_on_a_guarded_workspace_of_any_contents(models, record, n, h, w):
    """dc_fid_features on a guarded workspace of exactly dc_fid_ws_bytes under the NaN, zero and stale fills: the rows are the
    bits FrechetInceptionDistance.features returns"""
    import ctypes
    import edge_cases as E
    from diffcodec_amd import lib, metrics
    model = models["u8"]
    wts = model._weights(torch.device(DEV))
    sets = []
    for seed in (h * 7 + w + n, 977):
        u = torch.randint(0, 256, (n, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
        g = E.Guarded((n, h, w, 3), torch.uint8, DEV)
        sets.append((g, g.fill(u.to(DEV))))
    strides = (ctypes.c_longlong * 4)(h * w * 3, 1, w * 3, 3)
    st = torch.cuda.current_stream().cuda_stream

    def launch(ws, outs, prime):
        lib.call("dc_fid_features", sets[int(prime)][1].data_ptr(), 1, strides, n, h, w, wts.data_ptr(), ws.data_ptr(),
                 outs[0].data_ptr(), st)

    what = f"dc_fid_features {n}x{h}x{w}"
    (out,), share = E.run_on_fills(launch, lib.load().dc_fid_ws_bytes(n, h, w), [((n, metrics.FID_FEATURES), torch.float32)], what,
                                   operands=[s[0] for s in sets], device=DEV)
    record(f"ws_unwritten_share[{what}]", share)
    assert torch.equal(E.ws_bits(out), E.ws_bits(model.features(sets[0][1]))), what
