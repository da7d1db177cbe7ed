"""GPU: LPIPS (AlexNet) of csrc/lpips.hip (diffcodec_amd.metrics.LPIPS) against the fp64 restatement tests/lpips_ref.py with seeded
synthetic weights: the five feature maps element by element, the value and its per-layer terms, exactness properties, the dead
layer, NormFix, reproducibility / graph capture / host tensors, and decode_clip(score=True, lpips=model) on one and two ranks.

Bars.  Measured against the fp64 restatement on an MI355X; each bar is four times the largest measured
value rounded up to one digit, and may not exceed BAR_F <= 1e-4 / BAR_V <= 2e-5: a sequential fp32 chain over K <= 3456 perturbs
a feature by about sqrt(K) 2^-24 = 4e-6, compounded over five layers, while a wrong tap, pad or edge mask is off by >= 1e-2 at
the pixels it hits.  Largest measured: features 2.24e-6 (relu3 of the 16 x 64x64 case) -> 9e-6; value / per-layer terms 5.9e-6
(relu5 of the 31x31 case, a single pixel per map: the difference of two nearly equal unit vectors amplifies the feature error)
-> 4x is 2.4e-5, above the ceiling, so the bar is the ceiling 2e-5."""
import os

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

import lpips_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BAR_F = 9e-6          # max |dev - ref| / max |ref| per feature map
BAR_V = 2e-5          # relative error of the value and of each per-layer term
SEED = 20


def _pair_u8(n, h, w, seed):
    """a smooth random field and a noisy copy, quantised to 8 bits: uint8 NHWC on the CPU"""
    g = torch.Generator().manual_seed(seed)
    base = F.interpolate(torch.rand(n, 3, h // 16 + 2, w // 16 + 2, generator=g), size=(h, w), mode="bicubic", align_corners=False)
    base = (base + 0.1 * torch.rand(n, 3, h, w, generator=g)).clamp(0, 1)
    noisy = (base + 0.06 * torch.randn(n, 3, h, w, generator=g)).clamp(0, 1)
    q = lambda t: (t * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return q(base), q(noisy)


def _form(u, form):
    """the operand the case feeds: "u8" NHWC frames, "f1" fp32 NCHW in [0,1], "view" the same fp32 values stored NHWC and passed as
    a permuted (non-contiguous) NCHW view"""
    if form == "u8":
        return u
    f = u.float() / 255.0                                            # NHWC fp32
    return f.permute(0, 3, 1, 2) if form == "view" else f.permute(0, 3, 1, 2).contiguous()


# id -> (N, H, W, operand form, normalize)
CASES = {
    "n2_31x31_f1": (2, 31, 31, "f1", False),
    "n3_67x95_u8": (3, 67, 95, "u8", False),
    "n16_64x64_f1": (16, 64, 64, "f1", False),
    "n2_256x256_u8": (2, 256, 256, "u8", False),
    "n1_512x512_f1_normalize": (1, 512, 512, "f1", True),
    "n1_270x480_view": (1, 270, 480, "view", False),
}
MAPS = {"n2_31x31_f1": [(7, 7), (3, 3), (1, 1)], "n3_67x95_u8": [(16, 23), (7, 11), (3, 5)], "n2_256x256_u8": [(63, 63), (31, 31), (15, 15)],
        "n1_512x512_f1_normalize": [(127, 127), (63, 63), (31, 31)]}


@pytest.fixture(scope="module")
def sd():
    return R.synth_weights(seed=SEED)


@pytest.fixture(scope="module")
def model(sd):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd import metrics
    return metrics.LPIPS.from_state_dict(sd).to(DEV)


_REF = {}


def _case(name, sd):
    """operands and the fp64 restatement of one case, computed once and shared (never modified)"""
    if name not in _REF:
        n, h, w, form, normalize = CASES[name]
        xu, yu = _pair_u8(n, h, w, seed=h * 7 + w + n)
        x, y = _form(xu, form), _form(yu, form)
        fx, fy = R.features(sd, x, normalize), R.features(sd, y, normalize)
        _, lins = R._params(sd)
        layers = [R.tail(a, b, l) for a, b, l in zip(fx, fy, lins)]
        _REF[name] = dict(x=x, y=y, fx=fx, fy=fy, layers=layers, value=sum(layers), normalize=normalize)
    return _REF[name]


def _rel(dev, ref):
    return ((dev.double().cpu().reshape(-1) - ref.reshape(-1)).abs() / ref.reshape(-1).abs()).max().item()


@pytest.mark.parametrize("name", list(CASES))
def test_features_match_fp64_restatement(model, sd, record, name):
    c = _case(name, sd)
    if name == "n1_270x480_view":
        assert not c["x"].to(DEV).is_contiguous()                        # read in place through its strides
    if name in MAPS:
        assert [tuple(t.shape[2:]) for t in c["fx"][:3]] == MAPS[name]
    worst = [0.0] * 5
    for side, ref in (("x", c["fx"]), ("y", c["fy"])):
        dev = model.features(c[side].to(DEV), normalize=c["normalize"])
        assert len(dev) == 5
        for l, (d, r) in enumerate(zip(dev, ref)):
            assert d.is_cuda and d.dtype == torch.float32 and d.shape == r.shape and d.is_contiguous()
            zeros = (r == 0).double().mean().item()
            assert 0.2 < zeros < 0.8, (name, l, zeros)                    # the ReLU is exercised on both of its sides
            worst[l] = max(worst[l], (d.double().cpu() - r).abs().max().item() / r.abs().max().item())
    for l, err in enumerate(worst):
        record(f"lpips_{name}_feat{l + 1}_rel_err", err)
    assert max(worst) <= BAR_F, (name, worst)


@pytest.mark.parametrize("name", list(CASES))
def test_value_matches_fp64_restatement(model, sd, record, name):
    c = _case(name, sd)
    n = CASES[name][0]
    val, layers = model(c["x"].to(DEV), c["y"].to(DEV), retPerLayer=True, normalize=c["normalize"])
    assert val.is_cuda and val.dtype == torch.float32 and val.shape == (n, 1, 1, 1)
    assert len(layers) == 5 and all(t.shape == (n, 1, 1, 1) and t.dtype == torch.float32 for t in layers)
    assert c["value"].min().item() > 1e-4                                 # a non-trivial score
    e = _rel(val, c["value"])
    record(f"lpips_{name}_value_rel_err", e)
    el = [_rel(d, r) for d, r in zip(layers, c["layers"])]
    for l, v in enumerate(el):
        record(f"lpips_{name}_layer{l + 1}_rel_err", v)
    assert e <= BAR_V, (name, e)
    assert max(el) <= BAR_V, (name, el)
    assert torch.equal(model(c["x"].to(DEV), c["y"].to(DEV), normalize=c["normalize"]), val)


def test_single_layer_entry_on_guarded_maps(model, sd, record):
    """dc_lpips_conv (the one-stage entry point) on guarded operands and outputs: layer 0 from the uint8 frames, layers 1..4 from the
    device's own maps (max-pooled where AlexNet pools), twice; each output within BAR_F of the fp64 restatement's map"""
    import ctypes
    import edge_cases as E
    from diffcodec_amd import lib
    name = "n3_67x95_u8"
    c = _case(name, sd)
    n, h, w = CASES[name][:3]
    wts = model._weights(torch.device(DEV, torch.cuda.current_device()))
    st = torch.cuda.current_stream().cuda_stream
    feats = model.features(c["x"].to(DEV))
    gx = E.Guarded(tuple(c["x"].shape), torch.uint8, DEV)
    gx.fill(c["x"].to(DEV))
    strides = (ctypes.c_longlong * 4)(h * w * 3, 1, w * 3, 3)
    for layer in range(5):
        if layer == 0:
            gin, args = gx, (gx.view.data_ptr(), 1, strides, n, h, w)
        else:
            src = F.max_pool2d(feats[layer - 1], 3, 2) if layer <= 2 else feats[layer - 1]
            gin = E.Guarded(tuple(src.shape), torch.float32, DEV)
            gin.fill(src)
            args = (gin.view.data_ptr(), 0, None, n, src.shape[2], src.shape[3])
        outs = []
        for rep in range(2):
            go = E.Guarded(tuple(feats[layer].shape), torch.float32, DEV)
            lib.call("dc_lpips_conv", layer, *args, 0, wts.data_ptr(), go.view.data_ptr(), st)
            torch.cuda.synchronize()
            gin.assert_intact(f"lpips_conv layer {layer} input")
            go.assert_intact(f"lpips_conv layer {layer} output")
            assert go.unwritten() == 0
            outs.append(go.view)
        assert torch.equal(outs[0], outs[1])
        ref = c["fx"][layer]
        err = (outs[0].double().cpu() - ref).abs().max().item() / ref.abs().max().item()
        record(f"lpips_conv_layer{layer}_rel_err", err)
        assert err <= BAR_F, (layer, err)


def test_exactness(model, sd, record):
    c = _case("n16_64x64_f1", sd)
    x, y = c["x"].to(DEV), c["y"].to(DEV)
    val, layers = model(x, y, retPerLayer=True)
    same, same_layers = model(x, x.clone(), retPerLayer=True)
    assert torch.equal(same, torch.zeros_like(same)) and all(torch.equal(t, torch.zeros_like(t)) for t in same_layers)
    swapped, swapped_layers = model(y, x, retPerLayer=True)
    assert torch.equal(swapped, val) and all(torch.equal(a, b) for a, b in zip(swapped_layers, layers))
    for i in range(16):                                                   # alone == at position i of the batch of 16
        one, one_layers = model(x[i:i + 1], y[i:i + 1], retPerLayer=True)
        assert torch.equal(one[0], val[i]) and all(torch.equal(a[0], b[i]) for a, b in zip(one_layers, layers)), i
    perm = torch.randperm(16, generator=torch.Generator().manual_seed(1)).to(DEV)
    assert torch.equal(model(x[perm], y[perm]), val[perm])
    # uint8 NHWC frames and the same values as fp32 NCHW / 255
    cu = _case("n3_67x95_u8", sd)
    a = model(cu["x"].to(DEV), cu["y"].to(DEV))
    b = model((cu["x"].permute(0, 3, 1, 2).float() / 255).to(DEV), (cu["y"].permute(0, 3, 1, 2).float() / 255).to(DEV))
    e = ((a - b).abs() / b.abs()).max().item()
    record("lpips_u8_vs_f32_rel_diff", e)
    assert e <= BAR_V, e
    # fp16 operands are converted to fp32
    h = model(x[:2].half(), y[:2].half())
    assert h.dtype == torch.float32 and torch.equal(h, model(x[:2].half().float(), y[:2].half().float()))


def test_dead_layer_and_normfix(model, sd, record):
    from diffcodec_amd import metrics
    dead = dict(sd)
    dead["net.slice5.10.bias"] = torch.full((256,), -1e3)
    c = _case("n3_67x95_u8", sd)
    x, y = c["x"].to(DEV), c["y"].to(DEV)
    m = metrics.LPIPS.from_state_dict(dead)
    val, layers = m(x, y, retPerLayer=True)
    assert torch.equal(layers[4], torch.zeros_like(layers[4]))            # all-zero pixels give 0, not NaN
    assert torch.isfinite(val).all() and all(torch.isfinite(t).all() for t in layers)
    assert not m.features(x)[4].any()
    rv, rl = R.lpips(dead, c["x"], c["y"])
    assert rl[4].abs().max().item() == 0.0 and _rel(val, rv) <= BAR_V
    mf = metrics.LPIPS.from_state_dict(dead, normfix=True)
    fval, flayers = mf(x, y, retPerLayer=True)
    assert torch.equal(flayers[4], torch.zeros_like(flayers[4])) and torch.isfinite(fval).all()
    nf = metrics.LPIPS.from_state_dict(sd, normfix=True)
    nval, nlayers = nf(x, y, retPerLayer=True)
    rv, rl = R.lpips(sd, c["x"], c["y"], normfix=True)
    e = max([_rel(nval, rv)] + [_rel(d, r) for d, r in zip(nlayers, rl)])
    record("lpips_n3_67x95_u8_normfix_rel_err", e)
    assert e <= BAR_V, e
    assert not torch.equal(nval.cpu(), c["value"].float().reshape(-1, 1, 1, 1))       # NormFix is another function


def test_reproducible_graph_capturable_and_host_tensors(model, sd):
    c = _case("n2_256x256_u8", sd)
    x, y = c["x"].to(DEV), c["y"].to(DEV)
    a, la = model(x, y, retPerLayer=True)
    b, lb = model(x, y, retPerLayer=True)
    assert torch.equal(a, b) and all(torch.equal(p, q) for p, q in zip(la, lb))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model(x, y)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gv = model(x, y)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gv, a)
    x.copy_(y)                                                            # replay reads the captured operands
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gv, torch.zeros_like(gv))
    h, lh = model(c["x"], c["y"], retPerLayer=True)
    assert not h.is_cuda and torch.equal(h, a.cpu()) and all(not t.is_cuda for t in lh)
    fh = model.features(c["x"])
    assert all(not t.is_cuda for t in fh)


# ------------------------------------------------------------------------------------------- the caller-owned workspace
# (N, H, W, operand form): the minimum size (every map of relu3..5 is one pixel) and an odd batch of ragged pooled maps (16x23 ->
# 7x11 -> 3x5), one on each operand form
WS_CASES = [(1, 31, 31, "f1"), (3, 67, 95, "u8")]


def _ws_operands(n, h, w, form, seed):
    """(x, y) of one operand form inside guarded buffers on the device -> (guards, tensors, element strides (n, c, h, w))"""
    import edge_cases as E
    guards, tensors = [], []
    for t in _pair_u8(n, h, w, seed):
        t = _form(t, form)
        g = E.Guarded(tuple(t.shape), t.dtype, DEV)
        guards.append(g)
        tensors.append(g.fill(t.to(DEV)))
    strides = (h * w * 3, 1, w * 3, 3) if form == "u8" else (3 * h * w, h * w, w, 1)
    return guards, tensors, strides


@pytest.mark.parametrize("normfix", [False, True], ids=["plain", "normfix"])
@pytest.mark.parametrize("n,h,w,form", WS_CASES, ids=[f"n{c[0]}_{c[1]}x{c[2]}_{c[3]}" for c in WS_CASES])
def test_value_on_a_guarded_workspace_of_any_contents(sd, record, n, h, w, form, normfix):
    """dc_lpips_alex on a guarded workspace of exactly dc_lpips_ws_bytes under the NaN, zero and stale fills: the six rows are the
    bits LPIPS.__call__ returns"""
    import ctypes
    import edge_cases as E
    from diffcodec_amd import lib, metrics
    m = metrics.LPIPS.from_state_dict(sd, normfix=normfix).to(DEV)
    wts = m._weights(torch.device(DEV))
    sets = [_ws_operands(n, h, w, form, seed) for seed in (h * 7 + w + n, 977)]
    st = torch.cuda.current_stream().cuda_stream

    def launch(ws, outs, prime):
        _, (x, y), s = sets[int(prime)]
        lib.call("dc_lpips_alex", x.data_ptr(), y.data_ptr(), int(form == "u8"), (ctypes.c_longlong * 8)(*s, *s), n, h, w, 0, int(normfix),
                 wts.data_ptr(), ws.data_ptr(), outs[0].data_ptr(), st)

    what = f"dc_lpips_alex {n}x{h}x{w} {form} normfix={int(normfix)}"
    (out,), share = E.run_on_fills(launch, lib.load().dc_lpips_ws_bytes(n, h, w), [((6, n), torch.float64)], what,
                                   operands=sets[0][0] + sets[1][0], device=DEV)
    record(f"ws_unwritten_share[{what}]", share)
    val, layers = m(sets[0][1][0], sets[0][1][1], retPerLayer=True)
    got = out.float()
    assert torch.equal(E.ws_bits(got[5].reshape(n, 1, 1, 1)), E.ws_bits(val)), what
    for l in range(5):
        assert torch.equal(E.ws_bits(got[l].reshape(n, 1, 1, 1)), E.ws_bits(layers[l])), (what, l)


@pytest.mark.parametrize("n,h,w,form", WS_CASES, ids=[f"n{c[0]}_{c[1]}x{c[2]}_{c[3]}" for c in WS_CASES])
def test_features_on_a_guarded_workspace_of_any_contents(model, record, n, h, w, form):
    """dc_lpips_alex_features on a guarded workspace of exactly dc_lpips_features_ws_bytes under the three fills: the five maps
    are the bits LPIPS.features returns"""
    import ctypes
    import edge_cases as E
    from diffcodec_amd import lib, metrics
    wts = model._weights(torch.device(DEV))
    sets = [_ws_operands(n, h, w, form, seed) for seed in (h * 7 + w + n, 977)]
    st = torch.cuda.current_stream().cuda_stream
    shapes = [((n, co) + s, torch.float32) for co, s in zip(metrics.LPIPS_CHANNELS, metrics.lpips_map_sizes(h, w))]

    def launch(ws, outs, prime):
        _, (x, _), s = sets[int(prime)]
        lib.call("dc_lpips_alex_features", x.data_ptr(), int(form == "u8"), (ctypes.c_longlong * 4)(*s), n, h, w, 0, wts.data_ptr(),
                 ws.data_ptr(), *[o.data_ptr() for o in outs], st)

    what = f"dc_lpips_alex_features {n}x{h}x{w} {form}"
    outs, share = E.run_on_fills(launch, lib.load().dc_lpips_features_ws_bytes(n, h, w), shapes, what,
                                 operands=sets[0][0] + sets[1][0], device=DEV)
    record(f"ws_unwritten_share[{what}]", share)
    for l, (o, f) in enumerate(zip(outs, model.features(sets[0][1][0]))):
        assert torch.equal(E.ws_bits(o), E.ws_bits(f)), (what, l)


# ------------------------------------------------------------------------------------------- clip scoring
from test_gpu_metrics import KW, _free_port, _write_clip, small  # noqa: E402,F401  (the clip fixtures of the PSNR / MS-SSIM tests)


def _frame_lpips_ref(sd, out, root, video, size, f):
    from diffcodec_amd.io_utils import _load_rgb_u8
    gt = torch.from_numpy(_load_rgb_u8(os.path.join(root, video, "images", f"frame_{f:04d}.png"), size))[None]
    return R.lpips(sd, torch.from_numpy(out["frames"][f])[None], gt)[0].item()


def test_decode_clip_adds_lpips(small, model, sd, tmp_path, record):
    from diffcodec_amd import clip_decode as CD, metrics
    pipe, pe, npe = small
    root = str(tmp_path)
    _write_clip(root, "v256", (256, 256), seed=1)
    src = CD.DirectorySource(root, "v256", 4, (256, 256), device=DEV)
    kw = dict(tile=256, batch=4, seed=5, rank=0, world=1, score=True, **KW)
    out = CD.decode_clip(pipe, src, 5, 4, 256, 256, pe, npe, lpips=model, **kw)
    plain = CD.decode_clip(pipe, src, 5, 4, 256, 256, pe, npe, **kw)
    assert sorted(out["scores"]) == [1, 2, 3]
    for f, s in out["scores"].items():
        assert sorted(s) == ["lpips", "ms_ssim", "psnr"] and sorted(plain["scores"][f]) == ["ms_ssim", "psnr"]
        assert s["psnr"] == plain["scores"][f]["psnr"] and s["ms_ssim"] == plain["scores"][f]["ms_ssim"]     # the same bits
        ref = _frame_lpips_ref(sd, out, root, "v256", (256, 256), f)
        e = abs(s["lpips"] - ref) / ref
        record(f"clip_256_frame{f}_lpips_rel_err", e)
        assert isinstance(s["lpips"], float) and ref > 1e-4 and e <= BAR_V, (f, s, ref)
    m = metrics.summarize(out["scores"])
    assert m["frames"] == 3 and abs(m["lpips"] - sum(s["lpips"] for s in out["scores"].values()) / 3) < 1e-15
    assert "lpips" not in metrics.summarize(plain["scores"])


def _world2_worker(rank, world, port, root, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    from diffcodec_amd import clip_decode as CD, metrics, selftest as T, sharding
    sharding.init_from_env(backend="gloo")
    pipe, _ = T.build_small_pipeline()
    pe, npe = T.synth_text(1, dim=T.SMALL_UNET["cross_attention_dim"])
    src = CD.DirectorySource(root, "v256", 4, (256, 256), device=DEV)
    model = metrics.LPIPS.from_state_dict(R.synth_weights(seed=SEED))
    out = CD.decode_clip(pipe, src, 5, 4, 256, 256, pe.to(DEV), npe.to(DEV), tile=256, batch=1, seed=5, gather=False, score=True,
                         lpips=model, **KW)
    q.put((rank, [u.frame for u in out["mine"]], out["scores"]))
    dist.barrier()
    dist.destroy_process_group()


def test_world2_gloo_gathers_four_columns_on_rank0(small, model, tmp_path):
    """two ranks share the GPU over gloo, gather=False: rank 0 receives (scored, PSNR, MS-SSIM, LPIPS) of every frame through one
    gather; the values equal a single-rank run's."""
    from diffcodec_amd import clip_decode as CD
    pipe, pe, npe = small
    root = str(tmp_path)
    _write_clip(root, "v256", (256, 256), seed=1)
    src = CD.DirectorySource(root, "v256", 4, (256, 256), device=DEV)
    ref = CD.decode_clip(pipe, src, 5, 4, 256, 256, pe, npe, tile=256, batch=1, seed=5, rank=0, world=1, score=True, lpips=model,
                         **KW)["scores"]
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
    assert res[1][2] == {2: ref[2]}                               # rank 1 keeps its own
    assert res[0][2] == ref and all(sorted(s) == ["lpips", "ms_ssim", "psnr"] for s in ref.values()), (res[0][2], ref)
