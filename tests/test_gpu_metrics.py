"""GPU: PSNR / SSIM / MS-SSIM of csrc/metrics.hip (diffcodec_amd.metrics) against the fp64 restatement tests/metrics_ref.py, their
exactness, layouts and reproducibility, and decode_clip(score=True) — single rank, through the tile blend, and sharded over two
ranks with the scores (not the pixels) gathered.

The edge tests (tests/edge_cases.py: SSIM_CASES, MS_SSIM_CASES, PSNR_CASES, METRIC_REFUSALS) call dc_ssim / dc_ms_ssim / dc_psnr
directly on guarded operands, a guarded scratch of exactly dc_*_ws_bytes and a guarded fp64 output, under the three scratch fills of
E.run_on_fills (the NaN pattern, zeros, the leftovers of a launch on the swapped operands), and hold all three segments of the
output to R.expected within R.ssim_bound."""
import ctypes
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

import edge_cases as E
import metrics_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
MS_BAR, SSIM_BAR = 2e-6, 5e-6


def _pair(n, c, h, w, seed, peak=255.0):
    """a smooth random field and a noisy copy, in [0, peak], fp32 on the CPU"""
    g = torch.Generator().manual_seed(seed)
    base = F.interpolate(torch.rand(n, c, h // 16 + 2, w // 16 + 2, generator=g), size=(h, w), mode="bicubic", align_corners=False)
    base = (base + 0.1 * torch.rand(n, c, h, w, generator=g)).clamp(0, 1)
    noisy = (base + 0.06 * torch.randn(n, c, h, w, generator=g)).clamp(0, 1)
    return (base * peak).float(), (noisy * peak).float()


def _u8_nhwc(t):
    return t.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd import metrics
    return metrics


# (H, W, N, C, operand form, size_average, extra kwargs)
CASES = [
    (161, 161, 1, 3, "u8", True, {}),
    (256, 256, 4, 1, "f255", False, {}),
    (512, 512, 1, 3, "f1", True, {}),
    (513, 769, 4, 3, "u8", False, {}),
    (1080, 1920, 1, 3, "f1", False, {}),
    (256, 256, 4, 3, "f255", False, dict(weights=(0.2, 0.3, 0.5))),
    (200, 300, 1, 3, "u8", True, dict(win_size=7)),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}x{c[1]}_n{c[2]}c{c[3]}_{c[4]}_{'avg' if c[5] else 'pern'}{'_' + '_'.join(c[6]) if c[6] else ''}"
                                            for c in CASES])
def test_parity_with_fp64_restatement(M, record, case):
    h, w, n, c, form, size_average, kw = case
    peak = 1.0 if form == "f1" else 255.0
    x, y = _pair(n, c, h, w, seed=h * 7 + w + n + c, peak=peak)
    if form == "u8":
        x, y = _u8_nhwc(x), _u8_nhwc(y)
    xd, yd = x.to(DEV), y.to(DEV)
    ref_kw = dict(kw)
    ms = M.ms_ssim(xd, yd, data_range=peak, size_average=size_average, **kw)
    ref = R.ms_ssim(x, y, data_range=peak, size_average=size_average, **ref_kw)
    assert ms.is_cuda and ms.dtype == torch.float32 and ms.shape == ref.shape
    e_ms = (ms.double().cpu() - ref).abs().max().item()
    ss_kw = {k: v for k, v in kw.items() if k != "weights"}
    ss = M.ssim(xd, yd, data_range=peak, size_average=size_average, **ss_kw)
    e_ss = (ss.double().cpu() - R.ssim(x, y, data_range=peak, size_average=size_average, **ss_kw)).abs().max().item()
    p = M.psnr(xd, yd, data_range=peak)
    pr = R.psnr(x, y, data_range=peak)
    e_p = ((p.cpu() - pr).abs() / pr).max().item()
    record(f"metrics_{h}x{w}_n{n}c{c}_{form}_ms_ssim_abs_err", e_ms)
    record(f"metrics_{h}x{w}_n{n}c{c}_{form}_ssim_abs_err", e_ss)
    assert 0.05 < float(ref.min()) < 0.999                      # a non-trivial score
    assert e_ms <= MS_BAR, e_ms
    assert e_ss <= SSIM_BAR, e_ss
    assert p.dtype == torch.float64 and e_p <= 1e-12, e_p


def test_identical_inputs_and_exact_uint8_sse(M):
    x, y = _pair(2, 3, 300, 257, seed=11)
    xu, yu = _u8_nhwc(x).to(DEV), _u8_nhwc(y).to(DEV)
    assert M.ms_ssim(xu, xu).item() == 1.0 and M.ssim(xu, xu).item() == 1.0
    xf = x.to(DEV)
    assert M.ms_ssim(xf, xf, data_range=255).item() == 1.0
    assert torch.isinf(M.psnr(xu, xu)).all() and torch.isinf(M.psnr(xf, xf)).all()
    p = M.psnr(xu, yu).cpu()
    d = xu.cpu().numpy().astype(np.int64) - yu.cpu().numpy().astype(np.int64)
    sse = (d * d).reshape(2, -1).sum(1)                           # exact integers
    mse = sse / float(3 * 300 * 257)
    want = 10 * np.log10(255.0 ** 2 / mse)
    assert np.abs(p.numpy() - want).max() / want.min() <= 1e-14
    pf = M.psnr(xf, y.to(DEV)).cpu()
    assert ((pf - R.psnr(x, y)).abs() / R.psnr(x, y)).max().item() <= 1e-12


def test_layouts_give_the_same_bits(M):
    x, y = _pair(2, 3, 181, 203, seed=12)
    xu, yu = _u8_nhwc(x), _u8_nhwc(y)
    xf, yf = xu.permute(0, 3, 1, 2).float(), yu.permute(0, 3, 1, 2).float()          # the same values as float NCHW
    xu, yu = xu.to(DEV), yu.to(DEV)
    xfd, yfd = xf.contiguous().to(DEV), yf.contiguous().to(DEV)
    for f in (M.ms_ssim, M.ssim):
        a = f(xu, yu, data_range=255, size_average=False)
        b = f(xfd, yfd, data_range=255, size_average=False)
        assert torch.equal(a, b), (f.__name__, a, b)
    assert torch.equal(M.psnr(xu, yu), M.psnr(xfd, yfd))
    # a permuted (channels-last storage) float view reads in place and gives the bits of its contiguous copy
    xv, yv = xfd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), yfd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not xv.is_contiguous()
    for f in (M.ms_ssim, M.ssim):
        assert torch.equal(f(xv, yv, size_average=False), f(xfd, yfd, size_average=False))
    assert torch.equal(M.psnr(xv, yv), M.psnr(xfd, yfd))


def test_reproducible_graph_capturable_and_host_tensors(M):
    x, y = _pair(4, 3, 512, 512, seed=13)
    xd, yd = x.to(DEV), y.to(DEV)
    a = M.ms_ssim(xd, yd, size_average=False)
    b = M.ms_ssim(xd, yd, size_average=False)
    pa, pb = M.psnr(xd, yd), M.psnr(xd, yd)
    assert torch.equal(a, b) and torch.equal(pa, pb)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        M.ms_ssim(xd, yd, size_average=False)
        M.psnr(xd, yd)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gm = M.ms_ssim(xd, yd, size_average=False)
        gp = M.psnr(xd, yd)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gm, a) and torch.equal(gp, pa)
    xd.mul_(0.5)                                                   # replay reads the captured operands
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gm, M.ms_ssim(xd, yd, size_average=False))
    h = M.ms_ssim(x, y, size_average=False)
    assert not h.is_cuda and torch.equal(h, a.cpu())
    hp = M.psnr(x, y)
    assert not hp.is_cuda and torch.equal(hp, pa.cpu())


# ------------------------------------------------------------------------------------------- clip scoring
def _write_clip(root, video, size, frames=5, gop=4, seed=0):
    from PIL import Image
    from diffcodec_amd.io_utils import write_flo
    rng = np.random.default_rng(seed)
    base = os.path.join(root, video)
    sub = f"optical_flow_gop_{gop}_raft"
    for d in ("images", os.path.join("optical_flow", sub), os.path.join("optical_flow_bwd", sub)):
        os.makedirs(os.path.join(base, d), exist_ok=True)
    h, w = size
    for i in range(frames):
        coarse = torch.from_numpy(rng.random((1, 3, h // 32 + 2, w // 32 + 2))).float()
        img = F.interpolate(coarse, size=(h, w), mode="bicubic", align_corners=False)[0].permute(1, 2, 0).numpy()
        img = np.clip(img * 255 + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(base, "images", f"frame_{i:04d}.png"))
    for f in range(1, frames):
        if f % gop == 0:
            continue
        p, nx = (f // gop) * gop, (f // gop + 1) * gop
        write_flo(os.path.join(base, "optical_flow", sub, f"flow_{p:04d}_{f:04d}.flo"), rng.normal(0, 2, (h, w, 2)))
        write_flo(os.path.join(base, "optical_flow_bwd", sub, f"flow_{nx:04d}_{f:04d}.flo"), rng.normal(0, 2, (h, w, 2)))


KW = dict(num_inference_steps=2, guidance_scale=4.5, controlnet_conditioning_scale=1.7)


def _check_scores(out, root, video, size, record, tag):
    from diffcodec_amd.io_utils import _load_rgb_u8
    assert sorted(out["scores"]) == sorted(out["frames"]) == [1, 2, 3]
    for f, s in out["scores"].items():
        gt = torch.from_numpy(_load_rgb_u8(os.path.join(root, video, "images", f"frame_{f:04d}.png"), size))[None]
        pred = torch.from_numpy(out["frames"][f])[None]
        rp = R.psnr(pred, gt).item()
        rm = R.ms_ssim(pred, gt, data_range=255).item()
        record(f"clip_{tag}_frame{f}_ms_ssim_abs_err", abs(s["ms_ssim"] - rm))
        assert isinstance(s["psnr"], float) and abs(s["psnr"] - rp) <= 1e-12 * abs(rp), (f, s, rp)
        assert abs(s["ms_ssim"] - rm) <= MS_BAR, (f, s, rm)


@pytest.fixture(scope="module")
def small():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd import selftest as T
    pipe, _ = T.build_small_pipeline()
    pe, npe = T.synth_text(1, dim=T.SMALL_UNET["cross_attention_dim"])
    return pipe, pe.to(DEV), npe.to(DEV)


def test_decode_clip_scores_frames(small, tmp_path, record):
    from diffcodec_amd import clip_decode as CD, metrics
    pipe, pe, npe = small
    root = str(tmp_path)
    _write_clip(root, "v256", (256, 256), seed=1)
    src = CD.DirectorySource(root, "v256", 4, (256, 256), device=DEV)
    out = CD.decode_clip(pipe, src, 5, 4, 256, 256, pe, npe, tile=256, batch=4, seed=5, rank=0, world=1, score=True, **KW)
    _check_scores(out, root, "v256", (256, 256), record, "256")
    plain = CD.decode_clip(pipe, src, 5, 4, 256, 256, pe, npe, tile=256, batch=4, seed=5, rank=0, world=1, **KW)
    assert "scores" not in plain and all(np.array_equal(plain["frames"][f], out["frames"][f]) for f in out["frames"])
    s = metrics.summarize(out["scores"])
    assert s["frames"] == 3 and s["identical"] == 0
    # through the tile blend: 384x384 frames as 2 x 2 tiles of 256
    _write_clip(root, "v384", (384, 384), seed=2)
    src2 = CD.DirectorySource(root, "v384", 4, (384, 384), device=DEV)
    out2 = CD.decode_clip(pipe, src2, 5, 4, 384, 384, pe, npe, tile=256, overlap=64, batch=4, seed=5, rank=0, world=1, score=True, **KW)
    assert len(out2["units"]) == 12
    _check_scores(out2, root, "v384", (384, 384), record, "384_tiled")
    # a ground truth of another size is refused
    bad = CD.DirectorySource(root, "v256", 4, (384, 384), device=DEV)
    with pytest.raises(ValueError, match="ground truth"):
        CD.decode_clip(pipe, bad, 5, 4, 256, 256, pe, npe, tile=256, batch=4, seed=5, rank=0, world=1, score=True,
                       **dict(KW, num_inference_steps=1))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _world2_worker(rank, world, port, root, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    from diffcodec_amd import clip_decode as CD, selftest as T, sharding
    sharding.init_from_env(backend="gloo")
    pipe, _ = T.build_small_pipeline()
    pe, npe = T.synth_text(1, dim=T.SMALL_UNET["cross_attention_dim"])
    src = CD.DirectorySource(root, "v256", 4, (256, 256), device=DEV)
    out = CD.decode_clip(pipe, src, 5, 4, 256, 256, pe.to(DEV), npe.to(DEV), tile=256, batch=1, seed=5, gather=False, score=True, **KW)
    q.put((rank, [u.frame for u in out["mine"]], out["scores"]))
    dist.barrier()
    dist.destroy_process_group()


def test_world2_gloo_scores_gathered_on_rank0(small, tmp_path):
    """two ranks share the GPU over gloo, gather=False: each scores the frames it completed, rank 0 receives every frame's scores
    through one gather of a float64 tensor; they equal a single-rank run's."""
    from diffcodec_amd import clip_decode as CD
    pipe, pe, npe = small
    root = str(tmp_path)
    _write_clip(root, "v256", (256, 256), seed=1)
    src = CD.DirectorySource(root, "v256", 4, (256, 256), device=DEV)
    ref = CD.decode_clip(pipe, src, 5, 4, 256, 256, pe, npe, tile=256, batch=1, seed=5, rank=0, world=1, score=True, **KW)["scores"]
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
    assert res[0][2] == ref, (res[0][2], ref)


# ------------------------------------------------------------------------------------------- edge tables on guarded buffers
@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd import lib as l
    return l


_WORST = {}


def _note(record, key, ratio):
    k = "/".join(str(v) for v in key)
    _WORST[k] = max(_WORST.get(k, 0.0), ratio)
    record(f"edge[{k}]", f"worst_err_over_bound={_WORST[k]:.4f}")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    t = t.contiguous()
    return t if t.dtype == torch.uint8 else t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def _operands(c, X, Y):
    _, lx, ly = E.METRIC_FORMS[c.form]
    gx, sx = E.metric_operand(X, lx, DEV)
    gy, sy = E.metric_operand(Y, ly, DEV)
    assert (sx != sy) == (c.form == "mixed")
    return gx, gy, sx, sy, ((ctypes.c_longlong * 8)(*sx, *sy), (ctypes.c_longlong * 8)(*sy, *sx))


def _launch_twice(launch, nbytes, nout, operands, what):
    """E.run_on_fills on one guarded fp64 output: launch(ws, out, swap) into a guarded scratch of exactly dc_*_ws_bytes holding the
    NaN pattern (as floats), zeros, and what a launch on the swapped operands left; every guard intact and every output element
    written after each, the outputs bitwise equal -> the first output (CPU).  The outputs may be NaN or +inf by design (the `nan`
    family, PSNR of identical images), so finiteness is left to the callers' value checks."""
    def run(ws, outs, prime):
        launch(ws.data_ptr(), outs[0].data_ptr(), prime)

    (out,), _ = E.run_on_fills(run, nbytes, [((nout,), torch.float64)], what, operands=operands, device=DEV, finite=False)
    return out.cpu()


def _ssim_edge(lib, record, c, seed, key):
    X, Y = E.metric_inputs(c, seed)
    g = E.metric_window(c.ws)
    exp = R.case_expected(c, X, Y, g)
    gx, gy, sx, sy, strides = _operands(c, X, Y)
    u8 = int(c.dtype == "u8")
    win = (ctypes.c_float * c.ws)(*g.tolist())
    nbytes = lib.load().dc_ssim_ws_bytes(c.n, c.c, c.h, c.w, c.ws, c.levels or 1)
    if c.levels:
        wts = (ctypes.c_float * c.levels)(*c.weights)

        def launch(ws, out, swap):
            a, b = (gy, gx) if swap else (gx, gy)
            lib.call("dc_ms_ssim", a.view.data_ptr(), b.view.data_ptr(), u8, strides[int(swap)], c.n, c.c, c.h, c.w, win, c.ws, wts,
                     c.levels, c.K[0], c.K[1], c.L, ws, out, _st())
    else:
        def launch(ws, out, swap):
            a, b = (gy, gx) if swap else (gx, gy)
            lib.call("dc_ssim", a.view.data_ptr(), b.view.data_ptr(), u8, strides[int(swap)], c.n, c.c, c.h, c.w, win, c.ws, c.K[0], c.K[1],
                     c.L, int(c.nonneg), ws, out, _st())

    out = _launch_twice(launch, nbytes, c.n * c.c + c.n + 1, [gx, gy], c.label())
    for gop, t, st in ((gx, X, sx), (gy, Y, sy)):
        assert torch.equal(_bits(E.metric_read(gop, tuple(t.shape), st).cpu()), _bits(t)), f"{c.label()}: an operand was written"
    v = R.check_out(out, exp)
    print(f"{c.label()}: err/bound {v['ratio']:.4g} ({v['what']})")
    _note(record, key, v["ratio"])
    assert v["ok"], (c.label(), v, out.tolist()[:12])


@pytest.mark.parametrize("i", range(len(E.SSIM_CASES)), ids=[c.label() for c in E.SSIM_CASES])
def test_ssim_edge(lib, record, i):
    c = E.SSIM_CASES[i]
    _ssim_edge(lib, record, c, i, E.ssim_instance(c))


@pytest.mark.parametrize("i", range(len(E.MS_SSIM_CASES)), ids=[c.label() for c in E.MS_SSIM_CASES])
def test_ms_ssim_edge(lib, record, i):
    c = E.MS_SSIM_CASES[i]
    _ssim_edge(lib, record, c, i, ("ms_ssim", c.levels))


@pytest.mark.parametrize("i", range(len(E.PSNR_CASES)), ids=[c.label() for c in E.PSNR_CASES])
def test_psnr_edge(lib, record, i):
    """uint8: within 1e-14 max(|ref|, 1) of the value of the exact integer SSE; fp32 operands: 1e-12 max(|ref|, 1) of the fp64
    restatement; identical images: +inf"""
    c = E.PSNR_CASES[i]
    X, Y = E.metric_inputs(c, i)
    gx, gy, sx, sy, strides = _operands(c, X, Y)
    u8 = c.dtype == "u8"

    def launch(ws, out, swap):
        a, b = (gy, gx) if swap else (gx, gy)
        lib.call("dc_psnr", a.view.data_ptr(), b.view.data_ptr(), int(u8), strides[int(swap)], c.n, c.c, c.h, c.w, float(c.L), ws, out,
                 _st())

    out = _launch_twice(launch, lib.load().dc_psnr_ws_bytes(c.n), c.n, [gx, gy], c.label())
    if u8:
        d = X.numpy().astype(np.int64) - Y.numpy().astype(np.int64)
        sse = (d * d).reshape(c.n, -1).sum(1)
        with np.errstate(divide="ignore"):
            ref = torch.from_numpy(10 * np.log10(float(c.L) ** 2 / (sse / float(c.c * c.h * c.w))))
        rel = 1e-14
    else:
        ref, rel = R.psnr(X.double(), Y.double(), c.L), 1e-12
    if c.family == "identical":
        assert bool((ref == math.inf).all())
    inf = torch.isinf(ref)
    assert torch.equal(out[inf], ref[inf]), (c.label(), out)
    ratio = ((out - ref).abs()[~inf] / (rel * ref.abs().clamp_min(1.0)[~inf]))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{c.label()}: err/bound {worst:.4g}")
    _note(record, ("psnr", c.dtype), worst)
    assert not bool(torch.isnan(out).any()) and worst <= 1.0, (c.label(), out.tolist(), ref.tolist())


def test_metric_launches_refuse_what_ws_bytes_refuses(lib):
    """every METRIC_REFUSALS shape, a null window, null weights in MS mode and PSNR with N = 0 / 65536: dc_*_ws_bytes and the
    launch return -1 and a guarded output keeps its pattern"""
    L = lib.load()
    x, y = (E.Guarded((64,), torch.float32, DEV) for _ in range(2))
    x.view.fill_(0.5)
    y.view.fill_(0.25)
    ws = E.Guarded((1 << 16,), torch.uint8, DEV)
    out = E.Guarded((16,), torch.float64, DEV)
    xp, yp, wp, op = x.view.data_ptr(), y.view.data_ptr(), ws.view.data_ptr(), out.view.data_ptr()
    wts = (ctypes.c_float * 9)(*([0.1] * 9))
    for label, (n, c, h, w, wsz, lv) in E.METRIC_REFUSALS:
        strides = (ctypes.c_longlong * 8)(*((c * h * w, h * w, w, 1) * 2))
        win = (ctypes.c_float * 17)(*([1.0 / max(wsz, 1)] * 17))
        assert L.dc_ssim_ws_bytes(n, c, h, w, wsz, lv) == -1, label
        assert L.dc_ms_ssim(xp, yp, 0, strides, n, c, h, w, win, wsz, wts, lv, 0.01, 0.03, 1.0, wp, op, _st()) == -1, label
        if lv == 1:
            assert L.dc_ssim(xp, yp, 0, strides, n, c, h, w, win, wsz, 0.01, 0.03, 1.0, 0, wp, op, _st()) == -1, label
    strides = (ctypes.c_longlong * 8)(*((64, 64, 8, 1) * 2))
    win = (ctypes.c_float * 3)(0.25, 0.5, 0.25)
    assert L.dc_ssim_ws_bytes(1, 1, 8, 8, 3, 1) > 0
    assert L.dc_ssim(xp, yp, 0, strides, 1, 1, 8, 8, None, 3, 0.01, 0.03, 1.0, 0, wp, op, _st()) == -1
    assert L.dc_ms_ssim(xp, yp, 0, strides, 1, 1, 8, 8, None, 3, wts, 1, 0.01, 0.03, 1.0, wp, op, _st()) == -1
    assert L.dc_ms_ssim(xp, yp, 0, strides, 1, 1, 8, 8, win, 3, None, 1, 0.01, 0.03, 1.0, wp, op, _st()) == -1
    for n in (0, 65536):
        assert L.dc_psnr_ws_bytes(n) == -1, n
        assert L.dc_psnr(xp, yp, 0, strides, n, 1, 8, 8, 1.0, wp, op, _st()) == -1, n
    assert L.dc_psnr_ws_bytes(65535) == 65535 * 512
    torch.cuda.synchronize()
    for g in (x, y, ws, out):
        g.assert_intact("refusals")
    assert out.unwritten() == 16
