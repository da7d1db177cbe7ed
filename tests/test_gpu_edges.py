"""GPU: every case of tests/edge_cases.py — each conv / linear, fp32 extractor conv and attention kernel instance the dispatchers can
reach, the normalisation kernels at their template and chunking edges, and the fused loop's state kernels — launched on guarded operands and outputs, its route asserted first,
its output held to the fp64 reference of oracle/launch_ref.py with L.check, its guards checked bit for bit, and a second launch
into a second guarded output required to be bitwise equal.  Worst err/tol per instance goes to `record`."""
import math

import pytest
import torch

import edge_cases as E
from oracle import launch_ref as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd import ops as o
    return o


_WORST = {}


def _note(record, key, verdict, what):
    k = E.key_str(key) if isinstance(key[0], str) else str(key)
    _WORST[k] = max(_WORST.get(k, 0.0), verdict["ratio"])
    record(f"edge[{k}]", f"worst_err_over_tol={_WORST[k]:.4f}")
    assert verdict["ok"], (f"{what}: worst {verdict['worst']} err {verdict['err']:.3e} tol {verdict['tol']:.3e} "
                           f"err/tol {verdict['ratio']:.3g} rel-rms {verdict['rms']:.3e}")


def _g(shape, dtype, data=None, pitch=None):
    g = E.Guarded(shape, dtype, DEV, pitch=pitch)
    if data is not None:
        g.fill(data)
    return g


def _same_bits(a, b):
    it = torch.int16 if a.dtype == BF else torch.int32
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ------------------------------------------------------------------------------------------ conv / linear
def _capture(lib):
    seen = []
    real = lib.call

    def call(name, *args, meta=None):
        if name == "dc_conv_igemm_bf16":
            d = args[0]
            seen.append(type(d).from_buffer_copy(d))
        return real(name, *args, meta=meta)
    return seen, real, call


@pytest.mark.parametrize("i", range(len(E.CONV_CASES)), ids=[c.label() for c in E.CONV_CASES])
def test_conv_edge(ops, record, i):
    from diffcodec_amd import lib
    c = E.CONV_CASES[i]
    assert E.conv_key(E.case_desc(c)) == c.key, c.label()
    gen = torch.Generator().manual_seed(1000 + i)
    cin = c.c1 + c.c2
    ho, wo, m = c.ho, c.wo, c.m
    cout_eff = c.cout // 2 if c.geglu else c.cout
    w = torch.randn(c.cout, cin, c.k, c.k, generator=gen) / math.sqrt(cin * c.k * c.k)
    b = torch.randn(c.cout, generator=gen) * 0.1
    ln = None
    if c.ln is not None:
        ln = (1 + 0.1 * torch.randn(cin, generator=gen), 0.1 * torch.randn(cin, generator=gen), 1e-5)
    pc = ops.PackedConv(w, b, DEV, geglu=c.geglu, ln=ln, mfma_small_cout=c.cout < 16)
    gw, gb = _g(tuple(pc.w.shape), BF, pc.w), _g(tuple(pc.bias.shape), F32, pc.bias)
    pc.w, pc.bias = gw.view, gb.view
    guards = {"w": gw, "bias": gb}
    x1 = guards.setdefault("x1", _g((c.n, c.h, c.w, c.c1), BF, (torch.randn(c.n, c.h, c.w, c.c1, generator=gen) + 0.3).to(DEV)))
    kw = dict(stride=c.stride, pad=c.pad, upsample=c.up, out_scale=c.out_scale, out_f32=c.out_f32, splitk=c.splitk, act=c.act,
              gn_part=c.gn_part)
    if c.c2:
        kw["x2"] = guards.setdefault("x2", _g((c.n, c.h, c.w, c.c2), BF, torch.randn(c.n, c.h, c.w, c.c2, generator=gen).to(DEV))).view
    if c.gn:
        ab = torch.stack([1 + 0.2 * torch.randn(c.n, cin, generator=gen), 0.2 * torch.randn(c.n, cin, generator=gen)], 2)
        kw["gn_ab"] = guards.setdefault("gn_ab", _g((c.n, cin, 2), F32, ab.to(DEV))).view
        kw["gn_silu"] = c.gn_silu
    if c.row_add:
        kw["row_add"] = guards.setdefault("row_add", _g((c.n, c.cout), F32, torch.randn(c.n, c.cout, generator=gen).to(DEV),
                                                          pitch=c.cout + 8)).view
    if c.residual:
        kw["residual"] = guards.setdefault("residual", _g((c.n, ho, wo, c.cout), BF,
                                                          torch.randn(c.n, ho, wo, c.cout, generator=gen).to(DEV))).view
    xr = x1.view.reshape(-1, c.c1).to(torch.float64)
    if c.ln == "pairs":
        mean = xr.mean(1)
        rstd = 1.0 / torch.sqrt(xr.var(1, unbiased=False) + 1e-5)
        kw["ln_stats"] = guards.setdefault("ln_stats", _g((m, 2), F32, torch.stack([mean, rstd], 1).float())).view
    elif c.ln is not None:
        parts = c.ln
        bounds = [(p * cin) // parts for p in range(parts + 1)]
        pr = torch.stack([torch.stack([xr[:, lo:hi].sum(1), (xr[:, lo:hi] ** 2).sum(1)], 1) for lo, hi in zip(bounds, bounds[1:])], 1)
        kw["ln_partials"] = (guards.setdefault("ln_partials", _g((m, parts, 2), F32, pr.float())).view, 1e-5)
    outs = []
    seen, real, call = _capture(lib)
    for rep in range(2):
        og = _g((c.n, ho, wo, cout_eff), F32 if c.out_f32 else BF)
        sog = _g((m, ops.row_stats_parts(c.cout), 2), F32) if c.stats_out else None
        lib.call = call
        try:
            y = ops.conv(x1.view, pc, out=og.view, stats_out=None if sog is None else sog.view, **kw)
        finally:
            lib.call = real
        torch.cuda.synchronize()
        outs.append((og, sog, y))
    assert len(seen) == 2 and E.conv_key(seen[0]) == c.key, (c.label(), [E.key_str(E.conv_key(d)) for d in seen])
    for name, g in guards.items():
        g.assert_intact(f"{c.label()} operand {name}")
    og, sog, y = outs[0]
    for o in (outs[0], outs[1]):
        o[0].assert_intact(f"{c.label()} out")
        if o[1] is not None:
            o[1].assert_intact(f"{c.label()} stats_out")
    assert og.unwritten() == 0, f"{c.label()}: {og.unwritten()} output elements never written"
    assert bool(torch.isfinite(og.view).all()), f"{c.label()}: non-finite output (a poisoned operand element was read)"
    assert _same_bits(outs[0][0].view, outs[1][0].view), f"{c.label()}: launch-to-launch difference"
    rows = L.sample_rows(m, spatial=(c.n, ho, wo) if c.k == 3 else None) if m > 4096 else torch.arange(m)
    r, s = L.conv_ref(x1.view, pc, rows, x2=kw.get("x2"), gn_ab=kw.get("gn_ab"), gn_silu=c.gn_silu, row_add=kw.get("row_add"),
                      residual=kw.get("residual"), stride=c.stride, pad=c.pad, upsample=c.up, out_scale=c.out_scale, act=c.act)
    yr = og.view.reshape(m, cout_eff)[rows.to(DEV)]
    _note(record, c.key, L.check(yr, r, s, og.dtype), c.label())
    if sog is not None:
        tr, ts = L.row_stats_totals_ref(yr)
        _note(record, c.key + ("stats_out",), L.check(sog.view[rows.to(DEV)].to(torch.float64).sum(1), tr, ts, F32), c.label())
    gp = getattr(y, "gn_part", None)
    if ("gn_part", True) in c.key or ("st", 2) in c.key or ("st", 3) in c.key:
        assert gp is not None, f"{c.label()}: no GroupNorm partials"
    if gp is not None:
        tr, ts = L.gn_part_totals_ref(og.view)
        _note(record, c.key + ("gn_part",), L.check(gp.to(torch.float64).sum(0), tr, ts, F32), c.label())


@pytest.mark.parametrize("i", range(len(E.SMALL_CASES)), ids=[c.label() for c in E.SMALL_CASES])
def test_small_conv_edge(ops, record, i):
    from diffcodec_amd import lib
    c = E.SMALL_CASES[i]
    gen = torch.Generator().manual_seed(1500 + i)
    w = torch.randn(c.cout, c.cin, c.k, c.k, generator=gen) / math.sqrt(c.cin * c.k * c.k)
    b = torch.randn(c.cout, generator=gen) * 0.1
    pc = ops.PackedConv(w, b, DEV)
    assert pc.kind == c.kind, (c.label(), pc.kind)
    gw, gb = _g(tuple(pc.w.shape), BF, pc.w), _g(tuple(pc.bias.shape), F32, pc.bias)
    pc.w, pc.bias = gw.view, gb.view
    x = _g((c.n, c.h, c.w, c.cin), BF, (torch.randn(c.n, c.h, c.w, c.cin, generator=gen) + 0.3).to(DEV))
    guards = [x, gw, gb]
    gab = None
    if c.gn:
        ab = torch.stack([1 + 0.2 * torch.randn(c.n, c.cin, generator=gen), 0.2 * torch.randn(c.n, c.cin, generator=gen)], 2)
        gab = _g((c.n, c.cin, 2), F32, ab.to(DEV))
        guards.append(gab)
    ho, wo = c.ho, c.wo
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for rep in range(2):
        go = _g((c.n, ho, wo, c.cout), F32 if c.out_f32 else BF)
        if c.kind == "small_cin":
            lib.call("dc_conv_small_cin_bf16", x.view.data_ptr(), pc.w.data_ptr(), pc.bias.data_ptr(), go.view.data_ptr(), c.n, c.h, c.w,
                     c.cin, c.cout, c.k, c.stride, c.pad if c.k == 3 else 0, ho, wo, st)
        else:
            lib.call("dc_conv_small_cout_bf16", x.view.data_ptr(), pc.w.data_ptr(), pc.bias.data_ptr(), 0 if gab is None else gab.view.data_ptr(),
                     int(c.gn), c.n if c.gn else 0, go.view.data_ptr(), int(c.out_f32), c.n, c.h, c.w, c.cin, c.cout, c.k, st)
        torch.cuda.synchronize()
        outs.append(go)
    for g in guards + outs:
        g.assert_intact(c.label())
    assert outs[0].unwritten() == 0 and bool(torch.isfinite(outs[0].view).all()), c.label()
    assert _same_bits(outs[0].view, outs[1].view), f"{c.label()}: launch-to-launch difference"
    m = c.n * ho * wo
    rows = torch.arange(m)
    r, s = L.conv_ref(x.view, pc, rows, gn_ab=None if gab is None else gab.view, gn_silu=c.gn, stride=c.stride, pad=c.pad)
    key = (c.kind, "strip" if c.strip_kernel else f"cout={c.cout}" if c.kind == "small_cout" else "pixel")
    _note(record, key, L.check(outs[0].view.reshape(m, c.cout), r, s, outs[0].dtype), c.label())


# ------------------------------------------------------------------------------------------ fp32 extractor conv
@pytest.mark.parametrize("i", range(len(E.F32_CONV_CASES)), ids=[c.label() for c in E.F32_CONV_CASES])
def test_f32_conv_edge(ops, record, i):
    """dc_conv3x3_nchw_f32 on a channel-slice view whose neighbouring channel planes, like every guard, hold the NaN pattern: an
    over-read of x, w or bias makes the output non-finite.  With bias and SiLU, then without either."""
    from diffcodec_amd import lib
    c = E.F32_CONV_CASES[i]
    assert E.f32_conv_key(c.cin, c.h, c.w, c.cout, c.stride) == c.key, c.label()
    x, w, b = E.f32_conv_inputs(c, i)
    gx = E.Guarded((c.n, c.cin + 2, c.h, c.w), F32, DEV)
    xv = gx.view[:, 1:c.cin + 1]
    xv.copy_(x.to(DEV))
    gw, gb = _g(tuple(w.shape), F32, w.to(DEV)), _g(tuple(b.shape), F32, b.to(DEV))
    ho, wo, m = c.ho, c.wo, c.m
    rows = L.sample_rows(m, spatial=(c.n, ho, wo)) if m > 4096 else torch.arange(m)
    pat = E._signed(E.NAN_BITS[F32], F32)
    for bias, silu in ((True, True), (False, False)):
        what = f"{c.label()} bias={int(bias)} silu={int(silu)}"
        outs = []
        for rep in range(2):
            go = _g((c.n, c.cout, ho, wo), F32)
            lib.call("dc_conv3x3_nchw_f32", xv.data_ptr(), xv.stride(0), gw.view.data_ptr(), gb.view.data_ptr() if bias else 0,
                     go.view.data_ptr(), c.n, c.cin, c.h, c.w, c.cout, c.stride, int(silu), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            outs.append(go)
        for name, g in (("x", gx), ("w", gw), ("bias", gb), ("out", outs[0]), ("out (second launch)", outs[1])):
            g.assert_intact(f"{what} {name}")
        planes = gx.view[:, [0, c.cin + 1]].contiguous().view(torch.int32)
        assert bool((planes == pat).all()), f"{what}: a neighbouring channel plane of x was written"
        assert outs[0].unwritten() == 0, f"{what}: {outs[0].unwritten()} output elements never written"
        assert bool(torch.isfinite(outs[0].view).all()), f"{what}: non-finite output (a poisoned operand element was read)"
        assert _same_bits(outs[0].view, outs[1].view), f"{what}: launch-to-launch difference"
        r, s = L.conv3x3_nchw_f32_ref(xv, gw.view, gb.view if bias else None, rows, stride=c.stride, silu=silu)
        y = outs[0].view.permute(0, 2, 3, 1).reshape(m, c.cout)[rows.to(DEV)]
        _note(record, c.key, L.check(y, r, s, F32), what)


# ------------------------------------------------------------------------------------------ loop-state kernels
_SHAPE_IDS = ["x".join(str(v) for v in s) for s in E.STATE_SHAPES]


@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("shape,t", [(E.STATE_SHAPES[0], t) for t in E.DDIM_ROWS_T] + [(E.STATE_SHAPES[1], 501), (E.STATE_SHAPES[1], 1)])
def test_cfg_ddim_step_edge(ops, record, shape, t, cfg):
    """dc_cfg_ddim_step (the default scheduler step of the fused loop): a three-row coefficient table whose rows 0 and 2 hold the NaN
    pattern and a step counter that starts at 1, so that any other row index poisons the latents."""
    b, c, h, w = shape
    ts, table = E.ddim_table()
    row = table[ts.index(t)]
    eps, lat = E.ddim_inputs(shape, cfg, 9300 + t)
    g = E.STATE_GUIDANCE if cfg else 1.0
    geps = _g(tuple(eps.shape), F32, eps.to(DEV))
    gcoef = E.Guarded((3, 4), F32, DEV)
    gcoef.view[1] = row.to(DEV)
    pat = E._signed(E.NAN_BITS[F32], F32)
    runs = []
    for rep in range(2):
        glat = _g(shape, F32, lat.to(DEV))
        gin = _g((2 * b, h, w, c), BF)
        step = torch.tensor([-7, 1, -7], dtype=torch.int32, device=DEV)
        ops.cfg_ddim_step(geps.view, glat.view, gin.view, gcoef.view, step[1:2], g, cfg)
        torch.cuda.synchronize()
        runs.append((glat, gin, step))
    what = f"cfg_ddim_step {shape} t={t} cfg={int(cfg)}"
    geps.assert_intact(f"{what} eps")
    gcoef.assert_intact(f"{what} coef")
    assert torch.equal(geps.view.cpu(), eps), f"{what}: eps written"
    assert bool((gcoef.view[[0, 2]].contiguous().view(torch.int32) == pat).all()) and torch.equal(gcoef.view[1].cpu(), row)
    for glat, gin, step in runs:
        glat.assert_intact(f"{what} latents")
        gin.assert_intact(f"{what} model_in")
        assert step.tolist() == [-7, 2, -7], f"{what}: step counter {step.tolist()}"
    glat, gin, _ = runs[0]
    assert _same_bits(glat.view, runs[1][0].view) and _same_bits(gin.view, runs[1][1].view), f"{what}: launch-to-launch difference"
    r, s = L.cfg_ddim_step_ref(geps.view, lat.to(DEV), row, g, cfg, b)
    _note(record, ("cfg_ddim_step", "cfg" if cfg else "nocfg"), L.check(glat.view, r, s, F32), what)
    want_in = glat.view.permute(0, 2, 3, 1).to(BF)
    assert _same_bits(gin.view[:b], want_in), f"{what}: model_in is not bf16(new latents) in NHWC"
    if cfg:
        assert _same_bits(gin.view[b:], want_in), f"{what}: the CFG half of model_in differs"
        assert gin.unwritten() == 0
    else:
        assert gin.unwritten() == b * h * w * c, f"{what}: the second half of a 2B-sized model_in was written"
        assert bool((gin.view[b:].contiguous().view(torch.int16) == E._signed(E.NAN_BITS[BF], BF)).all())


@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "nocfg"])
def test_cfg_unipc_step_large_state_is_bit_identical_with_the_generic_step(ops, cfg):
    """tests/test_gpu_round3.py::test_fused_unipc_step_is_bit_identical_with_the_generic_scheduler_step at the state size that
    enters the second trip of the kernel's grid-stride loop, over a three-step schedule (order warm-up, corrector, lower-order
    final step)."""
    import numpy as np
    from diffcodec_amd.scheduler import UniPCMultistepScheduler
    b, c, h, w = E.STATE_SHAPES[1]
    guidance, n = E.STATE_GUIDANCE, 3
    sg, sf = UniPCMultistepScheduler(), UniPCMultistepScheduler()
    sg.set_timesteps(n)
    sf.set_timesteps(n)
    coef, _ = sf.device_tables(DEV)
    g = torch.Generator().manual_seed(9400)
    x0 = torch.randn(b, c, h, w, generator=g)
    lat_g, lat_f = x0.to(DEV), x0.to(DEV).clone()
    ms = [torch.full((b, c, h, w), float("nan"), device=DEV) for _ in range(3)]        # never read before they are written
    gin = _g(((2 if cfg else 1) * b, h, w, c), BF)
    step = torch.zeros(1, device=DEV, dtype=torch.int32)
    for i, t in enumerate(sg.timesteps.tolist()):
        eps = torch.randn((2 if cfg else 1) * b, h, w, c, generator=g).to(DEV)
        e = eps.permute(0, 3, 1, 2).contiguous()
        if cfg:
            nu, nt = (v.contiguous() for v in e.chunk(2))
            g32 = np.float32(guidance)
            e = ops.lincomb([(float(np.float32(1.0) - g32), nu), (float(g32), nt)])
        lat_g = sg.step(e, t, lat_g, return_dict=False)[0]
        ops.cfg_unipc_step(eps, lat_f, ms[0], ms[1], ms[2], gin.view, coef, step, guidance if cfg else 1.0, cfg)
        assert torch.equal(lat_f, lat_g), i
        assert bool(torch.isfinite(lat_f).all())
        want_in = lat_f.permute(0, 2, 3, 1).to(BF)
        assert torch.equal(gin.view[:b], want_in) and (not cfg or torch.equal(gin.view[b:], want_in))
        gin.assert_intact(f"cfg_unipc_step model_in, step {i}")
    assert int(step.item()) == n


@pytest.mark.parametrize("mul", [1.0, 1.0 / 0.18215], ids=["mul1", "unscale"])
@pytest.mark.parametrize("rep", [1, 2])
@pytest.mark.parametrize("shape", E.STATE_SHAPES, ids=_SHAPE_IDS)
def test_latents_to_model_input_edge(ops, record, shape, rep, mul):
    b, c, h, w = shape
    lat = torch.randn(shape, generator=torch.Generator().manual_seed(9500 + rep))
    glat = _g(shape, F32, lat.to(DEV))
    outs = []
    for k in range(2):
        go = _g((rep * b, h, w, c), BF)
        assert ops.latents_to_model_input(glat.view, mul, rep, out=go.view) is go.view
        torch.cuda.synchronize()
        outs.append(go)
    what = f"latents_to_model_input {shape} rep={rep} mul={mul:.4f}"
    for g in [glat] + outs:
        g.assert_intact(what)
    assert torch.equal(glat.view.cpu(), lat)
    assert outs[0].unwritten() == 0 and _same_bits(outs[0].view, outs[1].view)
    if rep == 2:
        assert _same_bits(outs[0].view[:b], outs[0].view[b:]), f"{what}: the two copies differ"
    r, s = L.latents_to_model_input_ref(glat.view, mul, rep)
    _note(record, ("latents_to_model_input",), L.check(outs[0].view, r, s, BF), what)


@pytest.mark.parametrize("scale", [0.18215, 1.0])
@pytest.mark.parametrize("shape", E.STATE_SHAPES, ids=_SHAPE_IDS)
def test_vae_sample_latents_edge(ops, record, shape, scale):
    from diffcodec_amd import lib
    n, c, h, w = shape
    mom, noise = E.vae_inputs(shape, 9600)
    gm, gz = _g(tuple(mom.shape), F32, mom.to(DEV)), _g(shape, F32, noise.to(DEV))
    outs = []
    for k in range(2):
        go = _g(shape, F32)
        lib.call("dc_vae_sample_latents", gm.view.data_ptr(), gz.view.data_ptr(), go.view.data_ptr(), float(scale), n, c, h, w,
                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append(go)
    what = f"vae_sample_latents {shape} scale={scale}"
    for g in [gm, gz] + outs:
        g.assert_intact(what)
    assert outs[0].unwritten() == 0 and bool(torch.isfinite(outs[0].view).all()) and _same_bits(outs[0].view, outs[1].view)
    r, s = L.vae_sample_latents_ref(gm.view, gz.view, scale)
    _note(record, ("vae_sample_latents",), L.check(outs[0].view, r, s, F32), what)
    assert torch.equal(ops.vae_sample_latents(gm.view, gz.view, scale), outs[0].view)      # the wrapper launches the same


# ------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("family", ["random", "flat", "peaked"])
@pytest.mark.parametrize("i", range(len(E.ATTN_CASES)), ids=[c.label() for c in E.ATTN_CASES])
def test_attention_edge(ops, record, i, family):
    from diffcodec_amd import lib
    c = E.ATTN_CASES[i]
    b, heads, nq, nk, d = c.b, c.heads, c.nq, c.nk, c.d
    assert E.attention_key(b, heads, nq, nk, d) == c.key, c.label()
    gen = torch.Generator().manual_seed(2000 + i)
    ch = heads * d
    q, k, v = E.attention_inputs(family, b, heads, nq, nk, d, gen)
    # strided views with a poisoned column gap (Q: pitch C + 16, K / V: slices of one fused [K | gap | V | gap] row)
    gq = _g((b, nq, ch), BF, q.to(DEV), pitch=ch + 16)
    kv = E.Guarded((b, nk, 2 * ch + 16), BF, DEV)
    kvv = kv.view
    kvv[..., :ch] = k.to(DEV).to(BF)
    kvv[..., ch + 8:2 * ch + 8] = v.to(DEV).to(BF)
    kview, vview = kvv[..., :ch], kvv[..., ch + 8:2 * ch + 8]
    outs = []
    for rep in range(2):
        go = _g((b, nq, ch), BF, pitch=ch + 8)
        lib.call("dc_attention_bf16", gq.view.data_ptr(), kview.data_ptr(), vview.data_ptr(), go.view.data_ptr(), b, heads, nq, nk, d,
                 gq.pitch, kv.pitch, kv.pitch, go.pitch, float(d ** -0.5), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append(go)
    gq.assert_intact(f"{c.label()} q")
    # K / V: the gaps between the slices and after V must hold the pattern (the fused row itself was fully written)
    bits = kvv.contiguous().view(torch.int16)
    pat = E._signed(E.NAN_BITS[BF], BF)
    assert bool((bits[..., ch:ch + 8] == pat).all()) and bool((bits[..., 2 * ch + 8:] == pat).all()), f"{c.label()}: K/V gap written"
    kv.assert_intact(f"{c.label()} kv")
    for go in outs:
        go.assert_intact(f"{c.label()} out")
        assert go.unwritten() == 0, f"{c.label()}: {go.unwritten()} output elements never written"
        assert bool(torch.isfinite(go.view).all()), f"{c.label()} {family}: non-finite output (a poisoned operand element was read)"
    assert _same_bits(outs[0].view, outs[1].view), f"{c.label()} {family}: launch-to-launch difference"
    rows = L.sample_rows(b * nq) if b * nq > 4096 else torch.arange(b * nq)
    r, s = L.attention_ref(gq.view, kview, vview, heads, rows)
    y = outs[0].view.reshape(b * nq, ch)[rows.to(DEV)]
    _note(record, c.key + (family,), L.check(y, r, s, BF), f"{c.label()} {family}")


@pytest.mark.parametrize("t", [1, 77, 128])
def test_attention_causal_small_edge(ops, record, t):
    from diffcodec_amd import lib
    gen = torch.Generator().manual_seed(3000 + t)
    b, heads, d = 3, 12, 64
    ch = heads * d
    gq, gk, gv = (_g((b, t, ch), BF, torch.randn(b, t, ch, generator=gen).to(DEV), pitch=ch + 8) for _ in range(3))
    outs = []
    for rep in range(2):
        go = _g((b, t, ch), BF, pitch=ch + 16)
        lib.call("dc_attention_causal_small_bf16", gq.view.data_ptr(), gk.view.data_ptr(), gv.view.data_ptr(), go.view.data_ptr(), b,
                 heads, t, d, gq.pitch, gk.pitch, gv.pitch, go.pitch, float(d ** -0.5), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append(go)
    for g in (gq, gk, gv) + tuple(outs):
        g.assert_intact(f"causal T={t}")
    assert outs[0].unwritten() == 0
    assert _same_bits(outs[0].view, outs[1].view)
    rows = torch.arange(b * t)
    r, s = L.attention_ref(gq.view, gk.view, gv.view, heads, rows, causal=True)
    _note(record, ("attention_causal_small", t), L.check(outs[0].view.reshape(b * t, ch), r, s, BF), f"causal T={t}")


# ------------------------------------------------------------------------------------------ normalisation
@pytest.mark.parametrize("case", E.GN_CASES)
@pytest.mark.parametrize("direct", [False, True])
def test_group_norm_edge(ops, record, case, direct):
    from diffcodec_amd import lib
    n, h, w, c1, c2, groups = case
    gen = torch.Generator().manual_seed(4000 + n * h * w + c1 + c2)
    x1 = _g((n, h, w, c1), BF, (2 * torch.randn(n, h, w, c1, generator=gen) + 0.5).to(DEV))
    x2 = _g((n, h, w, c2), BF, torch.randn(n, h, w, c2, generator=gen).to(DEV)) if c2 else None
    c = c1 + c2
    gamma = _g((c,), F32, (1 + 0.1 * torch.randn(c, generator=gen)).to(DEV))
    beta = _g((c,), F32, (0.1 * torch.randn(c, generator=gen)).to(DEV))
    hw = h * w
    st = torch.cuda.current_stream().cuda_stream
    x2p = 0 if x2 is None else x2.view.data_ptr()
    guards = [x1, gamma, beta] + ([x2] if x2 is not None else [])
    abs_ = []
    for rep in range(2):          # the two paths of ops.group_norm_ab (GN_DIRECT_MAX_PIXELS), each into guarded outputs
        gab = _g((n, c, 2), F32)
        if direct:
            lib.call("dc_gn_direct_nhwc_bf16", x1.view.data_ptr(), c1, x2p, c2, gamma.view.data_ptr(), beta.view.data_ptr(),
                     gab.view.data_ptr(), n, hw, groups, 1e-5, st)
        else:
            parts = []
            for t, ct in ((x1, c1), (x2, c2)):
                if t is None:
                    parts.append((0, 0))
                    continue
                ch = lib.load().dc_gn_stats_chunks(hw, ct)
                gp = _g((ch, n, ct, 2), F32)
                lib.call("dc_gn_stats_nhwc_bf16", t.view.data_ptr(), gp.view.data_ptr(), n, hw, ct, st)
                guards.append(gp)
                parts.append((gp.view.data_ptr(), ch))
            lib.call("dc_gn_finalize", parts[0][0], c1, parts[0][1], parts[1][0], c2, parts[1][1], gamma.view.data_ptr(),
                     beta.view.data_ptr(), gab.view.data_ptr(), n, groups, hw, 1e-5, st)
        torch.cuda.synchronize()
        abs_.append(gab)
    for g in guards + abs_:
        g.assert_intact(f"group_norm_ab {case}")
    assert abs_[0].unwritten() == 0 and _same_bits(abs_[0].view, abs_[1].view)
    ab = abs_[0].view
    ref, st_ = L.group_norm_ab_ref(x1.view, gamma.view, beta.view, groups, 1e-5, x2=None if x2 is None else x2.view)
    what = f"group_norm_ab {case} {'direct' if direct else 'chunked'}"
    _note(record, ("group_norm_ab", "direct" if direct else "chunked"), L.check_group_norm_ab(ab, ref, st_), what)
    # gn_apply (+ SiLU) of the same tensors into a guarded output
    abg = _g((n, c, 2), F32, ab)
    outs = []
    for rep in range(2):
        go = _g((n, h, w, c), BF)
        lib.call("dc_gn_apply_nhwc_bf16", x1.view.data_ptr(), c1, 0 if x2 is None else x2.view.data_ptr(), c2, abg.view.data_ptr(),
                 go.view.data_ptr(), n, hw, 1, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append(go)
    for g in [x1, gamma, beta, abg] + ([x2] if x2 is not None else []) + outs:
        g.assert_intact(what)
    assert outs[0].unwritten() == 0 and _same_bits(outs[0].view, outs[1].view)
    rows = torch.arange(n * hw)
    r, s = L.gn_apply_ref(x1.view, abg.view, rows, silu=True, x2=None if x2 is None else x2.view)
    _note(record, ("gn_apply",), L.check(outs[0].view.reshape(n * hw, c), r, s, BF), f"gn_apply {case}")


@pytest.mark.parametrize("m,c", E.LN_CASES)
def test_layer_norm_edge(ops, record, m, c):
    from diffcodec_amd import lib
    gen = torch.Generator().manual_seed(5000 + c)
    x = _g((m, c), BF, (torch.randn(m, c, generator=gen) * 2 + 1).to(DEV))
    gamma = _g((c,), F32, (1 + 0.1 * torch.randn(c, generator=gen)).to(DEV))
    beta = _g((c,), F32, (0.1 * torch.randn(c, generator=gen)).to(DEV))
    outs = []
    for rep in range(2):
        go = _g((m, c), BF)
        lib.call("dc_layernorm_bf16", x.view.data_ptr(), gamma.view.data_ptr(), beta.view.data_ptr(), go.view.data_ptr(), m, c, 1e-5,
                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append(go)
    for g in [x, gamma, beta] + outs:
        g.assert_intact(f"layer_norm {m}x{c}")
    assert outs[0].unwritten() == 0 and _same_bits(outs[0].view, outs[1].view)
    r, s = L.layer_norm_ref(x.view, gamma.view, beta.view, 1e-5, torch.arange(m))
    _note(record, ("layer_norm", c), L.check(outs[0].view, r, s, BF), f"layer_norm {m}x{c}")


@pytest.mark.parametrize("m,c", E.ROW_STATS_CASES)
def test_row_stats_edge(ops, record, m, c):
    from diffcodec_amd import lib
    gen = torch.Generator().manual_seed(6000 + c)
    x = _g((m, c), BF, (torch.randn(m, c, generator=gen) + 0.5).to(DEV))
    outs = []
    for rep in range(2):
        go = _g((m, 1, 2), F32)
        lib.call("dc_row_stats_bf16", x.view.data_ptr(), go.view.data_ptr(), m, c, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append(go)
    for g in [x] + outs:
        g.assert_intact(f"row_stats {m}x{c}")
    go = outs[0]
    assert go.unwritten() == 0 and _same_bits(go.view, outs[1].view)
    r, s = L.row_stats_ref(x.view, torch.arange(m))
    _note(record, ("row_stats",), L.check(go.view, r, s, F32), f"row_stats {m}x{c}")


@pytest.mark.parametrize("m,parts,c", E.LN_FINALIZE_CASES)
def test_ln_finalize_edge(ops, record, m, parts, c):
    from diffcodec_amd import lib
    gen = torch.Generator().manual_seed(7000 + parts)
    x = (torch.randn(m, c, generator=gen, dtype=torch.float64) + 0.7)
    bounds = [(p * c) // parts for p in range(parts + 1)]
    pr = torch.stack([torch.stack([x[:, lo:hi].sum(1), (x[:, lo:hi] ** 2).sum(1)], 1) for lo, hi in zip(bounds, bounds[1:])], 1)
    gp = _g((m, parts, 2), F32, pr.float().to(DEV))
    outs = []
    for rep in range(2):
        go = _g((m, 2), F32)
        lib.call("dc_ln_finalize", gp.view.data_ptr(), go.view.data_ptr(), m, parts, c, 1e-5, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append(go)
    for g in [gp] + outs:
        g.assert_intact(f"ln_finalize {m}x{parts}x{c}")
    go = outs[0]
    assert go.unwritten() == 0 and _same_bits(go.view, outs[1].view)
    r, s = L.ln_finalize_ref(gp.view, c, 1e-5, torch.arange(m))
    _note(record, ("ln_finalize",), L.check(go.view, r, s, F32), f"ln_finalize {m}x{parts}x{c}")


@pytest.mark.parametrize("rows,cols", E.SOFTMAX_CASES)
def test_softmax_rows_edge(ops, record, rows, cols):
    from diffcodec_amd import lib
    gen = torch.Generator().manual_seed(8000 + cols)
    sg = _g((rows, cols), F32, (3 * torch.randn(rows, cols, generator=gen)).to(DEV))
    outs = []
    for rep in range(2):
        go = _g((rows, cols), BF)
        lib.call("dc_softmax_rows_f32_to_bf16", sg.view.data_ptr(), go.view.data_ptr(), rows, cols, 0.125,
                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append(go)
    for g in [sg] + outs:
        g.assert_intact(f"softmax_rows {rows}x{cols}")
    assert outs[0].unwritten() == 0 and _same_bits(outs[0].view, outs[1].view)
    r, s = L.softmax_rows_ref(sg.view, 0.125, torch.arange(rows))
    _note(record, ("softmax_rows",), L.check(outs[0].view, r, s, BF), f"softmax_rows {rows}x{cols}")
