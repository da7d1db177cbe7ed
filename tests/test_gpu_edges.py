"""GPU: every case of tests/edge_cases.py — each conv / linear, fp32 extractor conv and attention kernel instance the dispatchers can
reach, the normalisation kernels at their template and chunking edges, the fused loop's state kernels, the control stage (splat,
occlusion mask, flow resize, fusion), the plain elementwise launchers, FDN modulate, the input-side launchers (flow resize from the
.flo layout, the six-channel pack) and the tile blend — launched on guarded operands and outputs, its route asserted first,
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
    if a.dtype == torch.uint8:
        return torch.equal(a, b)
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
    plan = E.case_plan(c)
    assert E.conv_key(plan.desc) == c.key, c.label()
    ho, wo, m = c.ho, c.wo, c.m
    cout_eff = c.cout // 2 if c.geglu else c.cout
    pc, guards, x1, kw = E.conv_operands(ops, c, i, DEV)
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
    for d in seen:                              # the plan and the launch cannot part: every field, and which pointers are set
        assert E.desc_fields(d) == E.desc_fields(plan.desc), (c.label(), E.desc_fields(d), E.desc_fields(plan.desc))
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


@pytest.mark.parametrize("i", E.CONV_SCRATCH_CASES, ids=[E.CONV_CASES[i].label() for i in E.CONV_SCRATCH_CASES])
def test_conv_scratch_of_any_contents(ops, monkeypatch, i):
    """every split-K, finalize-first and GroupNorm-partials case again with the scratch ops.conv allocates (ops._scratch) handed out
    as guarded buffers, holding the NaN pattern and then zeros: guards intact, the output (and the partials) finite, fully written
    and bit for bit those of the unpatched launch"""
    from diffcodec_amd import lib
    c = E.CONV_CASES[i]
    plan = E.case_plan(c)
    cout_eff = c.cout // 2 if c.geglu else c.cout
    pc, guards, x1, kw = E.conv_operands(ops, c, i, DEV)
    handed = []
    fill = [None]
    seen, real, call = _capture(lib)
    monkeypatch.setattr(lib, "call", call)

    def scratch(shape, device, what):
        g = E.Guarded(tuple(shape), F32, DEV)
        if fill[0] == "zeros":
            g.view.zero_()
        handed.append((what, g))
        return g.view

    runs = {}
    for tag in ("plain", "nan", "zeros"):
        fill[0] = tag
        if tag != "plain":
            monkeypatch.setattr(ops, "_scratch", scratch)
        del handed[:]
        og = _g((c.n, c.ho, c.wo, cout_eff), F32 if c.out_f32 else BF)
        sog = _g((c.m, ops.row_stats_parts(c.cout), 2), F32) if c.stats_out else None
        y = ops.conv(x1.view, pc, out=og.view, stats_out=None if sog is None else sog.view, **kw)
        torch.cuda.synchronize()
        what = f"{c.label()} [{tag}]"
        for name, g in list(guards.items()) + [("out", og)] + ([("stats_out", sog)] if sog is not None else []) + handed:
            g.assert_intact(f"{what} {name}")
        assert og.unwritten() == 0 and bool(torch.isfinite(og.view).all()), what
        gp = getattr(y, "gn_part", None)
        if tag != "plain":
            assert [(w, g.shape) for w, g in handed] == plan.scratch and (gp is not None) == ("gn_part" in dict(plan.scratch)), (what, plan.scratch)
            slabs = sum(g.view.numel() * 4 for w, g in handed if w == "splitk")          # what ops.conv sized, against the library's figure
            assert slabs == lib.load().dc_conv_igemm_ws_bytes(seen[-1]), (what, slabs)
            for w, g in handed:
                if w == "gn_part":
                    assert g.unwritten() == 0 and bool(torch.isfinite(g.view).all()), what
        runs[tag] = [og.view] + ([sog.view] if sog is not None else []) + ([gp] if gp is not None else [])
    for tag in ("nan", "zeros"):
        assert len(runs[tag]) == len(runs["plain"]), (c.label(), tag)
        for k, (a, b) in enumerate(zip(runs["plain"], runs[tag])):
            assert _same_bits(a, b), f"{c.label()}: result {k} with the scratch holding '{tag}' differs from the plain launch"


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


# ------------------------------------------------------------------------------------------ control stage
def _st():
    return torch.cuda.current_stream().cuda_stream


def _twice(launch, shape, dtype, operands, what):
    """two launches into two guarded outputs: guards intact, every element written, bitwise equal -> the first output's Guarded"""
    outs = []
    for rep in range(2):
        go = _g(shape, dtype)
        launch(go.view)
        torch.cuda.synchronize()
        outs.append(go)
    for k, g in enumerate(list(operands) + outs):
        g.assert_intact(f"{what} buffer {k}")
    if dtype != torch.uint8:
        assert outs[0].unwritten() == 0, f"{what}: {outs[0].unwritten()} output elements never written"
    assert _same_bits(outs[0].view, outs[1].view), f"{what}: launch-to-launch difference"
    return outs[0]


def _unchanged(g, t, what):
    assert _same_bits(g.view, t.to(DEV)), f"{what}: an operand was written"


def _splat_ws(lib, n, h, w):
    """the workspace as a guarded buffer of exactly dc_splat_ws_bytes, interior zeroed (never the NaN pattern: an unwritten entry read
    as an index must not become an out-of-range access)"""
    nbytes = int(lib.load().dc_splat_ws_bytes(n, h, w))
    assert nbytes > 0 and nbytes % 4 == 0
    ws = E.Guarded((nbytes,), torch.uint8, DEV)
    ws.view.zero_()
    return ws


@pytest.mark.parametrize("i", range(len(E.SPLAT_CASES)), ids=[E.splat_label(c) for c in E.SPLAT_CASES])
def test_splat_soft_edge(ops, record, i):
    """dc_splat_soft_f32 with and without the mask and dc_splat_sum_f32 (splat_sum: bit for bit the C oracle) on guarded operands, a
    guarded workspace of exactly dc_splat_ws_bytes — zeroed for the first launch, left behind by a launch on another flow field
    for the second — and guarded outputs."""
    from diffcodec_amd import lib
    from oracle import splat as OS
    case = E.SPLAT_CASES[i]
    n, c, h, w = case[:4]
    what = E.splat_label(case)
    x, flow, metric, mask = E.splat_inputs(case, E.splat_seed(i))
    other = E.splat_flow("smooth", n, h, w, torch.Generator().manual_seed(77 + i))
    gx, gf, gm, gk, gother = (_g(tuple(t.shape), F32, t.to(DEV)) for t in (x, flow, metric, mask, other))
    ws = _splat_ws(lib, n, h, w)
    ops_ = [gx, gf, gm, gk, gother, ws]

    def soft(out, mk, fl=gf):
        lib.call("dc_splat_soft_f32", gx.view.data_ptr(), fl.view.data_ptr(), gm.view.data_ptr(), mk.view.data_ptr() if mk else 0,
                 out.data_ptr(), ws.view.data_ptr(), n, c, h, w, _st())

    outs = []
    for rep in range(2):
        go = _g((n, c, h, w), F32)
        soft(go.view, gk)
        torch.cuda.synchronize()
        outs.append(go)
        if rep == 0:                                    # leave the workspace as a launch on another flow field leaves it
            scratch = _g((n, c, h, w), F32)
            soft(scratch.view, None, gother)
            torch.cuda.synchronize()
            scratch.assert_intact(f"{what} scratch out")
    gnm = _g((n, c, h, w), F32)
    soft(gnm.view, None)
    gsum = _g((n, c, h, w), F32)
    lib.call("dc_splat_sum_f32", gx.view.data_ptr(), gf.view.data_ptr(), gsum.view.data_ptr(), ws.view.data_ptr(), n, c, h, w, _st())
    torch.cuda.synchronize()
    for k, g in enumerate(ops_ + outs + [gnm, gsum]):
        g.assert_intact(f"{what} buffer {k}")
    for g, t in ((gx, x), (gf, flow), (gm, metric), (gk, mask)):
        _unchanged(g, t, what)
    for g in outs + [gnm, gsum]:
        assert g.unwritten() == 0, f"{what}: {g.unwritten()} output elements never written"
        assert bool(torch.isfinite(g.view).all()), f"{what}: non-finite output"
    assert _same_bits(outs[0].view, outs[1].view), f"{what}: the output depends on what the workspace held"
    r, s, _ = L.splat_soft_ref(gx.view, gf.view, gm.view, gk.view)
    _note(record, ("splat_soft", "mask"), L.check(outs[0].view, r, s, F32), what)
    r, s, _ = L.splat_soft_ref(gx.view, gf.view, gm.view)
    _note(record, ("splat_soft",), L.check(gnm.view, r, s, F32), what)
    r, s, _ = L.splat_sum_ref(gx.view, gf.view)
    _note(record, ("splat_sum",), L.check(gsum.view, r, s, F32), what)
    assert torch.equal(gsum.view.cpu(), OS.splat_sum(x, flow)), f"{what}: splat_sum is not bit for bit the C oracle"


@pytest.mark.parametrize("case", E.OCCLUSION_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in E.OCCLUSION_CASES])
def test_occlusion_mask_edge(ops, record, case):
    from diffcodec_amd import lib
    n, h, w, _ = case
    what = f"occlusion_mask {n}x{h}x{w}"
    fa, fb = E.occlusion_inputs(case)
    other = E.splat_flow("smooth", n, h, w, torch.Generator().manual_seed(5))
    ga, gb, gother = (_g(tuple(t.shape), F32, t.to(DEV)) for t in (fa, fb, other))
    ws = _splat_ws(lib, n, h, w)

    def launch(out, b=gb):
        lib.call("dc_occlusion_mask_f32", ga.view.data_ptr(), b.view.data_ptr(), out.data_ptr(), ws.view.data_ptr(), n, h, w, _st())

    outs = []
    for rep in range(2):
        go = _g((n, 1, h, w), F32)
        launch(go.view)
        torch.cuda.synchronize()
        outs.append(go)
        if rep == 0:
            scratch = _g((n, 1, h, w), F32)
            launch(scratch.view, gother)
            torch.cuda.synchronize()
            scratch.assert_intact(f"{what} scratch out")
    for k, g in enumerate([ga, gb, gother, ws] + outs):
        g.assert_intact(f"{what} buffer {k}")
    _unchanged(ga, fa, what)
    _unchanged(gb, fb, what)
    assert outs[0].unwritten() == 0 and _same_bits(outs[0].view, outs[1].view), what
    v = L.check_occlusion_mask(outs[0].view, L.occlusion_mask_ref(ga.view, gb.view))
    record("edge[occlusion_mask]", f"{what} band_share={v['band']:.5f} flips_outside={v['flips']} ones={v['ones']:.3f}")
    assert v["ok"], (what, v)


def _flow_cases():
    return [(c, False) for c in E.FLOW_RESIZE_CASES] + [(c, True) for c in E.FLOW_RESIZE_CASES + E.FLOW_RESIZE_DIVIDE_ONLY]


@pytest.mark.parametrize("case,divide", _flow_cases(), ids=[("divide-" if d else "normalize-") + "x".join(map(str, c)) for c, d in _flow_cases()])
def test_flow_resize_edge(ops, record, case, divide):
    """dc_flow_resize_normalize_f32 / dc_flow_resize_divide_f32 reading planes 2:4 of a guarded [n, 6, H, W] tensor whose other planes
    hold the NaN pattern"""
    from diffcodec_amd import lib
    n, hh, ww, h, w = case
    name = "flow_resize_divide" if divide else "flow_resize_normalize"
    what = f"{name} {case}"
    full = E.flow_resize_input(case, 0)
    g6 = E.Guarded((n, 6, hh, ww), F32, DEV)
    src = g6.view[:, 2:4]
    src.copy_(full[:, 2:4].to(DEV))
    dx, dy = E.FLOW_DIVISORS if divide else ((w - 1) / 2.0, (h - 1) / 2.0)

    def launch(out):
        if divide:
            lib.call("dc_flow_resize_divide_f32", src.data_ptr(), src.stride(0), out.data_ptr(), n, hh, ww, h, w, dx, dy, _st())
        else:
            lib.call("dc_flow_resize_normalize_f32", src.data_ptr(), src.stride(0), out.data_ptr(), n, hh, ww, h, w, _st())

    go = _twice(launch, (n, 2, h, w), F32, [g6], what)
    pat = E._signed(E.NAN_BITS[F32], F32)
    assert bool((g6.view[:, [0, 1, 4, 5]].contiguous().view(torch.int32) == pat).all()), f"{what}: a neighbouring plane was written"
    assert torch.equal(src.cpu(), full[:, 2:4]), f"{what}: the source was written"
    assert bool(torch.isfinite(go.view).all()), f"{what}: non-finite output (a poisoned plane was read)"
    r, s = L.flow_resize_ref(src, h, w, dx, dy)
    _note(record, (name,), L.check(go.view, r, s, F32), what)
    wrapped = ops.flow_resize_divide(src, h, w, dx, dy) if divide else ops.flow_resize_normalize(src, h, w)
    assert torch.equal(wrapped, go.view), f"{what}: the ops wrapper launches something else"


@pytest.mark.parametrize("occ", [True, False], ids=["holes", "noholes"])
@pytest.mark.parametrize("i", range(len(E.FUSE_CASES)), ids=["x".join(map(str, c)) for c in E.FUSE_CASES])
def test_fuse_warped_edge(ops, record, i, occ):
    from diffcodec_amd import lib
    n, c, h, w = E.FUSE_CASES[i]
    what = f"fuse_warped {E.FUSE_CASES[i]} occ={int(occ)}"
    ts = E.fuse_inputs(E.FUSE_CASES[i], i)
    gs = [_g(tuple(t.shape), F32, t.to(DEV)) for t in ts]
    p = [g.view.data_ptr() for g in gs]

    def launch(out):
        lib.call("dc_fuse_warped_f32", p[0], p[1], p[2], p[3], p[4] if occ else 0, p[5] if occ else 0, out.data_ptr(), n, c, h, w, _st())

    go = _twice(launch, (n, c, h, w), F32, gs, what)
    for g, t in zip(gs, ts):
        _unchanged(g, t, what)
    assert bool(torch.isfinite(go.view).all()), what
    r, s = L.fuse_warped_ref(*(g.view for g in gs[:4]), *((gs[4].view, gs[5].view) if occ else ()))
    _note(record, ("fuse_warped", "holes" if occ else "noholes"), L.check(go.view, r, s, F32), what)
    assert torch.equal(ops.fuse_warped(*(g.view for g in gs[:4]), *((gs[4].view, gs[5].view) if occ else ())), go.view)


# ------------------------------------------------------------------------------------------ plain elementwise launchers
@pytest.mark.parametrize("n", E.ELEMENTWISE_CASES["silu_f32"])
def test_silu_f32_edge(ops, record, n):
    from diffcodec_amd import lib
    x = E.elementwise_input(n, n, E.SILU_SPECIALS)
    gx = _g((n,), F32, x.to(DEV))
    go = _twice(lambda o: lib.call("dc_silu_f32", gx.view.data_ptr(), o.data_ptr(), n, _st()), (n,), F32, [gx], f"silu_f32 {n}")
    _unchanged(gx, x, "silu_f32")
    assert bool(torch.isfinite(go.view).all()), f"silu_f32 {n}: non-finite output"
    r, s = L.silu_f32_ref(gx.view)
    _note(record, ("silu_f32",), L.check(go.view, r, s, F32), f"silu_f32 {n}")
    assert torch.equal(ops.silu_f32(gx.view), go.view)


@pytest.mark.parametrize("n", E.ELEMENTWISE_CASES["add_f32"])
def test_add_f32_edge(ops, record, n):
    from diffcodec_amd import lib
    a, b = E.elementwise_input(n, 1), E.elementwise_input(n, 2)
    ga, gb = _g((n,), F32, a.to(DEV)), _g((n,), F32, b.to(DEV))
    go = _twice(lambda o: lib.call("dc_add_f32", ga.view.data_ptr(), gb.view.data_ptr(), o.data_ptr(), n, _st()), (n,), F32, [ga, gb],
                f"add_f32 {n}")
    r, s = L.add_f32_ref(ga.view, gb.view)
    _note(record, ("add_f32",), L.check(go.view, r, s, F32), f"add_f32 {n}")
    assert torch.equal(go.view, ga.view + gb.view)                      # one IEEE sum
    assert torch.equal(ops.add_f32(ga.view, gb.view), go.view)


@pytest.mark.parametrize("n,terms", E.ELEMENTWISE_CASES["lincomb"])
def test_lincomb_edge(ops, record, n, terms):
    from diffcodec_amd import lib
    ts = [E.elementwise_input(n, 10 + j) for j in range(terms)]
    gs = [_g((n,), F32, t.to(DEV)) for t in ts]
    p = [g.view.data_ptr() for g in gs] + [0] * (4 - terms)
    cf = list(E.LINCOMB_COEFS[:terms]) + [0.0] * (4 - terms)
    go = _twice(lambda o: lib.call("dc_lincomb4_f32", *p, *cf, o.data_ptr(), n, _st()), (n,), F32, gs, f"lincomb {n}x{terms}")
    r, s = L.lincomb_ref([(cf[j], gs[j].view) for j in range(terms)])
    _note(record, ("lincomb", terms), L.check(go.view, r, s, F32), f"lincomb {n}x{terms}")
    assert torch.equal(ops.lincomb([(cf[j], gs[j].view) for j in range(terms)]), go.view)


@pytest.mark.parametrize("n", E.ELEMENTWISE_CASES["f32_to_bf16"])
def test_f32_to_bf16_edge(ops, record, n):
    from diffcodec_amd import lib
    x = E.elementwise_input(n, 3, (1.00390625, 1.01171875, -1.00390625, 3.0e38, 1e-30, -0.0))     # ties to even, both ways; near overflow
    gx = _g((n,), F32, x.to(DEV))
    go = _twice(lambda o: lib.call("dc_f32_to_bf16", gx.view.data_ptr(), o.data_ptr(), n, _st()), (n,), BF, [gx], f"f32_to_bf16 {n}")
    assert _same_bits(go.view, gx.view.to(BF)), f"f32_to_bf16 {n}: not one round-to-nearest-even"
    r, s = L.f32_to_bf16_ref(gx.view[:, None], torch.arange(n))
    _note(record, ("f32_to_bf16",), L.check(go.view[:, None], r, s, BF), f"f32_to_bf16 {n}")


@pytest.mark.parametrize("n", E.ELEMENTWISE_CASES["add_bf16"])
def test_add_bf16_edge(ops, record, n):
    from diffcodec_amd import lib
    a, b = E.elementwise_input(n, 4).to(BF), E.elementwise_input(n, 5).to(BF)
    ga, gb = _g((n,), BF, a.to(DEV)), _g((n,), BF, b.to(DEV))
    go = _twice(lambda o: lib.call("dc_add_bf16", ga.view.data_ptr(), gb.view.data_ptr(), o.data_ptr(), n, _st()), (n,), BF, [ga, gb],
                f"add_bf16 {n}")
    assert _same_bits(go.view, (ga.view.float() + gb.view.float()).to(BF)), f"add_bf16 {n}: not the fp32 sum rounded once"
    r, s = L.add_ref(ga.view.reshape(-1, 8), gb.view.reshape(-1, 8), torch.arange(n // 8))
    _note(record, ("add_bf16",), L.check(go.view.reshape(-1, 8), r, s, BF), f"add_bf16 {n}")


@pytest.mark.parametrize("name", ["nchw_f32_to_nhwc_bf16", "nhwc_bf16_to_nchw_f32", "nhwc_f32_to_nchw_f32"])
@pytest.mark.parametrize("shape", E.ELEMENTWISE_CASES["nchw_f32_to_nhwc_bf16"], ids=lambda s: "x".join(map(str, s)))
def test_layout_conversion_edge(ops, record, name, shape):
    """nchw_f32_to_nhwc_bf16 / nhwc_bf16_to_nchw_f32 / nhwc_f32_to_nchw_f32: exact (a permutation, at most one rounding to bf16)"""
    from diffcodec_amd import lib
    assert shape in E.ELEMENTWISE_CASES[name]
    n, c, h, w = shape
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(17000 + c))
    if name == "nchw_f32_to_nhwc_bf16":
        gx, oshape, odt = _g(shape, F32, x.to(DEV)), (n, h, w, c), BF
        want = L.nchw_f32_to_nhwc_bf16_ref(gx.view)
    else:
        idt = BF if name == "nhwc_bf16_to_nchw_f32" else F32
        gx, oshape, odt = _g((n, h, w, c), idt, x.permute(0, 2, 3, 1).to(DEV)), shape, F32
        want = L.nhwc_to_nchw_f32_ref(gx.view)
    args = lambda o: (gx.view.data_ptr(), o.data_ptr(), n, c, h, w, _st())
    launch = {"nchw_f32_to_nhwc_bf16": lambda o: lib.call("dc_nchw_f32_to_nhwc_bf16", *args(o)),
              "nhwc_bf16_to_nchw_f32": lambda o: lib.call("dc_nhwc_bf16_to_nchw_f32", *args(o)),
              "nhwc_f32_to_nchw_f32": lambda o: lib.call("dc_nhwc_f32_to_nchw_f32", *args(o))}[name]
    go = _twice(launch, oshape, odt, [gx], f"{name} {shape}")
    assert _same_bits(go.view, want.contiguous()), f"{name} {shape}: not the exact permutation"
    assert _same_bits(getattr(ops, name)(gx.view), go.view)
    record(f"edge[{name}]", "exact")


@pytest.mark.parametrize("shape", E.ELEMENTWISE_CASES["transpose_bf16"], ids=lambda s: "x".join(map(str, s)))
def test_transpose_bf16_edge(ops, record, shape):
    from diffcodec_amd import lib
    b, r, c = shape
    x = torch.randn(b, r, c, generator=torch.Generator().manual_seed(18000 + r))
    gx = _g(shape, BF, x.to(DEV))
    go = _twice(lambda o: lib.call("dc_transpose_bf16", gx.view.data_ptr(), o.data_ptr(), b, r, c, _st()), (b, c, r), BF, [gx],
                f"transpose_bf16 {shape}")
    assert _same_bits(go.view, gx.view.transpose(1, 2).contiguous()), f"transpose_bf16 {shape}"
    record("edge[transpose_bf16]", "exact")


@pytest.mark.parametrize("shape", E.ELEMENTWISE_CASES["freeu_lowfreq"], ids=lambda s: "x".join(map(str, s)))
def test_freeu_lowfreq_edge(ops, record, shape):
    from diffcodec_amd import lib
    n, h, w, c = shape
    x = torch.randn(shape, generator=torch.Generator().manual_seed(19000 + w)) + 0.4
    gx = _g(shape, BF, x.to(DEV))
    go = _twice(lambda o: lib.call("dc_freeu_lowfreq_nhwc_bf16", gx.view.data_ptr(), o.data_ptr(), n, h, w, c, 0.2, _st()), shape, BF, [gx],
                f"freeu_lowfreq {shape}")
    rows = torch.arange(n * h * w)
    r, s = L.freeu_lowfreq_ref(gx.view, 0.2, rows)
    _note(record, ("freeu_lowfreq",), L.check(go.view.reshape(-1, c), r, s, BF), f"freeu_lowfreq {shape}")


@pytest.mark.parametrize("shape", E.ELEMENTWISE_CASES["freeu_backbone"], ids=lambda s: "x".join(map(str, s)))
def test_freeu_backbone_edge(ops, record, shape):
    from diffcodec_amd import lib
    n, px, c = shape
    x = torch.randn(shape, generator=torch.Generator().manual_seed(20000 + c))
    gx = _g(shape, BF, x.to(DEV))
    go = _twice(lambda o: lib.call("dc_freeu_backbone_nhwc_bf16", gx.view.data_ptr(), o.data_ptr(), n * px, c, 1.4, _st()), shape, BF, [gx],
                f"freeu_backbone {shape}")
    r, s = L.freeu_backbone_ref(gx.view, 1.4, torch.arange(n * px))
    _note(record, ("freeu_backbone",), L.check(go.view.reshape(-1, c), r, s, BF), f"freeu_backbone {shape}")
    assert _same_bits(go.view[..., c // 2:], gx.view[..., c // 2:]), "freeu_backbone: the second half of the channels moved"


@pytest.mark.parametrize("n,dim,step", E.ELEMENTWISE_CASES["timestep_embedding"])
def test_timestep_embedding_edge(ops, record, n, dim, step):
    """a device step index into a four-entry timestep table"""
    from diffcodec_amd import lib
    gt = _g((4,), F32, torch.tensor(E.TIMESTEP_TABLE).to(DEV))
    st = torch.tensor([-1, step, -1], dtype=torch.int32, device=DEV)
    go = _twice(lambda o: lib.call("dc_timestep_embedding_f32", gt.view.data_ptr(), st[1:2].data_ptr(), o.data_ptr(), n, dim, _st()),
                (n, dim), F32, [gt], f"timestep_embedding {n}x{dim}")
    assert st.tolist() == [-1, step, -1]
    r, s = L.timestep_embedding_ref(E.TIMESTEP_TABLE[step], n, dim)
    _note(record, ("timestep_embedding",), L.check(go.view, r.to(DEV), s.to(DEV), F32), f"timestep_embedding {n}x{dim} step {step}")


@pytest.mark.parametrize("b,t,c,vocab", E.ELEMENTWISE_CASES["embed_tokens"])
def test_embed_tokens_edge(ops, record, b, t, c, vocab):
    """ids in range only (0 and vocab - 1 among them): the fp32 sum of two bf16 rows, rounded once"""
    from diffcodec_amd import lib
    gen = torch.Generator().manual_seed(21000 + c)
    ids = torch.randint(0, vocab, (b, t), generator=gen)
    ids[0, 0], ids[-1, -1] = 0, vocab - 1
    assert int(ids.min()) == 0 and int(ids.max()) == vocab - 1
    gtok, gpos = _g((vocab, c), BF, torch.randn(vocab, c, generator=gen).to(DEV)), _g((t, c), BF, torch.randn(t, c, generator=gen).to(DEV))
    ids_d = ids.to(DEV)
    go = _twice(lambda o: lib.call("dc_embed_tokens_bf16", ids_d.data_ptr(), gtok.view.data_ptr(), gpos.view.data_ptr(), o.data_ptr(), b, t,
                                   c, vocab, _st()), (b, t, c), BF, [gtok, gpos], f"embed_tokens {(b, t, c, vocab)}")
    assert torch.equal(ids_d.cpu(), ids)
    assert _same_bits(go.view, L.embed_tokens_ref(ids_d, gtok.view, gpos.view)), "embed_tokens: not the fp32 sum rounded once"
    assert _same_bits(ops.embed_tokens(ids_d, gtok.view, gpos.view), go.view)
    record("edge[embed_tokens]", "exact")


@pytest.mark.parametrize("n,c,h,w,xs,f32,u8", E.ELEMENTWISE_CASES["postprocess_image"])
def test_postprocess_image_edge(ops, record, n, c, h, w, xs, f32, u8):
    """dc_postprocess_image on a contiguous input and on a pixel-stride-4 view whose fourth channel holds the NaN pattern; fp32 only,
    uint8 only and both.  The guarded fp32 output of the launch itself is held to the fp64 reference.  The uint8 image must be
    round-half-even(255 o32) exactly, o32 being the guarded fp32 output of the same launch — or, in the uint8-only case, which writes
    no fp32 output, that of a separate fp32 launch on the same input (`own32`; where both exist they must agree bit for bit)."""
    from diffcodec_amd import lib
    what = f"postprocess_image xs={xs} f32={int(f32)} u8={int(u8)}"
    x = E.postprocess_input(n, c, h, w, xs)
    gx = E.Guarded((n, h, w, xs), F32, DEV)
    xv = gx.view[..., :c]
    xv.copy_(x[..., :c].to(DEV))
    own32, _ = ops.postprocess_image(xv, want_u8=False)
    runs = []
    for rep in range(2):
        g32 = _g((n, c, h, w), F32) if f32 else None
        g8 = _g((n, h, w, c), torch.uint8) if u8 else None
        lib.call("dc_postprocess_image", xv.data_ptr(), g32.view.data_ptr() if f32 else 0, g8.view.data_ptr() if u8 else 0, n, c, h, w, xs, _st())
        torch.cuda.synchronize()
        runs.append((g32, g8))
    gx.assert_intact(f"{what} x")
    assert torch.equal(xv.cpu(), x[..., :c]), f"{what}: the input was written"
    if xs > c:
        assert bool((gx.view[..., c:].contiguous().view(torch.int32) == E._signed(E.NAN_BITS[F32], F32)).all())
    r, s = L.postprocess_image_ref(xv)
    for g32, g8 in runs:
        if g32 is not None:
            g32.assert_intact(f"{what} o32")
            assert g32.unwritten() == 0 and _same_bits(g32.view, runs[0][0].view) and _same_bits(g32.view, own32)
        o32 = own32 if g32 is None else g32.view
        if g8 is not None:
            g8.assert_intact(f"{what} o8")
            assert torch.equal(g8.view, torch.round(o32 * 255.0).to(torch.uint8).permute(0, 2, 3, 1)), f"{what}: uint8 image"
    o32 = runs[0][0].view if f32 else own32
    _note(record, ("postprocess_image",), L.check(o32, r, s, F32), what)
    assert float(o32.min()) == 0.0 and float(o32.max()) == 1.0


# ------------------------------------------------------------------------------------------ FDN modulate, input side, tile blend
@pytest.mark.parametrize("i", range(len(E.FDN_CASES)), ids=["x".join(map(str, c)) for c in E.FDN_CASES])
def test_fdn_modulate_edge(ops, record, i):
    """dc_fdn_modulate_nhwc_bf16: one vector, C off 64, Bp = N, Bp = 1, and 1,081,344 vectors (past the 4096 x 256 grid cap: sampled
    rows, whose last block lies in the second trip)"""
    from diffcodec_amd import lib
    case = E.FDN_CASES[i]
    n, bp, hw, c = case
    what = f"fdn_modulate {case}"
    x, ab, gam, bet = E.fdn_inputs(case, i)
    gx, gg, gb = (_g(tuple(t.shape), BF, t.to(DEV)) for t in (x, gam, bet))
    gab = _g((n, c, 2), F32, ab.to(DEV))

    def launch(out):
        lib.call("dc_fdn_modulate_nhwc_bf16", gx.view.data_ptr(), gab.view.data_ptr(), gg.view.data_ptr(), gb.view.data_ptr(),
                 out.data_ptr(), n, bp, hw, c, _st())

    go = _twice(launch, (n, hw, c), BF, [gx, gab, gg, gb], what)
    large = n * hw * (c // 8) > E.FDN_VEC_CAP
    rows = L.sample_rows(n * hw) if large else torch.arange(n * hw)
    if large:
        assert int(rows.max()) * (c // 8) >= E.FDN_VEC_CAP                   # rows of the second trip are sampled
    r, s = L.fdn_modulate_ref(gx.view, gab.view, gg.view, gb.view, rows)
    _note(record, ("fdn_modulate",), L.check(go.view.reshape(n * hw, c)[rows.to(DEV)], r, s, BF), what)
    assert torch.equal(ops.fdn_modulate(gx.view, gab.view, gg.view, gb.view), go.view), f"{what}: the ops wrapper launches something else"


@pytest.mark.parametrize("case", E.FLOW_HW2_CASES, ids=lambda c: "x".join(map(str, c)))
def test_flow_hw2_resize_scale_edge(ops, record, case):
    """dc_flow_hw2_resize_scale_f32 on a guarded [H, W, 2] source: a float2 read one pair past the end gives a non-finite output"""
    from diffcodec_amd import lib
    hh, ww, th, tw = case
    what = f"flow_hw2_resize_scale {case}"
    flow = E.flow_hw2_input(case, 0)
    gs = _g((hh, ww, 2), F32, flow.to(DEV))
    go = _twice(lambda o: lib.call("dc_flow_hw2_resize_scale_f32", gs.view.data_ptr(), hh, ww, o.data_ptr(), th, tw, _st()),
                (2, th, tw), F32, [gs], what)
    _unchanged(gs, flow, what)
    assert bool(torch.isfinite(go.view).all()), f"{what}: non-finite output (a guard element was read)"
    r, s = L.flow_hw2_resize_scale_ref(gs.view, th, tw)
    _note(record, ("flow_hw2_resize_scale",), L.check(go.view, r, s, F32), what)
    assert torch.equal(ops.flow_hw2_resize_scale(gs.view, th, tw), go.view), f"{what}: the ops wrapper launches something else"


@pytest.mark.parametrize("case", E.PACK_CASES, ids=lambda c: "x".join(map(str, c)))
def test_pack_sixch_edge(ops, record, case):
    """dc_pack_sixch_u8_f32: bit for bit fp32 x / 255 of every byte value; 1450 x 1450 takes the loop's second trip"""
    from diffcodec_amd import lib
    h, w = case
    what = f"pack_sixch {case}"
    a, b = E.pack_inputs(case)
    if h * w * 3 >= 256:
        assert len(torch.unique(a)) == 256 and len(torch.unique(b)) == 256
    ga, gb = _g((h, w, 3), torch.uint8, a.to(DEV)), _g((h, w, 3), torch.uint8, b.to(DEV))
    go = _twice(lambda o: lib.call("dc_pack_sixch_u8_f32", ga.view.data_ptr(), gb.view.data_ptr(), o.data_ptr(), h, w, _st()),
                (1, 6, h, w), F32, [ga, gb], what)
    _unchanged(ga, a, what)
    _unchanged(gb, b, what)
    ref = torch.cat([a.permute(2, 0, 1).float().div(255.0), b.permute(2, 0, 1).float().div(255.0)], 0).unsqueeze(0)
    wrong = int((go.view.cpu().view(torch.int32) != ref.view(torch.int32)).sum())
    record("edge[pack_sixch]", f"{what} elements_off={wrong}")
    assert wrong == 0, f"{what}: {wrong} elements differ from fp32 x / 255"
    assert torch.equal(ops.pack_sixch(ga.view, gb.view), go.view)


@pytest.mark.parametrize("i", range(len(E.BLEND_CASES)), ids=[c.name for c in E.BLEND_CASES])
def test_blend_tiles_ramp_edge(ops, record, i):
    """dc_blend_tiles_ramp_u8 on guarded tiles and a guarded ramp of exactly `feather` taps: bit for bit tiling.merge_ramp, and within
    0.5 + 1e-3 of the fp64 weighted mean (L.blend_tiles_ramp_ref), so that the host merge is not the only witness"""
    import numpy as np
    from diffcodec_amd import lib, tiling
    c = E.BLEND_CASES[i]
    what = f"blend_tiles_ramp {c.name}"
    tiles = E.blend_inputs(c, i)
    t = len(c.coords)
    assert tuple(tiles.shape) == (t, c.c, c.th, c.tw) and 2 * c.feather <= min(c.th, c.tw)
    gt = _g(tuple(tiles.shape), F32, tiles.to(DEV))
    f = c.feather
    ramp = (0.5 - 0.5 * np.cos(np.pi * (np.arange(f, dtype=np.float32) + 0.5) / f)).astype(np.float32) if f else None
    gr = _g((f,), F32, torch.from_numpy(ramp).to(DEV)) if f else None
    coords = torch.tensor(c.coords, dtype=torch.int32).reshape(-1, 4).to(DEV)

    def launch(out):
        lib.call("dc_blend_tiles_ramp_u8", gt.view.data_ptr(), coords.data_ptr(), t, c.c, c.th, c.tw, gr.view.data_ptr() if f else 0, f,
                 out.data_ptr(), c.h, c.w, float(c.scale), _st())

    go = _twice(launch, (c.h, c.w, c.c), torch.uint8, [gt] + ([gr] if f else []), what)
    _unchanged(gt, tiles, what)
    assert torch.equal(coords.cpu(), torch.tensor(c.coords, dtype=torch.int32).reshape(-1, 4))
    dev = go.view.cpu()
    host = tiling.merge_ramp([np.asarray(x.permute(1, 2, 0).numpy() * np.float32(c.scale), np.float32) for x in tiles], list(c.coords),
                             (c.h, c.w), order="hwc", feather=f)
    off = int((dev != torch.from_numpy(host)).sum())
    mean = L.blend_tiles_ramp_ref(tiles, c.coords, c.h, c.w, f, c.scale)
    dist = float((dev.double() - mean).abs().max())
    record("edge[blend_tiles_ramp]", f"{what} elements_off_host_merge={off} max_distance_from_fp64_mean={dist:.6f}")
    assert off == 0, f"{what}: {off} elements differ from tiling.merge_ramp"
    assert dist <= 0.5 + 1e-3, f"{what}: {dist} from the fp64 weighted mean"
    if c.values == "ties":
        assert bool((dev % 2 == 0).all()) and bool(((mean - mean.floor()) == 0.5).all()), f"{what}: ties must round to even"
    if c.values == "clip":
        assert bool((dev == 0).any()) and bool((dev == 255).any())
    assert torch.equal(ops.blend_tiles_ramp(gt.view, list(c.coords), (c.h, c.w), f, c.scale), go.view)
