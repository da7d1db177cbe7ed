"""GPU: the softsplat drop-in — dc_splat_ingrad_f32, dc_splat_flowgrad_f32 and dc_splat_norm_f32 on guarded buffers against the
yardsticks of tests/splat_grad_ref.py (themselves held by tests/test_splat_grad_ref.py), then diffcodec_amd.softsplat: fused
against composed, mode strings read literally, autocast, needs_input_grad, graph capture, and end-to-end gradients against fp64
autograd."""
import pytest
import torch

import edge_cases as E
import splat_grad_ref as R
from oracle import launch_ref as L
from oracle import splat as OS

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32

# (shape, flow family): the splat edge shapes x every family; C = 161 / 641 at 8x8 (the channel sum split over 16 lanes, C odd);
# C = 19 on a 32x33 map (the 4-lane split of maps of >= 1024 pixels); 1450 x 1450 (past one trip of the grid-stride loops)
GRAD_CASES = [(s, f) for s in E.SPLAT_SHAPES for f in E.FLOW_FAMILIES] + \
             [(s, f) for s in ((2, 161, 8, 8), (1, 641, 8, 8), (2, 19, 32, 33)) for f in ("smooth", "nonfinite")] + \
             [((1, 1, 1450, 1450), "smooth")]
GRAD_IDS = ["x".join(map(str, s)) + "-" + f for s, f in GRAD_CASES]
FUSED_CASES = [(s, f) for s in E.SPLAT_SHAPES for f in E.FLOW_FAMILIES]
FUSED_IDS = GRAD_IDS[:len(FUSED_CASES)]
EPS = ("addeps", "zeroeps", "clipeps")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd import ops as o
    return o


def _st():
    return torch.cuda.current_stream().cuda_stream


def _g(t):
    g = E.Guarded(tuple(t.shape), F32, DEV)
    g.fill(t.to(DEV))
    return g


def _out(shape):
    return E.Guarded(tuple(shape), F32, DEV)


def _ws(lib, n, h, w):
    nbytes = int(lib.load().dc_splat_ws_bytes(n, h, w))
    ws = E.Guarded((nbytes,), torch.uint8, DEV)
    ws.view.zero_()
    return ws


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _inputs(i):
    (n, c, h, w), family = GRAD_CASES[i]
    gen = torch.Generator().manual_seed(24000 + i)
    x = torch.randn(n, c, h, w, generator=gen) + 0.3
    flow = E.splat_flow(family, n, h, w, gen)
    og = torch.randn(n, c, h, w, generator=gen)
    return x, flow, og


def _finish(bufs, outs, what):
    torch.cuda.synchronize()
    for k, g in enumerate(bufs + outs):
        g.assert_intact(f"{what} buffer {k}")
    for k, g in enumerate(outs):
        assert g.unwritten() == 0, f"{what}: output {k} has {g.unwritten()} unwritten elements"


# ------------------------------------------------------------------------------------------ 1. ingrad
@pytest.mark.parametrize("i", range(len(GRAD_CASES)), ids=GRAD_IDS)
def test_ingrad_bit_exact(ops, i):
    from diffcodec_amd import lib
    (n, c, h, w), _ = GRAD_CASES[i]
    _, flow, og = _inputs(i)
    gf, go, out = _g(flow), _g(og), _out(og.shape)
    lib.call("dc_splat_ingrad_f32", gf.view.data_ptr(), go.view.data_ptr(), out.view.data_ptr(), n, c, h, w, _st())
    _finish([gf, go], [out], GRAD_IDS[i])
    assert torch.equal(out.view.cpu(), R.ingrad_f32(flow, og)), f"{GRAD_IDS[i]}: ingrad is not bit for bit the fp32 restatement"


# ------------------------------------------------------------------------------------------ 2. flowgrad
@pytest.mark.parametrize("i", range(len(GRAD_CASES)), ids=GRAD_IDS)
def test_flowgrad(ops, record, i):
    from diffcodec_amd import lib
    (n, c, h, w), _ = GRAD_CASES[i]
    x, flow, og = _inputs(i)
    gx, gf, go = _g(x), _g(flow), _g(og)
    outs = [_out(flow.shape), _out(flow.shape)]
    for o in outs:
        lib.call("dc_splat_flowgrad_f32", gx.view.data_ptr(), gf.view.data_ptr(), go.view.data_ptr(), o.view.data_ptr(), n, c, h, w, _st())
    # the same images at batch 1 and inside a batch of 3 (image 0 at positions 1 and 2, the last image in front)
    pick = [n - 1, 0, 0]
    b3 = [_g(t[pick]) for t in (x, flow, og)]
    b1 = [_g(t[:1]) for t in (x, flow, og)]
    o3, o1 = _out((3, 2, h, w)), _out((1, 2, h, w))
    lib.call("dc_splat_flowgrad_f32", *[g.view.data_ptr() for g in b3], o3.view.data_ptr(), 3, c, h, w, _st())
    lib.call("dc_splat_flowgrad_f32", *[g.view.data_ptr() for g in b1], o1.view.data_ptr(), 1, c, h, w, _st())
    _finish([gx, gf, go] + b3 + b1, outs + [o3, o1], GRAD_IDS[i])
    r, s = R.flowgrad_ref(gx.view, gf.view, go.view)
    res = L.check(outs[0].view, r, s, F32)
    record(f"softsplat[flowgrad {GRAD_IDS[i]}]", f"err_over_tol={res['ratio']:.4f}")
    assert res["ok"], (GRAD_IDS[i], res)
    assert _bits(outs[0].view, outs[1].view), f"{GRAD_IDS[i]}: two launches differ"
    assert _bits(o1.view[0], outs[0].view[0]), f"{GRAD_IDS[i]}: batch 1 differs from the same image in the case's batch"
    assert _bits(o3.view[1], o1.view[0]) and _bits(o3.view[2], o1.view[0]), f"{GRAD_IDS[i]}: batch of 3 differs from batch 1"
    assert _bits(o3.view[0], outs[0].view[n - 1])


# ------------------------------------------------------------------------------------------ 3. fused modes
def _fused_metrics(i):
    (n, c, h, w), _ = FUSED_CASES[i]
    return {fam: R.metric_family(fam, n, h, w, i) for fam in ("positive", "signed")}


def test_signed_metric_reaches_zero_and_negative_denominators():
    """on the reference: over the fused cases, the 'linear' denominator with the signed metric family is exactly 0 on some
    targets and negative on others (every eps variant runs on every case, so each meets both)"""
    zero = neg = 0
    for i in range(len(FUSED_CASES)):
        x, flow, _ = _inputs(i)
        den = OS.splat_sum(_fused_metrics(i)["signed"], flow)
        zero += int((den == 0).sum())
        neg += int((den < 0).sum())
    assert zero > 0 and neg > 0, (zero, neg)


@pytest.mark.parametrize("i", range(len(FUSED_CASES)), ids=FUSED_IDS)
def test_fused_modes(ops, i):
    from diffcodec_amd import lib
    (n, c, h, w), _ = FUSED_CASES[i]
    what = FUSED_IDS[i]
    x, flow, _ = _inputs(i)
    metrics = _fused_metrics(i)
    mask = (torch.rand(n, 1, h, w, generator=torch.Generator().manual_seed(25000 + i)) < 0.3).float()
    gx, gf, gk = _g(x), _g(flow), _g(mask)
    gm = {fam: _g(m) for fam, m in metrics.items()}
    ws = _ws(lib, n, h, w)
    bufs = [gx, gf, gk, ws] + list(gm.values())
    outs = {}

    def norm(mode, eps, fam, mk=None):
        out = _out(x.shape)
        lib.call("dc_splat_norm_f32", gx.view.data_ptr(), gf.view.data_ptr(), gm[fam].view.data_ptr() if fam else 0,
                 mk.view.data_ptr() if mk else 0, out.view.data_ptr(), ws.view.data_ptr(), n, c, h, w, ops.SPLAT_MODES[mode],
                 ops.SPLAT_EPS[eps], _st())
        return out

    for eps in EPS:
        outs[("avg", eps, None)] = norm("avg", eps, None)
        for fam in metrics:
            for mode in ("linear", "soft"):
                outs[(mode, eps, fam)] = norm(mode, eps, fam)
    masked = {fam: norm("soft", "addeps", fam, gk) for fam in metrics}
    soft = {}
    for fam in metrics:
        for mk in (None, gk):
            o = _out(x.shape)
            lib.call("dc_splat_soft_f32", gx.view.data_ptr(), gf.view.data_ptr(), gm[fam].view.data_ptr(), mk.view.data_ptr() if mk else 0,
                     o.view.data_ptr(), ws.view.data_ptr(), n, c, h, w, _st())
            soft[(fam, mk is not None)] = o
    _finish(bufs, list(outs.values()) + list(masked.values()) + list(soft.values()), what)

    acc = {}
    for (mode, eps, fam), out in outs.items():
        if (mode, fam) not in acc:
            acc[(mode, fam)] = OS.splat_sum(R.cat_for(mode, x, metrics[fam] if fam else None), flow)
        want = R.normalise_f32(acc[(mode, fam)], eps)
        if mode == "soft":
            torch.testing.assert_close(out.view.cpu(), want, rtol=1e-4, atol=1e-5, msg=lambda m: f"{what} {mode}-{eps} {fam}: {m}")
        else:
            torch.testing.assert_close(out.view.cpu(), want, rtol=0, atol=0, equal_nan=True,
                                       msg=lambda m: f"{what} {mode}-{eps} {fam}: {m}")
    for fam in metrics:
        assert _bits(outs[("soft", "addeps", fam)].view, soft[(fam, False)].view), f"{what} {fam}: norm(soft, add) != splat_soft"
        assert _bits(masked[fam].view, soft[(fam, True)].view), f"{what} {fam}: norm(soft, add, mask) != splat_soft(mask)"


def test_norm_and_grad_entry_points_refuse_bad_arguments(ops):
    lib = __import__("diffcodec_amd.lib", fromlist=["lib"]).load()
    t = torch.zeros(64, device=DEV)
    ws = torch.zeros(int(lib.dc_splat_ws_bytes(1, 2, 2)), dtype=torch.uint8, device=DEV)
    p, w_ = t.data_ptr(), ws.data_ptr()
    assert lib.dc_splat_ingrad_f32(0, p, p, 1, 1, 2, 2, _st()) == -1
    assert lib.dc_splat_ingrad_f32(p, p, p, 1, 0, 2, 2, _st()) == -1
    assert lib.dc_splat_flowgrad_f32(p, p, 0, p, 1, 1, 2, 2, _st()) == -1
    assert lib.dc_splat_flowgrad_f32(p, p, p, p, 1, 1, 2, -1, _st()) == -1
    assert lib.dc_splat_norm_f32(p, p, 0, 0, p, w_, 1, 1, 2, 2, 1, 0, _st()) == -1        # linear without a metric
    assert lib.dc_splat_norm_f32(p, p, p, 0, p, w_, 1, 1, 2, 2, 0, 0, _st()) == -1        # avg with a metric
    assert lib.dc_splat_norm_f32(p, p, p, 0, p, w_, 1, 1, 2, 2, 3, 0, _st()) == -1        # no such mode
    assert lib.dc_splat_norm_f32(p, p, p, 0, p, w_, 1, 1, 2, 2, 2, 3, _st()) == -1        # no such eps
    assert lib.dc_splat_norm_f32(p, p, p, 0, p, 0, 1, 1, 2, 2, 2, 0, _st()) == -1         # no workspace


# ------------------------------------------------------------------------------------------ 4. module
MODULE_CASES = [((3, 7, 7, 9), f) for f in E.FLOW_FAMILIES] + [((2, 5, 24, 40), "smooth"), ((1, 1, 1, 1), "smooth")]


def _module_inputs(k):
    (n, c, h, w), family = MODULE_CASES[k]
    gen = torch.Generator().manual_seed(26000 + k)
    x = torch.randn(n, c, h, w, generator=gen) + 0.3
    flow = E.splat_flow(family, n, h, w, gen)
    return x, flow, R.metric_family("signed", n, h, w, k), R.metric_family("positive", n, h, w, k)


def _calls(monkeypatch):
    from diffcodec_amd import lib
    seen, real = [], lib.call

    def call(name, *args, meta=None):
        seen.append(name)
        return real(name, *args, meta=meta)
    monkeypatch.setattr(lib, "call", call)
    return seen


@pytest.mark.parametrize("k", range(len(MODULE_CASES)), ids=["x".join(map(str, s)) + "-" + f for s, f in MODULE_CASES])
def test_fused_and_composed_paths_give_the_same_bits(ops, monkeypatch, k):
    from diffcodec_amd.softsplat import softsplat
    seen = _calls(monkeypatch)
    x, flow, signed, positive = (t.to(DEV) for t in _module_inputs(k))
    for mode, metric in (("sum", None), ("avg", None), ("linear", signed), ("linear-zeroeps", signed), ("linear-clipeps", signed),
                         ("linear-addeps", positive)):
        del seen[:]
        with torch.no_grad():
            fused = softsplat(x, flow, metric, mode)
        assert seen == ["dc_splat_sum_f32" if mode == "sum" else "dc_splat_norm_f32"], (mode, seen)
        del seen[:]
        xg = x.clone().requires_grad_(True)
        composed = softsplat(xg, flow, metric, mode)
        assert seen == ["dc_splat_sum_f32"] and composed.requires_grad and not fused.requires_grad, (mode, seen)
        torch.testing.assert_close(fused, composed.detach(), rtol=0, atol=0, equal_nan=True, msg=lambda m: f"{mode}: {m}")
        # grad mode on but nothing requires a gradient: still the fused path
        del seen[:]
        again = softsplat(x, flow, metric, mode)
        assert seen == ["dc_splat_sum_f32" if mode == "sum" else "dc_splat_norm_f32"]
        torch.testing.assert_close(again, fused, rtol=0, atol=0, equal_nan=True)


def test_avg_addeps_is_read_literally(ops):
    """'avg-addeps' fails the exact test strMode == 'avg': no ones channel, the last input channel normalises (C - 1 channels out)"""
    from diffcodec_amd.softsplat import softsplat
    x, flow, _, _ = _module_inputs(0)
    out = softsplat(x.to(DEV), flow.to(DEV), None, "avg-addeps")
    assert out.shape == (3, 6, 7, 9)
    r, s = R.quotient_ref(x, flow, "addeps")
    assert torch.allclose(R.softsplat_f64(x, flow, None, "avg-addeps"), r, rtol=1e-12, atol=1e-12)
    res = L.check(out.cpu(), R.softsplat_f64(x, flow, None, "avg-addeps"), s, F32)
    assert res["ok"], res
    with pytest.raises(ValueError):
        softsplat(x.to(DEV), flow.to(DEV), torch.ones(3, 1, 7, 9, device=DEV), "avg")


def test_autocast_bf16_inputs_give_the_fp32_results(ops):
    from diffcodec_amd.softsplat import softsplat, softsplat_func
    x, flow, _, _ = _module_inputs(0)
    xb, fb = x.to(DEV).bfloat16(), flow.to(DEV).bfloat16()
    G = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    xf, ff = xb.float().requires_grad_(True), fb.float().requires_grad_(True)
    ref = softsplat_func.apply(xf, ff)
    gref = torch.autograd.grad((ref * G).sum(), (xf, ff))
    xl, fl = xb.clone().requires_grad_(True), fb.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = softsplat_func.apply(xl, fl)
        out2 = softsplat(xl, fl, None, "sum")
    assert out.dtype == F32 and out2.dtype == F32
    assert _bits(out, ref) and _bits(out2, ref)
    gx, gf = torch.autograd.grad((out * G).sum(), (xl, fl))
    # the gradient of a bf16 leaf is bf16: the fp32 gradient of the .float() call, rounded once
    assert gx.dtype == torch.bfloat16 and torch.equal(gx, gref[0].bfloat16()) and torch.equal(gf, gref[1].bfloat16())
    # fp32 leaves cast inside the autocast region keep the fp32 gradients bit for bit
    xl32, fl32 = xb.float().requires_grad_(True), fb.float().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out3 = softsplat_func.apply(xl32, fl32)
    g3 = torch.autograd.grad((out3 * G).sum(), (xl32, fl32))
    assert _bits(out3, ref) and _bits(g3[0], gref[0]) and _bits(g3[1], gref[1])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert _bits(softsplat(xb, fb, None, "sum"), ref)


def test_needs_input_grad_is_honoured(ops, monkeypatch):
    from diffcodec_amd.softsplat import softsplat
    seen = _calls(monkeypatch)
    x, flow, _, _ = (t.to(DEV) for t in _module_inputs(0))
    x.requires_grad_(True)
    softsplat(x, flow, None, "sum").sum().backward()
    assert flow.grad is None and x.grad is not None
    assert seen == ["dc_splat_sum_f32", "dc_splat_ingrad_f32"], seen
    del seen[:]
    x2, f2 = x.detach(), flow.clone().requires_grad_(True)
    softsplat(x2, f2, None, "sum").sum().backward()
    assert seen == ["dc_splat_sum_f32", "dc_splat_flowgrad_f32"], seen
    assert f2.grad is not None and f2.grad.shape == flow.shape


def test_forward_and_backward_replay_from_a_graph(ops):
    from diffcodec_amd.softsplat import softsplat
    x, flow, _, metric = (t.to(DEV) for t in _module_inputs(5))
    gen = torch.Generator().manual_seed(27000)                                                # same shape, other values
    x2 = torch.randn(x.shape, generator=gen).to(DEV)
    flow2 = E.splat_flow("nonfinite", 2, 24, 40, gen).to(DEV)
    metric2 = torch.randn(metric.shape, generator=gen).to(DEV)
    G = torch.randn(x.shape, generator=torch.Generator().manual_seed(6)).to(DEV)

    def run(a, b, c):
        out = softsplat(a, b, c, "soft")
        return (out,) + torch.autograd.grad((out * G).sum(), (a, b, c))

    sx, sf, sm = (t.clone().requires_grad_(True) for t in (x, flow, metric))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run(sx, sf, sm)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(sx, sf, sm)
    for a, b, c in ((x2, flow2, metric2), (x, flow, metric)):
        with torch.no_grad():
            sx.copy_(a), sf.copy_(b), sm.copy_(c)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(*(t.clone().requires_grad_(True) for t in (a, b, c)))
        for got, want in zip(captured, eager):
            torch.testing.assert_close(got, want, rtol=0, atol=0, equal_nan=True)


# ------------------------------------------------------------------------------------------ 5. end to end
# max |g32 - g64| / max |g64| per tensor (in, flow, metric) of softsplat_f64's arithmetic run in fp32 on the CPU
# (splat_grad_ref.e2e_fp32_error; tests/test_splat_grad_ref.py re-measures it).  The bar of each gradient is E2E_FACTOR = 4 times
# its entry: the factor is for the different accumulation order and the device exp.  'linear' with the signed `normal` metric has
# denominators near zero, which is why its fp32 error — and its bar — is larger.
E2E_FP32_ERROR = {
    "soft-3x7x7x9-smooth": (1.015e-07, 7.130e-07, 4.749e-07),
    "soft-3x7x7x9-border": (1.393e-07, 5.267e-08, 1.929e-07),
    "soft-3x7x7x9-nonfinite": (1.138e-07, 1.165e-06, 7.419e-07),
    "soft-2x5x24x40-smooth": (1.443e-07, 4.327e-07, 4.488e-07),
    "soft-2x5x24x40-border": (1.298e-07, 8.327e-08, 2.099e-07),
    "soft-2x5x24x40-nonfinite": (9.721e-08, 6.648e-07, 4.765e-07),
    "linear-3x7x7x9-smooth": (1.658e-06, 3.130e-06, 4.139e-06),
    "linear-3x7x7x9-border": (8.693e-08, 1.041e-07, 5.912e-08),
    "linear-3x7x7x9-nonfinite": (1.706e-07, 2.095e-07, 2.397e-07),
    "linear-2x5x24x40-smooth": (2.834e-05, 5.661e-05, 5.656e-05),
    "linear-2x5x24x40-border": (3.462e-07, 6.591e-08, 5.769e-07),
    "linear-2x5x24x40-nonfinite": (3.933e-05, 7.840e-05, 7.847e-05),
}


@pytest.mark.parametrize("case", R.E2E_CASES, ids=[R.e2e_label(c) for c in R.E2E_CASES])
def test_end_to_end_gradients_against_fp64_autograd(ops, record, case):
    from diffcodec_amd.softsplat import softsplat
    x, flow, metric, G = R.e2e_inputs(case)
    leaves = [t.to(DEV).requires_grad_(True) for t in (x, flow, metric)]
    out = softsplat(*leaves, case[0])
    got = torch.autograd.grad((out * G.to(DEV)).sum(), leaves)
    ref = R.e2e_fp64(case)
    errs = [R.grad_norm_error(g, r) for g, r in zip(got, ref)]
    bars = [R.E2E_FACTOR * e for e in E2E_FP32_ERROR[R.e2e_label(case)]]
    for name, e, b in zip(("in", "flow", "metric"), errs, bars):
        print(f"e2e {R.e2e_label(case)} d{name}: error {e:.3e} bar {b:.3e}")
        record(f"softsplat[e2e {R.e2e_label(case)} d{name}]", f"error={e:.3e} bar={b:.3e}")
    for name, e, b in zip(("in", "flow", "metric"), errs, bars):
        assert e <= b, f"{R.e2e_label(case)} d{name}: max|d|/max|ref| = {e:.3e} > {b:.3e}"
