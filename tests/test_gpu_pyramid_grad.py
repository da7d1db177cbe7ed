"""GPU: the trainable control pyramid (csrc/pyramid_grad.hip, diffcodec_amd.pyramid_train) against the fp64 restatements and the bars of
tests/pyramid_grad_ref.py.

`warp_fuse` on every case of pyramid_grad_ref.CASES: the forward has the bits of `ops.splat_soft` twice and `ops.fuse_warped`; every
gradient is held to fp64 autograd under its bar (4 x the fp32 restatement's own error, no element excluded), with every plane and
gradient the backward allocates in a guarded buffer (guards intact, nothing unwritten); two runs give the same bits.  The three
launchers chained by hand give the bits of the autograd operator, one-sided and single-output launches included.  Image i has the same
gradient bits in a batch of 1 and of 3; every subset of needs_input_grad gives the bits of the full backward and launches nothing
for a side nobody asked for; the operator runs under torch.autocast; a captured forward + backward replays to the eager bits; the
gate of the clamp is checked pixel by pixel where one confidence is exactly 0 and the other is not positive (S = 1e-6).  The
whole module at two widths: forward bits of the inference extractor, every parameter gradient against fp64 at the device's own masks
(`return_aux`), and one SGD step through `from_inference` moves the inference pyramid to the bits of the module's next forward.

Every test prints its figures (run with -s); `record` keeps them when $DC_TEST_LOG is set."""
import functools
import itertools

import pytest
import torch

import edge_cases as E
import pyramid_grad_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd import lib as l
    return l


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()


@functools.lru_cache(maxsize=None)
def device_inputs(case):
    """the case's operands on the device: computed once, never changed"""
    return tuple(t.to(DEV) for t in R.inputs(case))


@functools.lru_cache(maxsize=None)
def reference(case):
    return R.fp64_grads(case)


def run(PT, d, wrt=(0, 1, 2, 3), sl=slice(None)):
    """forward and backward of warp_fuse on the case's operands (images `sl`) -> (fused, {index: gradient})"""
    ts = [t[sl].detach().clone() for t in d[:8]]
    for i in wrt:
        ts[i].requires_grad_(True)
    y = PT.warp_fuse(*ts)
    if not wrt:
        return y, {}
    return y.detach(), dict(zip(wrt, torch.autograd.grad(y, [ts[i] for i in wrt], d[8][sl])))


def bits_equal(a, b):
    return torch.equal(E.ws_bits(a), E.ws_bits(b))


@pytest.mark.parametrize("case", R.CASES, ids=R.label)
def test_forward_bits_and_every_gradient_against_fp64(lib, case, record, monkeypatch):
    from diffcodec_amd import ops, pyramid_train as PT
    d = device_inputs(case)
    first, last, mf, mb, ff, fb, of, ob, G = d
    wf, wl = ops.splat_soft(first, ff, mf, mask=of), ops.splat_soft(last, fb, mb, mask=ob)
    want = ops.fuse_warped(wf, wl, mf, mb, of, ob)
    guards = []

    def guarded(shape, device):
        guards.append(E.Guarded(tuple(shape), F32, device))
        return guards[-1].view

    monkeypatch.setattr(PT, "_plane", guarded)
    monkeypatch.setattr(PT, "_like", lambda t: guarded(t.shape, t.device))
    y, g = run(PT, d)
    torch.cuda.synchronize()
    assert bits_equal(y, want)
    assert len(guards) == 2 * 4 + 2 + 4                                   # per side e, den, coef, gden; g_cf, g_cb; four gradients
    for i, gd in enumerate(guards):
        gd.assert_intact(f"buffer {i} {gd.shape}")
        assert gd.unwritten() == 0, (i, gd.shape, gd.unwritten())
    for i, nm in enumerate(R.GRAD_NAMES):
        err, bar = R.norm_error(g[i], reference(case)[i]), R.BARS[case][i]
        print(f"{R.label(case)} d {nm}: error {err:.3g}, bar {bar:.3g}")
        record(f"pyramid_grad/{R.label(case)}/{nm}", f"{err:.3g}\t{bar:.3g}")
        assert err <= bar, (nm, err, bar)
    monkeypatch.undo()
    y2, g2 = run(PT, d)
    assert bits_equal(y2, y) and all(bits_equal(g2[i], g[i]) for i in range(4))


def test_the_gate_at_exactly_zero_where_the_sum_of_confidences_is_1e_6(lib, record):
    """pixels with one confidence exactly 0 and the other <= 0 (S = 1e-6, g_conf = A / S), each against its own reference"""
    from diffcodec_amd import pyramid_train as PT
    t = R.gate_inputs()
    _, g = run(PT, tuple(x.to(DEV) for x in t))
    for which, at, err, tol, ref in R.gate_report([g[i] for i in range(4)], t):
        print(f"d {R.GRAD_NAMES[which]}[{at}]: reference {ref:.6g}, error {err:.3g}, tol {tol:.3g}")
        record(f"pyramid_gate/{R.GRAD_NAMES[which]}/{at}", f"{err:.3g}\t{tol:.3g}")
        assert err <= tol, (which, at, err, tol, ref)


HAND_CASES = [(3, 20, 5, 9, "nonfinite"), (1, 17, 33, 33, "nonfinite"), (2, 640, 8, 8, "smooth"), (1, 5, 1, 257, "smooth")]


@pytest.mark.parametrize("case", HAND_CASES, ids=R.label)
def test_the_launchers_chained_by_hand_give_the_operators_bits(lib, case):
    from diffcodec_amd import ops, pyramid_train as PT
    d = device_inputs(case)
    first, last, mf, mb, ff, fb, of, ob, G = d
    n, c, h, w = first.shape
    _, g = run(PT, d)
    wf, wl = ops.splat_soft(first, ff, mf, mask=of), ops.splat_soft(last, fb, mb, mask=ob)
    guards = []

    def out(shape):
        guards.append(E.Guarded(tuple(shape), F32, DEV))
        return guards[-1].view

    def planes(sides):
        """exp, den and the target-side launch for the wanted sides -> (e, g_conf, coef, gden) per side"""
        e, den, coef, gden = ([None, None] for _ in range(4))
        for s, (m, fl) in enumerate(((mf, ff), (mb, fb))):
            if s in sides:
                e[s], den[s], coef[s], gden[s] = (out(m.shape) for _ in range(4))
                lib.call("dc_pyramid_exp_f32", m.data_ptr(), e[s].data_ptr(), m.numel(), stream())
                ws = ops._splat_ws(n, h, w, DEV)
                lib.call("dc_splat_sum_f32", e[s].data_ptr(), fl.data_ptr(), den[s].data_ptr(), ws.data_ptr(), n, 1, h, w, stream())
        g_conf = [out(mf.shape), out(mf.shape)]
        lib.call("dc_pyramid_fuse_grad_f32", G.data_ptr(), wf.data_ptr(), wl.data_ptr(), mf.data_ptr(), mb.data_ptr(), of.data_ptr(),
                 ob.data_ptr(), ptr(den[0]), ptr(den[1]), g_conf[0].data_ptr(), g_conf[1].data_ptr(), ptr(coef[0]), ptr(gden[0]),
                 ptr(coef[1]), ptr(gden[1]), n, c, h, w, stream())
        return e, g_conf, coef, gden

    def warp(s, pl, want_x, want_m):
        e, g_conf, coef, gden = pl
        x, fl = ((first, ff), (last, fb))[s]
        gx = out(x.shape) if want_x else None
        gm = out(mf.shape) if want_m else None
        lib.call("dc_pyramid_warp_grad_f32", x.data_ptr() if want_m else 0, e[s].data_ptr(), fl.data_ptr(), G.data_ptr(), coef[s].data_ptr(),
                 gden[s].data_ptr() if want_m else 0, g_conf[s].data_ptr() if want_m else 0, ptr(gx), ptr(gm), n, c, h, w, stream())
        return gx, gm

    both = planes((0, 1))
    for s in (0, 1):
        gx, gm = warp(s, both, True, True)
        assert bits_equal(gx, g[s]) and bits_equal(gm, g[2 + s]), s
        assert bits_equal(warp(s, both, True, False)[0], g[s]) and bits_equal(warp(s, both, False, True)[1], g[2 + s]), s
        one = planes((s,))                                                # the other side's den, coef and gden are null
        gx, gm = warp(s, one, True, True)
        assert bits_equal(gx, g[s]) and bits_equal(gm, g[2 + s]), s
        assert bits_equal(one[1][0], both[1][0]) and bits_equal(one[1][1], both[1][1])
    torch.cuda.synchronize()
    for i, gd in enumerate(guards):
        gd.assert_intact(f"buffer {i} {gd.shape}")
        assert gd.unwritten() == 0, (i, gd.shape)


@pytest.mark.parametrize("case", [(3, 20, 5, 9, "smooth"), (3, 160, 16, 16, "collapse")], ids=R.label)
def test_an_images_gradients_do_not_depend_on_the_batch(lib, case):
    from diffcodec_amd import pyramid_train as PT
    d = device_inputs(case)
    y, g = run(PT, d)
    for i in range(case[0]):
        y1, g1 = run(PT, d, sl=slice(i, i + 1))
        assert bits_equal(y1, y[i:i + 1])
        for k in range(4):
            assert bits_equal(g1[k], g[k][i:i + 1]), (i, R.GRAD_NAMES[k])


def test_every_subset_of_the_wanted_gradients(lib, monkeypatch):
    from diffcodec_amd import pyramid_train as PT
    case = (3, 20, 5, 9, "nonfinite")
    d = device_inputs(case)
    y, g = run(PT, d)
    calls = []
    real = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    forward = ["dc_splat_soft_f32", "dc_splat_soft_f32", "dc_fuse_warped_f32"]
    for r in range(0, 5):
        for wrt in itertools.combinations(range(4), r):
            del calls[:]
            y1, g1 = run(PT, d, wrt=wrt)
            assert bits_equal(y1, y) and sorted(g1) == list(wrt)
            for k in wrt:
                assert bits_equal(g1[k], g[k]), (wrt, k)
            sides = sum(1 for s in (0, 1) if s in wrt or 2 + s in wrt)
            assert calls[:3] == forward
            back = calls[3:]
            assert back.count("dc_pyramid_warp_grad_f32") == back.count("dc_pyramid_exp_f32") == back.count("dc_splat_sum_f32") == sides
            assert back.count("dc_pyramid_fuse_grad_f32") == (1 if sides else 0) and len(back) == 3 * sides + (1 if sides else 0), (wrt, back)


def test_under_autocast(lib):
    from diffcodec_amd import pyramid_train as PT
    case = (3, 20, 5, 9, "smooth")
    d = device_inputs(case)
    y, g = run(PT, d)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y1, g1 = run(PT, d)
        assert y1.dtype == F32 and bits_equal(y1, y) and all(bits_equal(g1[k], g[k]) for k in range(4))
        # bf16 features are widened to fp32 as custom_fwd(cast_inputs=torch.float32) does
        ts = [t.detach().clone() for t in d[:8]]
        half = ts[0].to(torch.bfloat16).requires_grad_(True)
        yh = PT.warp_fuse(half, *ts[1:])
        (gh,) = torch.autograd.grad(yh, [half], d[8])
    ts[0] = half.detach().float().requires_grad_(True)
    yw = PT.warp_fuse(*ts)
    (gw,) = torch.autograd.grad(yw, [ts[0]], d[8])
    assert yh.dtype == F32 and bits_equal(yh.detach(), yw.detach()) and gh.dtype == torch.bfloat16 and torch.equal(gh, gw.to(torch.bfloat16))


@pytest.mark.parametrize("case", [(3, 20, 5, 9, "nonfinite"), (2, 33, 17, 70, "smooth")], ids=R.label)
def test_captured_forward_and_backward_replay_to_the_eager_bits(lib, case):
    from diffcodec_amd import pyramid_train as PT
    a = device_inputs(case)
    b = tuple(t.roll(1, 0).contiguous() if i < 4 else t for i, t in enumerate(a))          # other features and metrics, same flows
    st = [t.clone() for t in a]

    def go():
        ts = [t.requires_grad_(True) if i < 4 else t for i, t in enumerate(st[:8])]
        y = PT.warp_fuse(*ts)
        return (y,) + torch.autograd.grad(y, ts[:4], st[8])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        go()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = go()
    for src in (b, a):
        with torch.no_grad():
            for t, s in zip(st, src):
                t.copy_(s)
        graph.replay()
        torch.cuda.synchronize()
        y, g = run(PT, src)
        assert bits_equal(captured[0].detach(), y)
        for k in range(4):
            assert bits_equal(captured[1 + k], g[k]), R.GRAD_NAMES[k]


# ------------------------------------------------------------------------------------------ the whole module
def _module(case):
    from diffcodec_amd import pyramid_train as PT
    sd, cond, flow, G = R.module_inputs(case)
    m = PT.BiDirFeatureExtractor(case[0]).to(DEV)
    m.load_state_dict(sd)
    return m, sd, cond.to(DEV), flow.to(DEV), [g.to(DEV) for g in G]


@pytest.mark.parametrize("case", R.MODULE_CASES, ids=R.module_label)
def test_module_forward_bits_and_parameter_gradients_at_the_devices_masks(lib, case, record):
    from diffcodec_amd import controlnet
    m, sd, cond, flow, G = _module(case)
    ext = controlnet.BiDirFeatureExtractor(sd, "", DEV)
    want = ext(cond, flow)
    outs, aux = m(cond, flow, return_aux=True)
    assert len(outs) == len(aux) == 4
    for k, (o, wv) in enumerate(zip(outs, want)):
        assert tuple(o.shape) == (case[1], case[0][k], R.MODULE_SIZE >> (3 + k), R.MODULE_SIZE >> (3 + k)) and bits_equal(o.detach(), wv), k
    with torch.no_grad():
        plain = m(cond, flow)
    assert all(bits_equal(p, o.detach()) for p, o in zip(plain, outs))
    for k, a in enumerate(aux):
        assert sorted(a) == ["flow_b", "flow_f", "occ_b", "occ_f"] and not any(t.requires_grad for t in a.values())
        for nm in ("occ_f", "occ_b"):
            assert float((1 - a[nm]).flatten(1).sum(1).min()) >= 1, (k, nm)
    names = [n for n, _ in m.named_parameters()]
    loss = sum((o * g).sum() for o, g in zip(outs, G))
    grads = dict(zip(names, torch.autograd.grad(loss, list(m.parameters()))))
    ref = R.module_grads(sd, cond.cpu(), [{k: v.cpu() for k, v in a.items()} for a in aux], [g.cpu() for g in G], F64)
    assert sorted(grads) == sorted(ref)
    worst = (0.0, None)
    for k in sorted(ref):
        assert float(ref[k].abs().max()) > 0, k
        err, bar = R.norm_error(grads[k], ref[k]), R.module_bar(case, k)
        record(f"pyramid_module/{R.module_label(case)}/{k}", f"{err:.3g}\t{bar:.3g}")
        worst = max(worst, (err / bar, k))
        print(f"{R.module_label(case)} {k}: error {err:.3g}, bar {bar:.3g}")
    print(f"{R.module_label(case)}: worst error / bar {worst[0]:.3g} ({worst[1]})")
    for k in sorted(ref):
        assert R.norm_error(grads[k], ref[k]) <= R.module_bar(case, k), k


def test_an_sgd_step_through_from_inference_is_what_the_inference_pyramid_reads(lib):
    from diffcodec_amd import controlnet, pyramid_train as PT
    case = R.MODULE_CASES[1]
    sd, cond, flow, G = R.module_inputs(case)
    cond, flow, G = cond.to(DEV), flow.to(DEV), [g.to(DEV) for g in G]
    ext = controlnet.BiDirFeatureExtractor(sd, "", DEV)
    before = ext(cond, flow)
    m = PT.BiDirFeatureExtractor.from_inference(ext)
    opt = torch.optim.SGD(m.parameters(), lr=1e-2)
    outs = m(cond, flow)
    assert all(bits_equal(o.detach(), b) for o, b in zip(outs, before))
    sum((o * g).sum() for o, g in zip(outs, G)).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    opt.step()
    after = ext(cond, flow)
    with torch.no_grad():
        again = m(cond, flow)
    for k in range(4):
        assert bits_equal(after[k], again[k]) and not torch.equal(after[k], before[k]), k
