"""GPU: the trainable FDN injection (csrc/fdn_grad.hip, diffcodec_amd.fdn_train) against the fp64 restatements and the bars of
tests/fdn_grad_ref.py.

`fdn` on every case of fdn_grad_ref.CASES: y, the saved mean and rstd, g_x and g_gamma are held to fp64 under their bars (4 x the
error of torch fp32 on the CPU, never below 2^-23, no element excluded; exact zeros where the reference is identically zero), the
gradient of beta is the incoming gradient, every output lies in a guarded buffer (guards intact, nothing unwritten), two runs give
the same bits.  The two launchers called by hand give the operator's bits; a null g_x or g_gamma leaves the other output's bits
unchanged; gamma and beta as the halves of one [N, 2C, H, W] tensor and g_gamma into the half of another give the bits of the dense
call, also at an offset that is not 16-byte aligned.  A sample has the same bits at N = 1 and inside N = 3; every subset of
needs_input_grad gives the bits of the full backward and launches nothing for a gradient nobody asked for; the operator runs under
torch.autocast; a captured forward + backward replays to the eager bits; what must be refused is refused.  `FDN` on the weights of
tests/golden/control_fdn.npz reproduces the reference module's output.  `DualFlowControlLayers` end to end: every parameter gradient
and the gradient of every sample against fp64 at the device's own occlusion masks, and the state-dict slices it loads.

Every test prints its figures (run with -s); `record` keeps them when $DC_TEST_LOG is set."""
import functools
import itertools

import pytest
import torch

import edge_cases as E
import fdn_grad_ref as R
import pyramid_grad_ref as P

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
    return R.evaluate(R.inputs(case), F64)


def run(T, d, wrt=(0, 1, 2), sl=slice(None)):
    """forward and backward of fdn on the case's operands (samples `sl`) -> (y, {index: gradient})"""
    ts = [t[sl].detach().clone() for t in d[:3]]
    for i in wrt:
        ts[i].requires_grad_(True)
    y = T.fdn(*ts)
    if not wrt:
        return y, {}
    return y.detach(), dict(zip(wrt, torch.autograd.grad(y, [ts[i] for i in wrt], d[3][sl])))


def bits_equal(a, b):
    return torch.equal(E.ws_bits(a), E.ws_bits(b))


class Outputs:
    """guarded buffers handed out in place of fdn_train._like and _stats"""

    def __init__(self, monkeypatch, T):
        self.guards = []
        monkeypatch.setattr(T, "_like", lambda t: self.new(t.shape, t.device))
        monkeypatch.setattr(T, "_stats", lambda n, device: self.new((n, R.GROUPS), device))

    def new(self, shape, device=DEV):
        self.guards.append(E.Guarded(tuple(shape), F32, device))
        return self.guards[-1].view

    def check(self):
        torch.cuda.synchronize()
        for i, gd in enumerate(self.guards):
            gd.assert_intact(f"buffer {i} {gd.shape}")
            assert gd.unwritten() == 0, (i, gd.shape, gd.unwritten())


@pytest.mark.parametrize("case", R.CASES, ids=R.label)
def test_every_output_against_fp64_in_guarded_buffers(lib, case, record, monkeypatch):
    from diffcodec_amd import fdn_train as T
    d = device_inputs(case)
    out = Outputs(monkeypatch, T)
    y, g = run(T, d)
    out.check()
    assert len(out.guards) == 5                                            # y, mean, rstd; g_x, g_gamma
    mean, rstd = out.guards[1].view, out.guards[2].view
    assert tuple(mean.shape) == tuple(rstd.shape) == (case[0], R.GROUPS) and bits_equal(y, out.guards[0].view)
    ref = reference(case)
    assert torch.equal(g[2], d[3])                                         # the gradient of beta is g itself
    m = R.group_size(case)
    if m > 1:                                                              # the constant group: var = 0, rstd = eps^-1/2, xh = 0
        n, grp = R.CONSTANT_GROUP
        assert float(mean[n, grp]) == float(d[0].reshape(case[0], R.GROUPS, m)[n, grp, 0])
        assert abs(float(rstd[n, grp]) * R.EPS ** 0.5 - 1) <= 2.0 ** -22
    for nm, got, want, bar in zip(R.TENSORS, (y, mean, rstd, g[0], g[1]), ref, R.BARS[case]):
        err = R.norm_error(got, want)
        print(f"{R.label(case)} {nm}: error {err:.3g}, bar {bar:.3g}")
        record(f"fdn_grad/{R.label(case)}/{nm}", f"{err:.3g}\t{bar:.3g}")
    for nm, got, want, bar in zip(R.TENSORS, (y, mean, rstd, g[0], g[1]), ref, R.BARS[case]):
        assert R.norm_error(got, want) <= bar, (nm, R.norm_error(got, want), bar)
    monkeypatch.undo()
    y2, g2 = run(T, d)
    assert bits_equal(y2, y) and all(bits_equal(g2[i], g[i]) for i in range(3))


HAND_CASES = [(2, 32, 3, 5, "plain"), (3, 64, 7, 9, "plain"), (2, 96, 16, 16, "far"), (2, 1280, 8, 8, "plain")]


def by_hand(lib, d, out, gamma=None, beta=None, g_gamma=None, want_x=True, want_gamma=True):
    """the two launchers on a case's operands; gamma, beta and g_gamma default to dense tensors -> (y, mean, rstd, g_x, g_gamma)"""
    x, gm, bt, g = d
    n, c, h, w = x.shape
    gamma = gm if gamma is None else gamma
    beta = bt if beta is None else beta
    y, mean, rstd = out(x.shape), out((n, R.GROUPS)), out((n, R.GROUPS))
    lib.call("dc_fdn_f32", x.data_ptr(), gamma.data_ptr(), gamma.stride(0), beta.data_ptr(), beta.stride(0), y.data_ptr(), mean.data_ptr(),
             rstd.data_ptr(), n, c, h, w, R.EPS, stream())
    gx = out(x.shape) if want_x else None
    if want_gamma and g_gamma is None:
        g_gamma = out(x.shape)
    gg = g_gamma if want_gamma else None
    lib.call("dc_fdn_grad_f32", g.data_ptr(), x.data_ptr(), gamma.data_ptr() if want_x else 0, gamma.stride(0), mean.data_ptr(),
             rstd.data_ptr(), ptr(gx), ptr(gg), gg.stride(0) if gg is not None else 0, n, c, h, w, stream())
    return y, mean, rstd, gx, gg


@pytest.mark.parametrize("case", HAND_CASES, ids=R.label)
def test_the_launchers_by_hand_and_each_output_alone(lib, case):
    from diffcodec_amd import fdn_train as T
    d = device_inputs(case)
    y, g = run(T, d)
    guards = []

    def out(shape):
        guards.append(E.Guarded(tuple(shape), F32, DEV))
        return guards[-1].view

    y1, mean, rstd, gx, gg = by_hand(lib, d, out)
    assert bits_equal(y1, y) and bits_equal(gx, g[0]) and bits_equal(gg, g[1])
    only_x = by_hand(lib, d, out, want_gamma=False)
    only_gamma = by_hand(lib, d, out, want_x=False)                        # no reduction pass, gamma not read (null)
    assert only_x[4] is None and only_gamma[3] is None
    assert bits_equal(only_x[3], g[0]) and bits_equal(only_gamma[4], g[1])
    torch.cuda.synchronize()
    for i, gd in enumerate(guards):
        gd.assert_intact(f"buffer {i} {gd.shape}")
        assert gd.unwritten() == 0, (i, gd.shape)


def halves(a, b, shift):
    """[N, 2C, H, W] holding a and b as its channel halves, its first element `shift` floats past a 16-byte boundary"""
    n, c, h, w = a.shape
    base = torch.empty(n * 2 * c * h * w + 4, device=a.device, dtype=F32)
    assert base.data_ptr() % 16 == 0
    both = base[shift:shift + n * 2 * c * h * w].view(n, 2 * c, h, w)
    both[:, :c] = a
    both[:, c:] = b
    return both


@pytest.mark.parametrize("case,shift", [((2, 96, 16, 16, "plain"), 0), ((2, 96, 16, 16, "far"), 1), ((3, 64, 7, 9, "plain"), 0),
                                        ((2, 1280, 8, 8, "plain"), 3)], ids=lambda v: R.label(v) if isinstance(v, tuple) else f"shift{v}")
def test_channel_halves_of_one_tensor_give_the_bits_of_the_dense_call(lib, case, shift):
    """gamma and beta are the two halves of one [N, 2C, H, W] tensor, g_gamma goes into the first half of another; with shift != 0
    the views are not 16-byte aligned, so the 4-byte path runs on operands whose dense call took the 16-byte path"""
    from diffcodec_amd import fdn_train as T
    d = device_inputs(case)
    x, gm, bt, g = d
    n, c, h, w = x.shape
    gb = halves(gm, bt, shift)
    assert (gb.data_ptr() % 16 != 0) == (shift != 0) and gb[:, :c].stride(0) == 2 * c * h * w
    dense = by_hand(lib, d, lambda shape: torch.empty(shape, device=DEV, dtype=F32))
    target = halves(torch.zeros_like(x), torch.zeros_like(x), shift)
    target[:, c:] = 7.0
    view = by_hand(lib, d, lambda shape: torch.empty(shape, device=DEV, dtype=F32), gamma=gb[:, :c], beta=gb[:, c:], g_gamma=target[:, :c])
    torch.cuda.synchronize()
    for nm, a, b in zip(R.TENSORS, dense, view):
        assert bits_equal(a, b), nm
    assert bool((target[:, c:] == 7.0).all())                              # the other half is untouched
    # and through the operator: the views are read in place
    ts = [x.clone().requires_grad_(True), gb[:, :c].detach().requires_grad_(True), gb[:, c:].detach().requires_grad_(True)]
    y = T.fdn(*ts)
    grads = torch.autograd.grad(y, ts, g)
    assert bits_equal(y.detach(), dense[0]) and bits_equal(grads[0], dense[3]) and bits_equal(grads[1], dense[4]) and torch.equal(grads[2], g)


def test_a_sample_does_not_depend_on_the_batch(lib):
    from diffcodec_amd import fdn_train as T
    d = device_inputs(R.BATCH_CASE)
    y, g = run(T, d)
    for i in range(R.BATCH_CASE[0]):
        y1, g1 = run(T, d, sl=slice(i, i + 1))
        assert bits_equal(y1, y[i:i + 1]), i
        for k in range(3):
            assert bits_equal(g1[k], g[k][i:i + 1]), (i, k)


def test_every_subset_of_the_wanted_gradients(lib, monkeypatch):
    from diffcodec_amd import fdn_train as T
    d = device_inputs(R.BATCH_CASE)
    y, g = run(T, d)
    calls = []
    real = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a, **k: (calls.append((name, a)), real(name, *a, **k))[1])
    for r in range(0, 4):
        for wrt in itertools.combinations(range(3), r):
            del calls[:]
            y1, g1 = run(T, d, wrt=wrt)
            assert bits_equal(y1, y) and sorted(g1) == list(wrt)
            for k in wrt:
                assert bits_equal(g1[k], g[k]), (wrt, k)
            assert calls[0][0] == "dc_fdn_f32" and len(calls) == (2 if (0 in wrt or 1 in wrt) else 1), (wrt, [c[0] for c in calls])
            if len(calls) == 2:
                name, a = calls[1]
                assert name == "dc_fdn_grad_f32" and (a[6] != 0) == (0 in wrt) and (a[7] != 0) == (1 in wrt), wrt


def test_under_autocast(lib):
    from diffcodec_amd import fdn_train as T
    d = device_inputs(R.BATCH_CASE)
    y, g = run(T, d)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y1, g1 = run(T, d)
        assert y1.dtype == F32 and bits_equal(y1, y) and all(bits_equal(g1[k], g[k]) for k in range(3))
        half = [t.detach().to(torch.bfloat16).requires_grad_(True) for t in d[:3]]       # bf16 inputs are widened to fp32
        yh = T.fdn(*half)
        gh = torch.autograd.grad(yh, half, d[3])
    wide = [t.detach().float().requires_grad_(True) for t in half]
    yw = T.fdn(*wide)
    gw = torch.autograd.grad(yw, wide, d[3])
    assert yh.dtype == F32 and bits_equal(yh.detach(), yw.detach())
    assert all(a.dtype == torch.bfloat16 and torch.equal(a, b.to(torch.bfloat16)) for a, b in zip(gh, gw))


@pytest.mark.parametrize("case", [(3, 64, 7, 9, "plain"), (2, 96, 16, 16, "far")], ids=R.label)
def test_captured_forward_and_backward_replay_to_the_eager_bits(lib, case):
    from diffcodec_amd import fdn_train as T
    a = device_inputs(case)
    b = tuple(t.roll(1, 1).contiguous() for t in a)                        # other values, same shapes
    st = [t.clone() for t in a]

    def go():
        ts = [t.requires_grad_(True) for t in st[:3]]
        y = T.fdn(*ts)
        return (y,) + torch.autograd.grad(y, ts, st[3])

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
        y, g = run(T, src)
        assert bits_equal(captured[0].detach(), y)
        for k in range(3):
            assert bits_equal(captured[1 + k], g[k]), k


def test_refusals(lib):
    from diffcodec_amd import fdn_train as T
    x = torch.zeros(2, 64, 4, 4, device=DEV)
    bad = torch.zeros(2, 48, 4, 4, device=DEV)
    with pytest.raises(ValueError, match="multiple of 32"):
        T.fdn(bad, bad, bad)
    assert lib.load().dc_fdn_f32(x.data_ptr(), x.data_ptr(), 768, x.data_ptr(), 768, x.data_ptr(), x.data_ptr(), x.data_ptr(), 2, 48, 4, 4,
                                 1e-5, None) == -1                         # C = 48 at the launcher: DC_ERR_INVALID, nothing launched
    with pytest.raises(RuntimeError, match="no CPU path"):
        T.fdn(x, x.cpu(), x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        T.fdn(x.cpu(), x, x)
    for i in range(3):                                                     # a bf16 operand outside autocast
        ts = [x, x, x]
        ts[i] = x.to(torch.bfloat16)
        with pytest.raises(ValueError, match="float32"):
            T.fdn(*ts)
    with pytest.raises(ValueError, match="gamma"):
        T.fdn(x, torch.zeros(2, 64, 4, 5, device=DEV), x)                  # control_utils.py:30
    with pytest.raises(ValueError, match="beta"):
        T.fdn(x, x, torch.zeros(2, 64, 2, 2, device=DEV))
    with pytest.raises(ValueError, match="spatial"):
        T.FDN(64, 64).to(DEV)(x, torch.zeros(2, 64, 8, 8, device=DEV))


def test_the_module_on_the_golden_weights_reproduces_the_reference_module(lib, record):
    from diffcodec_amd import fdn_train as T
    sd, x, local, y = R.golden()
    m = T.FDN(x.shape[1], local.shape[1]).to(DEV)
    m.load_state_dict(sd)
    with torch.no_grad():
        got = m(x.to(DEV), local.to(DEV))
    err, bar = R.norm_error(got, y), R.bar_of(R.GOLDEN_DISTANCE)
    own = R.norm_error(got, R.fdn_module(sd, "", x, local, F64))
    print(f"golden: error {err:.3g}, bar {bar:.3g}; against the fp64 restatement {own:.3g}")
    record("fdn_grad/golden/y", f"{err:.3g}\t{bar:.3g}")
    assert err <= bar


# ------------------------------------------------------------------------------------------ the module end to end
def test_control_layers_every_gradient_at_the_devices_masks(lib, record):
    from diffcodec_amd import fdn_train as T
    sd, cond, flow, samples, G = R.module_inputs()
    inject, n = R.MODULE_CASE
    m = T.DualFlowControlLayers(inject).to(DEV)
    assert not any(bool(z.weight.any()) for z in m.feature_extractor.zero_convs)          # zero_module: seeded non-zero below
    m.load_state_dict(sd)
    cond, flow = cond.to(DEV), flow.to(DEV)
    smp = [s.to(DEV).requires_grad_(True) for s in samples]
    levels, aux = m.pyramid(cond, flow, return_aux=True)
    assert [tuple(l.shape) for l in levels] == [(n, inject[k], P.MODULE_SIZE >> (3 + k), P.MODULE_SIZE >> (3 + k)) for k in range(4)]
    for k, a in enumerate(aux):
        for nm in ("occ_f", "occ_b"):
            assert float((1 - a[nm]).flatten(1).sum(1).min()) >= 1, (k, nm)               # no level is dead
    outs = [m.inject(i, s, levels) for i, s in enumerate(smp)]
    loss = sum((o * g.to(DEV)).sum() for o, g in zip(outs, G))
    names = [k for k, _ in m.named_parameters()]
    grads = torch.autograd.grad(loss, list(m.parameters()) + smp)
    got = dict(zip(names + [f"sample.{i}" for i in range(len(smp))], grads))
    cpu_aux = [{k: v.cpu() for k, v in a.items()} for a in aux]
    ref = R.module_grads(sd, cond.cpu(), cpu_aux, samples, G, F64)
    assert sorted(got) == sorted(ref)
    fwd = R.module_forward({k: v.to(F64) for k, v in sd.items()}, cond.cpu(), cpu_aux, [s.to(F64) for s in samples], F64)
    for i, (o, r) in enumerate(zip(outs, fwd)):
        assert R.norm_error(o, r) <= 1e-5, (i, R.norm_error(o, r))                        # the forward, loosely: the gradients are the test
    worst = (0.0, None)
    for k in sorted(ref):
        assert float(ref[k].abs().max()) > 0, k
        err, bar = R.norm_error(got[k], ref[k]), R.module_bar(k)
        record(f"fdn_module/{k}", f"{err:.3g}\t{bar:.3g}")
        worst = max(worst, (err / bar, k))
        print(f"{k}: error {err:.3g}, bar {bar:.3g}")
    print(f"worst error / bar {worst[0]:.3g} ({worst[1]})")
    for k in sorted(ref):
        assert R.norm_error(got[k], ref[k]) <= R.module_bar(k), k


def test_control_layers_load_exactly_their_slices_of_a_controlnet_state_dict(lib):
    from diffcodec_amd import fdn_train as T, weights
    cfg = dict(weights.SD15_UNET_CONFIG, block_out_channels=(64, 128, 128, 128), cross_attention_dim=64)
    assert weights.inject_channels(cfg) == R.MODULE_CASE[0]
    full = weights.synthesize(weights.controlnet_spec(cfg), seed=5, bf16_round=False)
    own = sorted(k for k in full if k.startswith(("feature_extractor.", "fdn")))
    m = T.DualFlowControlLayers(weights.inject_channels(cfg)).to(DEV)
    res = m.load_state_dict(full, strict=False)
    assert res.missing_keys == [] and sorted(set(full) - set(res.unexpected_keys)) == own == sorted(m.state_dict())
    assert not [k for k in res.unexpected_keys if k.startswith(("feature_extractor.", "fdn"))] and len(res.unexpected_keys) > 100
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), full[k].float()), k
