"""GPU: the training losses of diffcodec_amd.losses (csrc/lpips_grad.hip, csrc/edge_loss.hip) against tests/loss_ref.py with seeded
synthetic weights.

The device's gradient is held to the fp64 backward LINEARISED AT THE DEVICE'S OWN post-ReLU maps (loss_ref.backward_from_maps fed
model.features(...)): a ReLU or argmax decision that differs between an fp32 and an fp64 forward is no arithmetic error.  Bars
(tests/test_loss_ref.py: 4 x the error of the reference's own fp32 arithmetic on the CPU, max |d| / max |ref|, no element
excluded) and what the MI355X measured:

    case       bar       measured: dx, dy, both
    2x31x31    1.9e-6    4.7e-7, 7.9e-7, 7.9e-7
    3x67x95    2.3e-6    9.4e-7, 1.13e-6, 1.13e-6      (normalize=True 1.13e-6, lpips=False 8.3e-7)
    2x70x146   2.3e-6    9.2e-7, 9.0e-7, 9.2e-7
    Sobel gradients: 1.6e-7 at 2x3x1x70 and 2x3x70x1 (bar 6.4e-7), 1.4e-7 at 3x3x17x70 (4.4e-6), 1.7e-7 at 2x2x17x65 (3.8e-6)

Every stage launcher is run on its own on guarded operands and outputs (intact guards, nothing unwritten, two runs equal) and held
to its fp64 stage reference with oracle.launch_ref.check and the stage's S term."""
import ctypes
import functools

import pytest
import torch

import edge_cases as E
import loss_ref as R
from oracle import launch_ref as L
from loss_ref import BARS, SEED, SOBEL_BARS, SOBEL_SEED, SOBEL_SHAPES

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
IDS = [f"{n}x{h}x{w}" for n, h, w in R.SHAPES]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd import lib as l
    return l


@functools.lru_cache(maxsize=None)
def weights():
    return R.synth_weights(seed=20)


@functools.lru_cache(maxsize=None)
def model(lpips=True):
    from diffcodec_amd import losses
    return losses.NormFixLPIPS.from_state_dict(weights(), lpips=lpips).to(DEV)


@functools.lru_cache(maxsize=None)
def case(i, normalize=False, lpips=True):
    """device inputs of case i, the device's own maps and the fp64 reference linearised at them: computed once, never changed"""
    n, h, w = R.SHAPES[i]
    x, y, g = R.loss_inputs(n, h, w, SEED + i)
    if normalize:
        x, y = (x + 1) / 2, (y + 1) / 2
    m = model(lpips)
    fx = [f.cpu() for f in m.features(x.to(DEV), normalize=normalize)]
    fy = [f.cpu() for f in m.features(y.to(DEV), normalize=normalize)]
    for f in fx + fy:                                                # the inputs exercise the ReLU masks
        assert 0.2 <= float((f == 0).double().mean()) <= 0.8
    ref = R.backward_from_maps(weights(), fx, fy, g, (h, w), normalize=normalize, lpips=lpips)
    assert float(ref["dx"].abs().max()) > 0 and float(ref["dy"].abs().max()) > 0
    return dict(x=x.to(DEV), y=y.to(DEV), g=g.to(DEV), fx=fx, fy=fy, ref=ref, hw=(h, w), n=n)


def grads(m, x, y, g, wrt, normalize=False):
    """(value, gradients w.r.t. the operands `wrt` names) of (m(x, y).view(-1) * g).sum()"""
    xs = x.detach().clone().requires_grad_("x" in wrt)
    ys = y.detach().clone().requires_grad_("y" in wrt)
    val = m(xs, ys, normalize=normalize)
    return (val.detach(),) + torch.autograd.grad((val.view(-1) * g).sum(), [t for t in (xs, ys) if t.requires_grad])


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(t):
    g = E.Guarded(tuple(t.shape), F32, DEV)
    g.fill(t.to(DEV, F32))
    return g


def run_stage(name, shape, operands, launch, r, s):
    """launch(out view) twice on fresh guarded outputs: intact guards, nothing unwritten, equal runs, within the stage's bound"""
    outs = []
    for _ in range(2):
        o = E.Guarded(shape, F32, DEV)
        launch(o.view)
        torch.cuda.synchronize()
        o.assert_intact(name + " output")
        assert o.unwritten() == 0, f"{name}: {o.unwritten()} output elements never written"
        outs.append(o.view.clone())
    for k, op in enumerate(operands):
        op.assert_intact(f"{name} operand {k}")
    assert torch.equal(outs[0], outs[1]), f"{name}: two runs differ"
    v = L.check(outs[0].cpu(), r, s, F32)
    print(f"{name}: err/tol {v['ratio']:.3f} rms {v['rms']:.2e}")
    assert v["ok"], (name, v)
    return outs[0]


# ------------------------------------------------------------------------------------------------ stages
@pytest.mark.parametrize("i", range(3), ids=IDS)
def test_tail_gradient_of_each_layer(lib, i):
    c = case(i)
    n = c["n"]
    _, lins = R.params(weights())
    wts = model()._weights(torch.device(DEV))
    g = guarded(c["g"])
    for l in range(5):
        f = guarded(torch.cat([c["fx"][l], c["fy"][l]]))
        hw = c["fx"][l].shape[2] * c["fx"][l].shape[3]
        rx, sx = R.tail_grad_ref(c["fx"][l], c["fy"][l], lins[l], c["g"].cpu())
        ry, sy = R.tail_grad_ref(c["fy"][l], c["fx"][l], lins[l], c["g"].cpu())
        for sides, r, s in ((3, torch.cat([rx, ry]), torch.cat([sx, sy])), (1, rx, sx), (2, ry, sy)):
            run_stage(f"tail_grad layer {l} sides {sides}", tuple(r.shape), [f, g],
                      lambda o: lib.call("dc_lpips_tail_grad", l, f.view.data_ptr(), n, hw, sides, wts.data_ptr(), g.view.data_ptr(),
                                         o.data_ptr(), stream()), r, s)


@pytest.mark.parametrize("i", range(3), ids=IDS)
def test_each_mfma_data_gradient(lib, i):
    """conv5 and conv4 with the tail gradient added and the ReLU mask of the layer below, conv3 and conv2 plain (into the pooled
    maps), fed the reference's gradient at the device's own maps"""
    c = case(i)
    convs, _ = R.params(weights())
    dw = model()._dgrad_weights(torch.device(DEV))
    ref = c["ref"]
    for layer in (4, 3, 2, 1):
        gin = ref["d_x"][layer].float()
        fused = layer >= 3
        add = ref["tail_x"][layer - 1].float() if fused else None
        mapv = c["fx"][layer - 1] if fused else None
        r, s = R.conv_dgrad_ref(gin, convs[layer][0], R.PAD[layer], add, mapv)
        ops = [guarded(gin)] + ([guarded(add), guarded(mapv)] if fused else [])
        n, _, h, w = gin.shape
        run_stage(f"conv_dgrad layer {layer}", tuple(r.shape), ops,
                  lambda o: lib.call("dc_lpips_conv_dgrad", layer, ops[0].view.data_ptr(), n, h, w, dw.data_ptr(),
                                     ops[1].view.data_ptr() if fused else None, ops[2].view.data_ptr() if fused else None, o.data_ptr(),
                                     stream()), r, s)


@pytest.mark.parametrize("i", range(3), ids=IDS)
def test_both_pool_gradients(lib, i):
    c = case(i)
    ref = c["ref"]
    for l in (1, 0):
        gp, mapv, add = ref["pool_x"][l].float(), c["fx"][l], ref["tail_x"][l].float()
        r, s = R.pool_grad_ref(gp, mapv, add)
        ops = [guarded(gp), guarded(mapv), guarded(add)]
        n, ch, h, w = mapv.shape
        out = run_stage(f"pool_grad relu{l + 1}", tuple(r.shape), ops,
                        lambda o: lib.call("dc_lpips_pool_grad", ops[0].view.data_ptr(), ops[1].view.data_ptr(), ops[2].view.data_ptr(),
                                           n * ch, h, w, o.data_ptr(), stream()), r, s)
        if (h - 3) % 2:                                              # the last row lies in no window: the tail gradient alone
            assert torch.equal(out[:, :, h - 1].cpu(), (add * (mapv > 0))[:, :, h - 1])
    if i == 2:
        assert tuple(c["fx"][0].shape[2:]) == (16, 35)
    # the tie rule: a constant window sends its gradient to element 0
    ones, two = guarded(torch.ones(1, 1, 3, 3)), guarded(torch.full((1, 1, 1, 1), 2.0))
    want = torch.zeros(1, 1, 3, 3, dtype=F64)
    want[0, 0, 0, 0] = 2.0
    run_stage("pool_grad constant window", (1, 1, 3, 3), [ones, two],
              lambda o: lib.call("dc_lpips_pool_grad", two.view.data_ptr(), ones.view.data_ptr(), None, 1, 3, 3, o.data_ptr(), stream()),
              want, torch.zeros_like(want))


@pytest.mark.parametrize("i", range(3), ids=IDS)
def test_conv1_data_gradient(lib, i):
    c = case(i)
    convs, _ = R.params(weights())
    wts = model()._weights(torch.device(DEV))
    n, (h, w) = c["n"], c["hw"]
    gin = torch.cat([c["ref"]["d_x"][0], c["ref"]["d_y"][0]]).float()
    r, s = R.conv1_dgrad_ref(gin, convs[0][0], (h, w))
    op = guarded(gin)
    dy = E.Guarded((n, 3, h, w), F32, DEV)
    out = run_stage("conv1_dgrad", (n, 3, h, w), [op],
                    lambda o: lib.call("dc_lpips_conv1_dgrad", op.view.data_ptr(), 2 * n, n, h, w, 0, wts.data_ptr(), o.data_ptr(),
                                       dy.view.data_ptr(), stream()), r[:n], s[:n])
    dy.assert_intact("conv1_dgrad second output")
    assert dy.unwritten() == 0
    assert L.check(dy.view.cpu(), r[n:], s[n:], F32)["ok"]
    if (h + 4 - 11) % 4:                                             # rows and columns no window reaches: exactly 0
        assert float(out[:, :, h - 1].abs().max()) == 0 and float(out[:, :, :, w - 1].abs().max()) == 0 and (h, w) == (70, 146)
    two = E.Guarded((2 * n, 3, h, w), F32, DEV)                      # normalize: the factor 2, all images to the first output
    lib.call("dc_lpips_conv1_dgrad", op.view.data_ptr(), 2 * n, 2 * n, h, w, 1, wts.data_ptr(), two.view.data_ptr(), None, stream())
    r2, s2 = R.conv1_dgrad_ref(gin, convs[0][0], (h, w), normalize=True)
    assert L.check(two.view.cpu(), r2, s2, F32)["ok"] and not two.bad() and two.unwritten() == 0


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("i", range(3), ids=IDS)
def test_gradient_to_each_side_and_to_both_is_within_the_bar(lib, i):
    c = case(i)
    n, h, w = R.SHAPES[i]
    bar = BARS[(n, h, w)]
    m = model()
    ref = c["ref"]
    _, gx = grads(m, c["x"], c["y"], c["g"], "x")
    _, gy = grads(m, c["x"], c["y"], c["g"], "y")
    _, bx, by = grads(m, c["x"], c["y"], c["g"], "xy")
    fig = [R.relative_to_max(gx.cpu(), ref["dx"]), R.relative_to_max(gy.cpu(), ref["dy"]),
           max(R.relative_to_max(bx.cpu(), ref["dx"]), R.relative_to_max(by.cpu(), ref["dy"]))]
    print(f"{IDS[i]}: max|d|/max|ref| dx {fig[0]:.3e} dy {fig[1]:.3e} both {fig[2]:.3e} (bar {bar:.2e})")
    assert gx.dtype == F32 and gx.shape == c["x"].shape and bool(torch.isfinite(gx).all())
    assert max(fig) <= bar, fig
    assert torch.equal(gx, bx) and torch.equal(gy, by)               # a side's gradient does not depend on who else asks
    if (h, w) == (70, 146):
        for g in (gx, gy):
            assert float(g[:, :, 69].abs().max()) == 0 and float(g[:, :, :, 145].abs().max()) == 0
            assert float(g[:, :, 68].abs().max()) > 0 and float(g[:, :, :, 144].abs().max()) > 0


def test_normalize_gradient_is_held_to_its_own_reference(lib):
    c = case(1, normalize=True)
    _, gx, gy = grads(model(), c["x"], c["y"], c["g"], "xy", normalize=True)
    fig = max(R.relative_to_max(gx.cpu(), c["ref"]["dx"]), R.relative_to_max(gy.cpu(), c["ref"]["dy"]))
    print(f"normalize=True {IDS[1]}: {fig:.3e}")
    assert fig <= BARS[R.SHAPES[1]]
    plain = case(1)["ref"]["dx"]
    assert 1.9 < float(c["ref"]["dx"].abs().max() / plain.abs().max()) < 2.1      # the factor 2 is in the reference


def test_unweighted_form_is_held_to_unit_lin_weights(lib):
    c = case(1, lpips=False)
    val, gx = grads(model(False), c["x"], c["y"], c["g"], "x")
    fig = R.relative_to_max(gx.cpu(), c["ref"]["dx"])
    print(f"lpips=False {IDS[1]}: {fig:.3e}")
    assert fig <= BARS[R.SHAPES[1]]
    want, _, _, _ = R.lpips_loss(weights(), c["x"].cpu(), c["y"].cpu(), lpips=False)
    assert float((val.view(-1).cpu().double() - want).abs().max() / want.abs().max()) < 2e-5     # the value bar of tests/test_gpu_lpips.py


def test_per_layer_outputs_combine_their_upstream_gradients(lib):
    c = case(0)
    m = model()
    g5 = torch.linspace(-1, 1, 10).view(5, 2).to(DEV)
    xs = c["x"].clone().requires_grad_(True)
    val, layers = m(xs, c["y"], retPerLayer=True)
    loss = sum((l.view(-1) * g).sum() for l, g in zip(layers, g5)) + (val.view(-1) * c["g"]).sum()
    gx, = torch.autograd.grad(loss, xs)
    ref = R.backward_from_maps(weights(), c["fx"], c["fy"], g5.cpu().double() + c["g"].cpu().double(), c["hw"])["dx"]
    assert R.relative_to_max(gx.cpu(), ref) <= BARS[R.SHAPES[0]]
    assert len(layers) == 5 and all(l.shape == (2, 1, 1, 1) for l in layers) and val.shape == (2, 1, 1, 1)


def test_operand_forms(lib):
    """a permuted NHWC view is read in place, an fp16 operand gets an fp16 gradient, uint8 frames stay on the metric path"""
    c = case(1)
    m = model()
    _, want = grads(m, c["x"], c["y"], c["g"], "x")
    view = c["x"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).detach().requires_grad_(True)
    assert not view.is_contiguous()
    g, = torch.autograd.grad((m(view, c["y"]).view(-1) * c["g"]).sum(), view)
    assert torch.equal(g, want) and g.shape == view.shape
    xh = c["x"].half().requires_grad_(True)
    gh, = torch.autograd.grad((m(xh, c["y"].half()).view(-1) * c["g"]).sum(), xh)
    _, w16 = grads(m, c["x"].half().float(), c["y"].half().float(), c["g"], "x")
    assert gh.dtype == torch.float16 and torch.equal(gh, w16.half())
    u8 = (c["x"][:, :, :, :].permute(0, 2, 3, 1) * 127 + 128).clamp(0, 255).to(torch.uint8)
    out = m(u8, u8.clone())
    assert out.grad_fn is None and float(out.abs().max()) == 0
    with torch.no_grad():
        assert m(c["x"].clone().requires_grad_(True), c["y"]).grad_fn is None


# ------------------------------------------------------------------------------------------------ the caller-owned buffers
# (N, H, W, sides): the ragged pooled maps (16x23 -> 7x11 -> 3x5) of an odd batch for each operand and for both (M = N and 2N
# images in the backward), and the minimum size.  The stage entries (dc_lpips_tail_grad, _conv_dgrad, _pool_grad, _conv1_dgrad)
# take no workspace.
KEEP_CASES = [(3, 67, 95, 1), (3, 67, 95, 2), (3, 67, 95, 3), (1, 31, 31, 3)]


@pytest.mark.parametrize("n,h,w,sides", KEEP_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}_sides{c[3]}" for c in KEEP_CASES])
def test_keep_and_backward_on_guarded_buffers_of_any_contents(lib, record, n, h, w, sides):
    """dc_lpips_alex_keep into a guarded keep buffer of exactly dc_lpips_keep_ws_bytes, then dc_lpips_alex_backward from that
    buffer (still holding the NaN pattern wherever the forward wrote nothing) on a guarded workspace of exactly
    dc_lpips_train_ws_bytes, each under the NaN, zero and stale fills: the kept bits do not depend on the fill, the backward
    leaves them untouched, and the value and the gradients are the bits NormFixLPIPS returns through autograd"""
    m = model()
    dev = torch.device(DEV)
    wts, dwts = m._weights(dev), m._dgrad_weights(dev)
    sets = []
    for seed in (SEED + 40 + n, 977):
        x, y, g = R.loss_inputs(n, h, w, seed)
        gx, gy = guarded(x), guarded(y)
        sets.append(dict(gx=gx, gy=gy, x=gx.view, y=gy.view, g=g.to(DEV, F32)))
    s = (3 * h * w, h * w, w, 1)
    strides = (ctypes.c_longlong * 8)(*s, *s)
    ops = [c[k] for c in sets for k in ("gx", "gy")]

    def keep_launch(ws, outs, prime):
        c = sets[int(prime)]
        lib.call("dc_lpips_alex_keep", c["x"].data_ptr(), c["y"].data_ptr(), strides, n, h, w, 0, wts.data_ptr(), ws.data_ptr(),
                 outs[0].data_ptr(), stream())

    tag = f"{n}x{h}x{w} sides={sides}"
    L_ = lib.load()
    (out, kept), share = E.run_on_fills(keep_launch, L_.dc_lpips_keep_ws_bytes(n, h, w), [((6, n), F64)], f"dc_lpips_alex_keep {tag}",
                                        operands=ops, device=DEV, keep=True)
    record(f"ws_unwritten_share[dc_lpips_alex_keep {tag}]", share)
    # the backward's operands: the kept maps of each input set in guarded buffers, g [5][N] as the wrapper forms it
    keeps = []
    for c in sets:
        gk = E.Guarded(tuple(kept.shape), F32, DEV)
        if c is sets[0]:
            gk.view.copy_(kept)
        else:
            lib.call("dc_lpips_alex_keep", c["x"].data_ptr(), c["y"].data_ptr(), strides, n, h, w, 0, wts.data_ptr(), gk.view.data_ptr(),
                     torch.empty(6 * n, dtype=F64, device=DEV).data_ptr(), stream())
        keeps.append(gk)
    g5 = [c["g"].view(1, n).repeat(5, 1).contiguous() for c in sets]
    before = E.ws_bits(keeps[0].view).clone()

    def backward(ws, outs, prime):
        d = iter(outs)
        dx = next(d).data_ptr() if sides & 1 else None
        dy = next(d).data_ptr() if sides & 2 else None
        lib.call("dc_lpips_alex_backward", keeps[int(prime)].view.data_ptr(), g5[int(prime)].data_ptr(), n, h, w, 0, sides, wts.data_ptr(),
                 dwts.data_ptr(), ws.data_ptr(), dx, dy, stream())

    what = f"dc_lpips_alex_backward {tag}"
    got, share = E.run_on_fills(backward, L_.dc_lpips_train_ws_bytes(n, h, w, sides), [((n, 3, h, w), F32)] * bin(sides).count("1"), what,
                                operands=keeps, device=DEV)
    record(f"ws_unwritten_share[{what}]", share)
    assert torch.equal(E.ws_bits(keeps[0].view), before), f"{what}: the backward wrote into the keep buffer"
    c = sets[0]
    val, *want = grads(m, c["x"], c["y"], c["g"], {1: "x", 2: "y", 3: "xy"}[sides])
    assert torch.equal(E.ws_bits(out.float()[5].reshape(n, 1, 1, 1)), E.ws_bits(val))
    assert len(got) == len(want) and all(torch.equal(E.ws_bits(a), E.ws_bits(b)) for a, b in zip(got, want))


# ------------------------------------------------------------------------------------------------ exactness
def test_value_under_grad_has_the_bits_of_the_metric(lib):
    from diffcodec_amd import metrics
    metric = metrics.LPIPS.from_state_dict(weights(), normfix=True).to(DEV)
    for i in range(3):
        c = case(i)
        xs = c["x"].clone().requires_grad_(True)
        val, layers = model()(xs, c["y"], retPerLayer=True)
        assert val.grad_fn is not None
        with torch.no_grad():
            want, wl = metric(c["x"], c["y"], retPerLayer=True)
        assert torch.equal(val.detach(), want) and all(torch.equal(a.detach(), b) for a, b in zip(layers, wl))


def test_equal_operands_give_a_zero_gradient_and_sides_mirror(lib):
    c = case(1)
    m = model()
    _, gx, gy = grads(m, c["x"], c["x"].clone(), c["g"], "xy")
    assert float(gx.abs().max()) == 0 and float(gy.abs().max()) == 0
    _, gy = grads(m, c["x"], c["y"], c["g"], "y")
    _, gx = grads(m, c["y"], c["x"], c["g"], "x")
    assert torch.equal(gy, gx)                                       # the y-gradient of (x, y) is the x-gradient of (y, x)


def test_pair_alone_equals_its_position_in_a_batch_of_16_run_to_run(lib):
    gen = torch.Generator().manual_seed(5)
    x = (torch.rand(16, 3, 64, 64, generator=gen) * 2 - 1).to(DEV)
    y = (torch.rand(16, 3, 64, 64, generator=gen) * 2 - 1).to(DEV)
    g = (torch.rand(16, generator=gen) - 0.5).to(DEV)
    m = model()
    val, gx, gy = grads(m, x, y, g, "xy")
    val2, gx2, gy2 = grads(m, x, y, g, "xy")
    assert torch.equal(gx, gx2) and torch.equal(gy, gy2) and torch.equal(val, val2)
    assert float(gx.abs().max()) > 0
    for i in (0, 7, 15):
        v1, a, b = grads(m, x[i:i + 1], y[i:i + 1], g[i:i + 1], "xy")
        assert torch.equal(a[0], gx[i]) and torch.equal(b[0], gy[i]) and torch.equal(v1[0], val[i])


def test_forward_and_backward_replay_from_a_graph(lib):
    c, c2 = case(1), case(1, normalize=True)                         # same shape, other values
    m = model()

    def run(a, b):
        val = m(a, b)
        return (val,) + torch.autograd.grad((val.view(-1) * c["g"]).sum(), (a, b))

    sx, sy = c["x"].clone().requires_grad_(True), c["y"].clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run(sx, sy)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(sx, sy)
    for a, b in ((c2["x"], c2["y"]), (c["x"], c["y"])):
        with torch.no_grad():
            sx.copy_(a), sy.copy_(b)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(a.clone().requires_grad_(True), b.clone().requires_grad_(True))
        for got, want in zip(captured, eager):
            assert torch.equal(got, want)


def test_dead_layer_has_a_finite_gradient_and_contributes_nothing(lib):
    """conv5 bias -1e3: relu5 is all zero, the case NormFix exists for"""
    from diffcodec_amd import losses
    sd = dict(weights())
    sd["net.slice5.10.bias"] = torch.full((256,), -1e3)
    dead = losses.NormFixLPIPS.from_state_dict(sd).to(DEV)
    c = case(1)
    xs = c["x"].clone().requires_grad_(True)
    val, layers = dead(xs, c["y"], retPerLayer=True)
    gx, = torch.autograd.grad((val.view(-1) * c["g"]).sum(), xs, retain_graph=True)
    assert bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0 and float(layers[4].detach().abs().max()) == 0
    g4, = torch.autograd.grad(layers[4].sum(), xs, allow_unused=True)
    assert g4 is not None and float(g4.abs().max()) == 0
    fx, fy = [f.cpu() for f in dead.features(c["x"])], [f.cpu() for f in dead.features(c["y"])]
    assert float(fx[4].abs().max()) == 0
    ref = R.backward_from_maps(sd, fx, fy, c["g"].cpu(), c["hw"])["dx"]
    assert R.relative_to_max(gx.cpu(), ref) <= BARS[R.SHAPES[1]]


# ------------------------------------------------------------------------------------------------ Sobel
REDUCTIONS = ("mean", "sum", "none")


def sobel_reference(shape, reduction):
    p, t = R.sobel_inputs(shape, SOBEL_SEED)
    p64, t64 = p.double().requires_grad_(True), t.double().requires_grad_(True)
    out = R.sobel_edge_loss(p64, t64, reduction)
    gen = torch.Generator().manual_seed(11)
    up = torch.rand(out.shape, generator=gen, dtype=F64) + 0.5
    gp, gt = torch.autograd.grad((out * up).sum(), (p64, t64))
    # the reference's own fp32 arithmetic on the CPU: the bar of the forward is 4 x its error, in the gradient's norm
    out32 = R.sobel_edge_loss(p, t, "none")
    ref_map = R.sobel_edge_loss(p.double(), t.double(), "none")
    fwd = 4 * float((out32.double() - ref_map).abs().max())          # absolute, per element
    return p, t, out.detach(), up, gp, gt, fwd, ref_map


@pytest.mark.parametrize("shape", SOBEL_SHAPES, ids=["x".join(map(str, s)) for s in SOBEL_SHAPES])
@pytest.mark.parametrize("reduction", REDUCTIONS)
def test_sobel_forward_and_both_gradients(lib, shape, reduction):
    from diffcodec_amd import losses
    p, t, ref, up, gp, gt, fwd_bar, ref_map = sobel_reference(shape, reduction)
    ps, ts = p.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
    out = losses.SobelEdgeLoss(reduction)(ps, ts)
    dp, dt = torch.autograd.grad((out * up.to(DEV, F32)).sum(), (ps, ts))
    assert out.dtype == F32 and out.shape == ref.shape and dp.shape == p.shape
    count = ref_map.numel()
    tol = fwd_bar * (1 if reduction != "sum" else count)              # a sum of `count` elements, each within the element bar
    err = float((out.detach().cpu().double() - ref).abs().max())
    print(f"sobel {shape} {reduction}: forward err {err:.3e} (tol {tol:.3e})")
    assert err <= tol
    if shape == (1, 1, 1, 1):                                        # gx = gy = 0 on both sides: e_p = e_t, sign(0) = 0
        assert float(dp.abs().max()) == 0 and float(dt.abs().max()) == 0 and float(gp.abs().max()) == 0 and float(out.detach().abs().max()) == 0
        return
    fig = max(R.relative_to_max(dp.cpu(), gp), R.relative_to_max(dt.cpu(), gt))
    print(f"sobel {shape} {reduction}: gradient max|d|/max|ref| {fig:.3e} (bar {SOBEL_BARS[shape]:.2e})")
    assert fig <= SOBEL_BARS[shape]
    only, = torch.autograd.grad((losses.SobelEdgeLoss(reduction)(ps, t.to(DEV)) * up.to(DEV, F32)).sum(), ps)
    assert torch.equal(only, dp)


def test_sobel_launchers_on_guarded_buffers(lib):
    shape = SOBEL_SHAPES[-1]
    n, ch, h, w = shape
    p, t = R.sobel_inputs(shape, SOBEL_SEED)
    # operands as pitched rows inside guarded allocations, read through their strides
    gp_, gt_ = E.Guarded(shape, F32, DEV, pitch=w + 3), E.Guarded(shape, F32, DEV, pitch=w + 5)
    gp_.fill(p.to(DEV)), gt_.fill(t.to(DEV))
    strides = (ctypes.c_longlong * 8)(*gp_.view.stride(), *gt_.view.stride())
    p64, t64 = p.double().requires_grad_(True), t.double().requires_grad_(True)
    ref_map = R.sobel_edge_loss(p64, t64, "none")
    up = torch.rand(shape, generator=torch.Generator().manual_seed(3)) + 0.5
    refs = torch.autograd.grad((ref_map * up.double()).sum(), (p64, t64))
    fwd_bar = 4 * float((R.sobel_edge_loss(p, t, "none").double() - ref_map).abs().max())
    omap = E.Guarded(shape, F32, DEV)
    lib.call("dc_sobel_edge_loss", gp_.view.data_ptr(), gt_.view.data_ptr(), strides, n, ch, h, w, 0, None, omap.view.data_ptr(), None, stream())
    ws = E.Guarded((lib.load().dc_sobel_edge_ws_bytes(*shape) // 8,), F64, DEV)
    acc = E.Guarded((1,), F64, DEV)
    lib.call("dc_sobel_edge_loss", gp_.view.data_ptr(), gt_.view.data_ptr(), strides, n, ch, h, w, 2, ws.view.data_ptr(), None,
             acc.view.data_ptr(), stream())
    gu = guarded(up)
    outs = []
    for side in (0, 1):
        for _ in range(2):
            o = E.Guarded(shape, F32, DEV)
            lib.call("dc_sobel_edge_grad", gp_.view.data_ptr(), gt_.view.data_ptr(), strides, n, ch, h, w, side, gu.view.data_ptr(), 1, 1.0,
                     o.view.data_ptr(), stream())
            torch.cuda.synchronize()
            o.assert_intact("sobel grad")
            assert o.unwritten() == 0
            outs.append(o.view.clone())
    for g in (gp_, gt_, omap, ws, acc, gu):
        g.assert_intact("sobel")
    assert omap.unwritten() == 0 and ws.unwritten() == 0 and acc.unwritten() == 0
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[2], outs[3])
    assert float((omap.view.cpu().double() - ref_map.detach()).abs().max()) <= fwd_bar
    assert abs(float(acc.view[0]) - float(ref_map.sum())) <= fwd_bar * ref_map.numel()
    assert R.relative_to_max(outs[0].cpu(), refs[0]) <= SOBEL_BARS[shape] and R.relative_to_max(outs[2].cpu(), refs[1]) <= SOBEL_BARS[shape]


def test_sobel_flat_and_equal_images_and_graph_replay(lib):
    from diffcodec_amd import losses
    loss = losses.SobelEdgeLoss()
    shape = SOBEL_SHAPES[3]
    p, t = (v.to(DEV) for v in R.sobel_inputs(shape, SOBEL_SEED))
    flat = torch.full(shape, -1.0, device=DEV, requires_grad=True)   # 0 after the mapping: gx = gy = 0 everywhere
    g, = torch.autograd.grad(loss(flat, t), flat)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) == 0
    same = p.clone().requires_grad_(True)
    out = loss(same, p)
    g, = torch.autograd.grad(out, same)
    assert float(out) == 0 and float(g.abs().max()) == 0
    half = p.half().requires_grad_(True)
    gh, = torch.autograd.grad(loss(half, t.half()), half)
    assert gh.dtype == torch.float16 and float(gh.float().abs().max()) > 0

    def run(a, b):
        v = loss(a, b)
        return (v,) + torch.autograd.grad(v, (a, b))

    sp, st = p.clone().requires_grad_(True), t.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run(sp, st)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(sp, st)
    for a, b in ((t, p), (p, t)):
        with torch.no_grad():
            sp.copy_(a), st.copy_(b)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(a.clone().requires_grad_(True), b.clone().requires_grad_(True))
        for got, want in zip(captured, eager):
            assert torch.equal(got, want)
