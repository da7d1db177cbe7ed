"""GPU: the backward of the fp32 extractor convolution (csrc/conv_f32_grad.hip, diffcodec_amd.train) against the fp64 restatements
and derived bounds of tests/conv_grad_ref.py.

Every case of conv_grad_ref.CASES runs with SiLU on and off and with and without a bias.  Each launcher is checked on its own,
every output element, from the operands it read (dgrad and wgrad get the device's own gz): outputs sit in guarded buffers (guards
intact, nothing unwritten), the wgrad workspace goes through edge_cases.run_on_fills at exactly its declared size, two runs give
the same bits.  Then the autograd surface: the training forward has the bits of the inference call, dx of an image does not depend
on the batch, a captured forward + backward replays to the eager bits, views and non-contiguous gradients are accepted, and two
compositions (the reference's first_pre_extractor chain; metric_net into softsplat 'soft') are held to fp64.

Measured on an MI355X, worst error over bound across the table (relative RMS at most 9.2e-7): SiLU gradient 0.41, dgrad 0.12,
dw 0.08, db 0.03; the chain 0.03 of its propagated bound; metric_net -> softsplat 1.2e-7 (feat) to 1.5e-6 (first bias) against bars
of 3.7e-7 to 3.5e-6.  Every test prints its figures (run with -s)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_grad_ref as R
import edge_cases as E
import splat_grad_ref as SG

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
VARIANTS = [(silu, bias) for silu in (False, True) for bias in (False, True)]


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
def device_inputs(case, seed, silu, bias):
    """the case's operands on the device: computed once, never changed"""
    return {k: None if v is None else v.to(DEV) for k, v in R.case_inputs(case, seed, silu, bias).items()}


def forward_z(lib, case, d):
    n, cin, h, w, cout, s = case
    ho, wo = R.out_size(h, w, s)
    z = torch.empty((n, cout, ho, wo), device=DEV, dtype=F32)
    lib.call("dc_conv3x3_nchw_f32", d["x"].data_ptr(), d["x"].stride(0), d["w"].data_ptr(), ptr(d["b"]), z.data_ptr(), n, cin, h, w, cout,
             s, 0, stream())
    return z


def held(y, ref, what):
    res = R.check(y, *ref)
    print(f"{what}: worst err/tol {res['ratio']:.3f} (err {res['err']:.3e}, tol {res['tol']:.3e}), relative rms {res['rms']:.3e}")
    assert res["ok"], (what, res)


@pytest.mark.parametrize("case", R.CASES, ids=str)
def test_every_launcher_against_fp64(lib, case):
    n, cin, h, w, cout, s = case
    ho, wo = R.out_size(h, w, s)
    nbytes = lib.load().dc_conv3x3_f32_wgrad_ws_bytes(n, cin, h, w, cout, s)
    for i, (silu, bias) in enumerate(VARIANTS):
        d = device_inputs(case, i, silu, bias)
        what = f"{case} silu={silu} bias={bias}"
        z = forward_z(lib, case, d)
        gz = d["gy"]
        if silu:
            g = E.Guarded(z.shape, F32, DEV)
            lib.call("dc_silu_grad_f32", z.data_ptr(), d["gy"].data_ptr(), g.view.data_ptr(), z.numel(), stream())
            torch.cuda.synchronize()
            g.assert_intact(what + " silu grad")
            assert g.unwritten() == 0
            held(g.view, R.silu_grad_ref(z, d["gy"]), what + " silu grad")
            gz = g.view.clone()

        runs = []
        for _ in range(2):
            g = E.Guarded((n, cin, h, w), F32, DEV)
            lib.call("dc_conv3x3_f32_dgrad", gz.data_ptr(), d["w"].data_ptr(), g.view.data_ptr(), n, cin, h, w, cout, s, stream())
            torch.cuda.synchronize()
            g.assert_intact(what + " dgrad")
            assert g.unwritten() == 0
            runs.append(g.view.clone())
        assert torch.equal(E.ws_bits(runs[0]), E.ws_bits(runs[1]))
        held(runs[0], R.dgrad_ref(gz, d["w"], h, w, s), what + " dgrad")

        other = device_inputs(case, i + 10, silu, bias)             # the prime launch: other values, same shape

        def launch(ws, outs, prime):
            src = other if prime else d
            lib.call("dc_conv3x3_f32_wgrad", src["x"].data_ptr(), src["x"].stride(0), (src["gy"] if prime else gz).data_ptr(),
                     outs[0].data_ptr(), outs[1].data_ptr() if bias else 0, ws.data_ptr(), n, cin, h, w, cout, s, stream())

        outputs = [((cout, cin, 3, 3), F32)] + ([((cout,), F32)] if bias else [])
        got, _ = E.run_on_fills(launch, nbytes, outputs, what + " wgrad")
        r_w, r_b = R.wgrad_ref(d["x"], gz, s)
        held(got[0], r_w, what + " dw")
        if bias:
            held(got[1], r_b, what + " db")


def _grads(train, d, s, silu, wrt="xwb", gy=None):
    """(y, gradients of <y, gy> w.r.t. the operands `wrt` names) through the autograd function"""
    x = d["x"].detach().clone().requires_grad_("x" in wrt)
    w = d["w"].detach().clone().requires_grad_("w" in wrt)
    b = None if d["b"] is None else d["b"].detach().clone().requires_grad_("b" in wrt)
    y = train.conv3x3_f32(x, w, b, s, silu)
    leaves = [t for t in (x, w, b) if t is not None and t.requires_grad]
    return (y.detach(),) + torch.autograd.grad(y, leaves, d["gy"] if gy is None else gy)


@pytest.mark.parametrize("case", R.CASES, ids=str)
def test_training_forward_has_the_inference_bits_and_autograd_the_launchers(lib, case):
    from diffcodec_amd import ops, train
    n, cin, h, w, cout, s = case
    for i, (silu, bias) in enumerate(VARIANTS):
        d = device_inputs(case, i, silu, bias)
        pc = ops.PackedConvF32(d["w"], d["b"], DEV)
        want = ops.conv3x3_nchw_f32(d["x"], pc, s, silu)
        y, dx, dw, *db = _grads(train, d, s, silu)
        assert torch.equal(E.ws_bits(y), E.ws_bits(want)), f"{case} silu={silu} bias={bias}"
        # the function's gradients are the launchers': same bits as calling them by hand
        z = forward_z(lib, case, d)
        gz = d["gy"]
        if silu:
            gz = torch.empty_like(z)
            lib.call("dc_silu_grad_f32", z.data_ptr(), d["gy"].data_ptr(), gz.data_ptr(), z.numel(), stream())
        hx = torch.empty_like(d["x"])
        lib.call("dc_conv3x3_f32_dgrad", gz.data_ptr(), d["w"].data_ptr(), hx.data_ptr(), n, cin, h, w, cout, s, stream())
        assert torch.equal(E.ws_bits(dx), E.ws_bits(hx))
        assert dx.is_contiguous() and dw.shape == d["w"].shape and (not bias or db[0].shape == (cout,))


@pytest.mark.parametrize("case", [(3, 3, 7, 9, 5, 1), (3, 2, 9, 6, 7, 2), (3, 40, 12, 36, 96, 1), (3, 32, 10, 34, 160, 2)], ids=str)
def test_dx_of_an_image_does_not_depend_on_the_batch(lib, case):
    from diffcodec_amd import train
    d = device_inputs(case, 3, True, True)
    _, dx = _grads(train, d, case[5], True, wrt="x")
    for k in range(case[0]):
        one = {key: (v[k:k + 1].contiguous() if key in ("x", "gy") else v) for key, v in d.items()}
        _, dk = _grads(train, one, case[5], True, wrt="x")
        assert torch.equal(E.ws_bits(dk[0]), E.ws_bits(dx[k])), (case, k)


@pytest.mark.parametrize("case", [(3, 16, 4, 130, 8, 1), (2, 64, 16, 16, 64, 2)], ids=str)
def test_captured_forward_and_backward_replay_to_the_eager_bits(lib, case):
    from diffcodec_amd import train
    s = case[5]
    a, b = device_inputs(case, 1, True, True), device_inputs(case, 2, True, True)
    st = {k: v.clone() for k, v in a.items()}

    def run():
        x, w, bb = (st[k].requires_grad_(True) for k in ("x", "w", "b"))
        y = train.conv3x3_f32(x, w, bb, s, True)
        return (y,) + torch.autograd.grad(y, [x, w, bb], st["gy"])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for src in (b, a):
        with torch.no_grad():
            for k in st:
                st[k].copy_(src[k])
        graph.replay()
        torch.cuda.synchronize()
        eager = _grads(train, src, s, True)
        for got, want in zip(captured, eager):
            assert torch.equal(E.ws_bits(got), E.ws_bits(want))


def test_channel_slice_view_and_noncontiguous_gy(lib):
    from diffcodec_amd import train
    case = R.SLICE_CASE
    d = device_inputs(case, 2, True, True)
    dense = _grads(train, d, case[5], True)
    wide = torch.randn((case[0], case[1] + 9, case[2], case[3]), device=DEV)
    wide[:, 5:5 + case[1]] = d["x"]
    wide.requires_grad_(True)
    view = wide[:, 5:5 + case[1]]
    assert not view.is_contiguous()
    w, b = d["w"].clone().requires_grad_(True), d["b"].clone().requires_grad_(True)
    y = train.conv3x3_f32(view, w, b, case[5], True)
    gw, gwt, gb = torch.autograd.grad(y, [wide, w, b], d["gy"])
    assert torch.equal(E.ws_bits(y.detach()), E.ws_bits(dense[0]))
    assert torch.equal(E.ws_bits(gw[:, 5:5 + case[1]]), E.ws_bits(dense[1])) and float(gw[:, :5].abs().max()) == 0
    assert torch.equal(E.ws_bits(gwt), E.ws_bits(dense[2])) and torch.equal(E.ws_bits(gb), E.ws_bits(dense[3]))

    case = R.NONCONTIGUOUS_GY_CASE
    d = device_inputs(case, 2, False, True)
    dense = _grads(train, d, case[5], False)
    gy = d["gy"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not gy.is_contiguous() and torch.equal(gy, d["gy"])
    got = _grads(train, d, case[5], False, gy=gy)
    for p, q in zip(got, dense):
        assert torch.equal(E.ws_bits(p), E.ws_bits(q))


def test_only_the_wanted_gradients_are_launched(lib, monkeypatch):
    from diffcodec_amd import train
    case = (3, 3, 7, 9, 5, 1)
    d = device_inputs(case, 0, True, True)
    calls = []
    real = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    for wrt, want in (("x", {"dc_silu_grad_f32", "dc_conv3x3_f32_dgrad"}), ("w", {"dc_silu_grad_f32", "dc_conv3x3_f32_wgrad"}),
                      ("b", {"dc_silu_grad_f32", "dc_conv3x3_f32_wgrad"}), ("xwb", {"dc_silu_grad_f32", "dc_conv3x3_f32_dgrad", "dc_conv3x3_f32_wgrad"})):
        del calls[:]
        got = _grads(train, d, 1, True, wrt=wrt)
        assert len(got) == 1 + len(wrt)
        assert set(calls) - {"dc_conv3x3_nchw_f32", "dc_silu_f32"} == want, (wrt, calls)
    del calls[:]
    _grads(train, d, 1, False, wrt="x")
    assert calls == ["dc_conv3x3_nchw_f32", "dc_conv3x3_f32_dgrad"]


def test_autocast_double_backward_and_refusals(lib):
    from diffcodec_amd import train
    case = (3, 3, 7, 9, 5, 1)
    d = device_inputs(case, 0, True, True)
    want = _grads(train, d, 1, True)
    x = d["x"].clone().requires_grad_(True)
    w = d["w"].clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = train.conv3x3_f32(x, w, d["b"], 1, True)
    assert y.dtype == F32 and torch.equal(E.ws_bits(y.detach()), E.ws_bits(want[0]))
    dx, dw = torch.autograd.grad(y, [x, w], d["gy"])
    assert torch.equal(E.ws_bits(dx), E.ws_bits(want[1])) and torch.equal(E.ws_bits(dw), E.ws_bits(want[2]))
    y = train.conv3x3_f32(x, w, d["b"], 1, True)
    (g,) = torch.autograd.grad(y, [x], d["gy"], create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    with pytest.raises(RuntimeError):
        train.conv3x3_f32(d["x"].cpu(), d["w"], None)
    with pytest.raises(ValueError):
        train.conv3x3_f32(d["x"].double(), d["w"].double(), None)
    with pytest.raises(ValueError):
        train.conv3x3_f32(d["x"], d["w"], None, stride=3)
    with pytest.raises(ValueError):
        train.conv3x3_f32(d["x"], d["w"][:, :2], None)


# ------------------------------------------------------------------------------------------ compositions
def test_first_pre_extractor_chain_against_fp64(lib):
    """five convs (strides 1, 2, 1, 2, 1, SiLU after each) built from train.Conv3x3 at 20 x 24: the gradients of a seeded linear
    functional w.r.t. the input and all ten parameters, inside the chain's propagated first-order bound (conv_grad_ref.chain_ref)"""
    from diffcodec_amd import train
    torch.manual_seed(11)
    chans, strides = (3, 16, 32, 32, 64, 64), (1, 2, 1, 2, 1)
    mods = [train.Conv3x3(ci, co, s, silu=True) for ci, co, s in zip(chans[:-1], chans[1:], strides)]
    for m in mods:
        with torch.no_grad():
            m.weight.mul_(3.0)                                       # activations of order one through all five layers
            m.bias.normal_(0, 0.3)
    x = torch.randn(2, 3, 20, 24)
    c = torch.randn(2, 64, 5, 6)
    params = [(m.weight.detach().clone(), m.bias.detach().clone()) for m in mods]
    (dx, grads), (tx, tols) = R.chain_ref(x, params, strides, (True,) * 5, c)
    net = torch.nn.Sequential(*mods).to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    (net(xd) * c.to(DEV)).sum().backward()
    held(xd.grad, (dx, tx), "chain dx")
    for l, (m, (dw, db), (tw, tb)) in enumerate(zip(mods, grads, tols)):
        held(m.weight.grad, (dw, tw), f"chain layer {l} dw")
        held(m.bias.grad, (db, tb), f"chain layer {l} db")


def test_metric_net_into_softsplat_soft(lib):
    """metric = conv(16 -> 64, SiLU), conv(64 -> 1) of feat, out = softsplat(feat, flow, metric, 'soft') at 20 x 24: the gradients
    w.r.t. feat and the four metric parameters against fp64: tests/splat_grad_ref.py's splat composed
    with the restated convolution gradients.  Bar per tensor: 4 x the error of the same composition run in fp32 on the CPU, in
    splat_grad_ref.grad_norm_error's norm (max |g - ref| / max |ref|), as the end-to-end splat tests hold theirs.  The last bias is
    the exception: 'soft' does not change when a constant is added to the metric, so its gradient sum d metric cancels to (nearly)
    nothing (3e-7 of the sum of the magnitudes here) and any norm relative to its value measures noise.  It is held to the bound of
    the sum itself: the wgrad bound 2^-20 |r| + 4 * 2^-24 sqrt(K) sum |d metric|, K = N H W, plus the operand's error in
    quadrature, sqrt(K) e, e = 4 x the largest error of an element of d metric in the CPU's fp32 run of the splat."""
    from diffcodec_amd import train
    from diffcodec_amd.softsplat import softsplat
    torch.manual_seed(12)
    m1, m2 = train.Conv3x3(16, 64, 1, silu=True), train.Conv3x3(64, 1, 1)
    feat = torch.randn(2, 16, 20, 24)
    flow = torch.randn(2, 2, 20, 24) * 2.5
    G = torch.randn(2, 16, 20, 24)
    params = [(m.weight.detach().clone(), m.bias.detach().clone()) for m in (m1, m2)]

    def cpu(dtype):
        f = feat.to(dtype).requires_grad_(True)
        ps = [(w.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)) for w, b in params]
        metric = F.conv2d(F.silu(F.conv2d(f, *ps[0], padding=1)), *ps[1], padding=1)
        out = (SG.softsplat_f64 if dtype == F64 else SG.softsplat_f32)(f, flow.to(dtype), metric, "soft")
        return torch.autograd.grad((out * G.to(dtype)).sum(), [f, ps[0][0], ps[0][1], ps[1][0], ps[1][1]])

    ref, low = cpu(F64), cpu(F32)
    bars = [4 * SG.grad_norm_error(a, b) for a, b in zip(low, ref)]

    # the composed restatement: the splat's fp64 gradients, then d metric through the two restated convolutions
    d_in, _, d_metric = SG.grads(SG.softsplat_f64, feat, flow, R.conv_ref(R.conv_ref(feat, *params[0], 1, True)[1], *params[1], 1, False)[1],
                                 "soft", G, F64)
    z1, y1 = R.conv_ref(feat, *params[0], 1, True)
    (dw2, _), (db2, _) = R.wgrad_ref(y1, d_metric, 1)
    gy1, _ = R.dgrad_ref(d_metric, params[1][0], 20, 24, 1)
    gz1, _ = R.silu_grad_ref(z1, gy1)
    (dw1, _), (db1, _) = R.wgrad_ref(feat, gz1, 1)
    dfeat = d_in + R.dgrad_ref(gz1, params[0][0], 20, 24, 1)[0]
    composed = [dfeat, dw1, db1, dw2, db2]
    assert float(db2.abs()) < 1e-3 * float(d_metric.abs().sum())      # the cancellation the docstring speaks of
    metric = R.conv_ref(R.conv_ref(feat, *params[0], 1, True)[1], *params[1], 1, False)[1]
    dm32 = SG.grads(SG.softsplat_f32, feat, flow, metric, "soft", G, F32)[2]
    tol_b2 = float(R.wgrad_ref(y1, d_metric, 1)[1][1]) + d_metric.numel() ** 0.5 * 4 * float((dm32.to(F64) - d_metric).abs().max())
    for a, b in zip(composed, ref):                                  # the composition is fp64 autograd's
        assert SG.grad_norm_error(a, b) <= 1e-10

    m1, m2 = m1.to(DEV), m2.to(DEV)
    fd = feat.to(DEV).requires_grad_(True)
    out = softsplat(fd, flow.to(DEV), m2(m1(fd)), "soft")
    got = torch.autograd.grad((out * G.to(DEV)).sum(), [fd, m1.weight, m1.bias, m2.weight, m2.bias])
    for name, g, r, bar in zip(("feat", "w1", "b1", "w2", "b2"), got, composed, bars):
        err = SG.grad_norm_error(g, r)
        if name == "b2":
            err, bar = float((g.detach().cpu().to(F64) - r).abs().max()), tol_b2
        print(f"metric_net -> softsplat d{name}: {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (name, err, bar)
