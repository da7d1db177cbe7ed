"""CPU: the fp64 restatements of tests/conv_grad_ref.py equal fp64 autograd of F.conv2d (+ F.silu) on every table case, and their
bounds are sharp: torch's own fp32 autograd passes them on each case's inputs and every planted fault fails them."""
import pytest
import torch
import torch.nn.functional as F

import conv_grad_ref as R

F64 = torch.float64
VARIANTS = [(silu, bias) for silu in (False, True) for bias in (False, True)]


def _autograd(case, inp, silu, dtype):
    """torch autograd of F.conv2d (+ F.silu) in `dtype` -> dict(z, gz, dx, dw, db)"""
    s = case[5]
    x = inp["x"].to(dtype).requires_grad_()
    w = inp["w"].to(dtype).requires_grad_()
    b = None if inp["b"] is None else inp["b"].to(dtype).requires_grad_()
    z = F.conv2d(x, w, b, stride=s, padding=1)
    z.retain_grad()
    y = F.silu(z) if silu else z
    y.backward(inp["gy"].to(dtype))
    return dict(z=z.detach(), gz=z.grad, dx=x.grad, dw=w.grad, db=None if b is None else b.grad)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("case", R.CASES, ids=str)
def test_restatements_equal_fp64_autograd(case):
    for i, (silu, bias) in enumerate(VARIANTS):
        inp = R.case_inputs(case, i, silu, bias)
        a = _autograd(case, inp, silu, F64)
        z, _ = R.conv_ref(inp["x"], inp["w"], inp["b"], case[5], silu)
        assert _rel(z, a["z"]) <= 1e-12
        gz = R.silu_grad_ref(z, inp["gy"])[0] if silu else inp["gy"].to(F64)
        assert _rel(gz, a["gz"]) <= 1e-12
        assert _rel(R.dgrad_ref(gz, inp["w"], case[2], case[3], case[5])[0], a["dx"]) <= 1e-12
        (dw, _), (db, _) = R.wgrad_ref(inp["x"], gz, case[5])
        assert _rel(dw, a["dw"]) <= 1e-12
        if bias:
            assert _rel(db, a["db"]) <= 1e-12


def _trunc(t, bits=10):
    """keep `bits` mantissa bits of an fp32 tensor (truncation)"""
    return (t.contiguous().view(torch.int32) & ~((1 << (23 - bits)) - 1)).view(torch.float32)


@pytest.mark.parametrize("case", R.CASES, ids=str)
def test_bounds_pass_torch_fp32_and_reject_faults(case):
    n, cin, h, w, cout, s = case
    inp = R.case_inputs(case, 1, True, True)
    a = _autograd(case, inp, True, torch.float32)
    z, gz, x, wt = a["z"], a["gz"], inp["x"], inp["w"]
    ho, wo = R.out_size(h, w, s)
    r_s = R.silu_grad_ref(z, inp["gy"])
    r_x = R.dgrad_ref(gz, wt, h, w, s)
    r_w, r_b = R.wgrad_ref(x, gz, s)
    for name, y, ref in (("silu", gz, r_s), ("dx", a["dx"], r_x), ("dw", a["dw"], r_w), ("db", a["db"], r_b)):
        res = R.check(y, *ref)
        assert res["ok"], (name, res)
    center = [(ky, kx) for ky in range(3) for kx in range(3) if (ky, kx) != (1, 1)]
    faults = {
        "silu at 10 bits": (R.silu_grad_ref(_trunc(z), _trunc(inp["gy"]))[0], r_s),
        "dgrad at 10 bits": (R.dgrad_ref(_trunc(gz), _trunc(wt), h, w, s)[0], r_x),
        "wgrad at 10 bits": (R.wgrad_ref(_trunc(x), _trunc(gz), s)[0][0], r_w),
        "dgrad without the centre tap": (R.dgrad_ref(gz, wt, h, w, s, taps=center)[0], r_x),
        "wgrad without the centre tap": (R.wgrad_ref(x, gz, s, taps=center)[0][0], r_w),
        "dgrad without the last output channel": (R.dgrad_ref(gz, wt, h, w, s, channels=cout - 1)[0], r_x),
        "wgrad without the last pixel row": (R.wgrad_ref(x, gz, s, rows=ho - 1)[0][0], r_w),
        "db without the last image": (R.wgrad_ref(x, gz, s, images=n - 1)[1][0], r_b),
    }
    if s == 2 and h >= 2:
        faults["dgrad without the odd row phase"] = (R.dgrad_ref(gz, wt, h, w, s, drop_odd_rows=True)[0], r_x)
    for name, (y, ref) in faults.items():
        res = R.check(y.to(torch.float32), *ref)
        assert not res["ok"], (name, res)


def test_chain_restatement_and_its_bound():
    """the five-conv chain of the reference's first_pre_extractor: the restated gradients equal fp64 autograd, and torch's fp32
    autograd of the same chain passes the propagated bound"""
    torch.manual_seed(5)
    chans, strides, silus = (3, 8, 16, 16, 24, 24), (1, 2, 1, 2, 1), (True,) * 5
    x = torch.randn(2, 3, 20, 24)
    params = [(torch.randn(co, ci, 3, 3) * (1.5 / (9 * ci) ** 0.5), torch.randn(co) * 0.3) for ci, co in zip(chans[:-1], chans[1:])]
    c = torch.randn(2, 24, 5, 6)

    def run(dtype):
        xx = x.to(dtype).requires_grad_()
        ps = [(w.to(dtype).requires_grad_(), b.to(dtype).requires_grad_()) for w, b in params]
        y = xx
        for (w, b), s in zip(ps, strides):
            y = F.silu(F.conv2d(y, w, b, stride=s, padding=1))
        (y * c.to(dtype)).sum().backward()
        return xx.grad, [(w.grad, b.grad) for w, b in ps]

    (dx, grads), (tx, tols) = R.chain_ref(x, params, strides, silus, c)
    ax, ag = run(F64)
    assert _rel(dx, ax) <= 1e-12
    for (dw, db), (aw, ab) in zip(grads, ag):
        assert _rel(dw, aw) <= 1e-12 and _rel(db, ab) <= 1e-12
    fx, fg = run(torch.float32)
    assert R.check(fx, dx, tx)["ok"]
    for (dw, db), (tw, tb), (fw, fb) in zip(grads, tols, fg):
        assert R.check(fw, dw, tw)["ok"] and R.check(fb, db, tb)["ok"]
    # the propagated bound stays a bound on rounding: far below the gradients themselves
    assert float(tx.max() / dx.abs().max()) < 1e-3
