"""CPU: the yardsticks of the softsplat drop-in hold each other (tests/splat_grad_ref.py), before the GPU tests hold the kernels
to them: fp64 autograd of the restated wrapper against the fp32 restatements of the two backward kernels, the restated wrapper's
forward against the C oracle, the sharpness of the bounds against four wrong kernels, and the module's argument checks."""
import pytest
import torch

import edge_cases as E
import splat_grad_ref as R
from oracle import launch_ref as L
from oracle import splat as OS

F32 = torch.float32
CASES = [(s, f) for s in E.SPLAT_SHAPES for f in E.FLOW_FAMILIES]
IDS = ["x".join(map(str, s)) + "-" + f for s, f in CASES]
MODES = ["avg", "linear", "linear-addeps", "linear-zeroeps", "linear-clipeps", "soft-addeps", "soft-zeroeps", "soft-clipeps", "avg-addeps"]


def _inputs(shape, family, seed):
    n, c, h, w = shape
    gen = torch.Generator().manual_seed(22000 + seed)
    x = torch.randn(n, c, h, w, generator=gen) + 0.3
    flow = E.splat_flow(family, n, h, w, gen)
    og = torch.randn(n, c, h, w, generator=gen)
    return x, flow, og


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_fp64_autograd_agrees_with_the_fp32_backward_restatements(i):
    shape, family = CASES[i]
    x, flow, og = _inputs(shape, family, i)
    xl, fl = x.double().requires_grad_(True), flow.double().requires_grad_(True)
    out = R.softsplat_f64(xl, fl, None, "sum")
    gin, gflow = torch.autograd.grad((out * og.double()).sum(), (xl, fl))
    # ingrad: four individually rounded terms; the autograd value is the fp64 reference of the same sum
    r, s = R.ingrad_ref(flow, og)
    assert torch.allclose(gin, r, rtol=1e-12, atol=1e-12)
    res = L.check(R.ingrad_f32(flow, og), r, s, F32)
    assert res["ok"], (IDS[i], "ingrad", res)
    r, s = R.flowgrad_ref(x, flow, og)
    assert torch.allclose(gflow, r, rtol=1e-12, atol=1e-12), (gflow - r).abs().max()
    res = L.check(R.flowgrad_f32(x, flow, og), r, s, F32)
    assert res["ok"], (IDS[i], "flowgrad", res)
    # non-finite sources: exactly zero in both
    if family == "nonfinite":
        n, c, h, w = shape
        gy, gx = torch.meshgrid(torch.arange(h, dtype=F32), torch.arange(w, dtype=F32), indexing="ij")
        bad = ~(torch.isfinite(gx + flow[:, 0]) & torch.isfinite(gy + flow[:, 1]))
        if bool(bad.any()):
            assert float(R.ingrad_f32(flow, og)[bad[:, None].expand(n, c, h, w)].abs().max()) == 0.0
            assert float(R.flowgrad_f32(x, flow, og)[bad[:, None].expand(n, 2, h, w)].abs().max()) == 0.0
            assert float(gflow[bad[:, None].expand(n, 2, h, w)].abs().max()) == 0.0


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_forward_agrees_with_the_c_oracle(i):
    """'sum' and 'soft' against oracle.splat.softsplat; the other modes against splat_sum(cat[...]) + the fp32 normaliser.  The
    oracle is fp32 with its own summation order: held with `check` to the launch_ref bounds of the same sums (splat_sum_ref,
    splat_soft_ref, and their form for a general quotient, splat_grad_ref.quotient_ref)."""
    shape, family = CASES[i]
    n, c, h, w = shape
    x, flow, _ = _inputs(shape, family, i)
    metric = R.metric_family("positive", n, h, w, i)
    r, s, _ = L.splat_sum_ref(x, flow)
    assert torch.allclose(R.softsplat_f64(x, flow, None, "sum"), r, rtol=1e-12, atol=1e-12)
    assert L.check(OS.softsplat(x, flow, None, "sum"), R.softsplat_f64(x, flow, None, "sum"), s, F32)["ok"]
    r, s, _ = L.splat_soft_ref(x, flow, metric)
    got = R.softsplat_f64(x, flow, metric, "soft")
    assert torch.allclose(got, r, rtol=1e-9, atol=1e-12)
    assert L.check(OS.softsplat(x, flow, metric, "soft"), got, s, F32)["ok"]
    for mode in MODES:
        base, eps = (mode.split("-") + ["addeps"])[:2]
        if mode == "avg-addeps":                                   # read literally: no ones channel, the last input channel normalises
            if c < 2:
                continue
            cat, m = x, None
        else:
            m = None if base == "avg" else metric
            cat = R.cat_for(base, x, metric)
        want = R.normalise_f32(OS.splat_sum(cat, flow), eps)
        got = R.softsplat_f64(x, flow, m, mode)
        r, s = R.quotient_ref(cat, flow, eps, extra={"avg": 0, "linear": 1, "soft": 2}[base])
        if base == "avg":                                          # same planes: the two fp64 evaluations coincide
            assert torch.allclose(got, r, rtol=1e-12, atol=1e-12), (IDS[i], mode)
        res = L.check(want, got, s, F32)
        assert res["ok"], (IDS[i], mode, res)


def test_mode_strings_are_read_literally():
    x, flow, _ = _inputs((2, 3, 5, 6), "smooth", 0)
    m = R.metric_family("positive", 2, 5, 6, 0)
    # 'avg-addeps': no ones channel appended, normalised by the last input channel -> one channel fewer
    assert R.softsplat_f64(x, flow, None, "avg-addeps").shape == (2, 2, 5, 6)
    s = R.softsplat_f64(x, flow, None, "sum")
    assert torch.equal(R.softsplat_f64(x, flow, None, "avg-addeps"), s[:, :-1] / (s[:, -1:] + R.EPS))
    assert R.softsplat_f64(x, flow, None, "avg").shape == (2, 3, 5, 6)
    assert torch.equal(R.softsplat_f64(x, flow, m, "linear"), R.softsplat_f64(x, flow, m, "linear-addeps"))
    for bad in (("sum", m), ("avg", m), ("linear", None), ("soft-clipeps", None), ("mean", None)):
        with pytest.raises(ValueError):
            R.softsplat_f64(x, flow, bad[1], bad[0])


def test_bounds_are_sharp_on_the_border_family():
    """A wrong kernel fails `check`: flowgrad that drops the last channel, flips the sign of one corner's term, or uses the
    x-derivative weights for the y component; ingrad that skips the out-of-bounds test.  Inputs: the `border` family (weights
    exactly 0 or 1, landing coordinates -1, 0, W-1, W / -1, 0, H-1, H)."""
    shape = (3, 7, 7, 9)
    x, flow, og = _inputs(shape, "border", 3)
    r, s = R.flowgrad_ref(x, flow, og)
    assert L.check(R.flowgrad_f32(x, flow, og), r, s, F32)["ok"]
    assert not L.check(R.flowgrad_f32(x, flow, og, drop_last_channel=True), r, s, F32)["ok"]
    for k in range(4):
        mut = R.flowgrad_f32(x, flow, og, flip_corner=k)
        if torch.equal(mut, R.flowgrad_f32(x, flow, og)):
            continue                                   # this corner never lies inside the map with a non-zero derivative weight
        assert not L.check(mut, r, s, F32)["ok"], k
    assert not torch.equal(R.flowgrad_f32(x, flow, og, flip_corner=0), R.flowgrad_f32(x, flow, og))
    assert not L.check(R.flowgrad_f32(x, flow, og, swap_weights=True), r, s, F32)["ok"]
    r, s = R.ingrad_ref(flow, og)
    assert L.check(R.ingrad_f32(flow, og), r, s, F32)["ok"]
    assert not L.check(R.ingrad_f32(flow, og, bounds_test=False), r, s, F32)["ok"]


def test_module_refuses_cpu_tensors_and_bad_combinations():
    from diffcodec_amd.softsplat import softsplat, softsplat_func
    x, flow, _ = _inputs((1, 2, 3, 4), "smooth", 1)
    m = torch.zeros(1, 1, 3, 4)
    for mode, metric in (("sum", None), ("avg", None), ("linear", m), ("soft", m), ("soft-zeroeps", m), ("avg-addeps", None)):
        with pytest.raises(RuntimeError, match="cpu"):
            softsplat(x, flow, metric, mode)
    with pytest.raises(RuntimeError, match="cpu"):
        softsplat_func.apply(x, flow)
    for mode, metric in (("sum", m), ("avg", m), ("linear", None), ("soft", None), ("linear-zeroeps", None), ("mean", None),
                         ("", None), ("Soft", m)):
        with pytest.raises(ValueError):
            softsplat(x, flow, metric, mode)


def test_end_to_end_bars_are_the_measured_fp32_error():
    """the table next to tests/test_gpu_softsplat.py's end-to-end test is what splat_grad_ref.e2e_fp32_error measures: the error of
    the reference's own arithmetic in fp32 (within a factor of 2: the maximum moves with the libm's last bit)"""
    import test_gpu_softsplat as G
    assert sorted(G.E2E_FP32_ERROR) == sorted(R.e2e_label(c) for c in R.E2E_CASES)
    for c in R.E2E_CASES:
        for got, listed in zip(R.e2e_fp32_error(c), G.E2E_FP32_ERROR[R.e2e_label(c)]):
            assert 0.5 * listed <= got <= 2.0 * listed, (R.e2e_label(c), got, listed)
