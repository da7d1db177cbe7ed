"""CPU: the yardsticks of tests/fdn_grad_ref.py are what they claim to be.  The fp64 restatement reproduces the golden of the
reference's own FDN module and its distance from it is the stored one; the closed forms of include/diffcodec_fdn_hip.h equal fp64
autograd to 1e-12; torch fp32 passes every bar and the stored fp32 errors are what a recomputation gives; each planted fault of the
closed forms fails the bars on the cases named here; a one-pass fp32 variance fails them where |mean| / sigma = 100; the conditions on
the inputs hold; and the whole-module recipe leaves no gradient identically zero."""
import pytest
import torch

import fdn_grad_ref as R
import pyramid_grad_ref as P
from diffcodec_amd import fdn_train as T

F64 = torch.float64
MULTI = [c for c in R.CASES if R.group_size(c) > 1]
# the cases each planted fault must fail: a fault of the divisor or of the channel range shows only with several channels per group
FAULT_CASES = {f: MULTI for f in R.FAULTS}
FAULT_CASES["m_is_hw"] = FAULT_CASES["skip_last_channel"] = [c for c in MULTI if c[1] > R.GROUPS]


def test_the_yardsticks_and_the_package_agree_on_the_constants():
    assert T.GROUPS == R.GROUPS == 32 and float(torch.tensor(T.EPS, dtype=torch.float32)) == R.EPS
    assert T.DualFlowControlLayers.SITES == R.SITES


def test_the_restatement_reproduces_the_golden_of_the_reference_module():
    sd, x, local, y = R.golden()
    ref = R.fdn_module(sd, "", x, local, F64)
    torch.testing.assert_close(ref.float(), y, rtol=1e-5, atol=1e-5)               # the bound of tests/test_oracle_golden.py
    # oracle.control_ref.fdn and this module's operator are one function of (x, gamma, beta)
    from oracle import control_ref as C
    gamma, beta = C.fdn_gamma_beta({k: v.to(F64) for k, v in sd.items()}, "", local.to(F64))
    assert R.norm_error(R.fdn(x.to(F64), gamma, beta, 1e-5), ref) <= 1e-12
    d = R.golden_distance()
    print(f"golden: distance from fp64 {d:.3g}, stored {R.GOLDEN_DISTANCE:.3g}")
    assert 0 < d and R.GOLDEN_DISTANCE / 1.5 <= d <= R.GOLDEN_DISTANCE * 1.5


@pytest.mark.parametrize("case", R.CASES, ids=R.label)
def test_closed_forms_equal_fp64_autograd(case):
    t = R.inputs(case)
    auto, closed = R.evaluate(t), R.closed_form(t)
    for nm, a, c in zip(R.TENSORS + ("g_beta",), auto, closed):
        assert R.norm_error(c, a) <= 1e-12, (nm, R.norm_error(c, a))
    assert torch.equal(auto[5], t[3].to(F64))                                      # the gradient of beta is g itself
    if t[0].numel() > R.GROUPS:                                                    # `normalize` is F.group_norm written out
        x = t[0].to(F64)
        assert R.norm_error(R.normalize(x), torch.nn.functional.group_norm(x, R.GROUPS, None, None, R.EPS)) <= 1e-12


@pytest.mark.parametrize("case", R.CASES, ids=R.label)
def test_fp32_passes_every_bar_and_the_stored_errors_are_recomputed(case):
    err = R.fp32_error(case)
    for nm, e, stored, bar in zip(R.TENSORS, err, R.CPU_FP32[case], R.BARS[case]):
        print(f"{R.label(case)} {nm}: fp32 error {e:.3g}, stored {stored:.3g}, bar {bar:.3g}")
        assert e <= bar and bar >= R.ULP, (nm, e, bar)
        assert (stored == 0.0) == (e == 0.0) and stored / 1.5 <= e <= stored * 1.5, (nm, e, stored)


def test_case_table_is_the_one_the_gpu_tests_need():
    assert set(R.CPU_FP32) == set(R.CASES) and R.BATCH_CASE in R.CASES and R.FAR_CASE in R.CASES
    shapes = {c[:4] for c in R.CASES}
    assert shapes == {(1, 32, 1, 1), (2, 32, 3, 5), (3, 64, 7, 9), (2, 96, 16, 16), (1, 320, 32, 32), (2, 1280, 8, 8)}
    m = {R.group_size(c) for c in R.CASES}
    assert m == {1, 15, 126, 768, 10240, 2560}
    assert any(v % 4 for v in m) and any(v % 4 == 0 and v > 4 * 256 for v in m) and any(1 < v < 256 for v in m)
    assert [c for c in R.CASES if c[4] == "far"] == [R.FAR_CASE] and R.BATCH_CASE[0] == 3
    assert not [c for c in R.CASES if c[:4] == (16, 320, 64, 64)]


@pytest.mark.parametrize("case", R.CASES, ids=R.label)
def test_conditions_on_the_inputs_hold(case):
    assert R.conditions(case) == []


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_fail_the_bars(fault):
    assert len(FAULT_CASES[fault]) >= 3
    for case in FAULT_CASES[fault]:
        t = R.inputs(case)
        ref = R.evaluate(t)
        err = [R.norm_error(a, b) for a, b in zip(R.closed_form(t, fault)[:5], ref[:5])]
        over = [nm for nm, e, bar in zip(R.TENSORS, err, R.BARS[case]) if e > bar]
        print(f"{fault} {R.label(case)}: over the bar {over}, worst {max(e / b for e, b in zip(err, R.BARS[case])):.3g} bars")
        assert over, (fault, case, err)


def test_one_pass_fp32_statistics_fail_where_the_mean_is_100_sigma():
    x = R.inputs(R.FAR_CASE)[0]
    mean, rstd = R.stats(x.to(F64))
    mean1, rstd1 = R.one_pass_fp32(x)
    e, bar = R.norm_error(rstd1, rstd), R.BARS[R.FAR_CASE][2]
    print(f"one-pass fp32 rstd on {R.label(R.FAR_CASE)}: error {e:.3g}, bar {bar:.3g}")
    assert e > 10 * bar
    # the two-pass form in the same fp32 passes, as does the mean either way
    mean2, rstd2 = R.stats(x)
    assert R.norm_error(rstd2, rstd) <= bar and R.norm_error(mean2, mean) <= R.BARS[R.FAR_CASE][1]


def test_module_recipe_leaves_no_gradient_zero_and_fp32_passes_the_bars():
    sd, cond, flow, samples, G = R.module_inputs()
    assert cond.shape[-1] == P.MODULE_SIZE == 192 and R.MODULE_CASE == ((64, 64, 128, 128), 2) and len(samples) == len(R.SITES) == 5
    assert [tuple(s.shape) for s in samples] == [(2, 64, 24, 24), (2, 64, 12, 12), (2, 128, 6, 6), (2, 128, 3, 3), (2, 128, 3, 3)]
    aux = P.cpu_aux(cond, flow)
    g64 = R.module_grads(sd, cond, aux, samples, G, F64)
    assert sorted(g64) == sorted(R.MODULE_CPU_FP32) == sorted(list(sd) + [f"sample.{i}" for i in range(5)])
    for k, g in g64.items():
        assert float(g.abs().max()) > 0, k
    g32 = R.module_grads(sd, cond, aux, samples, G, torch.float32)
    for k in sorted(g64):
        e, stored = R.norm_error(g32[k], g64[k]), R.MODULE_CPU_FP32[k]
        assert e <= R.module_bar(k) and stored / 1.5 <= e <= stored * 1.5, (k, e, stored)
    assert all(float(sd[f"feature_extractor.zero_convs.{i}.weight"].abs().max()) > 0 for i in range(4))


def test_module_state_dict_has_the_keys_and_shapes_of_the_weights_spec():
    """at the production widths: what DualFlowControlNet adds to ControlNetModel, by diffcodec_amd.weights.controlnet_spec"""
    from diffcodec_amd import weights
    spec = weights.controlnet_spec()
    own = {k: shape for k, (_, shape) in spec.items() if k.startswith(("feature_extractor.", "fdn"))}
    assert len(own) == 60 + 16 and {k.split(".")[0] for k in own} == {"feature_extractor"} | set(R.FDN_NAMES)
    small = {k: tuple(v.shape) for k, v in R.module_state_dict().items()}
    assert set(small) == set(own)
    assert own["fdn08.conv_gamma.weight"] == (1280, 1280, 3, 3) and small["fdn08.conv_gamma.weight"] == (128, 128, 3, 3)
