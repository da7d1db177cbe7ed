"""CPU: the yardsticks of tests/pyramid_grad_ref.py are what they claim to be.  The fp64 level equals autograd of oracle/control_ref.py's
formulas on the same masks and the closed forms of include/diffcodec_pyramid_hip.h equal autograd, both to 1e-12; torch fp32 autograd
passes every bar and the stored fp32 errors are what a recomputation gives; each planted fault of the closed forms fails the bars; the
conditions on the inputs hold (mask shares, sign classes, exact zeros, no reference gradient identically zero); and the whole-module
recipe leaves no parameter gradient identically zero and an unoccluded pixel per image, level and direction."""
import pytest
import torch

import pyramid_grad_ref as R

F64 = torch.float64
SHARP_CASES = [c for c in R.CASES if c[4] in ("smooth", "nonfinite") and c[2] * c[3] >= 32]


@pytest.mark.parametrize("case", R.CASES, ids=R.label)
def test_fp64_level_and_closed_forms_equal_autograd_of_the_oracle_formulas(case):
    t = R.inputs(case)
    g64 = R.fp64_grads(case)
    oracle = R.level_grads(t[:8], t[8], F64, fn=R.level_oracle)
    closed = R.closed_form(t[:8], t[8])
    for nm, a, o, c in zip(R.GRAD_NAMES, g64, oracle, closed):
        assert R.norm_error(a, o) <= 1e-12, (nm, R.norm_error(a, o))
        assert R.norm_error(c, a) <= 1e-12, (nm, R.norm_error(c, a))
    with torch.no_grad():                                              # and the forward itself
        assert torch.equal(R.level(*t[:8]), R.level_oracle(*t[:8]))


@pytest.mark.parametrize("case", R.CASES, ids=R.label)
def test_fp32_autograd_passes_every_bar_and_the_stored_errors_are_recomputed(case):
    err = R.fp32_error(case)
    for nm, e, stored, bar in zip(R.GRAD_NAMES, err, R.CPU_FP32[case], R.BARS[case]):
        print(f"{R.label(case)} d {nm}: fp32 error {e:.3g}, stored {stored:.3g}, bar {bar:.3g}")
        assert e <= bar, (nm, e, bar)
        assert (stored == 0.0) == (e == 0.0) and stored / 1.5 <= e <= stored * 1.5, (nm, e, stored)


def test_case_table_covers_the_shapes_the_families_and_every_tile_edge():
    assert set(R.CPU_FP32) == set(R.CASES) and set(R.RESEED) <= set(R.CASES)
    for shape in ((1, 1, 1, 1), (2, 3, 1, 7), (2, 3, 7, 1), (3, 20, 5, 9), (2, 33, 17, 70), (2, 640, 8, 8), (3, 160, 16, 16)):
        assert shape in R.SHAPES
    # one pixel and one channel past a tile: 256 / slices pixels of the N * H * W, `slices` channels
    want = {1, 4, 16}
    for n, c, h, w in R.TILE_EDGE_SHAPES:
        sl = R.slices(c, h * w)
        assert (n * h * w) % (256 // sl) == 1 and n * h * w > 256 // sl, (n, c, h, w)
        assert c % sl == 1 or sl == 1, (c, sl)
        want.discard(sl)
    assert not want
    assert {R.slices(c[1], c[2] * c[3]) for c in R.CASES} == {1, 4, 16}
    assert R.slices(15, 4096) == 1 and R.slices(16, 1023) == 16 and R.slices(16, 1024) == 4


@pytest.mark.parametrize("case", R.CASES, ids=R.label)
def test_conditions_on_the_inputs_hold(case):
    assert R.conditions(case) == []
    if case[2] * case[3] >= 32:
        t = R.inputs(case)
        assert bool(((t[2] == 0) & (t[3] > 0)).any()) and bool(((t[3] == 0) & (t[2] > 0)).any())     # the gate at exactly 0 is live


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_fail_the_bars(fault):
    for case in SHARP_CASES:
        t = R.inputs(case)
        g64 = R.fp64_grads(case)
        err = [R.norm_error(a, b) for a, b in zip(R.closed_form(t[:8], t[8], fault), g64)]
        over = [nm for nm, e, bar in zip(R.GRAD_NAMES, err, R.BARS[case]) if e > bar]
        print(f"{fault} {R.label(case)}: over the bar {over}, worst {max(e / b for e, b in zip(err, R.BARS[case])):.3g} bars")
        assert over, (fault, case, err)


def test_sharp_cases_reach_every_kernel_form():
    assert len(SHARP_CASES) >= 6 and {R.slices(c[1], c[2] * c[3]) for c in SHARP_CASES} == {1, 4, 16}


@pytest.mark.parametrize("case", R.MODULE_CASES, ids=R.module_label)
def test_module_recipe_keeps_every_level_alive_and_fp32_passes_the_bars(case):
    sd, cond, flow, G = R.module_inputs(case)
    assert cond.shape[-1] == R.MODULE_SIZE == 192
    aux = R.cpu_aux(cond, flow)
    for k, a in enumerate(aux):
        for nm in ("occ_f", "occ_b"):
            free = (1 - a[nm]).flatten(1).sum(1)
            assert float(free.min()) >= 1, (k, nm, free)
    assert float(aux[3]["occ_f"].mean()) > 0.2                             # and occlusion is present where the threshold is 0.15 px
    g64 = R.module_grads(sd, cond, aux, G, F64)
    assert sorted(g64) == sorted(sd) == sorted(R.MODULE_CPU_FP32[R.module_label(case)])
    for k, g in g64.items():
        assert float(g.abs().max()) > 0, k
    g32 = R.module_grads(sd, cond, aux, G, torch.float32)
    for k in sorted(g64):
        e, stored = R.norm_error(g32[k], g64[k]), R.MODULE_CPU_FP32[R.module_label(case)][k]
        assert e <= R.module_bar(case, k) and stored / 1.5 <= e <= stored * 1.5, (k, e, stored)
    # a fresh module's zero convs would leave every upstream gradient zero: the recipe's are not
    assert all(float(sd[f"zero_convs.{i}.weight"].abs().max()) > 0 for i in range(4))
    assert all(float(sd[f"wrapper.{i}.metric_net.2.bias"].abs().max()) == 0 for i in range(4))


def test_the_gate_at_exactly_zero_next_to_a_confidence_that_is_not_positive():
    """S = 1e-6 there: each planted pixel is held against its own reference, the gate `> 0` misses every one of them"""
    t = R.gate_inputs()
    for at, cf, cb in R.GATE_PIXELS:
        assert float(t[2].reshape(-1)[at]) == cf <= 0 and float(t[3].reshape(-1)[at]) == cb <= 0 and 0.0 in (cf, cb)
        assert float(t[6].reshape(-1)[at]) == float(t[7].reshape(-1)[at]) == 0
    assert {w for w, _ in R.GATE_CHECKS} == {2, 3}
    for which, at in R.GATE_CHECKS:
        assert float(t[which].reshape(-1)[at]) == 0.0
    closed = R.gate_report(R.closed_form(t[:8], t[8]), t)
    fp32 = R.gate_report(R.level_grads(t[:8], t[8], torch.float32), t)
    fault = R.gate_report(R.closed_form(t[:8], t[8], "gate_gt"), t)
    for (which, at, e64, tol, ref), (_, _, e32, _, _), (_, _, ef, _, _) in zip(closed, fp32, fault):
        print(f"d {R.GRAD_NAMES[which]}[{at}]: reference {ref:.6g}, closed form off by {e64:.3g}, fp32 by {e32:.3g}, tol {tol:.3g}, gate > 0 by {ef:.3g}")
        assert abs(ref) > 1e5 and tol < 1e-4 * abs(ref)                      # the gate decides the value, and the check is tight
        assert e64 <= 1e-12 * abs(ref) and e32 <= tol and ef > 1e3 * tol
