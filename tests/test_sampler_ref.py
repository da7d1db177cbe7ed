"""CPU: the host algebra of both schedulers against the exact probability-flow ODE of a Gaussian prior (tests/sampler_ref.py,
DESIGN.md section 15).  Everything is fp64 with one set of constants, so the table in DESIGN.md is what these tests compute:
convergence orders of UniPC on a uniform lambda grid, exactness on a point mass over the real schedule (infinite last h, every
warm-up / lower-order-final combination), DDIM as DPM-Solver-1, the device table against `_plan`, and four faults that the
checks have to reject."""
import math

import numpy as np
import pytest

import sampler_ref as S

MU, SD = 0.7, 0.5
X_T = np.array([-1.3, 0.2, 2.1])
GRID = (32, 64, 128, 256)
# (solver_order, corrector, lower_order_final) -> (max abs error at n = 128, at n = 256, order the theory gives): DESIGN.md section 15
TABLE = {
    (1, False, True): (9.77e-3, 4.90e-3, 1),
    (1, True, True): (3.01e-4, 7.52e-5, 2),
    (2, False, False): (8.19e-5, 2.06e-5, 2),
    (2, True, False): (5.57e-6, 6.95e-7, 3),
}
SHIPPED = (2, True, True)
SHIPPED_ERR = (1.66e-5, 4.59e-6)


def _unipc(order, n, lower_order_final=True, uniform=True):
    from diffcodec_amd.scheduler import UniPCMultistepScheduler
    s = UniPCMultistepScheduler(solver_order=order, lower_order_final=lower_order_final)
    s.set_timesteps(n)
    if uniform:
        s.sigmas = S.uniform_lambda_sigmas(n)
    return s


def _model(sigmas, mu, sd):
    return lambda x, i: S.gaussian_eps(x, *S.alpha_sigma(sigmas[i]), mu, sd)


def _truth(sigmas, mu, sd, x_t=X_T):
    return S.gaussian_flow(x_t, *S.alpha_sigma(sigmas[0]), *S.alpha_sigma(sigmas[-1]), mu, sd)


def _unipc_err(order, n, corrector=True, lower_order_final=True, uniform=True, sd=SD, mutate=None):
    s = _unipc(order, n, lower_order_final, uniform)
    with np.errstate(all="ignore"):                 # the last fault of this file divides by an rks[0] of zero
        plans = S.unipc_plans(s)
        if mutate is not None:
            plans = mutate(s, plans)
        x = S.run_plans(plans, X_T, _model(s.sigmas, MU, sd), corrector)
    return float(np.max(np.abs(x - _truth(s.sigmas, MU, sd))))


# ------------------------------------------------------------------------------------------ the checks (shared with the faults)
def _check_order_row(key, mutate=None):
    order, corrector, lof = key
    errs = [_unipc_err(order, n, corrector, lof, mutate=mutate) for n in GRID]
    p = S.observed_order(errs)[-1]
    assert abs(p - TABLE[key][2]) <= 0.1, f"solver_order {order} corrector {corrector}: observed order {p:.3f}, errors {errs}"
    return errs


def _check_shipped(mutate=None):
    errs = [_unipc_err(*SHIPPED[:1], n, SHIPPED[1], SHIPPED[2], mutate=mutate) for n in GRID]
    bare = [_unipc_err(2, n, False, False) for n in GRID]
    p = S.observed_order(errs)[-1]
    assert p >= 1.7, f"shipped configuration: observed order {p:.3f}, errors {errs}"
    assert all(e < b for e, b in zip(errs, bare)), f"shipped configuration {errs} is not below the bare order-2 predictor {bare}"
    return errs


def _check_point_mass(order, n, uniform, lower_order_final=True, mutate=None):
    e = _unipc_err(order, n, True, lower_order_final, uniform, sd=0.0, mutate=mutate)
    assert math.isfinite(e) and e <= 1e-12, f"point mass, solver_order {order}, n {n}, uniform {uniform}: error {e}"


# ------------------------------------------------------------------------------------------ 1. orders
@pytest.mark.parametrize("key", list(TABLE), ids=lambda k: f"order{k[0]}-{'corr' if k[1] else 'nocorr'}")
def test_unipc_converges_at_its_order(key):
    """A solver of order p halves its error 2^p-fold per grid doubling on a smooth problem: 1, 2, 2, 3 for (order 1), (order 1 +
    corrector), (order 2), (order 2 + corrector), within 0.1 from n = 128 -> 256; the errors are the ones DESIGN.md tabulates."""
    errs = _check_order_row(key)
    for got, want in zip(errs[-2:], TABLE[key][:2]):
        assert abs(got - want) <= 0.01 * want, (key, errs)                  # the table holds three digits


def test_unipc_shipped_configuration_converges_and_beats_the_bare_predictor():
    """solver_order 2, corrector, lower_order_final: the last step is first order with a corrector, so the observed order rises
    towards 2 from below (1.85 at n = 128 -> 256; bar 1.7), and at every n the error is below the order-2 predictor's alone."""
    errs = _check_shipped()
    for got, want in zip(errs[-2:], SHIPPED_ERR):
        assert abs(got - want) <= 0.01 * want, errs


# ------------------------------------------------------------------------------------------ 2. point mass
@pytest.mark.parametrize("order", [1, 2])
def test_unipc_is_exact_on_a_point_mass(order):
    """s = 0: every x0-prediction is mu, so the exponential integrator is exact whatever the order, the warm-up and the grid.  The
    real schedule ends at sigma 0 (h infinite: the non-finite arms of `_rhos_and_h`); n = 1, 2, 3 walk every warm-up /
    lower-order-final combination of `_plan`."""
    for n in (1, 2, 3, 10, 50):
        _check_point_mass(order, n, uniform=False)
    for n in (1, 2, 3, 10, GRID[0]):
        _check_point_mass(order, n, uniform=True)


def test_unipc_order_sequence_of_short_schedules():
    for n, want in ((1, (1,)), (2, (1, 1)), (3, (1, 2, 1)), (5, (1, 2, 2, 2, 1))):
        assert tuple(p["order"] for p in S.unipc_plans(_unipc(2, n, uniform=False))) == want
        assert tuple(p["order"] for p in S.unipc_plans(_unipc(1, n, uniform=False))) == (1,) * n
    assert tuple(p["order"] for p in S.unipc_plans(_unipc(2, 3, lower_order_final=False))) == (1, 2, 2)


# ------------------------------------------------------------------------------------------ 3. DDIM is DPM-Solver-1
def _ddim(n):
    from diffcodec_amd.scheduler import DDIMScheduler
    s = DDIMScheduler()
    s.set_timesteps(n)
    return s


def _ddim_alphas(s):
    """fp64 (a_t, a_prev) per step from the scheduler's own alphas_cumprod, by the rule of `coefficients()`."""
    ac = s.alphas_cumprod.double().numpy()
    ratio = s.num_train_timesteps // s.num_inference_steps
    out = []
    for t in s.timesteps.tolist():
        prev = t - ratio
        out.append((ac[t], ac[prev] if prev >= 0 else float(s.final_alpha_cumprod.double())))
    return np.array(out)


EPS_ROW = 2.0 ** -22           # an fp32 entry formed as sqrt(fl(1 - a)) or sqrt(a): half an ulp of the difference, halved, plus one of the root


@pytest.mark.parametrize("n", [4, 20, 50, 100, 1000])
def test_ddim_rows_are_dpm_solver_1(n):
    """Every row of `DDIMScheduler.coefficients()` against the fp64 value of the same expression (relative 2^-22), and the update
    the row encodes, x' = (sqrt(a_p)/sqrt(a_t)) x + (sqrt(1-a_p) - sqrt(a_p) sqrt(1-a_t)/sqrt(a_t)) eps, against the first-order
    exponential integrator in lambda = log(alpha/sigma): x' = (sigma_p/sigma_t) x - alpha_p expm1(-h) x0 with
    x0 = (x - sigma_t eps)/alpha_t.  The bound of the two coefficients is the rounding of the entries they are formed from.

    n = 1000 is the densest schedule (ratio 1: the smallest h, the strongest cancellation in the eps coefficient, and the only n
    whose last step has prev >= 0).  Leading spacing with steps_offset = 1 asks for t = 1000 .. 1 there and the table ends at 999:
    `coefficients()` raised IndexError until `set_timesteps` dropped the timestep the table does not hold, so 999 rows remain and
    the schedule starts at the last entry.  Every n chains: a row starts at the alpha the row before it lands on."""
    s = _ddim(n)
    rows = s.coefficients().double().numpy()
    a = _ddim_alphas(s)
    ts = s.timesteps.tolist()
    assert ts == (list(range(999, 0, -1)) if n == 1000 else [i * (1000 // n) + 1 for i in range(n - 1, -1, -1)])
    assert rows.shape == (len(ts), 4)
    assert np.array_equal(rows[1:, :2], rows[:-1, [3, 2]])
    a_t, a_p = a[:, 0], a[:, 1]
    want = np.stack([np.sqrt(1 - a_t), np.sqrt(a_t), np.sqrt(a_p), np.sqrt(1 - a_p)], 1)
    assert np.all(np.abs(rows - want) <= EPS_ROW * want), np.max(np.abs(rows - want) / want)
    al_t, sg_t, al_p, sg_p = want[:, 1], want[:, 0], want[:, 2], want[:, 3]
    h = (np.log(al_p) - np.log(sg_p)) - (np.log(al_t) - np.log(sg_t))
    assert np.all(h > 0)
    c_x = sg_p / sg_t - al_p * np.expm1(-h) / al_t
    c_e = al_p * np.expm1(-h) * sg_t / al_t
    got_x = rows[:, 2] / rows[:, 1]
    got_e = rows[:, 3] - rows[:, 2] * rows[:, 0] / rows[:, 1]
    assert np.all(np.abs(got_x - c_x) <= 2 * EPS_ROW * c_x), np.max(np.abs(got_x - c_x) / c_x)
    tol_e = EPS_ROW * (sg_p + 3 * al_p * sg_t / al_t)                         # one entry in the first term, three in the second
    assert np.all(np.abs(got_e - c_e) <= tol_e), np.max(np.abs(got_e - c_e) / tol_e)


@pytest.mark.parametrize("n", [4, 20, 50, 100])
def test_ddim_table_is_exact_on_a_point_mass(n):
    """s = 0 through `run_ddim_table` in fp64 with the fp32 table lands on the closed form at the alpha the last row lands on
    (1e-5: the rows' sqrt(a)^2 + sqrt(1-a)^2 is 1 only to fp32 rounding)."""
    rows = _ddim(n).coefficients().double().numpy()
    a_T, s_T, a_0, s_0 = rows[0, 1], rows[0, 0], rows[-1, 2], rows[-1, 3]
    x = S.run_ddim_table(rows, X_T, lambda x, i: S.gaussian_eps(x, rows[i, 1], rows[i, 0], MU, 0.0))
    assert np.max(np.abs(x - S.gaussian_flow(X_T, a_T, s_T, a_0, s_0, MU, 0.0))) <= 1e-5


# ------------------------------------------------------------------------------------------ 4. DDIM converges
def test_ddim_converges_at_first_order_on_its_own_schedule():
    """The SD-1.5 schedule itself (every n starts at its own first timestep and ends at final_alpha_cumprod): the error against the
    ODE falls strictly over n = 10 .. 200 and at order 0.96 (bar [0.85, 1.15]) from 100 to 200; 0.195, 0.0247 and 0.0127 at n = 10,
    100 and 200."""
    ns = (10, 20, 25, 40, 50, 100, 200)
    errs = []
    for n in ns:
        s = _ddim(n)
        rows = s.coefficients().double().numpy()
        a = _ddim_alphas(s)
        assert s.timesteps[-1] - s.num_train_timesteps // n < 0 and a[-1, 1] == float(s.final_alpha_cumprod)
        al = lambda v: (math.sqrt(v), math.sqrt(1 - v))
        x = S.run_ddim_table(rows, X_T, lambda x, i: S.gaussian_eps(x, *al(a[i, 0]), MU, SD))
        errs.append(float(np.max(np.abs(x - S.gaussian_flow(X_T, *al(a[0, 0]), *al(a[-1, 1]), MU, SD)))))
    assert all(b < a_ for a_, b in zip(errs, errs[1:])), errs
    p = math.log2(errs[-2] / errs[-1])
    assert 0.85 <= p <= 1.15, (p, errs)
    for n, want in ((10, 0.195), (100, 0.0247), (200, 0.0127)):
        assert abs(errs[ns.index(n)] - want) <= 0.01 * want, errs


# ------------------------------------------------------------------------------------------ 5. the device table
@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "schedule"])
def test_unipc_device_table_lands_where_the_plan_lands(uniform):
    """The 12-float rows of `coefficients()` (fp32 entries, applied in fp64 by the documented flags and slots) against `_plan`
    applied directly: the same end point to 1e-6 on the shipped configuration, and therefore the same distance from the ODE."""
    for n in (3, 20) + GRID[:2]:
        s = _unipc(*SHIPPED[:1], n, SHIPPED[2], uniform)
        rows = s.coefficients().numpy()
        assert rows.shape == (n, s.UNIPC_ROW) and rows.dtype == np.float32
        for sd in (SD, 0.0):
            model, truth = _model(s.sigmas, MU, sd), _truth(s.sigmas, MU, sd)
            xp = S.run_plan(s, X_T, model)
            xt = S.run_plans(S.unipc_table_plans(rows), X_T, model)
            assert np.max(np.abs(xt - xp)) <= 1e-6, (n, sd)
            assert np.max(np.abs(xt - truth)) <= np.max(np.abs(xp - truth)) + 1e-6, (n, sd)
            if sd == 0.0:
                assert np.max(np.abs(xt - truth)) <= 1e-6


# ------------------------------------------------------------------------------------------ 6. the checks reject faults
def _lam(s, i):
    a, g = S.alpha_sigma(s.sigmas[i])
    return math.log(a) - math.log(g)


def _rho_04(s, plans):
    """order-1 corrector with rhos = 0.4: the m_t term is rho B(h), the m0 term takes the rest of -alpha_t h_phi_1"""
    out = []
    for pl in plans:
        pl = dict(pl)
        if pl["corr"] is not None and pl["corr"][3] is None:
            t_x, t_m0, t_mt, _ = pl["corr"]
            pl["corr"] = (t_x, t_m0 + t_mt - 0.8 * t_mt, 0.8 * t_mt, None)
        out.append(pl)
    return out


def _swap_m(s, plans):
    """predictor reads the two x0-predictions in each other's place"""
    out = []
    for pl in plans:
        pl = dict(pl)
        c_x, c_m0, c_m1 = pl["pred"]
        if c_m1 is not None:
            pl["pred"] = (c_x, c_m1, c_m0)
        out.append(pl)
    return out


def _no_rk(s, plans):
    """D1 = m1 - m0 without its division by rks[0], in the predictor and the corrector"""
    out = []
    for i, pl in enumerate(plans):
        pl = dict(pl)
        c_x, c_m0, c_m1 = pl["pred"]
        if c_m1 is not None:
            rk = (_lam(s, i - 1) - _lam(s, i)) / (_lam(s, i + 1) - _lam(s, i))
            pl["pred"] = (c_x, c_m0 + c_m1 - c_m1 * rk, c_m1 * rk)
        if pl["corr"] is not None and pl["corr"][3] is not None:
            t_x, t_m0, t_mt, t_m1 = pl["corr"]
            rk = (_lam(s, i - 2) - _lam(s, i - 1)) / (_lam(s, i) - _lam(s, i - 1))
            pl["corr"] = (t_x, t_m0 + t_m1 - t_m1 * rk, t_mt, t_m1 * rk)
        out.append(pl)
    return out


def test_the_checks_reject_the_faults_they_exist_for():
    """Each fault is applied to the plans this test's numpy loop runs, never to the package, and the assertion the tests above
    run on the clean plans has to fail on it."""
    _check_order_row((1, True, True))
    with pytest.raises(AssertionError, match="observed order"):
        _check_order_row((1, True, True), _rho_04)
    for mutate in (_swap_m, _no_rk):
        for key in ((2, False, False), (2, True, False)):
            with pytest.raises(AssertionError, match="observed order"):
                _check_order_row(key, mutate)
        with pytest.raises(AssertionError, match="shipped configuration"):
            _check_shipped(mutate)
    # order 2 kept through the last step of the real schedule (sigma ends at 0, h is infinite): rks[0] is 0 and the D1 term 0/0
    for n in (2, 3, 10):
        _check_point_mass(2, n, uniform=False)
        with pytest.raises(AssertionError, match="point mass"):
            _check_point_mass(2, n, uniform=False, lower_order_final=False)
        e = _unipc_err(2, n, True, False, uniform=False, sd=0.0)
        assert not math.isfinite(e) or e > 1e-6
