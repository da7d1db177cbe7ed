"""The sampler's witness: a Gaussian prior, whose probability-flow ODE has a closed solution.

With x0 ~ N(mu, s^2) per element and x_t = alpha_t x0 + sigma_t eps, the marginal of x_t is N(alpha_t mu, alpha_t^2 s^2 + sigma_t^2),
so the optimal noise prediction is linear in x (`gaussian_eps`) and the ODE transports a point along the standard deviations of
the marginals (`gaussian_flow`).  A solver of order p run on that model must converge at order p, and with s = 0 (a point mass)
every x0-prediction is the constant mu, so every exponential-integrator solver here must be exact: neither statement leans on a
library or on this project's restatement of one.

The loops below are the ones `diffcodec_amd.scheduler` runs, written out in numpy.  They import nothing of the package; the
callers hand them a scheduler object (for `_plan` / `coefficients()`) and a `model(x, i) -> eps` of step index i."""
import numpy as np


# ------------------------------------------------------------------------------------------ the closed form
def gaussian_eps(x, alpha, sigma, mu, s):
    """E[eps | x_t = x] for x0 ~ N(mu, s^2): sigma (x - alpha mu) / (alpha^2 s^2 + sigma^2), in fp64."""
    x, mu = np.asarray(x, np.float64), np.asarray(mu, np.float64)
    alpha, sigma, s = float(alpha), float(sigma), float(s)
    return sigma * (x - alpha * mu) / (alpha * alpha * s * s + sigma * sigma)


def gaussian_flow(x_T, alpha_T, sigma_T, alpha, sigma, mu, s):
    """The probability-flow ODE solution at (alpha, sigma) of the point that is x_T at (alpha_T, sigma_T), in fp64:
    alpha mu + (x_T - alpha_T mu) sqrt((alpha^2 s^2 + sigma^2) / (alpha_T^2 s^2 + sigma_T^2))."""
    x_T, mu = np.asarray(x_T, np.float64), np.asarray(mu, np.float64)
    alpha_T, sigma_T, alpha, sigma, s = (float(v) for v in (alpha_T, sigma_T, alpha, sigma, s))
    var = alpha * alpha * s * s + sigma * sigma
    var_T = alpha_T * alpha_T * s * s + sigma_T * sigma_T
    return alpha * mu + (x_T - alpha_T * mu) * np.sqrt(var / var_T)


def alpha_sigma(sigma_edm):
    """(alpha, sigma) of the variance-preserving state the schedulers keep, from their `sigmas` entry sigma/alpha."""
    alpha = 1.0 / np.sqrt(sigma_edm * sigma_edm + 1.0)
    return alpha, sigma_edm * alpha


def uniform_lambda_sigmas(n, lo=-2.5, hi=2.5):
    """n + 1 values of sigma/alpha = exp(-lambda) on a uniform grid of lambda = log(alpha/sigma) in [lo, hi].  A test assigns the
    result to `sched.sigmas` after `set_timesteps(n)`: that attribute is the only thing `UniPCMultistepScheduler._plan` reads of
    the schedule (beside the number of timesteps).  The last entry is not zero, so the last step has a finite h."""
    return np.exp(-np.linspace(lo, hi, n + 1))


def observed_order(errs):
    """log2 of the ratios of consecutive errors (the grid doubling from one to the next)."""
    e = np.asarray(errs, np.float64)
    return np.log2(e[:-1] / e[1:])


# ------------------------------------------------------------------------------------------ UniPC
def unipc_plans(sched):
    """`sched._plan(i, prev_order, lower)` of every step, the warm-up state advanced as `UniPCMultistepScheduler.step` does."""
    plans, prev_order, lower = [], 1, 0
    for i in range(len(sched.timesteps)):
        pl = sched._plan(i, prev_order, lower)
        plans.append(pl)
        prev_order = pl["order"]
        lower = min(lower + 1, sched.solver_order)
    return plans


def unipc_table_plans(coef_rows):
    """The same list read back from the 12-float rows of `coefficients()`, slots and flags as scheduler.py documents them:
    0 ca, 1 ce, 2 flags (1 corrector, 2 corrector uses m1, 4 predictor uses m1), 3..6 corrector coefficients of
    (last, m0, m_t, m1), 7..9 predictor coefficients of (x, m_t, m1).  Entries keep their fp32 values."""
    plans = []
    for r in np.asarray(coef_rows, np.float64):
        f = int(r[2])
        corr = (r[3], r[4], r[5], r[6] if f & 2 else None) if f & 1 else None
        plans.append(dict(ca=r[0], ce=r[1], corr=corr, pred=(r[7], r[8], r[9] if f & 4 else None)))
    return plans


def run_plans(plans, x_T, model, corrector=True, dtype=np.float64, state=False):
    """Apply a list of per-step plans: x0-prediction, corrector row, rotation of the two x0-predictions, predictor row.
    dtype=np.float32 rounds every coefficient, every product and every sum to fp32 (the arithmetic the device table imposes;
    the kernel's fused multiply-adds round once per term instead of twice).  state=True returns (x, m0, m1, last) as the
    kernel's three multistep buffers hold them after the last step."""
    f = dtype
    x = np.asarray(x_T, f)
    m0 = m1 = last = np.zeros_like(x)
    for i, pl in enumerate(plans):
        eps = np.asarray(model(x, i), f)
        mt = f(pl["ca"]) * x + f(pl["ce"]) * eps
        if corrector and pl["corr"] is not None:
            t_x, t_m0, t_mt, t_m1 = pl["corr"]
            xc = f(t_x) * last + f(t_m0) * m0 + f(t_mt) * mt
            if t_m1 is not None:
                xc = xc + f(t_m1) * m1
            x = xc
        last, m1, m0 = x, m0, mt
        c_x, c_m0, c_m1 = pl["pred"]
        xn = f(c_x) * x + f(c_m0) * mt
        if c_m1 is not None:
            xn = xn + f(c_m1) * m1
        x = xn
        assert x.dtype == f
    return (x, m0, m1, last) if state else x


def run_plan(sched, x_T, model, corrector=True, dtype=np.float64, state=False):
    """The loop `UniPCMultistepScheduler.step` runs, driven by `sched._plan`.  corrector=False skips the corrector update and
    nothing else (the warm-up of the orders stays what `_plan` says)."""
    return run_plans(unipc_plans(sched), x_T, model, corrector, dtype, state)


# ------------------------------------------------------------------------------------------ DDIM
def run_ddim_table(coef_rows, x_T, model, dtype=np.float64):
    """The loop over `DDIMScheduler.coefficients()` rows (sqrt(1-a_t), sqrt(a_t), sqrt(a_prev), sqrt(1-a_prev)), as the kernel
    writes it: x0 = (x - sqrt(1-a_t) eps) / sqrt(a_t), then x' = sqrt(a_prev) x0 + sqrt(1-a_prev) eps."""
    f = dtype
    x = np.asarray(x_T, f)
    for i, r in enumerate(np.asarray(coef_rows, np.float64)):
        eps = np.asarray(model(x, i), f)
        x0 = (x - f(r[0]) * eps) / f(r[1])
        x = f(r[2]) * x0 + f(r[3]) * eps
        assert x.dtype == f
    return x
