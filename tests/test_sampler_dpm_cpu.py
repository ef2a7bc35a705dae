"""CPU: the DPM-Solver++(2M) timestep grids and coefficient rows (morphablediffusion_amd/schedule.py).

The rows are checked by what they are for: a float64 numpy restatement of the update the HIP kernel (cfg_dpm_kernel) applies,
driven by DPMSolverSchedule's fp32 rows, integrates the probability-flow ODE of data whose exact noise prediction is known in
closed form -- a per-element Gaussian N(0, 0.5^2) and the two-Gaussian mixture +-1 with sigma 0.5 -- and is compared against an
RK4 solution of the same ODE in lambda = log(alpha / sigma) with 4000 steps."""
import numpy as np
import pytest

from morphablediffusion_amd.schedule import (DDIMSchedule, DPMSolverSchedule, _lambda_table, logsnr_timesteps,
                                             make_ddim_timesteps, solver_timesteps)

S20 = [999, 946, 888, 825, 757, 681, 597, 507, 413, 320, 233, 160, 103, 63, 36, 20, 11, 5, 2, 1, 0]
SD = 0.5  # standard deviation of the data Gaussian / of each mixture component


def eps_exact(kind, x, a, s):
    """E[eps | x_t = x] for x_t = a x_0 + s eps, eps ~ N(0, 1)."""
    v = a * a * SD * SD + s * s
    if kind == "gauss":
        return s * x / v
    return s * (x - a * np.tanh(x * a / v)) / v  # components N(+-a, v), equal weights


def x0_exact(kind, x, a, s):
    return (x - s * eps_exact(kind, x, a, s)) / a


def rk4_lambda(kind, x, lam0, lam1, n=4000):
    """The probability-flow ODE written for y = x / sigma: dy/dlambda = e^lambda x0(x, lambda), alpha^2 = sigmoid(2 lambda)."""
    def f(y, lam):
        a, s = np.sqrt(1.0 / (1.0 + np.exp(-2 * lam))), np.sqrt(1.0 / (1.0 + np.exp(2 * lam)))
        return np.exp(lam) * x0_exact(kind, s * y, a, s)

    s0 = np.sqrt(1.0 / (1.0 + np.exp(2 * lam0)))
    y, h = x / s0, (lam1 - lam0) / n
    for k in range(n):
        lam = lam0 + k * h
        k1 = f(y, lam)
        k2 = f(y + 0.5 * h * k1, lam + 0.5 * h)
        k3 = f(y + 0.5 * h * k2, lam + 0.5 * h)
        k4 = f(y + h * k3, lam + h)
        y = y + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    return y * np.sqrt(1.0 / (1.0 + np.exp(2 * lam1)))


def dpm_update(row, x, eps, x0_prev, noise=None):
    """float64 restatement of cfg_dpm_kernel's update, given one coefficient row."""
    s1m, sqrt_at, c_x, c_d, c_c, c_n = (float(v) for v in row)
    x0 = (x - s1m * eps) / sqrt_at
    xn = c_x * x + c_d * x0
    if c_c != 0.0:
        xn = xn + c_c * (x0 - x0_prev)
    if noise is not None:
        xn = xn + c_n * noise
    return xn, x0


def run_dpm(kind, sched, x):
    ac, _ = _lambda_table()
    x0_prev = None
    for i, t in enumerate(sched.timesteps[:-1]):
        a, s = np.sqrt(ac[t]), np.sqrt(1.0 - ac[t])
        x, x0_prev = dpm_update(sched.rows[i], x, eps_exact(kind, x, a, s), x0_prev)
    return x


def run_ddim(kind, S, x):
    """The reference's DDIM update at eta = 0 on its uniform grid, with DDIMSchedule's coefficients."""
    d = DDIMSchedule(S, 0.0)
    ac = d.alphas_cumprod.double().numpy()
    for index in range(S - 1, -1, -1):
        t = int(d.ddim_timesteps[index])
        s1m, sqrt_at, sqrt_aprev, dir_coef, _ = d.coefficients(index)
        e = eps_exact(kind, x, np.sqrt(ac[t]), np.sqrt(1.0 - ac[t]))
        x = sqrt_aprev * (x - s1m * e) / sqrt_at + dir_coef * e
    return x


_REF = {}


def err(kind, grid_t, x_final, x_T):
    """max |x - x_ref| over the samples, relative to max |x_ref|; x_ref is the RK4 solution from the grid's first timestep."""
    _, lam = _lambda_table()
    key = (kind, int(grid_t[0]), int(grid_t[-1]))
    if key not in _REF:
        _REF[key] = rk4_lambda(kind, x_T, lam[grid_t[0]], lam[grid_t[-1]])
    ref = _REF[key]
    return float(np.abs(x_final - ref).max() / np.abs(ref).max())


@pytest.fixture(scope="module")
def x_T():
    return np.random.default_rng(0).standard_normal(4096)


@pytest.mark.parametrize("S", [1, 2, 10, 20, 50, 999])
def test_logsnr_grid_is_strictly_decreasing_integers_from_999_to_0(S):
    t = logsnr_timesteps(S)
    assert t.dtype == np.int64 and len(t) == S + 1
    assert t[0] == 999 and t[-1] == 0 and (np.diff(t) < 0).all()
    assert np.array_equal(solver_timesteps(S, "logsnr"), t)


def test_logsnr_grid_of_20_steps_and_uniform_spacing():
    assert logsnr_timesteps(20).tolist() == S20
    for S in (5, 20, 50):
        u = solver_timesteps(S, "uniform")
        assert u.tolist() == np.flip(make_ddim_timesteps(S)).tolist() + [0]
    with pytest.raises(ValueError):
        logsnr_timesteps(0)
    with pytest.raises(ValueError):
        solver_timesteps(10, "quad")


def test_coefficient_rows():
    ac, lam = _lambda_table()
    for solver in ("dpmpp_2m", "dpmpp_2m_sde"):
        for order in (1, 2):
            d = DPMSolverSchedule(20, solver, order)
            assert d.rows.shape == (20, 6) and d.rows.dtype == np.float32 and np.isfinite(d.rows).all()
            t = d.timesteps
            assert np.allclose(d.rows[:, 0], np.sqrt(1 - ac[t[:-1]]), rtol=1e-6)
            assert np.allclose(d.rows[:, 1], np.sqrt(ac[t[:-1]]), rtol=1e-6)
            assert d.rows[0, 4] == 0.0  # no history on the first step
            assert (d.rows[1:, 4] != 0).all() if order == 2 else (d.rows[:, 4] == 0).all()
            assert (d.rows[:, 5] == 0).all() if solver == "dpmpp_2m" else (d.rows[:, 5] > 0).all()
    # first order on the reference grid is DDIM at eta = 0: c_x x + c_d x0 == sqrt(a_prev) x0 + sqrt(1 - a_prev) eps
    d, r = DDIMSchedule(5, 0.0), DPMSolverSchedule(5, order=1, spacing="uniform")
    x, e = np.random.default_rng(1).standard_normal((2, 64))
    for i in range(5):
        s1m, sqrt_at, sqrt_aprev, dir_coef, _ = d.coefficients(4 - i)
        want = sqrt_aprev * (x - s1m * e) / sqrt_at + dir_coef * e
        got, _ = dpm_update(r.rows[i], x, e, None)
        assert np.abs(got - want).max() < 1e-5 * np.abs(want).max()
    with pytest.raises(ValueError):
        DPMSolverSchedule(10, "dpmpp_3m")
    with pytest.raises(ValueError):
        DPMSolverSchedule(10, order=3)


@pytest.mark.parametrize("kind,bound", [("gauss", 7e-3), ("mix", 6e-3)])
def test_dpmpp_2m_on_the_logsnr_grid_is_second_order(kind, bound, x_T):
    e = {}
    for S in (10, 20):
        d = DPMSolverSchedule(S)
        e[S] = err(kind, d.timesteps, run_dpm(kind, d, x_T), x_T)
    print(f"[dpm] {kind}: err(10) = {e[10]:.3e}, err(20) = {e[20]:.3e}, ratio {e[10] / e[20]:.2f}")
    assert e[20] <= bound
    assert e[10] / e[20] >= 2.8


@pytest.mark.parametrize("kind", ["gauss", "mix"])
def test_dpmpp_2m_20_beats_ddim_50_on_the_reference_grid(kind, x_T):
    d = DPMSolverSchedule(20)
    e_dpm = err(kind, d.timesteps, run_dpm(kind, d, x_T), x_T)
    grid = solver_timesteps(50, "uniform")
    e_ddim = err(kind, grid, run_ddim(kind, 50, x_T), x_T)
    print(f"[dpm] {kind}: DPM++(2M)-20 = {e_dpm:.3e}, DDIM-50 uniform = {e_ddim:.3e}")
    assert e_ddim >= 4 * e_dpm
