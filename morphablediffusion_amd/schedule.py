"""DDPM schedule + DDIM tables on the host (pure scalar plumbing, identical arithmetic to the reference:
ldm/models/diffusion/morphable_diffusion.py:428-450 and :658-672; ldm/modules/diffusionmodules/util.py:46-60)."""
import numpy as np
import torch


def make_ddim_timesteps(num_ddim_timesteps, num_ddpm_timesteps=1000, method="uniform"):
    if method != "uniform":
        raise NotImplementedError(f'There is no ddim discretization method called "{method}"')
    c = num_ddpm_timesteps // num_ddim_timesteps
    return np.asarray(list(range(0, num_ddpm_timesteps, c))) + 1


class DDIMSchedule:
    def __init__(self, ddim_num_steps=50, ddim_eta=1.0, num_timesteps=1000, linear_start=0.00085, linear_end=0.0120):
        betas = torch.linspace(linear_start ** 0.5, linear_end ** 0.5, num_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.ddim_timesteps = make_ddim_timesteps(ddim_num_steps, num_timesteps)
        ts = torch.from_numpy(self.ddim_timesteps.astype(np.int64))
        ac = self.alphas_cumprod
        a = ac[ts].double()
        a_prev = torch.cat([ac[0:1], ac[ts[:-1]]], 0)
        sig = ddim_eta * torch.sqrt((1 - a_prev) / (1 - a) * (1 - a / a_prev))
        self.ddim_alphas = a.float()
        self.ddim_alphas_prev = a_prev.float()
        self.ddim_sigmas = sig.float()
        self.ddim_sqrt_one_minus_alphas = torch.sqrt(1.0 - self.ddim_alphas).float()
        self.eta = ddim_eta

    def coefficients(self, index):
        """(sqrt(1-a_t), sqrt(a_t), sqrt(a_prev), sqrt(clamp(1-a_prev-sigma^2, 1e-7)), sigma) as fp32 scalars,
        evaluated with the same fp32 tensor ops as denoise_apply_impl (morphable_diffusion.py:687-694)."""
        a_t = self.ddim_alphas[index]
        a_prev = self.ddim_alphas_prev[index]
        sig = self.ddim_sigmas[index]
        s1m = self.ddim_sqrt_one_minus_alphas[index]
        dir_coef = torch.clamp(1.0 - a_prev - sig ** 2, min=1e-7).sqrt()
        return (float(s1m), float(a_t.sqrt()), float(a_prev.sqrt()), float(dir_coef), float(sig))


# ---- DPM-Solver++ (Lu et al. 2022, "DPM-Solver++", Alg. 2) ------------------------------------------------------------
SOLVERS = ("dpmpp_2m", "dpmpp_2m_sde")


def _lambda_table(num_timesteps=1000):
    """lambda(t) = 1/2 log(abar_t / (1 - abar_t)) in float64, from the fp32 abar table DDIMSchedule uses."""
    ac = DDIMSchedule(1, 0.0, num_timesteps).alphas_cumprod.double().numpy()
    return ac, 0.5 * np.log(ac / (1.0 - ac))


def logsnr_timesteps(S, T=1000):
    """S + 1 strictly decreasing integer timesteps from T - 1 down to 0, uniform in lambda = log(alpha / sigma): each target
    lambda_k = lambda(T-1) + k / S (lambda(0) - lambda(T-1)) goes to the integer t of nearest lambda, the ends are pinned, and
    t_k = max(t_k, t_{k+1} + 1) from the clean end makes the grid strictly decreasing (exactly S evaluations, 1 <= S <= T - 1)."""
    if not 1 <= S <= T - 1:
        raise ValueError(f"logsnr_timesteps: need 1 <= S <= {T - 1}, got {S}")
    _, lam = _lambda_table(T)
    targets = lam[T - 1] + np.arange(S + 1) / S * (lam[0] - lam[T - 1])
    t = np.abs(lam[None, :] - targets[:, None]).argmin(1).astype(np.int64)
    t[0], t[S] = T - 1, 0
    for k in range(S - 1, -1, -1):
        t[k] = max(t[k], t[k + 1] + 1)
    return t


def solver_timesteps(S, spacing="logsnr", T=1000):
    """The S + 1 timesteps t_0 > ... > t_S = 0 a multistep solver walks.  "uniform": the reference's DDIM grid
    (make_ddim_timesteps) reversed, with the final target t = 0 -- the alphas_cumprod[0] DDIM's last a_prev uses."""
    if spacing == "logsnr":
        return logsnr_timesteps(S, T)
    if spacing == "uniform":
        return np.concatenate([np.flip(make_ddim_timesteps(S, T)), [0]]).astype(np.int64)
    raise ValueError(f"unknown timestep spacing {spacing!r}")


class DPMSolverSchedule:
    """One fp32 coefficient row per step i (t_i -> t_{i+1}), computed in float64: (s1m, sqrt_at, c_x, c_d, c_c, c_n).  With
    x0 = (x - s1m eps) / sqrt_at (the x0 prediction of DDIM) the update is

        x_{i+1} = c_x x + c_d x0 + c_c (x0 - x0_prev) + c_n z.

    alpha = sqrt(abar), sigma = sqrt(1 - abar), h_i = lambda_{i+1} - lambda_i, r_i = h_{i-1} / h_i:
      dpmpp_2m:      c_x = sigma_{i+1} / sigma_i,           c_d = -alpha_{i+1} expm1(-h_i),   c_n = 0
      dpmpp_2m_sde:  c_x = sigma_{i+1} / sigma_i e^{-h_i},  c_d = -alpha_{i+1} expm1(-2 h_i),
                     c_n = sigma_{i+1} sqrt(-expm1(-2 h_i))                                (eta = 1, midpoint form)
      c_c = c_d / (2 r_i) for order 2 and i >= 1, else 0.
    The sampler adds no noise on the last step (the reference's is_step0)."""

    def __init__(self, steps, solver="dpmpp_2m", order=2, spacing="logsnr", num_timesteps=1000):
        if solver not in SOLVERS:
            raise ValueError(f"unknown solver {solver!r} (one of {SOLVERS})")
        if order not in (1, 2):
            raise ValueError(f"order must be 1 or 2, not {order!r}")
        self.steps, self.solver, self.order, self.spacing = int(steps), solver, int(order), spacing
        self.timesteps = solver_timesteps(self.steps, spacing, num_timesteps)
        ac, lam_t = _lambda_table(num_timesteps)
        t = self.timesteps
        a, s, lam = np.sqrt(ac[t]), np.sqrt(1.0 - ac[t]), lam_t[t]
        h = np.diff(lam)
        rows = []
        for i in range(self.steps):
            if solver == "dpmpp_2m":
                c_x, c_d, c_n = s[i + 1] / s[i], -a[i + 1] * np.expm1(-h[i]), 0.0
            else:
                c_x = s[i + 1] / s[i] * np.exp(-h[i])
                c_d = -a[i + 1] * np.expm1(-2.0 * h[i])
                c_n = s[i + 1] * np.sqrt(-np.expm1(-2.0 * h[i]))
            c_c = c_d / (2.0 * (h[i - 1] / h[i])) if order == 2 and i >= 1 else 0.0
            rows.append((s[i], a[i], c_x, c_d, c_c, c_n))
        self.rows = np.asarray(rows, dtype=np.float32)

    def coefficients(self, i):
        """(s1m, sqrt_at, c_x, c_d, c_c, c_n) of step i as python floats (fp32 values)."""
        return tuple(float(v) for v in self.rows[i])


# ---- loss weighting ---------------------------------------------------------------------------------------------------
def min_snr_weights(alphas_cumprod, t, gamma):
    """Min-SNR-gamma loss weights (Hang et al. 2023, "Efficient Diffusion Training via Min-SNR Weighting Strategy") of the
    eps-prediction objective: min(SNR_t, gamma) / SNR_t with SNR = abar / (1 - abar).  1 where SNR_t <= gamma (the noisy steps),
    gamma / SNR_t < 1 on the low-noise steps that dominate a uniform-timestep mean squared error.  Computed in float64 from the
    schedule's abar table, returned as float32 on t's device."""
    gamma = float(gamma)
    if not gamma > 0.0:
        raise ValueError(f"min_snr_weights: gamma must be > 0, got {gamma!r}")
    t = torch.as_tensor(t)
    ac = torch.as_tensor(alphas_cumprod).detach().double().cpu()[t.detach().long().cpu()]
    snr = ac / (1.0 - ac)
    return (torch.clamp(snr, max=gamma) / snr).float().to(t.device)
