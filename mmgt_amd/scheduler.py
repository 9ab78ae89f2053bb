"""Schedulers of the Stage-2 sampler: host-side coefficient tables only (the tensor update is a HIP kernel: mmgt_cfg_ddim_step for
deterministic DDIM, mmgt_sampler_step for DDIM with eta > 0, guidance rescale and DPM-Solver++ 2M).

Restates diffusers==0.24.0 `DDIMScheduler` (un-vendored dependency of the reference, requirements.txt:36) under the
reference's settings config/prompts/animation.yaml:80-89: linear betas 0.00085..0.012, rescale_betas_zero_snr,
v_prediction, trailing timestep spacing, clip_sample False, set_alpha_to_one True, eta = 0.

`DPMSolverMultistepScheduler` is stated from Lu et al., arXiv 2211.01095, Alg. 2 ("2M", data prediction) on the same schedule; it carries diffusers'
class name but has not been compared with diffusers.  Both classes give `update_coefficients(t, eta)`: the scalars of the one linear form that
mmgt_sampler_step evaluates,

    x0 = sa_t x - sb_t v;    x_next = k_x x + k_0 x0 + k_1 x0_prev + k_v v + k_z z.

Re-voicing an existing clip: `set_timesteps(N, strength=)` keeps the last int(N strength) steps of the trailing list (diffusers' img2img
`get_timesteps`), `alpha_bar_after(t)` is where the step leaving t lands, and `known_scalars(alpha_bar)` are the two scalars of mmgt_known_latents
that noise the known clip to that level.
"""
import math

import numpy as np
import torch


def _rescale_zero_terminal_snr(betas):
    alphas_bar_sqrt = torch.cumprod(1.0 - betas, dim=0).sqrt()
    a0 = alphas_bar_sqrt[0].clone()
    aT = alphas_bar_sqrt[-1].clone()
    alphas_bar_sqrt = (alphas_bar_sqrt - aT) * (a0 / (a0 - aT))
    alphas_bar = alphas_bar_sqrt ** 2
    alphas = torch.cat([alphas_bar[0:1], alphas_bar[1:] / alphas_bar[:-1]])
    return 1 - alphas


class DDIMScheduler:
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear",
                 clip_sample=False, set_alpha_to_one=True, steps_offset=1, prediction_type="v_prediction",
                 rescale_betas_zero_snr=True, timestep_spacing="trailing", **unused):
        if beta_schedule != "linear":
            raise NotImplementedError(f"beta_schedule {beta_schedule}")
        if timestep_spacing != "trailing" or prediction_type != "v_prediction" or clip_sample:
            raise NotImplementedError("only the reference's sampler settings are implemented (animation.yaml:80-89)")
        self.num_train_timesteps = num_train_timesteps
        betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        if rescale_betas_zero_snr:
            betas = _rescale_zero_terminal_snr(betas)
        self.betas = betas
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.final_alpha_cumprod = 1.0 if set_alpha_to_one else float(self.alphas_cumprod[0])
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))

    def set_timesteps(self, num_inference_steps, device=None, strength=1.0):
        """strength < 1 keeps the LAST min(int(N strength), N) entries of the trailing list (diffusers' img2img `get_timesteps`, its float
        truncation included): the steps a clip noised to timesteps[0] still has to take.  num_inference_steps stays N, so the kept steps are
        the ones the full schedule takes."""
        if num_inference_steps > self.num_train_timesteps:
            raise ValueError("num_inference_steps exceeds num_train_timesteps")
        if not 0.0 <= strength <= 1.0:
            raise ValueError(f"strength must lie in [0, 1], got strength={strength}")
        keep = min(int(num_inference_steps * strength), num_inference_steps)
        if keep < 1:
            raise ValueError(f"num_inference_steps={num_inference_steps} at strength={strength} leaves no step to take "
                             f"(int({num_inference_steps} * {strength}) = 0)")
        self.num_inference_steps = num_inference_steps
        ratio = self.num_train_timesteps / num_inference_steps
        ts = np.round(np.arange(self.num_train_timesteps, 0, -ratio)).astype(np.int64) - 1
        self.timesteps = torch.from_numpy(ts[max(num_inference_steps - keep, 0):].copy())
        if device is not None:
            self.timesteps = self.timesteps.to(device)

    def alpha_bar_after(self, timestep):
        """the alpha-bar on which the step leaving `timestep` lands (fp64 Python float): alphas_cumprod[t - 1000 // N]; behind the last entry of
        self.timesteps final_alpha_cumprod.  (Where 1000 // N divides the last timestep -- N = 6: 166 - 166 = 0 -- the update itself lands on
        alphas_cumprod[0] = 0.9991, the reference's quirk; what is kept of a known clip ends as the clip, not with 3 % of noise on it.)"""
        if int(timestep) == int(self.timesteps[-1]):
            return float(self.final_alpha_cumprod)
        return self._alpha_bar(int(timestep) - self.num_train_timesteps // self.num_inference_steps)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step_coefficients(self, timestep):
        """(sqrt(abar_t), sqrt(1 - abar_t), sqrt(abar_prev), sqrt(1 - abar_prev)) as fp32-rounded Python floats."""
        t = int(timestep)
        prev = t - self.num_train_timesteps // self.num_inference_steps   # the reference's N=30 quirk included
        a_t = self.alphas_cumprod[t]
        a_p = self.alphas_cumprod[prev] if prev >= 0 else torch.tensor(self.final_alpha_cumprod, dtype=torch.float32)
        f = lambda x: float(x.to(torch.float32))
        return f(a_t ** 0.5), f((1 - a_t) ** 0.5), f(a_p ** 0.5), f((1 - a_p) ** 0.5)

    def _alpha_bar(self, t):
        """alphas_cumprod[t] as a Python float (fp64 from here on); final_alpha_cumprod below timestep 0"""
        return float(self.alphas_cumprod[t]) if t >= 0 else float(self.final_alpha_cumprod)

    def update_coefficients(self, timestep, eta=0.0):
        """(sa_t, sb_t, k_x, k_0, k_1, k_v, k_z) of the step that leaves `timestep`, computed in fp64 and rounded to fp32 (Python floats):
            sigma = eta sqrt((1 - a_s) / (1 - a_t)) sqrt(1 - a_t / a_s);     c = sqrt(max(0, 1 - a_s - sigma^2))
            x_s = sqrt(a_s) x0 + c (sqrt(a_t) v + sqrt(1 - a_t) x) + sigma z
        with s the previous timestep of `step_coefficients`.  eta = 0 is `step_coefficients`' update."""
        return _f32_tuple(ddim_coefficients(self._alpha_bar(int(timestep)),
                                            self._alpha_bar(int(timestep) - self.num_train_timesteps // self.num_inference_steps), eta))


def _f32_tuple(vals):
    return tuple(float(np.float32(v)) for v in vals)


def known_scalars(alpha_bar):
    """(sqrt(abar), sqrt(1 - abar)) as fp32-rounded Python floats: the scalars of hip.known_latents that noise a known clip to `alpha_bar`.
    abar = 0 gives exactly (0, 1) and abar = 1 exactly (1, 0), so the ends of the schedule are z's and x0's bits."""
    return _f32_tuple((math.sqrt(alpha_bar), math.sqrt(1 - alpha_bar)))


def ddim_coefficients(a_t, a_s, eta):
    """the DDIM update from alpha-bar a_t to a_s as (sa_t, sb_t, k_x, k_0, k_1, k_v, k_z), fp64"""
    al_t, sg_t, al_s = math.sqrt(a_t), math.sqrt(1 - a_t), math.sqrt(a_s)
    sigma = eta * math.sqrt((1 - a_s) / (1 - a_t)) * math.sqrt(1 - a_t / a_s)
    c = math.sqrt(max(0.0, 1 - a_s - sigma * sigma))
    return al_t, sg_t, c * sg_t, al_s, 0.0, c * al_t, sigma


def dpmpp2m_coefficients(a_prev, a_t, a_s):
    """One DPM-Solver++ 2M step (data prediction, midpoint) from alpha-bar a_t to a_s; a_prev: the alpha-bar the previous step left, None at the first
    step.  -> ((sa_t, sb_t, k_x, k_0, k_1, k_v, k_z), e, r0) in fp64; r0 is None where the step is first order:
        e = exp(-h) = alpha_t sigma_s / (sigma_t alpha_s)       (no logarithm: finite at a_t = 0, 0 at sigma_s = 0)
        first order    x_s = (sigma_s / sigma_t) x + alpha_s (1 - e) x0_t
                       -- no earlier x0; an earlier point at lambda = -inf (a_prev = 0); sigma_s = 0
        second order   r0 = (lambda_t - lambda_prev) / (lambda_s - lambda_t),    lambda = log(alpha / sigma)
                       x_s = (sigma_s / sigma_t) x - alpha_s (e - 1) x0_t - 1/2 alpha_s (e - 1) (x0_t - x0_prev) / r0"""
    al_t, sg_t, al_s, sg_s = math.sqrt(a_t), math.sqrt(1 - a_t), math.sqrt(a_s), math.sqrt(1 - a_s)
    e = al_t * sg_s / (sg_t * al_s)
    k_x, k_0, k_1, r0 = sg_s / sg_t, al_s * (1 - e), 0.0, None
    if a_prev is not None and a_prev > 0.0 and sg_s > 0.0:
        lam = lambda a: math.log(math.sqrt(a) / math.sqrt(1 - a))
        r0 = (lam(a_t) - lam(a_prev)) / (lam(a_s) - lam(a_t))
        k_1 = -k_0 / (2 * r0)
        k_0 = k_0 - k_1
    return (al_t, sg_t, k_x, k_0, k_1, 0.0, 0.0), e, r0


class DPMSolverMultistepScheduler(DDIMScheduler):
    """DPM-Solver++ 2M on DDIMScheduler's schedule: the same betas, zero-terminal-SNR rescale, trailing `set_timesteps`, `scale_model_input`,
    `init_noise_sigma` and `order`.  Step i goes from timesteps[i] to timesteps[i + 1] (not DDIM's t - 1000 // N), the last one to
    final_alpha_cumprod.  Deterministic: eta is refused."""

    def __init__(self, *args, algorithm_type="dpmsolver++", solver_order=2, solver_type="midpoint", **kwargs):
        if algorithm_type != "dpmsolver++" or solver_order != 2 or solver_type != "midpoint":
            raise NotImplementedError(f"DPMSolverMultistepScheduler builds dpmsolver++ / order 2 / midpoint only, got {algorithm_type} / "
                                      f"{solver_order} / {solver_type}")
        super().__init__(*args, **kwargs)

    def step_coefficients(self, timestep):
        raise NotImplementedError("step_coefficients is DDIM's update; DPMSolverMultistepScheduler gives update_coefficients")

    def step_details(self, timestep):
        """(coefficients in fp64, e, r0) of the step that leaves `timestep` (a member of self.timesteps)"""
        ts = [int(t) for t in self.timesteps]
        i = ts.index(int(timestep))
        a_prev = self._alpha_bar(ts[i - 1]) if i > 0 else None
        return dpmpp2m_coefficients(a_prev, self._alpha_bar(ts[i]), self._alpha_bar(ts[i + 1] if i + 1 < len(ts) else -1))

    def alpha_bar_after(self, timestep):
        """the alpha-bar of the next entry of self.timesteps, final_alpha_cumprod behind the last"""
        ts = [int(t) for t in self.timesteps]
        i = ts.index(int(timestep))
        return self._alpha_bar(ts[i + 1] if i + 1 < len(ts) else -1)

    def update_coefficients(self, timestep, eta=0.0):
        """(sa_t, sb_t, k_x, k_0, k_1, k_v, k_z) as fp32-rounded Python floats; k_1 != 0 marks a second-order step, which reads the x0 of the
        step before."""
        if eta != 0.0:
            raise ValueError(f"DPMSolverMultistepScheduler is deterministic: eta = {eta} is not an argument of its update")
        return _f32_tuple(self.step_details(timestep)[0])


SAMPLERS = {"ddim": DDIMScheduler, "dpmpp2m": DPMSolverMultistepScheduler}


def with_sampler(scheduler, name):
    """`scheduler`'s schedule (its tables and settings as they stand) under the update rule SAMPLERS[name]: the scripts' --sampler"""
    cls = SAMPLERS[name]
    if type(scheduler) is cls:
        return scheduler
    new = cls.__new__(cls)
    new.__dict__.update(vars(scheduler))
    return new
