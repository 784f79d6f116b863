"""Noise schedulers with the diffusers surface the reference uses.

``DDPMScheduler`` stands where diffusion/models/models.py:88 loads ``diffusers.DDPMScheduler`` (hyper-parameters
restated in-tree at models.py:134-145); the reference touches ``len(scheduler)`` (stable_diffusion.py:177),
``add_noise`` (:180) and ``num_train_timesteps`` (:235).  ``get_velocity`` follows the use at
diffusion/models/pixel_diffusion.py:90-91; ``prediction_type='sample'`` (x0 prediction, :86-87) is the third target the
pixel models train on.  ``DDIMScheduler`` (models.py:89) carries what ``generate()`` needs
(stable_diffusion.py:354-375): ``set_timesteps``, ``timesteps``, ``init_noise_sigma``, ``scale_model_input``, ``step``.
"""
from __future__ import annotations

import math

import numpy as np
import torch

TIMESTEP_SPACINGS = ('leading', 'trailing')
# DPM-Solver++ at a table value of exactly 0 (zero terminal SNR): lambda = ln(alpha / sigma) is -inf there, so the value is
# read as 2^-24, which is what diffusers' DPMSolverMultistepScheduler stores in its own table
ZERO_SNR_ALPHA_CUMPROD = 2.0**-24


def rescale_zero_terminal_snr(betas: torch.Tensor) -> torch.Tensor:
    """Algorithm 1 of Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed" (arXiv:2305.08891), in
    diffusers' operation order on the float32 betas: shift sqrt(abar) so that its last entry is 0, scale it so that its
    first entry keeps its value, and turn the result back into betas.  abar_T comes out exactly 0 and beta_T exactly 1."""
    s = torch.cumprod(1.0 - betas, dim=0).sqrt()
    s0, sT = s[0].clone(), s[-1].clone()
    s = s - sT
    s = s * (s0 / (s0 - sT))
    abar = s**2
    alphas = torch.cat([abar[0:1], abar[1:] / abar[:-1]])
    return 1.0 - alphas


def check_timestep_spacing(spacing):
    """``timestep_spacing=`` of the inference schedulers, the factory and ``generate()``: ``ValueError`` for anything but
    the names of ``TIMESTEP_SPACINGS``."""
    if spacing not in TIMESTEP_SPACINGS:
        raise ValueError(f'timestep_spacing must be one of {TIMESTEP_SPACINGS}, got {spacing!r}')
    return spacing


def trailing_timesteps(num_train_timesteps: int, num_inference_steps: int) -> torch.Tensor:
    """round(arange(T, 0, -T / n)) - 1 with numpy's round, as diffusers: the grid starts at T - 1."""
    ts = np.round(np.arange(num_train_timesteps, 0, -num_train_timesteps / num_inference_steps)) - 1
    return torch.from_numpy(ts.astype(np.int64))


def _zero_snr_epsilon_error(t):
    return ValueError(f'zero terminal SNR: alphas_cumprod[{t}] is 0, so an epsilon prediction says nothing about the sample '
                      "there; a schedule with rescale_betas_zero_snr needs prediction_type 'v_prediction' (or 'sample'), "
                      "got prediction_type 'epsilon'")


class DDPMScheduler:
    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = 'scaled_linear', prediction_type: str = 'epsilon', clip_sample: bool = False,
                 rescale_betas_zero_snr: bool = False):
        if beta_schedule != 'scaled_linear':
            raise ValueError('SD-2 uses the scaled_linear schedule')
        self.num_train_timesteps = num_train_timesteps
        self.prediction_type = prediction_type
        self.rescale_betas_zero_snr = bool(rescale_betas_zero_snr)
        self.betas = torch.linspace(beta_start**0.5, beta_end**0.5, num_train_timesteps, dtype=torch.float32)**2
        if self.rescale_betas_zero_snr:
            self.betas = rescale_zero_terminal_snr(self.betas)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self._dev_tables = {}

    def __len__(self):
        return self.num_train_timesteps

    def device_tables(self, device):
        """(sqrt(abar), sqrt(1-abar)) fp32 tables resident on `device` for the fused add_noise kernel."""
        key = str(device)
        if key not in self._dev_tables:
            ac = self.alphas_cumprod
            self._dev_tables[key] = ((ac**0.5).to(device).contiguous(), ((1 - ac)**0.5).to(device).contiguous())
        return self._dev_tables[key]

    # host-side reference forms (used by tests / non-HIP callers; the training path uses ops.add_noise)
    def _coef(self, t, like):
        ac = self.alphas_cumprod.to(device=like.device, dtype=like.dtype)
        shape = (-1,) + (1,) * (like.dim() - 1)
        return (ac[t]**0.5).reshape(shape), ((1 - ac[t])**0.5).reshape(shape)

    def add_noise(self, original_samples, noise, timesteps):
        a, s = self._coef(timesteps, original_samples)
        return a * original_samples + s * noise

    def get_velocity(self, sample, noise, timesteps):
        a, s = self._coef(timesteps, sample)
        return a * noise - s * sample

    def add_noise_coefficients(self, timestep):
        """``add_noise`` at one timestep as two Python floats (a, s), computed in float64 from the fp32 ``alphas_cumprod``
        table: noisy = a * original + s * noise.  What ``ops.sampler_init`` and the blended sampler steps apply on the
        device to start a sample from an image and to re-noise its kept part."""
        ac = float(self.alphas_cumprod[int(timestep)])
        return math.sqrt(ac), math.sqrt(1.0 - ac)


class _InferenceGrid:
    """The timestep grid both inference schedulers walk.  ``'leading'`` (SD-2's): multiples of T // n plus ``steps_offset``,
    clamped, and a step from t goes to t - T // n.  ``'trailing'`` (``trailing_timesteps``): the grid starts at T - 1 and a
    step from grid entry i goes to entry i + 1, after the last entry to ``final_alpha_cumprod``.  For n that does not divide
    T that is not t - T // n, where diffusers' DDIM steps off its own grid; here every step lands on the next timestep the
    model is evaluated at."""

    def _grid(self, num_inference_steps: int) -> torch.Tensor:
        if self.timestep_spacing == 'trailing':
            return trailing_timesteps(self.num_train_timesteps, num_inference_steps)
        ratio = self.num_train_timesteps // num_inference_steps
        return ((torch.arange(0, num_inference_steps) * ratio).flip(0) + self.steps_offset).clamp(
            max=self.num_train_timesteps - 1)

    def _prev_timestep(self, t: int) -> int:
        """Where the step from timestep ``t`` lands; negative: past the end (``final_alpha_cumprod``)."""
        if self.timestep_spacing != 'trailing':
            return t - self.num_train_timesteps // self.num_inference_steps
        grid = self.timesteps.tolist()
        if t not in grid:
            raise ValueError(f'timestep {t} is not on the current trailing grid of {len(grid)} steps')
        i = grid.index(t)
        return int(grid[i + 1]) if i + 1 < len(grid) else -1


class DDIMScheduler(_InferenceGrid, DDPMScheduler):
    """DDIM sampler (Song et al., arXiv:2010.02502, eq. 12 and 16), ``set_alpha_to_one=False``, ``steps_offset=1`` (SD-2
    scheduler_config.json).  ``eta`` = 0 (the default) is the deterministic sampler; ``eta`` in (0, 1] adds
    sigma = eta sqrt((1 - abar_prev) / (1 - abar_t)) sqrt(1 - abar_t / abar_prev) of fresh noise per step and points the
    rest of the variance, sqrt(1 - abar_prev - sigma^2), along the predicted noise; ``eta`` = 1 is DDPM ancestral sampling."""

    def __init__(self, *a, steps_offset: int = 1, timestep_spacing: str = 'leading', eta: float = 0.0, **kw):
        super().__init__(*a, **kw)
        self.eta = check_eta(eta)
        self.steps_offset = steps_offset
        self.timestep_spacing = check_timestep_spacing(timestep_spacing)
        self.final_alpha_cumprod = self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.timesteps = torch.arange(self.num_train_timesteps - 1, -1, -1)
        self.num_inference_steps = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        ts = self._grid(num_inference_steps)
        self.timesteps = ts.to(device) if device is not None else ts

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step_coefficients(self, timestep):
        """``step`` as three Python floats (cx, cm, cn), computed in float64: prev_sample = cx * sample + cm * model_output
        (+ cn * noise, 0 for eta = 0).  The step is linear in both for each prediction type; ``prediction_type`` and
        ``num_inference_steps`` are read now, like ``step`` does.  What ``ops.sampler_step`` applies on the device."""
        t = int(timestep)
        prev_t = self._prev_timestep(t)
        ac_t = float(self.alphas_cumprod[t])
        ac_prev = float(self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod)
        if ac_t == 0.0 and self.prediction_type == 'epsilon':
            raise _zero_snr_epsilon_error(t)
        a, s, A, S = math.sqrt(ac_t), math.sqrt(1 - ac_t), math.sqrt(ac_prev), math.sqrt(1 - ac_prev)
        if self.eta != 0.0:
            # eta > 0: the same table with S' = sqrt(S^2 - sigma^2) where S stood, and cn = sigma for every prediction type
            sigma = self._sigma(ac_t, ac_prev)
            S = math.sqrt(max((1 - ac_prev) - sigma * sigma, 0.0))
            if self.prediction_type == 'v_prediction':
                return A * a + S * s, S * a - A * s, sigma
            if self.prediction_type == 'sample':
                return S / s, A - S * a / s, sigma
            return A / a, S - A * s / a, sigma
        if self.prediction_type == 'v_prediction':
            return A * a + S * s, S * a - A * s, 0.0
        if self.prediction_type == 'sample':
            return S / s, A - S * a / s, 0.0
        return A / a, S - A * s / a, 0.0

    def _sigma(self, ac_t: float, ac_prev: float) -> float:
        """eta sqrt((1 - abar_prev) / (1 - abar_t)) sqrt(1 - abar_t / abar_prev) in float64; sigma^2 <= 1 - abar_prev because
        the grid descends (abar_prev >= abar_t).  A step that goes nowhere (abar_prev == abar_t) has sigma 0."""
        if self.eta == 0.0 or ac_t == 1.0:
            return 0.0
        return self.eta * math.sqrt((1 - ac_prev) / (1 - ac_t)) * math.sqrt(max(1 - ac_t / ac_prev, 0.0))

    def step(self, model_output, timestep, sample, generator=None, variance_noise=None, **kw):
        if self.eta != 0.0:
            return self._step_eta(model_output, timestep, sample, generator, variance_noise)
        t = int(timestep)
        prev_t = self._prev_timestep(t)
        if float(self.alphas_cumprod[t]) == 0.0 and self.prediction_type == 'epsilon':
            raise _zero_snr_epsilon_error(t)
        ac_t = self.alphas_cumprod[t].to(sample.device, sample.dtype)
        ac_prev = (self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod).to(sample.device, sample.dtype)
        if self.prediction_type == 'v_prediction':
            x0 = ac_t.sqrt() * sample - (1 - ac_t).sqrt() * model_output
            eps = ac_t.sqrt() * model_output + (1 - ac_t).sqrt() * sample
        elif self.prediction_type == 'sample':   # the pixel models' x0 prediction (pixel_diffusion.py:86-87)
            x0 = model_output
            eps = (sample - ac_t.sqrt() * x0) / (1 - ac_t).sqrt()
        else:
            eps = model_output
            x0 = (sample - (1 - ac_t).sqrt() * eps) / ac_t.sqrt()
        prev = ac_prev.sqrt() * x0 + (1 - ac_prev).sqrt() * eps

        class _Out(dict):
            prev_sample = prev

        return _Out(prev_sample=prev)


    def _step_eta(self, model_output, timestep, sample, generator, variance_noise):
        """``step`` for eta > 0, the coefficients in float64 from the fp32 table: prev = A x0 + sqrt(S^2 - sigma^2) eps +
        sigma z, with z = ``variance_noise`` (diffusers' keyword), else a draw from ``generator``."""
        t = int(timestep)
        prev_t = self._prev_timestep(t)
        ac_t = float(self.alphas_cumprod[t])
        ac_prev = float(self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod)
        if ac_t == 0.0 and self.prediction_type == 'epsilon':
            raise _zero_snr_epsilon_error(t)
        a, s, A = math.sqrt(ac_t), math.sqrt(1 - ac_t), math.sqrt(ac_prev)
        sigma = self._sigma(ac_t, ac_prev)
        Sp = math.sqrt(max((1 - ac_prev) - sigma * sigma, 0.0))
        if self.prediction_type == 'v_prediction':
            x0, eps = a * sample - s * model_output, a * model_output + s * sample
        elif self.prediction_type == 'sample':
            x0, eps = model_output, (sample - a * model_output) / s
        else:
            x0, eps = (sample - s * model_output) / a, model_output
        if variance_noise is None:
            variance_noise = torch.randn(sample.shape, generator=generator, device=sample.device, dtype=sample.dtype)
        prev = A * x0 + Sp * eps + sigma * variance_noise

        class _Out(dict):
            prev_sample = prev

        return _Out(prev_sample=prev)


def check_eta(eta) -> float:
    """``eta=`` of ``DDIMScheduler``, the factories (``inference_eta``) and ``generate()``: a number in [0, 1], else
    ``ValueError``.  Host only."""
    if isinstance(eta, bool) or not isinstance(eta, (int, float)) or not 0.0 <= float(eta) <= 1.0:
        raise ValueError(f'eta must be a number in [0, 1], got {eta!r}')
    return float(eta)


def with_eta(scheduler, eta):
    """``generate(eta=...)``: ``scheduler`` itself for None or its own eta, else a shallow copy (same noise tables) with the
    other eta for this call.  ``ValueError`` for eta outside [0, 1] and for a scheduler that is not a ``DDIMScheduler``."""
    if eta is None:
        return scheduler
    eta = check_eta(eta)
    if not isinstance(scheduler, DDIMScheduler):
        raise ValueError(f'eta is the DDIM sampler\'s parameter: {type(scheduler).__name__} has none')
    if scheduler.eta == eta:
        return scheduler
    import copy
    sch = copy.copy(scheduler)
    sch.eta = eta
    return sch


def is_stochastic(scheduler) -> bool:
    """Whether a discrete-time scheduler adds noise in its steps (DDIM with eta > 0, the SDE solver): such a sample needs
    per-image seeds."""
    return getattr(scheduler, 'eta', 0.0) != 0.0 or getattr(scheduler, 'algorithm_type', None) == 'sde-dpmsolver++'


class DPMSolverMultistepScheduler(_InferenceGrid, DDPMScheduler):
    """DPM-Solver++(2M) (Lu et al. 2022, arXiv:2211.01095, Algorithm 2): the second-order multistep solver of the diffusion ODE
    in the data-prediction parameterisation, deterministic, one model evaluation per step.  Same surface, timestep grid
    (``timestep_spacing``, ``steps_offset``) and last step (to ``final_alpha_cumprod = alphas_cumprod[0]``, so lambda
    stays finite) as ``DDIMScheduler``: both visit the same ``t``.  A table value of exactly 0 (zero terminal SNR) is read
    as 2^-24, as in diffusers, which keeps lambda finite there too.

    With alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = ln(alpha / sigma), all from the fp32 ``alphas_cumprod`` table
    taken to float64, a step s -> t with h = lambda_t - lambda_s is
        x0_s = ax x_s + am m                            (ax, am) = (1/alpha, -sigma/alpha) epsilon, (alpha, -sigma) v, (0, 1) sample
        x_t  = (sigma_t / sigma_s) x_s - alpha_t expm1(-h) D
        D    = x0_s                                                     first order (this is DDIM, eta = 0)
        D    = (1 + 1/(2r)) x0_s - (1/(2r)) x0_s',  r = (lambda_s - lambda_s') / h      second order, s' the step before s
    The first step is first order; with ``lower_order_final`` and fewer than 15 steps the last one is too.

    ``step()`` is stateful (the previous x0 and lambda and a step index, reset by ``set_timesteps``).
    ``step_coefficients_ms(i)`` is the same step as five floats, what ``ops.sampler_step_ms`` applies on the device.

    ``algorithm_type='sde-dpmsolver++'`` ("DPM++ 2M SDE", diffusers' midpoint update of the reverse SDE) is the same walk
    with noise: with K = -alpha_t expm1(-2h)
        x_t  = (sigma_t / sigma_s) e^{-h} x_s + K D + sigma_t sqrt(-expm1(-2h)) z,      z ~ N(0, I) fresh per step
    and the same D, grid, order rules, zero-SNR rule and ``set_begin_index``.  ``step_coefficients_sde(i)`` is that step as
    six floats (the row of ``ops.sampler_step_rng``); ``step()`` takes z as ``variance_noise=``, else draws it from
    ``generator``.  ``step_coefficients_ms`` stays the ODE's five floats."""

    multistep = True
    ALGORITHM_TYPES = ('dpmsolver++', 'sde-dpmsolver++')
    default_algorithm_type = 'dpmsolver++'

    def __init__(self, *a, solver_order: int = 2, lower_order_final: bool = True, steps_offset: int = 1,
                 timestep_spacing: str = 'leading', algorithm_type: str = None, **kw):
        super().__init__(*a, **kw)
        self.timestep_spacing = check_timestep_spacing(timestep_spacing)
        algorithm_type = self.default_algorithm_type if algorithm_type is None else algorithm_type
        if algorithm_type not in self.ALGORITHM_TYPES:
            raise ValueError(f'algorithm_type must be one of {self.ALGORITHM_TYPES}, got {algorithm_type!r}')
        self.algorithm_type = algorithm_type
        if solver_order not in (1, 2):
            raise ValueError(f'solver_order must be 1 or 2, got {solver_order}')
        if self.prediction_type not in ('epsilon', 'v_prediction', 'sample'):
            raise ValueError(f'prediction_type must be epsilon, v_prediction or sample, got {self.prediction_type!r}')
        self.solver_order = solver_order
        self.lower_order_final = lower_order_final
        self.steps_offset = steps_offset
        self.final_alpha_cumprod = self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.timesteps = torch.arange(self.num_train_timesteps - 1, -1, -1)
        self.num_inference_steps = None
        self._reset()

    def _reset(self):
        self._step_index, self._prev_x0, self._prev_lambda = 0, None, None

    def set_begin_index(self, i: int):
        """The stateful ``step()`` starts at step ``i`` of the schedule (image-to-image: only the tail is run) with no
        history, so its first step is first order and ``lower_order_final`` still finds the last one.  ``set_timesteps``
        resets it to 0."""
        self._reset()
        self._step_index = int(i)

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        ts = self._grid(num_inference_steps)
        self.timesteps = ts.to(device) if device is not None else ts
        self._reset()

    def scale_model_input(self, sample, timestep=None):
        return sample

    def _alpha_sigma_lambda(self, t: int):
        """(alpha, sigma, lambda) in float64 at timestep ``t``; a negative ``t`` is past the end: ``final_alpha_cumprod``."""
        ac = float(self.alphas_cumprod[t] if t >= 0 else self.final_alpha_cumprod)
        if ac == 0.0:
            if self.prediction_type == 'epsilon':
                raise _zero_snr_epsilon_error(t)
            ac = ZERO_SNR_ALPHA_CUMPROD
        a, s = math.sqrt(ac), math.sqrt(1.0 - ac)
        return a, s, math.log(a / s)

    def _data_prediction(self, a: float, s: float):
        if self.prediction_type == 'v_prediction':
            return a, -s
        if self.prediction_type == 'sample':
            return 0.0, 1.0
        if self.prediction_type == 'epsilon':
            return 1.0 / a, -s / a
        raise ValueError(f'prediction_type must be epsilon, v_prediction or sample, got {self.prediction_type!r}')

    def _second_order(self, i: int) -> bool:
        n = self.num_inference_steps
        return self.solver_order == 2 and i > 0 and not (self.lower_order_final and n < 15 and i == n - 1)

    def step_coefficients_ms(self, i: int, first: bool = False):
        """Step number ``i`` of the current schedule as five Python floats (ax, am, kx, k0, k1), computed in float64:
        x0 = ax * sample + am * model_output, prev_sample = kx * sample + k0 * x0 + k1 * (the x0 of step i - 1); k1 is
        exactly 0.0 on a first-order step.  ``prediction_type``, the order switches and the schedule are read now.
        ``first``: the step is the first one executed (a schedule entered at ``i`` > 0 has no history): first order."""
        i = int(i)
        t = int(self.timesteps[i])
        a_s, s_s, l_s = self._alpha_sigma_lambda(t)
        a_t, s_t, l_t = self._alpha_sigma_lambda(self._prev_timestep(t))
        ax, am = self._data_prediction(a_s, s_s)
        h = l_t - l_s
        kd = -a_t * math.expm1(-h)
        if first or not self._second_order(i):
            return ax, am, s_t / s_s, kd, 0.0
        r = (l_s - self._alpha_sigma_lambda(int(self.timesteps[i - 1]))[2]) / h
        return ax, am, s_t / s_s, kd * (1.0 + 0.5 / r), -kd * (0.5 / r)

    def step_coefficients_sde(self, i: int, first: bool = False):
        """Step number ``i`` of the SDE solver as six Python floats (ax, am, kx, k0, k1, kn), computed in float64:
        x0 = ax * sample + am * model_output, prev_sample = kx * sample + k0 * x0 + k1 * (the x0 of step i - 1) + kn * z.
        kx = (sigma_t / sigma_s) e^{-h}; K = -alpha_t expm1(-2h) is k0 on a first-order step (k1 exactly 0.0), else
        k0 = K (1 + 1/(2r)), k1 = -K / (2r); kn = sigma_t sqrt(-expm1(-2h)).  ``first`` as in ``step_coefficients_ms``."""
        i = int(i)
        t = int(self.timesteps[i])
        a_s, s_s, l_s = self._alpha_sigma_lambda(t)
        a_t, s_t, l_t = self._alpha_sigma_lambda(self._prev_timestep(t))
        ax, am = self._data_prediction(a_s, s_s)
        h = l_t - l_s
        K = -a_t * math.expm1(-2.0 * h)
        kx, kn = (s_t / s_s) * math.exp(-h), s_t * math.sqrt(-math.expm1(-2.0 * h))
        if first or not self._second_order(i):
            return ax, am, kx, K, 0.0, kn
        r = (l_s - self._alpha_sigma_lambda(int(self.timesteps[i - 1]))[2]) / h
        return ax, am, kx, K * (1.0 + 0.5 / r), -K * (0.5 / r), kn

    def step(self, model_output, timestep, sample, generator=None, variance_noise=None, **kw):
        t = int(timestep)
        a_s, s_s, l_s = self._alpha_sigma_lambda(t)
        a_t, s_t, l_t = self._alpha_sigma_lambda(self._prev_timestep(t))
        ax, am = self._data_prediction(a_s, s_s)
        x0 = ax * sample + am * model_output
        h = l_t - l_s
        d = x0
        if self._second_order(self._step_index) and self._prev_x0 is not None:
            r = (l_s - self._prev_lambda) / h
            d = (1.0 + 1.0 / (2.0 * r)) * x0 - (1.0 / (2.0 * r)) * self._prev_x0
        if self.algorithm_type == 'sde-dpmsolver++':
            if variance_noise is None:
                variance_noise = torch.randn(sample.shape, generator=generator, device=sample.device, dtype=sample.dtype)
            prev = ((s_t / s_s) * math.exp(-h)) * sample - (a_t * math.expm1(-2.0 * h)) * d \
                + (s_t * math.sqrt(-math.expm1(-2.0 * h))) * variance_noise
        else:
            prev = (s_t / s_s) * sample - (a_t * math.expm1(-h)) * d
        self._prev_x0, self._prev_lambda = x0, l_s
        self._step_index += 1

        class _Out(dict):
            prev_sample = prev

        return _Out(prev_sample=prev)


class DPMSolverSDEMultistepScheduler(DPMSolverMultistepScheduler):
    """``DPMSolverMultistepScheduler`` whose default ``algorithm_type`` is ``'sde-dpmsolver++'``: what the name
    ``'dpm++2m-sde'`` builds."""
    default_algorithm_type = 'sde-dpmsolver++'


INFERENCE_SCHEDULERS = {'ddim': DDIMScheduler, 'dpm++2m': DPMSolverMultistepScheduler}
# the solvers that add noise in every step, a table of their own: every place that takes a name looks in both
STOCHASTIC_INFERENCE_SCHEDULERS = {'dpm++2m-sde': DPMSolverSDEMultistepScheduler}


def inference_scheduler_class(name: str):
    """The class behind a scheduler name of either table; ``KeyError`` for an unknown one."""
    return INFERENCE_SCHEDULERS[name] if name in INFERENCE_SCHEDULERS else STOCHASTIC_INFERENCE_SCHEDULERS[name]


def check_inference_scheduler(scheduler, continuous_time: bool = False):
    """``inference_scheduler=`` of the factories and of ``generate()``: None, a name of ``INFERENCE_SCHEDULERS`` or a
    scheduler object.  Raises ``ValueError`` for an unknown name, and for a multistep scheduler on a continuous-time model
    (a discrete-time method), before anything touches the device."""
    if isinstance(scheduler, str) and scheduler not in INFERENCE_SCHEDULERS and scheduler not in STOCHASTIC_INFERENCE_SCHEDULERS:
        raise ValueError(f'inference_scheduler must be one of {(*INFERENCE_SCHEDULERS, *STOCHASTIC_INFERENCE_SCHEDULERS)}, '
                         f'got {scheduler!r}')
    if continuous_time and scheduler is not None and (isinstance(scheduler, str) or getattr(scheduler, 'multistep', False)):
        what = scheduler if isinstance(scheduler, str) else type(scheduler).__name__
        raise ValueError(f'inference_scheduler {what!r} is a discrete-time method: a continuous-time model samples with '
                         'its ContinuousTimeScheduler')


def make_inference_scheduler(name: str, like=None, **kw):
    """The inference scheduler called ``name``.  With ``like`` (a ``DDPMScheduler`` of any kind) it walks that scheduler's
    own noise tables with its ``prediction_type``, ``steps_offset`` and ``timestep_spacing``, read now."""
    check_inference_scheduler(name)
    cls = inference_scheduler_class(name)
    if like is None:
        return cls(**kw)
    kw.setdefault('timestep_spacing', getattr(like, 'timestep_spacing', 'leading'))
    sch = cls(num_train_timesteps=like.num_train_timesteps, prediction_type=like.prediction_type,
              steps_offset=getattr(like, 'steps_offset', 1), **kw)
    sch.rescale_betas_zero_snr = getattr(like, 'rescale_betas_zero_snr', False)
    sch.betas, sch.alphas, sch.alphas_cumprod = like.betas, like.alphas, like.alphas_cumprod
    sch.final_alpha_cumprod = getattr(like, 'final_alpha_cumprod', like.alphas_cumprod[0])
    return sch


def resolve_inference_scheduler(scheduler, own, continuous_time: bool = False):
    """What ``generate(inference_scheduler=...)`` samples with for this call: ``own`` (the model's) for None and for the
    name of its own class, a new scheduler on ``own``'s tables for another name, the object itself otherwise."""
    check_inference_scheduler(scheduler, continuous_time)
    if scheduler is None:
        return own
    if isinstance(scheduler, str):
        cls = inference_scheduler_class(scheduler)
        # the two DPM names differ in the algorithm type, whichever class carries it
        same = isinstance(own, cls) and getattr(own, 'algorithm_type', None) == getattr(cls, 'default_algorithm_type', None) \
            if issubclass(cls, DPMSolverMultistepScheduler) else type(own) is cls
        return own if same else make_inference_scheduler(scheduler, like=own)
    return scheduler


def with_timestep_spacing(scheduler, spacing):
    """``generate(timestep_spacing=...)``: ``scheduler`` itself for None or its own spacing, else a shallow copy (same noise
    tables) that walks the other grid for this call.  ``ValueError`` for an unknown name, and for a scheduler that has no
    discrete grid to respace."""
    if spacing is None:
        return scheduler
    check_timestep_spacing(spacing)
    if not hasattr(scheduler, 'timestep_spacing'):
        raise ValueError(f'timestep_spacing: {type(scheduler).__name__} has no discrete timestep grid to respace')
    if scheduler.timestep_spacing == spacing:
        return scheduler
    import copy
    sch = copy.copy(scheduler)
    sch.timestep_spacing = spacing
    return sch


def check_zero_snr_grid(scheduler):
    """After ``set_timesteps``: ``ValueError`` if an epsilon-prediction scheduler is about to visit a timestep whose
    ``alphas_cumprod`` is exactly 0 (zero terminal SNR).  Host only, so callers raise before anything is launched."""
    ac = getattr(scheduler, 'alphas_cumprod', None)
    if ac is None or getattr(scheduler, 'prediction_type', None) != 'epsilon':
        return
    ts = scheduler.timesteps
    for t in (ts.tolist() if isinstance(ts, torch.Tensor) else ts):
        if float(t) == int(t) and float(ac[int(t)]) == 0.0:
            raise _zero_snr_epsilon_error(int(t))


def check_snr_gamma(gamma):
    """``snr_gamma=``: None (no weighting) or a finite float > 0."""
    if gamma is None:
        return None
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not math.isfinite(gamma) or gamma <= 0:
        raise ValueError(f'snr_gamma must be None or a finite number > 0, got {gamma!r}')
    return float(gamma)


def min_snr_weights(alphas_cumprod: torch.Tensor, gamma: float, prediction_type: str) -> torch.Tensor:
    """The Min-SNR-gamma loss weight of every timestep (Hang et al., arXiv:2303.09556) as a float64 table, from the
    ``alphas_cumprod`` table taken to float64: with SNR = abar / (1 - abar), min(SNR, gamma) / SNR for ``epsilon`` (1 where
    SNR = 0, the limit) and min(SNR, gamma) / (SNR + 1) for ``v_prediction``."""
    gamma = check_snr_gamma(gamma)
    if gamma is None:
        raise ValueError('min_snr_weights needs a gamma')
    ac = alphas_cumprod.to(torch.float64)
    snr = ac / (1.0 - ac)
    capped = torch.clamp(snr, max=gamma)
    if prediction_type == 'v_prediction':
        return capped / (snr + 1.0)
    if prediction_type == 'epsilon':
        return torch.where(snr > 0, capped / torch.where(snr > 0, snr, torch.ones_like(snr)), torch.ones_like(snr))
    raise ValueError(f'Min-SNR weighting is defined for epsilon and v_prediction, got {prediction_type!r}')
