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

import torch


class DDPMScheduler:
    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = 'scaled_linear', prediction_type: str = 'epsilon', clip_sample: bool = False):
        if beta_schedule != 'scaled_linear':
            raise ValueError('SD-2 uses the scaled_linear schedule')
        self.num_train_timesteps = num_train_timesteps
        self.prediction_type = prediction_type
        self.betas = torch.linspace(beta_start**0.5, beta_end**0.5, num_train_timesteps, dtype=torch.float32)**2
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


class DDIMScheduler(DDPMScheduler):
    """eta = 0 DDIM sampler, ``set_alpha_to_one=False``, ``steps_offset=1`` (SD-2 scheduler_config.json)."""

    def __init__(self, *a, steps_offset: int = 1, **kw):
        super().__init__(*a, **kw)
        self.steps_offset = steps_offset
        self.final_alpha_cumprod = self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.timesteps = torch.arange(self.num_train_timesteps - 1, -1, -1)
        self.num_inference_steps = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        ratio = self.num_train_timesteps // num_inference_steps
        ts = (torch.arange(0, num_inference_steps) * ratio).flip(0) + self.steps_offset
        self.timesteps = ts.clamp(max=self.num_train_timesteps - 1).to(device) if device is not None else ts.clamp(
            max=self.num_train_timesteps - 1)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step_coefficients(self, timestep):
        """``step`` as three Python floats (cx, cm, cn), computed in float64: prev_sample = cx * sample + cm * model_output
        (+ cn * noise, 0 for eta = 0).  The step is linear in both for each prediction type; ``prediction_type`` and
        ``num_inference_steps`` are read now, like ``step`` does.  What ``ops.sampler_step`` applies on the device."""
        t = int(timestep)
        prev_t = t - self.num_train_timesteps // self.num_inference_steps
        ac_t = float(self.alphas_cumprod[t])
        ac_prev = float(self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod)
        a, s, A, S = math.sqrt(ac_t), math.sqrt(1 - ac_t), math.sqrt(ac_prev), math.sqrt(1 - ac_prev)
        if self.prediction_type == 'v_prediction':
            return A * a + S * s, S * a - A * s, 0.0
        if self.prediction_type == 'sample':
            return S / s, A - S * a / s, 0.0
        return A / a, S - A * s / a, 0.0

    def step(self, model_output, timestep, sample, generator=None, **kw):
        t = int(timestep)
        prev_t = t - self.num_train_timesteps // self.num_inference_steps
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


class DPMSolverMultistepScheduler(DDPMScheduler):
    """DPM-Solver++(2M) (Lu et al. 2022, arXiv:2211.01095, Algorithm 2): the second-order multistep solver of the diffusion ODE
    in the data-prediction parameterisation, deterministic, one model evaluation per step.  Same surface, timestep grid
    (leading spacing, ``steps_offset``, clamped) and last step (to ``final_alpha_cumprod = alphas_cumprod[0]``, so lambda
    stays finite) as ``DDIMScheduler``: both visit the same ``t``.

    With alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = ln(alpha / sigma), all from the fp32 ``alphas_cumprod`` table
    taken to float64, a step s -> t with h = lambda_t - lambda_s is
        x0_s = ax x_s + am m                            (ax, am) = (1/alpha, -sigma/alpha) epsilon, (alpha, -sigma) v, (0, 1) sample
        x_t  = (sigma_t / sigma_s) x_s - alpha_t expm1(-h) D
        D    = x0_s                                                     first order (this is DDIM, eta = 0)
        D    = (1 + 1/(2r)) x0_s - (1/(2r)) x0_s',  r = (lambda_s - lambda_s') / h      second order, s' the step before s
    The first step is first order; with ``lower_order_final`` and fewer than 15 steps the last one is too.

    ``step()`` is stateful (the previous x0 and lambda and a step index, reset by ``set_timesteps``).
    ``step_coefficients_ms(i)`` is the same step as five floats, what ``ops.sampler_step_ms`` applies on the device."""

    multistep = True

    def __init__(self, *a, solver_order: int = 2, lower_order_final: bool = True, steps_offset: int = 1, **kw):
        super().__init__(*a, **kw)
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
        ratio = self.num_train_timesteps // num_inference_steps
        ts = ((torch.arange(0, num_inference_steps) * ratio).flip(0) + self.steps_offset).clamp(
            max=self.num_train_timesteps - 1)
        self.timesteps = ts.to(device) if device is not None else ts
        self._reset()

    def scale_model_input(self, sample, timestep=None):
        return sample

    def _alpha_sigma_lambda(self, t: int):
        """(alpha, sigma, lambda) in float64 at timestep ``t``; a negative ``t`` is past the end: ``final_alpha_cumprod``."""
        ac = float(self.alphas_cumprod[t] if t >= 0 else self.final_alpha_cumprod)
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
        stride = self.num_train_timesteps // self.num_inference_steps
        t = int(self.timesteps[i])
        a_s, s_s, l_s = self._alpha_sigma_lambda(t)
        a_t, s_t, l_t = self._alpha_sigma_lambda(t - stride)
        ax, am = self._data_prediction(a_s, s_s)
        h = l_t - l_s
        kd = -a_t * math.expm1(-h)
        if first or not self._second_order(i):
            return ax, am, s_t / s_s, kd, 0.0
        r = (l_s - self._alpha_sigma_lambda(int(self.timesteps[i - 1]))[2]) / h
        return ax, am, s_t / s_s, kd * (1.0 + 0.5 / r), -kd * (0.5 / r)

    def step(self, model_output, timestep, sample, generator=None, **kw):
        t = int(timestep)
        a_s, s_s, l_s = self._alpha_sigma_lambda(t)
        a_t, s_t, l_t = self._alpha_sigma_lambda(t - self.num_train_timesteps // self.num_inference_steps)
        ax, am = self._data_prediction(a_s, s_s)
        x0 = ax * sample + am * model_output
        h = l_t - l_s
        d = x0
        if self._second_order(self._step_index) and self._prev_x0 is not None:
            r = (l_s - self._prev_lambda) / h
            d = (1.0 + 1.0 / (2.0 * r)) * x0 - (1.0 / (2.0 * r)) * self._prev_x0
        prev = (s_t / s_s) * sample - (a_t * math.expm1(-h)) * d
        self._prev_x0, self._prev_lambda = x0, l_s
        self._step_index += 1

        class _Out(dict):
            prev_sample = prev

        return _Out(prev_sample=prev)


INFERENCE_SCHEDULERS = {'ddim': DDIMScheduler, 'dpm++2m': DPMSolverMultistepScheduler}


def check_inference_scheduler(scheduler, continuous_time: bool = False):
    """``inference_scheduler=`` of the factories and of ``generate()``: None, a name of ``INFERENCE_SCHEDULERS`` or a
    scheduler object.  Raises ``ValueError`` for an unknown name, and for a multistep scheduler on a continuous-time model
    (a discrete-time method), before anything touches the device."""
    if isinstance(scheduler, str) and scheduler not in INFERENCE_SCHEDULERS:
        raise ValueError(f'inference_scheduler must be one of {tuple(INFERENCE_SCHEDULERS)}, got {scheduler!r}')
    if continuous_time and scheduler is not None and (isinstance(scheduler, str) or getattr(scheduler, 'multistep', False)):
        what = scheduler if isinstance(scheduler, str) else type(scheduler).__name__
        raise ValueError(f'inference_scheduler {what!r} is a discrete-time method: a continuous-time model samples with '
                         'its ContinuousTimeScheduler')


def make_inference_scheduler(name: str, like=None, **kw):
    """The inference scheduler called ``name``.  With ``like`` (a ``DDPMScheduler`` of any kind) it walks that scheduler's
    own noise tables with its ``prediction_type`` and ``steps_offset``, read now."""
    check_inference_scheduler(name)
    cls = INFERENCE_SCHEDULERS[name]
    if like is None:
        return cls(**kw)
    sch = cls(num_train_timesteps=like.num_train_timesteps, prediction_type=like.prediction_type,
              steps_offset=getattr(like, 'steps_offset', 1), **kw)
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
        return own if type(own) is INFERENCE_SCHEDULERS[scheduler] else make_inference_scheduler(scheduler, like=own)
    return scheduler
