"""Continuous-time (variance preserving) scheduler of the pixel models: the reference's
diffusion/schedulers/schedulers.py:10-114, which ``hydra_lite`` resolves ``diffusion.schedulers.schedulers.*`` to.

Training does not call ``add_noise`` / ``get_velocity`` here: ``PixelDiffusion.forward`` runs the same tangent schedule in
the fused noising kernel (``da_add_noise_ex``).  These host forms serve generation (``step``) and host-side callers.
"""
from __future__ import annotations

import numpy as np
import torch


def tangent_schedule(times):
    """beta(t), sin(phi(t)), cos(phi(t)) for the schedule angle = time, hence beta = 2 tan(t) (schedulers.py:10-24)."""
    if isinstance(times, torch.Tensor):
        return 2 * torch.tan(times), torch.sin(times), torch.cos(times)
    return 2 * np.tan(times), np.sin(times), np.cos(times)


class ContinuousTimeScheduler:
    """x_t = cos(t) x_0 + sin(t) eps for t in [0, t_max]; generation integrates the reverse SDE (Euler-Maruyama) or the
    probability-flow ODE (Euler) over ``num_inference_timesteps`` equal steps.  t_max should stay below pi/2 when
    generating: ``step`` divides by cos(t) and sin(t)^2 (schedulers.py:27-114)."""

    def __init__(self, t_max: float = 1.57, num_inference_timesteps: int = 50, prediction_type: str = 'epsilon',
                 use_ode: bool = False, schedule_function=tangent_schedule):
        self.t_max = t_max
        self.num_inference_timesteps = num_inference_timesteps
        self.prediction_type = prediction_type
        self.use_ode = use_ode
        self.schedule_function = schedule_function
        self.timesteps = np.linspace(self.t_max, 0, num=num_inference_timesteps, endpoint=False)
        self.init_noise_sigma = 1.0  # the generate() loops scale their initial noise by it, as for the diffusers schedulers

    def __len__(self):
        return self.num_inference_timesteps

    def set_timesteps(self, num_inference_timesteps):
        self.num_inference_timesteps = num_inference_timesteps
        self.timesteps = np.linspace(self.t_max, 0, num=num_inference_timesteps, endpoint=False)

    def _angles(self, timesteps, like):
        timesteps = timesteps.view(len(timesteps), *(1,) * (like.dim() - 1))
        _, sin_phi, cos_phi = self.schedule_function(timesteps)
        return sin_phi, cos_phi

    def add_noise(self, inputs, noise, timesteps):
        sin_phi, cos_phi = self._angles(timesteps, inputs)
        return cos_phi * inputs + sin_phi * noise

    def get_velocity(self, inputs, noise, timesteps):
        """v = -sin(t) x_0 + cos(t) eps."""
        sin_phi, cos_phi = self._angles(timesteps, inputs)
        return -sin_phi * inputs + cos_phi * noise

    def scale_model_input(self, model_input, t):
        return model_input

    def step_coefficients(self, timestep):
        """``step`` as three Python floats (cx, cm, cn), computed in float64: x_prev = cx * model_input + cm * model_output
        + cn * noise, noise the SDE's standard normal draw (cn = 0 for the ODE).  ``prediction_type``, ``use_ode`` and the
        number of inference steps are read now, like ``step`` does.  What ``ops.sampler_step`` applies on the device."""
        t = float(timestep)
        if t == 0:
            return 1.0, 0.0, 0.0
        beta, s, c = (float(v) for v in self.schedule_function(np.float64(t)))
        dt = self.t_max / self.timesteps.shape[0]
        if self.prediction_type == 'sample':          # x_0 = p * model_input + q * model_output
            p, q = 0.0, 1.0
        elif self.prediction_type == 'epsilon':
            p, q = 1.0 / c, -s / c
        elif self.prediction_type == 'v_prediction':
            p, q = c, -s
        else:
            raise ValueError(
                f'prediction type must be one of sample, epsilon, or v_prediction. Got {self.prediction_type}')
        h = 0.5 * beta * dt
        k = h if self.use_ode else beta * dt           # the weight of the score term
        cx = 1.0 + h - k * (1.0 - c * p) / (s * s)
        cm = k * c * q / (s * s)
        return cx, cm, 0.0 if self.use_ode else float(np.sqrt(beta * dt))

    def step(self, model_output, t, model_input, generator=None):
        """One step t -> t - t_max / num_inference_timesteps.  The SDE's noise term is drawn from torch's global generator
        (``torch.randn_like``), as the reference does; ``generator`` is accepted for the diffusers call surface."""
        if t == 0:
            return {'prev_sample': model_input}
        beta_t, sin_phi_t, cos_phi_t = self.schedule_function(t)
        dt = self.t_max / self.timesteps.shape[0]
        if self.prediction_type == 'sample':
            x_0 = model_output
        elif self.prediction_type == 'epsilon':
            x_0 = (model_input - sin_phi_t * model_output) / cos_phi_t
        elif self.prediction_type == 'v_prediction':
            x_0 = cos_phi_t * model_input - sin_phi_t * model_output
        else:
            raise ValueError(
                f'prediction type must be one of sample, epsilon, or v_prediction. Got {self.prediction_type}')
        score = -(model_input - cos_phi_t * x_0) / np.square(sin_phi_t)
        if self.use_ode:   # Euler on the probability-flow ODE
            x_prev = model_input + 0.5 * (model_input + score) * beta_t * dt
        else:              # Euler-Maruyama on the reverse SDE
            x_prev = model_input + (0.5 * model_input + score) * beta_t * dt
            x_prev += np.sqrt(beta_t * dt) * torch.randn_like(model_input)
        return {'prev_sample': x_prev}
