"""Host side of the second-order multistep sampler (``DPMSolverMultistepScheduler``, DPM-Solver++ 2M), all in float64:
  * with ``solver_order=1`` it is ``DDIMScheduler`` (which the oracle tests pin);
  * ``step_coefficients_ms`` is the stateful ``step()``, and both are the published update restated here;
  * on a case with a closed-form ODE solution it is second order: it beats DDIM by the factors measured for the correct
    formula, which a history term of the wrong sign or weight misses;
  * the public switch (factories, ``generate(inference_scheduler=...)``) resolves names and refuses bad ones before
    anything touches the device.
Bounds of 1e-12 are relative to max|step| (a handful of float64 roundings on either side, the convention of
tests/test_sampler_host.py)."""
import math
import os

import pytest
import torch

from diffusion_amd.models.schedulers import DDIMScheduler, DPMSolverMultistepScheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ('epsilon', 'v_prediction', 'sample')
TOL = 1e-12


def _xm(seed, k=2):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(2, 3, 4, 4, generator=g, dtype=torch.float64) for _ in range(k)]


def _check(got, ref, what):
    err = (got - ref).abs().max().item()
    bound = TOL * ref.abs().max().item()
    assert err <= bound, (what, err, bound)


# ---------------------------------------------------------------------------------------------------------------------
# 1. first order is DDIM
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ptype', TYPES)
@pytest.mark.parametrize('n', (4, 20, 50))
def test_first_order_is_ddim(ptype, n):
    ddim = DDIMScheduler(prediction_type=ptype)
    dpm = DPMSolverMultistepScheduler(prediction_type=ptype, solver_order=1)
    ddim.set_timesteps(n)
    dpm.set_timesteps(n)
    assert torch.equal(ddim.timesteps, dpm.timesteps)
    assert dpm.init_noise_sigma == 1.0 and float(dpm.final_alpha_cumprod) == float(ddim.final_alpha_cumprod)
    x, m = _xm(n)
    assert dpm.scale_model_input(x, dpm.timesteps[0]) is x
    for i in (0, n // 2, n - 1):   # step() at solver_order=1 keeps no state that matters: any timestep, any order of calls
        t = ddim.timesteps[i]
        _check(dpm.step(m, t, x)['prev_sample'], ddim.step(m, t, x)['prev_sample'], (ptype, n, int(t)))
    # and as a whole trajectory, every step
    dpm.set_timesteps(n)
    xa = xb = x
    for t in ddim.timesteps:
        xa, xb = ddim.step(m, t, xa)['prev_sample'], dpm.step(m, t, xb)['prev_sample']
    _check(xb, xa, (ptype, n, 'trajectory'))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the coefficients are the step, and the step is the published formula
# ---------------------------------------------------------------------------------------------------------------------
def _restated(sch, n, i, x, m, prev_x0, second):
    """The update of this step written out again from the float32 alphas_cumprod table in float64."""
    ac = sch.alphas_cumprod.double()
    T = sch.num_train_timesteps

    def asl(t):
        a2 = float(ac[t]) if t >= 0 else float(ac[0])
        return math.sqrt(a2), math.sqrt(1 - a2), 0.5 * math.log(a2 / (1 - a2))

    ts = [int(t) for t in sch.timesteps]
    a_s, s_s, l_s = asl(ts[i])
    a_t, s_t, l_t = asl(ts[i] - T // n)
    x0 = {'epsilon': (x - s_s * m) / a_s, 'v_prediction': a_s * x - s_s * m, 'sample': m}[sch.prediction_type]
    h = l_t - l_s
    d = x0
    if second:
        r = (l_s - asl(ts[i - 1])[2]) / h
        d = (1 + 1 / (2 * r)) * x0 - (1 / (2 * r)) * prev_x0
    return s_t / s_s * x - a_t * math.expm1(-h) * d, x0


@pytest.mark.parametrize('ptype', TYPES)
@pytest.mark.parametrize('n,order', [(4, 2), (14, 2), (15, 2), (20, 2), (50, 2), (20, 1)])
def test_coefficients_are_the_step(ptype, n, order):
    sch = DPMSolverMultistepScheduler(prediction_type=ptype, solver_order=order)
    sch.set_timesteps(n)
    g = torch.Generator().manual_seed(1000 + n)
    x = torch.randn(2, 3, 4, 4, generator=g, dtype=torch.float64)
    prev_x0 = None
    for i, t in enumerate(sch.timesteps):
        m = torch.randn(x.shape, generator=g, dtype=torch.float64)
        c = sch.step_coefficients_ms(i)
        assert len(c) == 5 and all(isinstance(v, float) for v in c)
        ax, am, kx, k0, k1 = c
        second = order == 2 and i > 0 and not (n < 15 and i == n - 1)
        assert (k1 != 0.0) == second, (n, i, k1)
        if not second:
            assert k1 == 0.0 and math.copysign(1.0, k1) == 1.0
        x0 = ax * x + am * m
        by_coef = kx * x + k0 * x0 + (k1 * prev_x0 if second else 0.0)
        ref = sch.step(m, t, x)['prev_sample']
        _check(by_coef, ref, ('coefficients', ptype, n, i))
        want, want_x0 = _restated(sch, n, i, x, m, prev_x0, second)
        _check(ref, want, ('restated', ptype, n, i))
        _check(x0, want_x0, ('x0', ptype, n, i))
        x, prev_x0 = ref, x0


def test_order_switches():
    for n, order, lof, firsts in [(4, 2, True, {0, 3}), (14, 2, True, {0, 13}), (15, 2, True, {0}), (4, 2, False, {0}),
                                  (6, 1, True, set(range(6)))]:
        sch = DPMSolverMultistepScheduler(solver_order=order, lower_order_final=lof)
        sch.set_timesteps(n)
        got = {i for i in range(n) if sch.step_coefficients_ms(i)[4] == 0.0}
        assert got == firsts, (n, order, lof, got)
    with pytest.raises(ValueError):
        DPMSolverMultistepScheduler(solver_order=3)
    with pytest.raises(ValueError):
        DPMSolverMultistepScheduler(prediction_type='nonsense')


def test_set_timesteps_resets_the_history():
    sch = DPMSolverMultistepScheduler()
    x, m = _xm(9)
    sch.set_timesteps(20)
    first = sch.step(m, sch.timesteps[0], x)['prev_sample']
    sch.step(m, sch.timesteps[1], first)
    sch.set_timesteps(20)
    assert torch.equal(sch.step(m, sch.timesteps[0], x)['prev_sample'], first)
    assert DPMSolverMultistepScheduler.multistep is True and not getattr(DDIMScheduler, 'multistep', False)


# ---------------------------------------------------------------------------------------------------------------------
# 3. second order where that can be known: the Gaussian case
# ---------------------------------------------------------------------------------------------------------------------
SIGMA_D2 = 4.0


def _gaussian_error(sch, n, step=None):
    """Data N(0, sigma_d^2): the exact epsilon is sigma_t x / (alpha_t^2 sigma_d^2 + sigma_t^2), and the ODE from the first
    timestep (alpha a, sigma s) to final_alpha_cumprod (A, S) maps x to x sqrt(A^2 sd^2 + S^2) / sqrt(a^2 sd^2 + s^2).
    Relative max-error of the final sample with the exact model output in the scheduler's parameterisation."""
    sch.set_timesteps(n)
    ac = sch.alphas_cumprod.double()
    x_first = torch.linspace(-3.0, 3.0, 13, dtype=torch.float64)
    x = x_first.clone()
    step = step or sch.step
    for t in sch.timesteps:
        a2 = float(ac[int(t)])
        a, s = math.sqrt(a2), math.sqrt(1 - a2)
        den = a2 * SIGMA_D2 + (1 - a2)
        eps, x0 = s * x / den, a * SIGMA_D2 * x / den
        m = {'epsilon': eps, 'sample': x0, 'v_prediction': a * eps - s * x0}[sch.prediction_type]
        x = step(m, t, x)['prev_sample']
    a2, A2 = float(ac[int(sch.timesteps[0])]), float(sch.final_alpha_cumprod.double())
    exact = x_first * math.sqrt(A2 * SIGMA_D2 + 1 - A2) / math.sqrt(a2 * SIGMA_D2 + 1 - a2)
    return ((x - exact).abs().max() / exact.abs().max()).item(), x


def _conditions(err_2m, err_ddim):
    return (err_2m[20] <= 0.4 * err_ddim[20] and err_2m[40] <= 0.4 * err_ddim[40] and err_2m[40] <= err_2m[20] / 2.5)


@pytest.fixture(scope='module')
def ddim_gaussian_errors():
    return {n: _gaussian_error(DDIMScheduler(prediction_type='epsilon'), n)[0] for n in (20, 40)}


def test_second_order_on_the_gaussian_case(ddim_gaussian_errors):
    err_ddim = ddim_gaussian_errors
    finals = {}
    for ptype in TYPES:
        err_2m = {}
        for n in (20, 40):
            err_2m[n], finals[(ptype, n)] = _gaussian_error(DPMSolverMultistepScheduler(prediction_type=ptype), n)
        print(f'{ptype}: err 2M / DDIM at 20 steps {err_2m[20]:.3e} / {err_ddim[20]:.3e} = {err_2m[20] / err_ddim[20]:.3f}, '
              f'at 40 steps {err_2m[40]:.3e} / {err_ddim[40]:.3e} = {err_2m[40] / err_ddim[40]:.3f}; '
              f'2M 20 -> 40 steps: {err_2m[20] / err_2m[40]:.2f}x, DDIM {err_ddim[20] / err_ddim[40]:.2f}x')
        assert err_2m[20] <= 0.4 * err_ddim[20], (ptype, err_2m, err_ddim)
        assert err_2m[40] <= 0.4 * err_ddim[40], (ptype, err_2m, err_ddim)
        assert err_2m[40] <= err_2m[20] / 2.5, (ptype, err_2m)
    for n in (20, 40):   # the three parameterisations are one method
        for ptype in TYPES[1:]:
            d = (finals[(ptype, n)] - finals[('epsilon', n)]).abs().max() / finals[('epsilon', n)].abs().max()
            assert d.item() <= 1e-9, (ptype, n, d.item())


@pytest.mark.parametrize('variant', ['sign', 'one', 'quarter'])
def test_the_gaussian_conditions_reject_wrong_history_terms(ddim_gaussian_errors, variant):
    """The conditions above are not vacuous: the same update with the history term's sign flipped, or with 1 or 1/4 in place
    of 1/2, fails them.  The variant is built here from the scheduler's own first-order pieces."""
    w = {'sign': -0.5, 'one': 1.0, 'quarter': 0.25}[variant]
    err = {}
    for n in (20, 40):
        sch = DPMSolverMultistepScheduler(prediction_type='epsilon')
        state = {}

        def step(m, t, x, sch=sch, state=state):
            a_s, s_s, l_s = sch._alpha_sigma_lambda(int(t))
            a_t, s_t, l_t = sch._alpha_sigma_lambda(int(t) - sch.num_train_timesteps // sch.num_inference_steps)
            x0 = (x - s_s * m) / a_s
            h, d = l_t - l_s, x0
            if 'x0' in state:
                r = (l_s - state['l']) / h
                d = (1 + w / r) * x0 - (w / r) * state['x0']
            state.update(x0=x0, l=l_s)
            return {'prev_sample': s_t / s_s * x - a_t * math.expm1(-h) * d}

        err[n] = _gaussian_error(sch, n, step)[0]
    assert not _conditions(err, ddim_gaussian_errors), (variant, err, ddim_gaussian_errors)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the interface
# ---------------------------------------------------------------------------------------------------------------------
def test_names_resolve():
    from diffusion_amd.models.schedulers import (INFERENCE_SCHEDULERS, make_inference_scheduler,
                                                 resolve_inference_scheduler)
    assert tuple(INFERENCE_SCHEDULERS) == ('ddim', 'dpm++2m')
    assert type(make_inference_scheduler('ddim')) is DDIMScheduler   # what the factories build by default
    own = make_inference_scheduler('ddim', prediction_type='v_prediction')
    assert type(own) is DDIMScheduler and own.prediction_type == 'v_prediction'
    assert resolve_inference_scheduler(None, own) is own and resolve_inference_scheduler('ddim', own) is own
    dpm = resolve_inference_scheduler('dpm++2m', own)
    assert type(dpm) is DPMSolverMultistepScheduler and dpm.prediction_type == 'v_prediction' and dpm.solver_order == 2
    assert dpm.alphas_cumprod is own.alphas_cumprod and dpm.steps_offset == own.steps_offset
    obj = DPMSolverMultistepScheduler(solver_order=1)
    assert resolve_inference_scheduler(obj, own) is obj
    assert type(resolve_inference_scheduler('ddim', dpm)) is DDIMScheduler
    with pytest.raises(ValueError, match='inference_scheduler'):
        resolve_inference_scheduler('euler', own)


def test_the_factories_default_to_ddim():
    import inspect
    from diffusion_amd.models import models
    for f in (models.stable_diffusion_2, models.discrete_pixel_diffusion):
        assert inspect.signature(f).parameters['inference_scheduler'].default == 'ddim'
    assert inspect.signature(models.continuous_pixel_diffusion).parameters['inference_scheduler'].default is None


def test_bad_names_raise_before_anything_touches_the_device(monkeypatch):
    """The factories check the name before they look for a GPU; ``generate`` is called with ``self`` None, so anything past
    the check would fail with another exception (the convention of tests/test_sampler_host.py)."""
    from diffusion_amd.models import models
    from diffusion_amd.models.pixel_diffusion import PixelDiffusion
    from diffusion_amd.models.stable_diffusion import StableDiffusion
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: pytest.fail('looked for a device'))
    for f in (models.stable_diffusion_2, models.discrete_pixel_diffusion):
        with pytest.raises(ValueError, match='inference_scheduler'):
            f(inference_scheduler='euler')
    with pytest.raises(ValueError, match='inference_scheduler'):
        models.continuous_pixel_diffusion(inference_scheduler='euler')
    for bad in ('dpm++2m', DPMSolverMultistepScheduler()):
        with pytest.raises(ValueError, match='discrete-time'):
            models.continuous_pixel_diffusion(inference_scheduler=bad)
    monkeypatch.delenv('DA_SAMPLER', raising=False)
    for cls in (StableDiffusion, PixelDiffusion):
        with pytest.raises(ValueError, match='inference_scheduler'):
            cls.generate(None, prompt=['a cool doge'], inference_scheduler='euler')


def test_a_continuous_model_refuses_a_multistep_scheduler_in_generate():
    from diffusion_amd.models.pixel_diffusion import PixelDiffusion

    class _Stub:
        continuous_time = True
        inference_scheduler = object()

    for bad in ('dpm++2m', DPMSolverMultistepScheduler()):
        with pytest.raises(ValueError, match='discrete-time'):
            PixelDiffusion.generate(_Stub(), prompt=['a cool doge'], inference_scheduler=bad)


def test_sampler_step_ms_is_declared_and_bound():
    from diffusion_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'diffusion_amd.h')).read()
    assert 'int da_sampler_step_ms(const float* pred, const float* x, float* hist, const float* coef,' in header
    assert len(_lib.SIGNATURES['da_sampler_step_ms']) == 12 and len(_lib.SIGNATURES['da_sampler_step']) == 12
    assert 'da_sampler_step_ms' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
