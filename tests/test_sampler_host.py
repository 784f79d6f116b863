"""Host side of the HIP sampling path: the schedulers' ``step_coefficients`` against their own ``step()`` in float64, the
C ABI declaration of ``da_sampler_step`` and the ``sampler=`` switch of ``generate()``.

Every scheduler step is linear in (sample, model output, noise draw), so ``cx * x + cm * m (+ cn * z)`` must reproduce
``step()`` on float64 inputs to rounding: the bound is 1e-12 * max|step| (both sides carry a handful of float64 roundings,
some through the cancellation ``step()`` itself has near t_max)."""
import os

import numpy as np
import pytest
import torch

from diffusion_amd.models.schedulers import DDIMScheduler
from diffusion_amd.schedulers.schedulers import ContinuousTimeScheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ('epsilon', 'v_prediction', 'sample')
STEPS = (1, 2, 4, 50)
TOL = 1e-12


def _xm(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 3, 4, 4, generator=g, dtype=torch.float64), torch.randn(2, 3, 4, 4, generator=g,
                                                                                 dtype=torch.float64)


def _check(got, ref, what):
    err = (got - ref).abs().max().item()
    bound = TOL * ref.abs().max().item()
    assert err <= bound, (what, err, bound)
    return err / max(ref.abs().max().item(), 1e-300)


@pytest.mark.parametrize('ptype', TYPES)
@pytest.mark.parametrize('n', STEPS)
def test_ddim_coefficients_reproduce_step(ptype, n):
    sch = DDIMScheduler(prediction_type=ptype)
    sch.set_timesteps(n)
    x, m = _xm(n)
    saw_final = False
    for t in sch.timesteps:
        saw_final |= int(t) - sch.num_train_timesteps // n < 0
        cx, cm, cn = sch.step_coefficients(t)
        assert all(isinstance(v, float) for v in (cx, cm, cn)) and cn == 0.0
        _check(cx * x + cm * m, sch.step(m, t, x)['prev_sample'], (ptype, n, int(t)))
    assert saw_final   # the last step of every schedule uses final_alpha_cumprod


@pytest.mark.parametrize('ptype', TYPES)
@pytest.mark.parametrize('n', STEPS)
def test_continuous_ode_coefficients_reproduce_step(ptype, n):
    sch = ContinuousTimeScheduler(t_max=1.56, prediction_type=ptype, use_ode=True)
    sch.set_timesteps(n)
    x, m = _xm(100 + n)
    for t in sch.timesteps:
        cx, cm, cn = sch.step_coefficients(t)
        assert all(isinstance(v, float) for v in (cx, cm, cn)) and cn == 0.0
        _check(cx * x + cm * m, sch.step(m, t, x)['prev_sample'], (ptype, n, float(t)))


@pytest.mark.parametrize('ptype', TYPES)
@pytest.mark.parametrize('n', STEPS)
def test_continuous_sde_coefficients_reproduce_step(ptype, n, monkeypatch):
    sch = ContinuousTimeScheduler(t_max=1.56, prediction_type=ptype, use_ode=False)
    sch.set_timesteps(n)
    x, m = _xm(200 + n)
    z = torch.randn(x.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    monkeypatch.setattr(torch, 'randn_like', lambda like: z.clone())
    for t in sch.timesteps:
        cx, cm, cn = sch.step_coefficients(t)
        beta = 2 * np.tan(t)
        assert abs(cn - np.sqrt(beta * sch.t_max / n)) <= 1e-14 * cn   # dt is formed in another order: an ulp or two
        ref = sch.step(m, t, x)['prev_sample']
        bound = TOL * ref.abs().max().item()
        # the deterministic part, after subtracting the draw; and the whole step
        assert ((ref - cn * z) - (cx * x + cm * m)).abs().max().item() <= bound, (ptype, n, float(t))
        _check(cx * x + cm * m + cn * z, ref, (ptype, n, float(t)))


def test_continuous_t_zero_is_the_identity():
    for ode in (True, False):
        for ptype in TYPES:
            sch = ContinuousTimeScheduler(prediction_type=ptype, use_ode=ode)
            assert sch.step_coefficients(0.0) == (1.0, 0.0, 0.0)
            assert sch.step_coefficients(np.float64(0)) == (1.0, 0.0, 0.0)


def test_coefficients_follow_attributes_flipped_after_construction():
    x, m = _xm(5)
    sch = DDIMScheduler(prediction_type='epsilon')
    sch.set_timesteps(4)
    t = sch.timesteps[1]
    eps = sch.step_coefficients(t)
    sch.prediction_type = 'v_prediction'
    v = sch.step_coefficients(t)
    assert v != eps
    _check(v[0] * x + v[1] * m, sch.step(m, t, x)['prev_sample'], 'ddim flipped to v')
    sch.set_timesteps(2)   # the stride of the step is read at call time too
    v2 = sch.step_coefficients(t)
    assert v2 != v
    _check(v2[0] * x + v2[1] * m, sch.step(m, t, x)['prev_sample'], 'ddim, stride of 2 steps')

    c = ContinuousTimeScheduler(t_max=1.56, prediction_type='epsilon', use_ode=False)
    c.set_timesteps(4)
    t = c.timesteps[2]
    sde = c.step_coefficients(t)
    c.use_ode, c.prediction_type = True, 'sample'
    ode = c.step_coefficients(t)
    assert sde[2] > 0 and ode[2] == 0.0 and ode[:2] != sde[:2]
    _check(ode[0] * x + ode[1] * m, c.step(m, t, x)['prev_sample'], 'continuous flipped to ode / sample')
    c.prediction_type = 'nonsense'
    with pytest.raises(ValueError):
        c.step_coefficients(t)


def test_sampler_step_is_declared_and_bound():
    from diffusion_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'diffusion_amd.h')).read()
    assert 'int da_sampler_step(const float* pred, const float* x, const float* noise, const float* coef,' in header
    assert len(_lib.SIGNATURES['da_sampler_step']) == 12
    assert 'sampler.hip' in open(os.path.join(ROOT, 'diffusion_amd', 'csrc', 'Makefile')).read()


def test_generate_rejects_an_unknown_sampler_before_touching_the_device(monkeypatch):
    """``self`` is None: anything past the check of ``sampler`` would fail with another exception."""
    from diffusion_amd.models.pixel_diffusion import PixelDiffusion
    from diffusion_amd.models.stable_diffusion import StableDiffusion
    from diffusion_amd.sampling import resolve_sampler
    for cls in (StableDiffusion, PixelDiffusion):
        with pytest.raises(ValueError, match='sampler'):
            cls.generate(None, prompt=['a cool doge'], sampler='nonsense')
    monkeypatch.delenv('DA_SAMPLER', raising=False)
    assert resolve_sampler(None) == 'hip'
    assert [resolve_sampler(s) for s in ('hip', 'graph', 'torch')] == ['hip', 'graph', 'torch']
    monkeypatch.setenv('DA_SAMPLER', 'torch')
    assert resolve_sampler(None) == 'torch' and resolve_sampler('graph') == 'graph'
    monkeypatch.setenv('DA_SAMPLER', 'nonsense')
    with pytest.raises(ValueError, match='sampler'):
        StableDiffusion.generate(None, prompt=['a cool doge'])
