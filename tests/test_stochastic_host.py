"""Stochastic samplers, host side (no GPU): the NumPy restatement of the Philox / Box-Muller stream against the published
known-answer vectors and the recorded statistics, the DDIM-eta and SDE-2M coefficient rows against float64 transcriptions
written out here and against the stateful ``step()``, the draw slot of the device rows, and every ``ValueError`` of the public
interface raised before anything looks for a device."""
import inspect
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_reference as P  # noqa: E402

from diffusion_amd.models.schedulers import (INFERENCE_SCHEDULERS, STOCHASTIC_INFERENCE_SCHEDULERS,  # noqa: E402
                                             DDIMScheduler, DPMSolverMultistepScheduler, check_inference_scheduler,
                                             is_stochastic, make_inference_scheduler, resolve_inference_scheduler, with_eta)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the generator's reference
# ---------------------------------------------------------------------------------------------------------------------
def test_philox_known_answer_vectors():
    for counter, key, out in P.KAT:
        got = P.philox4x32_10([np.uint64(c) for c in counter], key)
        assert tuple(int(g) for g in got) == out, (counter, key)


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def test_philox_normals_statistics():
    """Seed 1138, draw 0, stream 0, 4 x 64 x 64 values: every figure inside 5 / sqrt(N) (the variance: 5 sqrt(2 / N))."""
    N = 4 * 64 * 64
    z = P.randn([1138], 0, 0, 4, 64, 64)[0]
    z1 = P.randn([1138], 1, 0, 4, 64, 64)[0]
    zs = P.randn([1139], 0, 0, 4, 64, 64)[0]
    zl = P.randn([1138], 0, 1, 4, 64, 64)[0]
    b = 5 / math.sqrt(N)
    assert abs(z.mean()) < b and abs(z.var() - 1) < 5 * math.sqrt(2 / N)
    assert abs(z.mean() - 0.0055) < 1e-4 and abs(z.var() - 1.0076) < 1e-4           # the recorded values
    assert abs(_corr(z, z1)) < b and abs(_corr(z, zs)) < b and abs(_corr(z, zl)) < b
    assert abs(_corr(z[0], z[1])) < 5 / 64 and abs(_corr(z[0], z[2])) < 5 / 64      # 4096 values per channel
    assert abs(_corr(z[:, :, :-1], z[:, :, 1:])) < b and abs(_corr(z[:, :-1], z[:, 1:])) < b
    assert np.abs(z).max() <= math.sqrt(2 * 24 * math.log(2))


def test_philox_fp32_formula_error_and_layout():
    """The formula in NumPy fp32 against float64 (the recorded 1.6e-6, a tenth of the device tolerance), and the layout:
    channel c of a C = 3 draw is channel c of the C = 4 draw, channels 4..7 are block 1, images are independent of B."""
    worst = 0.0
    for seed in range(40):
        worst = max(worst, float(np.abs(P.randn([seed], 0, 0, 4, 128, 128, np.float32).astype(np.float64)
                                        - P.randn([seed], 0, 0, 4, 128, 128)).max()))
    assert worst < 2e-6, worst
    z8, z4, z3 = P.randn([7], 3, 0, 8, 5, 7), P.randn([7], 3, 0, 4, 5, 7), P.randn([7], 3, 0, 3, 5, 7)
    assert np.array_equal(z8[:, :4], z4) and np.array_equal(z4[:, :3], z3)
    w = P.words(7, 3, 0, 8, 5, 7)
    one = P.philox4x32_10([np.uint64(5 * 7 - 1), np.uint64(3), np.uint64(0), np.uint64(1)], (7, 0))
    assert [int(v) for v in w[4:, 4, 6]] == [int(v) for v in one]
    assert np.array_equal(P.randn([1, 7, 2], 3, 0, 4, 5, 7)[1], z4[0])
    big = 0x299f31d0a4093822
    assert np.array_equal(P.words(big, 2**32 - 1, 1, 4, 2, 2)[:, 1, 1],
                          np.array([int(v) for v in P.philox4x32_10(
                              [np.uint64(3), np.uint64(2**32 - 1), np.uint64(1), np.uint64(0)],
                              (0xa4093822, 0x299f31d0))], dtype=np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 2. DDIM with eta
# ---------------------------------------------------------------------------------------------------------------------
def _parent_ddim_table(sch, t):
    """The eta = 0 coefficients as the code before eta computed them, restated."""
    prev_t = sch._prev_timestep(t)
    ac_t = float(sch.alphas_cumprod[t])
    ac_prev = float(sch.alphas_cumprod[prev_t] if prev_t >= 0 else sch.final_alpha_cumprod)
    a, s, A, S = math.sqrt(ac_t), math.sqrt(1 - ac_t), math.sqrt(ac_prev), math.sqrt(1 - ac_prev)
    if sch.prediction_type == 'v_prediction':
        return A * a + S * s, S * a - A * s, 0.0
    if sch.prediction_type == 'sample':
        return S / s, A - S * a / s, 0.0
    return A / a, S - A * s / a, 0.0


def _ddim_cases():
    for pt in ('epsilon', 'v_prediction', 'sample'):
        for spacing in ('leading', 'trailing'):
            yield dict(prediction_type=pt, timestep_spacing=spacing)
    yield dict(prediction_type='v_prediction', timestep_spacing='trailing', rescale_betas_zero_snr=True)


def test_ddim_eta_zero_is_the_parents_table():
    for kw in _ddim_cases():
        for sch in (DDIMScheduler(**kw), DDIMScheduler(eta=0.0, **kw), with_eta(DDIMScheduler(eta=0.5, **kw), 0.0)):
            for n in (7, 50):
                sch.set_timesteps(n)
                for t in sch.timesteps.tolist():
                    assert sch.step_coefficients(t) == _parent_ddim_table(sch, t), (kw, n, t)
    zs = DDIMScheduler(prediction_type='v_prediction', timestep_spacing='trailing', rescale_betas_zero_snr=True)
    zs.set_timesteps(4)
    assert zs.timesteps[0] == 999 and float(zs.alphas_cumprod[999]) == 0.0
    assert zs.step_coefficients(999) == _parent_ddim_table(zs, 999)
    assert inspect.signature(DDIMScheduler.__init__).parameters['eta'].default == 0.0


@pytest.mark.parametrize('eta', [0.3, 1.0])
def test_ddim_eta_coefficients_match_the_formulas_and_the_stateful_step(eta):
    g = torch.Generator().manual_seed(5)
    x, m, z = (torch.randn(2, 4, 3, 5, generator=g, dtype=torch.float64) for _ in range(3))
    for kw in _ddim_cases():
        sch = DDIMScheduler(eta=eta, **kw)
        for n in (7, 50):
            sch.set_timesteps(n)
            for t in sch.timesteps.tolist():
                prev_t = sch._prev_timestep(t)
                a2 = float(sch.alphas_cumprod[t])
                A2 = float(sch.alphas_cumprod[prev_t] if prev_t >= 0 else sch.final_alpha_cumprod)
                a, s, A = math.sqrt(a2), math.sqrt(1 - a2), math.sqrt(A2)
                sigma = eta * math.sqrt((1 - A2) / (1 - a2)) * math.sqrt(1 - a2 / A2)
                Sp = math.sqrt((1 - A2) - sigma * sigma)
                want = {'epsilon': (A / a if a else None, Sp - A * s / a if a else None, sigma),
                        'v_prediction': (A * a + Sp * s, Sp * a - A * s, sigma),
                        'sample': (Sp / s, A - Sp * a / s, sigma)}[sch.prediction_type]
                cx, cm, cn = sch.step_coefficients(t)
                assert (cx, cm, cn) == pytest.approx(want, rel=1e-14, abs=0), (kw, n, t)
                assert cn > 0 or A2 == a2
                ref = sch.step(m, t, x, variance_noise=z)['prev_sample']
                got = cx * x + cm * m + cn * z
                assert float((got - ref).abs().max() / ref.abs().max()) < 1e-12, (kw, n, t)
    # without variance_noise the draw comes from the generator, and only then
    sch = DDIMScheduler(eta=eta)
    sch.set_timesteps(10)
    t = int(sch.timesteps[3])
    a = sch.step(m, t, x, generator=torch.Generator().manual_seed(3))['prev_sample']
    b = sch.step(m, t, x, generator=torch.Generator().manual_seed(3))['prev_sample']
    c = sch.step(m, t, x, generator=torch.Generator().manual_seed(4))['prev_sample']
    assert torch.equal(a, b) and not torch.equal(a, c)
    cx, cm, cn = sch.step_coefficients(t)
    zz = torch.randn(x.shape, generator=torch.Generator().manual_seed(3), dtype=x.dtype)
    assert torch.allclose(a, cx * x + cm * m + cn * zz, rtol=1e-12, atol=1e-12)


def test_ddim_eta_variance_stays_non_negative_on_every_grid():
    for kw in _ddim_cases():
        sch = DDIMScheduler(eta=1.0, **kw)
        for n in (1, 7, 50, 1000):
            sch.set_timesteps(n)
            for t in sch.timesteps.tolist():
                prev_t = sch._prev_timestep(t)
                a2 = float(sch.alphas_cumprod[t])
                A2 = float(sch.alphas_cumprod[prev_t] if prev_t >= 0 else sch.final_alpha_cumprod)
                sigma = sch._sigma(a2, A2)
                assert A2 >= a2 and (1 - A2) - sigma * sigma >= 0.0, (kw, n, t)
                assert all(math.isfinite(v) for v in sch.step_coefficients(t))


def test_eta_checks():
    for bad in (-0.1, 1.5, float('nan'), '0.5', None, True):
        with pytest.raises(ValueError, match='eta'):
            DDIMScheduler(eta=bad)
    own = DDIMScheduler()
    assert with_eta(own, None) is own and with_eta(own, 0.0) is own and not is_stochastic(own)
    hot = with_eta(own, 1)
    assert hot is not own and hot.eta == 1.0 and own.eta == 0.0 and hot.alphas_cumprod is own.alphas_cumprod
    assert is_stochastic(hot)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match='eta'):
            with_eta(own, bad)
    with pytest.raises(ValueError, match='eta'):
        with_eta(DPMSolverMultistepScheduler(), 0.5)


# ---------------------------------------------------------------------------------------------------------------------
# 3. DPM-Solver++ 2M SDE
# ---------------------------------------------------------------------------------------------------------------------
def _asl(sch, t):
    ac = float(sch.alphas_cumprod[t] if t >= 0 else sch.final_alpha_cumprod)
    if ac == 0.0:
        ac = 2.0**-24
    a, s = math.sqrt(ac), math.sqrt(1 - ac)
    return a, s, math.log(a / s)


def _sde_row(sch, i, first=False):
    """The update of the issue, transcribed: h = l_t - l_s, K = -a_t expm1(-2h), r = (l_s - l_s') / h."""
    n = sch.num_inference_steps
    t = int(sch.timesteps[i])
    a_s, s_s, l_s = _asl(sch, t)
    a_t, s_t, l_t = _asl(sch, sch._prev_timestep(t))
    ax, am = {'epsilon': (1 / a_s, -s_s / a_s), 'v_prediction': (a_s, -s_s), 'sample': (0.0, 1.0)}[sch.prediction_type]
    h = l_t - l_s
    K = -a_t * math.expm1(-2 * h)
    kx, kn = (s_t / s_s) * math.exp(-h), s_t * math.sqrt(-math.expm1(-2 * h))
    second = sch.solver_order == 2 and i > 0 and not first and not (sch.lower_order_final and n < 15 and i == n - 1)
    if not second:
        return ax, am, kx, K, 0.0, kn
    r = (l_s - _asl(sch, int(sch.timesteps[i - 1]))[2]) / h
    return ax, am, kx, K * (1 + 1 / (2 * r)), -K / (2 * r), kn


def _ode_row(sch, i, first=False):
    n = sch.num_inference_steps
    t = int(sch.timesteps[i])
    a_s, s_s, l_s = _asl(sch, t)
    a_t, s_t, l_t = _asl(sch, sch._prev_timestep(t))
    ax, am = {'epsilon': (1 / a_s, -s_s / a_s), 'v_prediction': (a_s, -s_s), 'sample': (0.0, 1.0)}[sch.prediction_type]
    h = l_t - l_s
    kd = -a_t * math.expm1(-h)
    second = sch.solver_order == 2 and i > 0 and not first and not (sch.lower_order_final and n < 15 and i == n - 1)
    if not second:
        return ax, am, s_t / s_s, kd, 0.0
    r = (l_s - _asl(sch, int(sch.timesteps[i - 1]))[2]) / h
    return ax, am, s_t / s_s, kd * (1.0 + 0.5 / r), -kd * (0.5 / r)


def _dpm_cases():
    for pt in ('epsilon', 'v_prediction', 'sample'):
        for spacing in ('leading', 'trailing'):
            yield dict(prediction_type=pt, timestep_spacing=spacing)
    yield dict(prediction_type='v_prediction', timestep_spacing='trailing', rescale_betas_zero_snr=True)
    yield dict(prediction_type='epsilon', lower_order_final=False)
    yield dict(prediction_type='epsilon', solver_order=1)


def test_sde_rows_match_the_transcribed_update():
    for kw in _dpm_cases():
        sch = DPMSolverMultistepScheduler(algorithm_type='sde-dpmsolver++', **kw)
        assert is_stochastic(sch) and sch.multistep
        for n in (5, 20):
            sch.set_timesteps(n)
            orders = []
            for i in range(n):
                row = sch.step_coefficients_sde(i)
                assert len(row) == 6 and row == pytest.approx(_sde_row(sch, i), rel=1e-13, abs=0), (kw, n, i)
                assert row[5] > 0
                orders.append(2 if row[4] != 0.0 else 1)
                rf = sch.step_coefficients_sde(i, first=True)
                assert rf[4] == 0.0 and rf == pytest.approx(_sde_row(sch, i, first=True), rel=1e-13, abs=0)
            if sch.solver_order == 2:
                last = 1 if (sch.lower_order_final and n < 15) else 2
                assert orders == [1] + [2] * (n - 2) + [last], (kw, n, orders)
            else:
                assert orders == [1] * n


def test_sde_stateful_step_follows_the_rows_over_a_schedule():
    g = torch.Generator().manual_seed(11)
    for kw in _dpm_cases():
        for n in (5, 20):
            for begin in (0, 2):
                sch = DPMSolverMultistepScheduler(algorithm_type='sde-dpmsolver++', **kw)
                sch.set_timesteps(n)
                if begin:
                    sch.set_begin_index(begin)
                x = torch.randn(2, 4, 3, 5, generator=g, dtype=torch.float64)
                y, hist = x.clone(), None
                for i in range(begin, n):
                    t = int(sch.timesteps[i])
                    m = torch.randn(x.shape, generator=g, dtype=torch.float64)
                    z = torch.randn(x.shape, generator=g, dtype=torch.float64)
                    ax, am, kx, k0, k1, kn = sch.step_coefficients_sde(i, first=(i == begin and begin > 0))
                    d = ax * y + am * m
                    y = kx * y + k0 * d + (k1 * hist if k1 != 0.0 else 0.0) + kn * z
                    hist = d
                    x = sch.step(m, t, x, variance_noise=z)['prev_sample']
                    assert float((x - y).abs().max() / x.abs().max()) < 1e-12, (kw, n, begin, i)
    sch = DPMSolverMultistepScheduler(algorithm_type='sde-dpmsolver++')
    sch.set_timesteps(5)
    x, m = torch.randn(1, 4, 2, 2, generator=g), torch.randn(1, 4, 2, 2, generator=g)
    a = sch.step(m, 801, x, generator=torch.Generator().manual_seed(1))['prev_sample']
    sch.set_timesteps(5)
    b = sch.step(m, 801, x, generator=torch.Generator().manual_seed(2))['prev_sample']
    assert not torch.equal(a, b)


def test_ode_rows_are_unchanged_and_names_resolve():
    for kw in _dpm_cases():
        for sch in (DPMSolverMultistepScheduler(**kw), DPMSolverMultistepScheduler(algorithm_type='sde-dpmsolver++', **kw)):
            for n in (5, 20):
                sch.set_timesteps(n)
                for i in range(n):
                    assert sch.step_coefficients_ms(i) == _ode_row(sch, i), (kw, n, i)
                    assert sch.step_coefficients_ms(i, first=True) == _ode_row(sch, i, first=True)
    assert not is_stochastic(DPMSolverMultistepScheduler()) and DPMSolverMultistepScheduler().algorithm_type == 'dpmsolver++'
    with pytest.raises(ValueError, match='algorithm_type'):
        DPMSolverMultistepScheduler(algorithm_type='dpmsolver')
    # the deterministic table keeps its two names; the SDE solver's name lives beside it and resolves wherever a name is taken
    assert tuple(INFERENCE_SCHEDULERS) == ('ddim', 'dpm++2m') and tuple(STOCHASTIC_INFERENCE_SCHEDULERS) == ('dpm++2m-sde',)
    assert type(make_inference_scheduler('dpm++2m-sde')).__name__ == 'DPMSolverSDEMultistepScheduler'
    own = DDIMScheduler(prediction_type='v_prediction', timestep_spacing='trailing')
    sde = make_inference_scheduler('dpm++2m-sde', like=own)
    assert isinstance(sde, DPMSolverMultistepScheduler) and sde.algorithm_type == 'sde-dpmsolver++'
    assert sde.prediction_type == 'v_prediction' and sde.timestep_spacing == 'trailing' and sde.alphas_cumprod is own.alphas_cumprod
    ode = DPMSolverMultistepScheduler()
    assert resolve_inference_scheduler('dpm++2m', ode) is ode and resolve_inference_scheduler('dpm++2m-sde', sde) is sde
    assert resolve_inference_scheduler('dpm++2m-sde', ode).algorithm_type == 'sde-dpmsolver++'
    assert resolve_inference_scheduler('dpm++2m', sde).algorithm_type == 'dpmsolver++'
    assert resolve_inference_scheduler('ddim', own) is own
    # the stateful ODE step does not look at variance_noise
    ode.set_timesteps(5)
    x = torch.ones(1, 4, 2, 2)
    a = ode.step(x, 801, x, variance_noise=torch.full_like(x, 9.0))['prev_sample']
    ode.set_timesteps(5)
    assert torch.equal(a, ode.step(x, 801, x)['prev_sample'])


def test_device_rows_carry_the_draw_number_as_a_bit_pattern():
    from diffusion_amd.sampling import coef_row_width, stochastic_rows
    assert [coef_row_width(ms, bl, False) for ms in (False, True) for bl in (False, True)] == [4, 8, 8, 8]
    assert [coef_row_width(ms, bl, True) for ms in (False, True) for bl in (False, True)] == [8, 8, 12, 12]
    draws = [0, 1, 2**24 + 1, 2**31, 2**32 - 1]
    rows = [[0.1 * (i + 1)] * 8 for i in range(len(draws))]
    tab = stochastic_rows(rows, 6, draws)
    assert tab.dtype == torch.float32 and tab.shape == (5, 8)
    assert [v & 0xffffffff for v in tab.view(torch.int32)[:, 6].tolist()] == draws
    keep = [c for c in range(8) if c != 6]
    assert torch.equal(tab[:, keep], torch.tensor(rows, dtype=torch.float64).to(torch.float32)[:, keep])


# ---------------------------------------------------------------------------------------------------------------------
# 4. every ValueError of the public interface, with no device present
# ---------------------------------------------------------------------------------------------------------------------
class _NoDeviceUNet:
    """Answers the host-side questions of LatentSampler.sample and fails the test at the first look for a device."""
    _sampler_graphs = None
    cfg = types.SimpleNamespace(in_channels=4)

    def check_spatial(self, H, W):
        pass

    def __getattr__(self, name):
        pytest.fail(f'looked for a device ({name})')


def test_latent_sampler_needs_seeds_for_a_stochastic_schedule():
    from diffusion_amd.sampling import LatentSampler
    lat, cond = torch.zeros(2, 4, 8, 8), torch.zeros(2, 77, 16)
    for sch in (DDIMScheduler(eta=1.0), DPMSolverMultistepScheduler(algorithm_type='sde-dpmsolver++')):
        smp = LatentSampler(_NoDeviceUNet(), sch)
        with pytest.raises(ValueError, match='seeds'):
            smp.sample(lat, cond, cond, num_inference_steps=4, guidance_scale=3.0)
        for bad in ([1], [1, 2, 3], [1, -2], [1, 2**64], [1.5, 2], 'ab'):
            with pytest.raises(ValueError, match='seeds'):
                smp.sample(lat, cond, cond, num_inference_steps=4, guidance_scale=3.0, seeds=bad)
    p = inspect.signature(LatentSampler.sample).parameters['seeds']
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY


def test_seed_argument_checks():
    from diffusion_amd.sampling import check_seed, image_seeds
    assert check_seed(None, 3) is None and check_seed(7, 3) == 7 and check_seed(0, 3) == 0
    assert check_seed([1, 2, 2**64 - 1], 3) == [1, 2, 2**64 - 1] and check_seed((4, 5), 2) == [4, 5]
    assert check_seed(torch.tensor([4, 5]), 2) == [4, 5]
    for bad in ([1, 2], [1, 2, 3, 4], [1, 2, -1], [1, 2, 2**64], [1, 2, 0.5], 'abc', 1.5, True):
        with pytest.raises(ValueError, match='seed'):
            check_seed(bad, 3)
    assert image_seeds([1, 2, 2**64 - 1], 3, False, None) == [1, 2, 2**64 - 1]     # a list is used whatever the sampler
    assert image_seeds(7, 3, False, None) is None and image_seeds(None, 3, False, None) is None
    assert image_seeds(7, 3, True, None) == [7, 8, 9] and image_seeds(2**64 - 1, 2, True, None) == [2**64 - 1, 0]
    gen = torch.Generator().manual_seed(3)
    a = image_seeds(None, 2, True, gen)
    assert a[1] == a[0] + 1 and a == image_seeds(None, 2, True, torch.Generator().manual_seed(3))


def _sd_stub(scheduler):
    class _Stub:
        inference_scheduler, guidance_rescale = scheduler, 0.0

        def __getattr__(self, name):
            pytest.fail(f'looked for a device ({name})')
    return _Stub()


def _pixel_stub(scheduler, continuous):
    class _Stub:
        inference_scheduler, continuous_time = scheduler, continuous

        def __getattr__(self, name):
            pytest.fail(f'looked for a device ({name})')
    return _Stub()


def test_generate_checks_raise_before_the_device():
    from diffusion_amd.models.pixel_diffusion import PixelDiffusion
    from diffusion_amd.models.stable_diffusion import StableDiffusion
    from diffusion_amd.schedulers.schedulers import ContinuousTimeScheduler
    sd, px = StableDiffusion.generate, PixelDiffusion.generate
    for gen, stub in ((sd, _sd_stub(DDIMScheduler())), (px, _pixel_stub(DDIMScheduler(), False))):
        for bad in (-0.1, 1.5, float('nan'), '1'):
            with pytest.raises(ValueError, match='eta'):
                gen(stub, prompt=['a', 'b'], eta=bad)
        for name in ('dpm++2m', 'dpm++2m-sde'):
            with pytest.raises(ValueError, match='eta'):
                gen(stub, prompt=['a', 'b'], eta=0.5, inference_scheduler=name)
        with pytest.raises(ValueError, match='eta'):
            gen(stub, prompt=['a', 'b'], eta=0.5, inference_scheduler=DPMSolverMultistepScheduler())
        for bad in ([1], [1, 2, 3], [1, -1], [1, 2**64]):
            with pytest.raises(ValueError, match='seed'):
                gen(stub, prompt=['a', 'b'], seed=bad, eta=1.0)
        with pytest.raises(ValueError, match='seed'):     # one seed per generated image, the copies included
            gen(stub, prompt=['a', 'b'], seed=[1, 2], num_images_per_prompt=2, inference_scheduler='dpm++2m-sde')
        with pytest.raises(ValueError, match='inference_scheduler'):
            gen(stub, prompt=['a'], inference_scheduler='dpm++2m-sde-karras')
        p = inspect.signature(gen).parameters
        assert p['eta'].default is None and p['seed'].default is None
    cont = _pixel_stub(ContinuousTimeScheduler(), True)
    with pytest.raises(ValueError, match='discrete-time'):
        px(cont, prompt=['a'], inference_scheduler='dpm++2m-sde')
    with pytest.raises(ValueError, match='eta'):
        px(cont, prompt=['a'], eta=0.5)
    with pytest.raises(ValueError, match='discrete-time'):
        check_inference_scheduler('dpm++2m-sde', continuous_time=True)


def test_factory_checks_raise_before_the_device(monkeypatch):
    from diffusion_amd.models import models as M
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: pytest.fail('looked for a device'))
    for factory, kw in ((M.stable_diffusion_2, dict(model_name='tiny', pretrained=False)), (M.discrete_pixel_diffusion, {})):
        for bad in (-0.5, 1.5, 'x'):
            with pytest.raises(ValueError, match='eta'):
                factory(inference_eta=bad, **kw)
        for name in ('dpm++2m', 'dpm++2m-sde'):
            with pytest.raises(ValueError, match='inference_eta'):
                factory(inference_eta=0.5, inference_scheduler=name, **kw)
        with pytest.raises(ValueError, match='inference_scheduler'):
            factory(inference_scheduler='dpm++2m-ode', **kw)
        assert inspect.signature(factory).parameters['inference_eta'].default == 0.0
    with pytest.raises(ValueError, match='discrete-time'):
        M.continuous_pixel_diffusion(inference_scheduler='dpm++2m-sde')


def test_entry_points_are_declared_and_bound():
    from diffusion_amd import _lib, ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'diffusion_amd.h')).read()
    for name, arity in (('da_randn_philox', 10), ('da_sampler_step_rng', 18)):
        assert f'int {name}(' in header and len(_lib.SIGNATURES[name]) == arity
    assert callable(ops.randn_philox) and callable(ops.sampler_step_rng) and callable(ops.philox_seeds)
    s = ops.philox_seeds([0, 1, 2**64 - 1, 0x299f31d0a4093822])
    assert s.dtype == torch.uint64 and s.view(torch.int64).tolist() == [0, 1, -1, 0x299f31d0a4093822]
