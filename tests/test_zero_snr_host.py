"""Host-side tests of zero-terminal-SNR schedules, trailing timestep spacing, the Min-SNR weight table and guidance rescale
in torch ops: everything here runs without a GPU.

  1. the rescaled beta table against a float64 restatement of the recipe, known values, and the unrescaled tables bit for bit
  2. trailing grids against the formula; leading grids and coefficients bit-equal to the values recorded before
     ``timestep_spacing`` existed (tests/golden/zero_snr_parent_leading.json, float.hex() strings)
  3. DDIM on a trailing grid against a float64 loop that steps to the next grid entry
  4. abar_t = 0 in the steps: the closed forms, the 2^-24 rule of DPM-Solver++, the epsilon refusals
  5. the Min-SNR table against float64, its argument checks
  6. the option checks of the factory and of ``generate()``, reached through their helper functions
  7. ``rescale_noise_cfg`` against float64
"""
import hashlib
import inspect
import json
import math
import os

import numpy as np
import pytest
import torch

from diffusion_amd.models.schedulers import (DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler,
                                             make_inference_scheduler, min_snr_weights, trailing_timesteps,
                                             with_timestep_spacing)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
GOLDEN = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'zero_snr_parent_leading.json')))
PRED_TYPES = ('epsilon', 'v_prediction', 'sample')


def fromhex(row):
    return tuple(float.fromhex(h) for h in row)


# ---------------------------------------------------------------------------------------------------------------------
# 1. tables
# ---------------------------------------------------------------------------------------------------------------------
def recipe64():
    """Algorithm 1 of arXiv:2305.08891 in float64 from float64 betas: (betas, alphas_cumprod)"""
    betas = torch.linspace(0.00085**0.5, 0.012**0.5, 1000, dtype=F64)**2
    s = torch.cumprod(1 - betas, 0).sqrt()
    s0, sT = s[0].clone(), s[-1].clone()
    s = (s - sT) * (s0 / (s0 - sT))
    abar = s**2
    alphas = torch.cat([abar[:1], abar[1:] / abar[:-1]])
    return 1 - alphas, torch.cumprod(alphas, 0)


@pytest.mark.parametrize('cls', [DDPMScheduler, DDIMScheduler, DPMSolverMultistepScheduler])
def test_rescaled_table(cls):
    sch, plain = cls(rescale_betas_zero_snr=True), cls()
    ac = sch.alphas_cumprod
    assert ac.dtype == torch.float32 and sch.rescale_betas_zero_snr and not plain.rescale_betas_zero_snr
    assert float(ac[999]) == 0.0 and float(sch.betas[999]) == 1.0
    assert float(ac[0]) == float(plain.alphas_cumprod[0]) == 0.9991499781608582
    _, ac64 = recipe64()
    rel = ((ac.double() - ac64).abs() / ac64)[:999].max().item()
    print(f'rescaled fp32 table vs the float64 recipe: worst relative difference {rel:.3g} over t < 999')
    assert rel <= 1e-4
    for t, v in ((1, 0.998233497), (249, 0.654188693), (499, 0.242358997), (500, 0.241018549), (749, 0.0331714563),
                 (998, 1.96796293e-07)):
        assert abs(float(ac[t]) - v) <= 5e-9 * v * 10, (t, float(ac[t]), v)     # nine printed digits
    assert bool((ac[1:] < ac[:-1]).all())
    # what add_noise / get_velocity give at the last timestep: x_t = eps, v = -x0
    g = torch.Generator().manual_seed(3)
    x0, eps = torch.randn(2, 4, 3, 3, generator=g), torch.randn(2, 4, 3, 3, generator=g)
    t = torch.tensor([999, 999])
    assert torch.equal(sch.add_noise(x0, eps, t), eps) and torch.equal(sch.get_velocity(x0, eps, t), -x0)
    assert sch.add_noise_coefficients(999) == (0.0, 1.0)
    sa, sb = sch.device_tables('cpu')
    assert float(sa[999]) == 0.0 and float(sb[999]) == 1.0


@pytest.mark.parametrize('cls', [DDPMScheduler, DDIMScheduler, DPMSolverMultistepScheduler])
def test_unrescaled_tables_keep_their_bits(cls):
    for sch in (cls(), cls(rescale_betas_zero_snr=False)):
        for k, digest in GOLDEN['table_sha256'].items():
            assert hashlib.sha256(getattr(sch, k).numpy().tobytes()).hexdigest() == digest, k
        for k, rows in GOLDEN['tables'].items():
            assert [float(getattr(sch, k)[i]).hex() for i in GOLDEN['table_index']] == rows, k


def test_make_inference_scheduler_copies_the_rescaled_tables_and_the_spacing():
    like = DDIMScheduler(prediction_type='v_prediction', rescale_betas_zero_snr=True, timestep_spacing='trailing')
    for name in ('ddim', 'dpm++2m'):
        sch = make_inference_scheduler(name, like=like)
        assert sch.alphas_cumprod is like.alphas_cumprod and sch.timestep_spacing == 'trailing'
        assert sch.rescale_betas_zero_snr and sch.prediction_type == 'v_prediction'
    assert make_inference_scheduler('dpm++2m', like=DDPMScheduler()).timestep_spacing == 'leading'


# ---------------------------------------------------------------------------------------------------------------------
# 2. grids
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls', [DDIMScheduler, DPMSolverMultistepScheduler])
@pytest.mark.parametrize('n', [1, 4, 20, 30, 50, 1000])
def test_trailing_grid(cls, n):
    sch = cls(timestep_spacing='trailing')
    sch.set_timesteps(n)
    ts = sch.timesteps.tolist()
    want = (np.round(np.arange(1000, 0, -1000 / n)) - 1).astype(np.int64).tolist()
    assert ts == want == trailing_timesteps(1000, n).tolist()
    assert len(ts) == n and ts[0] == 999 and all(a > b for a, b in zip(ts, ts[1:])) and ts[-1] >= 0
    known = {1: [999], 4: [999, 749, 499, 249], 1000: list(range(999, -1, -1))}
    if n in known:
        assert ts == known[n]
    if n == 30:
        assert ts[:4] == [999, 966, 932, 899] and ts[-3:] == [99, 66, 32]
    if n == 50:
        assert ts[:2] == [999, 979] and ts[-1] == 19


@pytest.mark.parametrize('cls', [DDIMScheduler, DPMSolverMultistepScheduler])
def test_unknown_spacing_raises(cls):
    for bad in ('linspace', 'Trailing', None, 0):
        with pytest.raises(ValueError, match='timestep_spacing'):
            cls(timestep_spacing=bad)
    with pytest.raises(ValueError, match='timestep_spacing'):
        with_timestep_spacing(cls(), 'linspace')
    sch = cls()
    assert with_timestep_spacing(sch, None) is sch and with_timestep_spacing(sch, 'leading') is sch
    other = with_timestep_spacing(sch, 'trailing')
    assert other is not sch and other.timestep_spacing == 'trailing' and sch.timestep_spacing == 'leading'
    assert other.alphas_cumprod is sch.alphas_cumprod


@pytest.mark.parametrize('case', GOLDEN['cases'], ids=lambda c: f"{c['solver']}-{c['n']}-{c['prediction_type']}")
@pytest.mark.parametrize('explicit', [False, True])
def test_leading_is_bit_equal_to_the_recorded_values(case, explicit):
    kw = dict(timestep_spacing='leading') if explicit else {}
    cls = DDIMScheduler if case['solver'] == 'ddim' else DPMSolverMultistepScheduler
    sch = cls(prediction_type=case['prediction_type'], **kw)
    sch.set_timesteps(case['n'])
    assert sch.timesteps.tolist() == case['timesteps']
    for i, (t, row) in enumerate(zip(case['timesteps'], case['coefficients'])):
        got = sch.step_coefficients(t) if case['solver'] == 'ddim' else sch.step_coefficients_ms(i)
        assert tuple(c.hex() for c in got) == tuple(row), (i, t)


# ---------------------------------------------------------------------------------------------------------------------
# 3. DDIM on a trailing grid
# ---------------------------------------------------------------------------------------------------------------------
def linear_model(x, t):
    """a fixed linear 'model' in float64"""
    return 0.3 * x.flip(-1) - 0.1 * x + 0.01 * (t / 1000.0)


def ddim_loop64(ac, final, ts, pt, x):
    """eta = 0 DDIM in float64; the step from grid entry i goes to entry i + 1, the last one to `final`"""
    for i, t in enumerate(ts):
        a_t = float(ac[t])
        a_p = float(ac[ts[i + 1]]) if i + 1 < len(ts) else float(final)
        m = linear_model(x, t)
        if pt == 'v_prediction':
            x0, eps = math.sqrt(a_t) * x - math.sqrt(1 - a_t) * m, math.sqrt(a_t) * m + math.sqrt(1 - a_t) * x
        elif pt == 'sample':
            x0, eps = m, (x - math.sqrt(a_t) * m) / math.sqrt(1 - a_t)
        else:
            eps, x0 = m, (x - math.sqrt(1 - a_t) * m) / math.sqrt(a_t)
        x = math.sqrt(a_p) * x0 + math.sqrt(1 - a_p) * eps
    return x


@pytest.mark.parametrize('pt', PRED_TYPES)
def test_ddim_trailing_steps_to_the_next_grid_entry(pt):
    sch = DDIMScheduler(prediction_type=pt, timestep_spacing='trailing')
    sch.set_timesteps(30)
    ts = sch.timesteps.tolist()
    assert any(a - b != 1000 // 30 for a, b in zip(ts, ts[1:]))        # the grid is not t - T // n
    x0 = torch.randn(2, 4, 5, 6, generator=torch.Generator().manual_seed(5), dtype=F64)
    want = ddim_loop64(sch.alphas_cumprod, sch.final_alpha_cumprod, ts, pt, x0)
    x, xc = x0, x0
    for t in ts:
        x = sch.step(linear_model(x, t), t, x)['prev_sample']
        cx, cm, cn = sch.step_coefficients(t)
        xc = cx * xc + cm * linear_model(xc, t)
        assert cn == 0.0
    assert x.dtype == F64
    for got in (x, xc):
        assert ((got - want).norm() / want.norm()).item() < 1e-12
    # the last step lands on final_alpha_cumprod: for x0-prediction the result is sqrt(final) m + sqrt(1 - final) eps
    t = ts[-1]
    a_t, a_f = float(sch.alphas_cumprod[t]), float(sch.final_alpha_cumprod)
    A, S, a, s = math.sqrt(a_f), math.sqrt(1 - a_f), math.sqrt(a_t), math.sqrt(1 - a_t)
    want_last = {'v_prediction': (A * a + S * s, S * a - A * s), 'sample': (S / s, A - S * a / s),
                 'epsilon': (A / a, S - A * s / a)}[pt]
    assert sch.step_coefficients(t)[:2] == pytest.approx(want_last, rel=1e-15)
    with pytest.raises(ValueError, match='grid'):
        sch.step_coefficients(ts[0] - 1)                               # not a grid entry


# ---------------------------------------------------------------------------------------------------------------------
# 4. abar_t = 0
# ---------------------------------------------------------------------------------------------------------------------
def zsnr(cls, pt, n=4):
    sch = cls(prediction_type=pt, rescale_betas_zero_snr=True, timestep_spacing='trailing')
    sch.set_timesteps(n)
    return sch


def test_ddim_first_step_from_pure_noise():
    for pt in ('v_prediction', 'sample'):
        sch = zsnr(DDIMScheduler, pt)
        ac = float(sch.alphas_cumprod[749])
        A, S = math.sqrt(ac), math.sqrt(1 - ac)
        cx, cm, cn = sch.step_coefficients(999)
        assert all(math.isfinite(c) for c in (cx, cm, cn))
        assert (cx, cm, cn) == ((S, -A, 0.0) if pt == 'v_prediction' else (S, A, 0.0))
        x = torch.randn(1, 4, 3, 3, generator=torch.Generator().manual_seed(7), dtype=F64)
        m = linear_model(x, 999)
        got = sch.step(m, 999, x)['prev_sample']
        assert bool(torch.isfinite(got).all()) and ((got - (cx * x + cm * m)).abs().max().item() < 1e-15)


@pytest.mark.parametrize('cls', [DDIMScheduler, DPMSolverMultistepScheduler])
def test_epsilon_on_a_zero_snr_table_raises(cls):
    sch = zsnr(cls, 'epsilon')
    x = torch.zeros(1, 4, 2, 2)
    calls = [lambda: sch.step(x, 999, x)]
    calls.append((lambda: sch.step_coefficients(999)) if cls is DDIMScheduler else (lambda: sch.step_coefficients_ms(0)))
    for call in calls:
        with pytest.raises(ValueError, match='zero terminal SNR') as e:
            call()
        assert 'prediction_type' in str(e.value)
    # the steps that do not touch the last timestep still work
    if cls is DDIMScheduler:
        assert all(math.isfinite(c) for c in sch.step_coefficients(749))
    from diffusion_amd.models.schedulers import check_zero_snr_grid
    with pytest.raises(ValueError, match='zero terminal SNR'):
        check_zero_snr_grid(sch)
    check_zero_snr_grid(zsnr(cls, 'v_prediction'))


def asl64(ac):
    a, s = math.sqrt(ac), math.sqrt(1 - ac)
    return a, s, math.log(a / s)


@pytest.mark.parametrize('pt', ['v_prediction', 'sample'])
def test_dpm_reads_a_zero_table_value_as_two_to_the_minus_24(pt):
    sch = zsnr(DPMSolverMultistepScheduler, pt)
    ts = sch.timesteps.tolist()
    assert ts == [999, 749, 499, 249]
    ac = [2.0**-24] + [float(sch.alphas_cumprod[t]) for t in ts[1:]] + [float(sch.final_alpha_cumprod)]
    (a_s, s_s, l_s), (a_t, s_t, l_t) = asl64(ac[0]), asl64(ac[1])
    h = l_t - l_s
    ax, am = (a_s, -s_s) if pt == 'v_prediction' else (0.0, 1.0)
    want = (ax, am, s_t / s_s, -a_t * math.expm1(-h), 0.0)
    got = sch.step_coefficients_ms(0)
    assert got == pytest.approx(want, rel=1e-15) and got[4] == 0.0 and all(math.isfinite(c) for c in got)
    assert sch._alpha_sigma_lambda(999)[0] == 2.0**-12
    # the second step is second order, with finite coefficients, and equals the float64 formula
    (a_s2, s_s2, l_s2), (a_t2, s_t2, l_t2) = asl64(ac[1]), asl64(ac[2])
    h2 = l_t2 - l_s2
    r = (l_s2 - l_s) / h2
    kd = -a_t2 * math.expm1(-h2)
    got2 = sch.step_coefficients_ms(1)
    assert all(math.isfinite(c) for c in got2) and got2[4] != 0.0
    assert got2[2:] == pytest.approx((s_t2 / s_s2, kd * (1 + 0.5 / r), -kd * 0.5 / r), rel=1e-14)
    # the stateful step() walks the same numbers
    x = torch.randn(1, 4, 3, 3, generator=torch.Generator().manual_seed(9), dtype=F64)
    xs, xc, hist = x, x, None
    for i, t in enumerate(ts):
        xs = sch.step(linear_model(xs, t), t, xs)['prev_sample']
        cax, cam, kx, k0, k1 = sch.step_coefficients_ms(i)
        d = cax * xc + cam * linear_model(xc, t)
        xc = kx * xc + k0 * d + (k1 * hist if k1 != 0.0 else 0.0)
        hist = d
    assert bool(torch.isfinite(xs).all()) and ((xs - xc).norm() / xc.norm()).item() < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# 5. the Min-SNR table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rescaled', [False, True])
@pytest.mark.parametrize('gamma', [1.0, 5.0, 20.0])
@pytest.mark.parametrize('pt', ['epsilon', 'v_prediction'])
def test_min_snr_table(pt, gamma, rescaled):
    ac = DDPMScheduler(rescale_betas_zero_snr=rescaled).alphas_cumprod
    w = min_snr_weights(ac, gamma, pt)
    assert w.dtype == F64 and w.shape == (1000,) and bool(torch.isfinite(w).all()) and bool((w >= 0).all())
    for t in range(1000):       # a scalar restatement in Python floats (float64)
        a = float(ac[t])
        snr = a / (1.0 - a)
        if pt == 'epsilon':
            want = 1.0 if snr == 0.0 else min(snr, gamma) / snr
        else:
            want = min(snr, gamma) / (snr + 1.0)
        assert abs(float(w[t]) - want) <= 4e-16 * max(want, 1e-300), (t, float(w[t]), want)
    if rescaled:                # SNR = 0 at the last timestep: the limit 1 for epsilon, 0 for v
        assert float(w[999]) == (1.0 if pt == 'epsilon' else 0.0)
    if rescaled and gamma == 5.0:
        # the values of the feature request were taken from a float64 table; the fp32 table's own rounding of abar, divided
        # by 1 - abar, moves them by up to 7e-5 relative (at t = 0, where 1 - abar = 8.5e-4)
        known = {'epsilon': {0: 0.00425362, 100: 0.638496, 500: 1.0},
                 'v_prediction': {0: 0.00425000, 100: 0.566194, 500: 0.241019, 999: 0.0}}[pt]
        for t, v in known.items():
            assert abs(float(w[t]) - v) <= 1e-4 * v, (t, float(w[t]), v)


def test_snr_gamma_argument_checks():
    from diffusion_amd.models.schedulers import check_snr_gamma
    from diffusion_amd.models.stable_diffusion import _check_loss_options
    import torch.nn.functional as F
    ac = DDPMScheduler().alphas_cumprod
    for bad in (0, 0.0, -1, -1.0, float('inf'), float('nan'), '5', True):
        with pytest.raises(ValueError, match='snr_gamma'):
            check_snr_gamma(bad)
        with pytest.raises(ValueError, match='snr_gamma'):
            _check_loss_options(bad, F.mse_loss)
        with pytest.raises(ValueError, match='snr_gamma'):
            min_snr_weights(ac, bad, 'epsilon')
    assert check_snr_gamma(None) is None and check_snr_gamma(5) == 5.0 and _check_loss_options(None, F.l1_loss) is None
    assert _check_loss_options(5.0, F.mse_loss) == 5.0
    with pytest.raises(ValueError, match='loss_fn'):
        _check_loss_options(5.0, F.l1_loss)
    with pytest.raises(ValueError, match='epsilon and v_prediction'):
        min_snr_weights(ac, 5.0, 'sample')


def test_stable_diffusion_constructor_checks_and_graph_cache_declines():
    """the constructor runs its checks first, before it touches any of its modules"""
    import torch.nn.functional as F
    from diffusion_amd.graph_step import GraphStepCache
    from diffusion_amd.models.stable_diffusion import StableDiffusion
    names = list(inspect.signature(StableDiffusion.__init__).parameters)
    assert names[names.index('prediction_type') + 1] == 'snr_gamma'
    assert inspect.signature(StableDiffusion.__init__).parameters['snr_gamma'].default is None
    kw = dict(unet=None, vae=None, text_encoder=None, tokenizer=None, noise_scheduler=DDPMScheduler(),
              inference_noise_scheduler=DDIMScheduler())
    with pytest.raises(ValueError, match='loss_fn'):
        StableDiffusion(**kw, snr_gamma=5.0, loss_fn=F.l1_loss)
    for bad in (0, -1, float('inf'), float('nan'), '5'):
        with pytest.raises(ValueError, match='snr_gamma'):
            StableDiffusion(**kw, snr_gamma=bad)
    with pytest.raises(ValueError, match='guidance_rescale'):
        StableDiffusion(**kw, guidance_rescale=1.5)

    class _Model:
        precomputed_latents, image_latents_key, text_latents_key = True, 'image_latents', 'caption_latents'
        snr_gamma = None
    batch = {'image_latents': 0, 'caption_latents': 0}
    m = _Model()
    m.loss_fn = F.mse_loss
    assert GraphStepCache(m).usable(batch)
    m.snr_gamma = 5.0
    assert not GraphStepCache(m).usable(batch)      # declining keeps the weighting: the eager path runs


# ---------------------------------------------------------------------------------------------------------------------
# 6. the option checks of the factory and of generate()
# ---------------------------------------------------------------------------------------------------------------------
def test_factory_option_checks(monkeypatch):
    from diffusion_amd.models import models as M
    from diffusion_amd.models.unet import UNetConfig
    chk = M._check_zero_snr_options
    assert chk(False, 'epsilon', None, 0.0, None) == 'leading' and chk(True, 'v_prediction', None, 0.7, 5.0) == 'trailing'
    assert chk(True, 'v_prediction', 'leading', 0.0, None) == 'leading' and chk(False, 'epsilon', 'trailing', 1, None) == 'trailing'
    with pytest.raises(ValueError, match='zero_terminal_snr'):
        chk(True, 'epsilon', None, 0.0, None)
    for bad in (1.5, -0.1, float('nan'), '0.5', None):
        with pytest.raises(ValueError, match='guidance_rescale'):
            chk(False, 'epsilon', None, bad, None)
    with pytest.raises(ValueError, match='timestep_spacing'):
        chk(False, 'epsilon', 'linspace', 0.0, None)
    with pytest.raises(ValueError, match='snr_gamma'):
        chk(False, 'epsilon', None, 0.0, -5.0)
    # in the factory these checks come before the device check
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: pytest.fail('looked for a device'))
    with pytest.raises(ValueError, match='zero_terminal_snr'):
        M.stable_diffusion_2(model_name='tiny', pretrained=False, zero_terminal_snr=True)           # tiny predicts epsilon
    with pytest.raises(ValueError, match='zero_terminal_snr'):
        M.stable_diffusion_2(model_name='stabilityai/stable-diffusion-2-base', pretrained=False, zero_terminal_snr=True)
    vcfg = UNetConfig.tiny()
    vcfg.prediction_type = 'v_prediction'
    for kw, what in ((dict(guidance_rescale=1.5), 'guidance_rescale'), (dict(timestep_spacing='x'), 'timestep_spacing'),
                     (dict(snr_gamma=0.0), 'snr_gamma')):
        with pytest.raises(ValueError, match=what):
            M.stable_diffusion_2(model_name='tiny', pretrained=False, unet_config=vcfg, zero_terminal_snr=True, **kw)
    p = inspect.signature(M.stable_diffusion_2).parameters
    assert [p[k].default for k in ('zero_terminal_snr', 'snr_gamma', 'timestep_spacing', 'guidance_rescale')] == \
        [False, None, None, 0.0]


def test_generate_option_checks():
    from diffusion_amd.models.stable_diffusion import StableDiffusion, _resolve_sampling_options as res
    own = DDIMScheduler(prediction_type='v_prediction', rescale_betas_zero_snr=True, timestep_spacing='trailing')
    sch, phi = res(None, own, None, 0.7, None, 4)
    assert sch is own and phi == 0.7 and sch.timesteps.tolist() == [999, 749, 499, 249]
    sch, phi = res(None, own, 0.25, 0.7, 'leading', 4)
    assert sch is not own and phi == 0.25 and sch.timesteps.tolist() == [751, 501, 251, 1] and own.timestep_spacing == 'trailing'
    sch, phi = res('dpm++2m', own, 0, 0.7, None, 4)
    assert isinstance(sch, DPMSolverMultistepScheduler) and sch.timestep_spacing == 'trailing' and phi == 0.0
    for bad in (1.5, -0.5, float('nan'), 'x'):
        with pytest.raises(ValueError, match='guidance_rescale'):
            res(None, own, bad, 0.0, None, 4)
    with pytest.raises(ValueError, match='timestep_spacing'):
        res(None, own, None, 0.0, 'linspace', 4)
    for name in (None, 'dpm++2m'):      # epsilon prediction on the rescaled table, on a grid that starts at T - 1
        eps = DDIMScheduler(prediction_type='epsilon', rescale_betas_zero_snr=True, timestep_spacing='trailing')
        with pytest.raises(ValueError, match='zero terminal SNR'):
            res(name, eps, None, 0.0, None, 4)
    p = inspect.signature(StableDiffusion.generate).parameters
    assert p['guidance_rescale'].default is None and p['timestep_spacing'].default is None


def test_latent_sampler_checks_guidance_rescale_before_the_device():
    from diffusion_amd.sampling import LatentSampler

    class _NoDevice:
        _sampler_graphs = None

        def __getattr__(self, name):
            pytest.fail(f'looked for a device ({name})')
    lat, cond = torch.zeros(1, 4, 8, 8), torch.zeros(1, 77, 16)
    for bad in (1.5, -0.1, float('nan')):
        with pytest.raises(ValueError, match='guidance_rescale'):
            LatentSampler(_NoDevice(), DDIMScheduler()).sample(lat, cond, cond, num_inference_steps=4, guidance_scale=3.0,
                                                               guidance_rescale=bad)
    p = inspect.signature(LatentSampler.sample).parameters['guidance_rescale']
    assert p.default == 0.0 and p.kind is inspect.Parameter.KEYWORD_ONLY


def test_entry_points_are_declared_and_bound():
    from diffusion_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'diffusion_amd.h')).read()
    for name, arity in (('da_mse_loss_w', 15), ('da_guidance_rescale', 9), ('da_sampler_step_rs', 13),
                        ('da_sampler_step_ms_rs', 13), ('da_sampler_step_blend_rs', 16), ('da_sampler_step_ms_blend_rs', 16)):
        assert f'int {name}(const float* ' in header, name
        assert len(_lib.SIGNATURES[name]) == arity, name
    assert callable(ops.mse_loss_w) and callable(ops.guidance_rescale)
    for fn in (ops.sampler_step, ops.sampler_step_ms, ops.sampler_step_blend, ops.sampler_step_ms_blend):
        p = inspect.signature(fn).parameters
        assert p['factor'].default is None and p['HW'].default is None


# ---------------------------------------------------------------------------------------------------------------------
# 7. guidance rescale in torch ops
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('phi', [0.3, 0.7, 1.0])
@pytest.mark.parametrize('g', [1.5, 7.5])
def test_rescale_noise_cfg_against_float64(g, phi):
    from diffusion_amd.sampling import rescale_noise_cfg
    gen = torch.Generator().manual_seed(11)
    pu, pt = torch.randn(3, 4, 5, 7, generator=gen), torch.randn(3, 4, 5, 7, generator=gen) + 0.5
    m = pu + g * (pt - pu)
    got = rescale_noise_cfg(m, pt, phi)
    m64, pt64 = m.double(), pt.double()
    n = 4 * 5 * 7
    std = lambda z: ((z - z.mean(dim=(1, 2, 3), keepdim=True))**2).sum(dim=(1, 2, 3), keepdim=True).div(n - 1).sqrt()  # noqa: E731
    want = m64 * (phi * std(pt64) / std(m64) + 1 - phi)
    assert got.dtype == torch.float32 and got.shape == m.shape
    assert ((got.double() - want).abs() <= 8 * 2.0**-24 * want.abs() + 1e-30).all()
    # with phi = 1 every sample has the conditional prediction's standard deviation
    if phi == 1.0:
        assert (std(got.double()) / std(pt64) - 1).abs().max().item() < 1e-6
    assert rescale_noise_cfg(m, pt, 0.0) is m and rescale_noise_cfg(m, pt, 0) is m      # phi = 0: the input's bits
