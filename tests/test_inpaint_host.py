"""Host side of image-to-image and masked inpainting in ``generate()``, all on the CPU:
  * ``strength`` -> the first executed step, as a table;
  * ``step_coefficients_ms(i, first=True)`` is the first-order row in closed form, and ``set_begin_index`` makes the stateful
    ``step()`` of a schedule entered late equal the coefficient form;
  * a float64 reference of the whole masked loop on a case with an analytic model: mask 0 returns the known sample exactly,
    mask 1 is the unmasked partial schedule exactly, and the rows ``LatentSampler`` uploads give the same loop;
  * an fp32 emulation of the blended step kernel, with and without FMA contraction, against float64 under the bound of
    tests/test_inpaint_gpu.py, and the three bit-exactness properties of the blend's form;
  * every ``ValueError`` of ``generate()`` and ``LatentSampler.sample`` is raised before a device is looked for;
  * the three entry points are declared, bound and documented.
Bounds of 1e-12 are relative to max|value| (a handful of float64 roundings on either side, the convention of
tests/test_dpm_host.py).

Bound of the blended step, elementwise with u = 2^-24, Bv the bound of the unblended value v (8u times the magnitudes of its
terms: tests/test_sampler_gpu.py, tests/test_dpm_gpu.py), K = |bA z0| + |bS e0|:
    m Bv + (1 - m) 6u K + 4u (|m v| + |(1 - m) kn|)
kn = bA z0 + bS e0 has two coefficient roundings, two products and a sum (under 6u K to first order), it enters scaled by
(1 - m); v's error enters scaled by m; the blend itself adds the rounding of 1 - m, two products and a sum (under 4u of the
two magnitudes)."""
import math
import os

import numpy as np
import pytest
import torch

from diffusion_amd.models.schedulers import DDIMScheduler, DPMSolverMultistepScheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ('epsilon', 'v_prediction', 'sample')
TOL = 1e-12
U = 2.0 ** -24


def _check(got, ref, what):
    err = (got - ref).abs().max().item()
    bound = TOL * ref.abs().max().item()
    assert err <= bound, (what, err, bound)


# ---------------------------------------------------------------------------------------------------------------------
# 1. strength
# ---------------------------------------------------------------------------------------------------------------------
# (num_inference_steps, strength) -> start_index; None: no step would run, a ValueError
STRENGTH_TABLE = {
    (1, 0.01): None, (4, 0.01): None, (20, 0.01): None, (50, 0.01): None,
    (1, 0.5): None, (4, 0.5): 2, (20, 0.5): 10, (50, 0.5): 25,
    (1, 0.8): None, (4, 0.8): 1, (20, 0.8): 4, (50, 0.8): 10,
    (1, 0.999): None, (4, 0.999): 1, (20, 0.999): 1, (50, 0.999): 1,
    (1, 1.0): 0, (4, 1.0): 0, (20, 1.0): 0, (50, 1.0): 0,
}


def test_strength_table():
    from diffusion_amd.models.stable_diffusion import _check_init_image
    img = torch.zeros(1, 3, 64, 128)
    for (n, strength), want in STRENGTH_TABLE.items():
        if want is None:
            with pytest.raises(ValueError, match='strength'):
                _check_init_image(img, strength, None, None, None, n, 2)
            continue
        assert _check_init_image(img, strength, None, None, None, n, 2) == (64, 128, want), (n, strength)
        assert 0 <= want < n
    for bad in (0.0, -0.5, 1.0001, 2.0, float('nan')):
        with pytest.raises(ValueError, match='strength'):
            _check_init_image(img, bad, None, None, None, 20, 2)
    assert _check_init_image(None, 0.8, None, 64, None, 20, 2) == (64, None, 0)   # no image: nothing changes


# ---------------------------------------------------------------------------------------------------------------------
# 2. the schedulers
# ---------------------------------------------------------------------------------------------------------------------
def test_add_noise_coefficients_are_add_noise():
    g = torch.Generator().manual_seed(3)
    x, e = (torch.randn(2, 3, 4, 4, generator=g, dtype=torch.float64) for _ in range(2))
    for sch in (DDIMScheduler(), DPMSolverMultistepScheduler()):
        for t in (0, 1, 501, 999):
            a, s = sch.add_noise_coefficients(t)
            assert isinstance(a, float) and isinstance(s, float)
            ac = float(sch.alphas_cumprod[t])   # the fp32 table's entry, taken to float64
            assert a == math.sqrt(ac) and s == math.sqrt(1.0 - ac)
            _check(a * x + s * e, sch.add_noise(x, e, torch.tensor([t])), ('add_noise', t))
            assert sch.add_noise_coefficients(torch.tensor(t)) == (a, s)


@pytest.mark.parametrize('ptype', TYPES)
@pytest.mark.parametrize('n', (4, 10, 20))
def test_first_order_override(ptype, n):
    sch = DPMSolverMultistepScheduler(prediction_type=ptype)
    sch.set_timesteps(n)
    ac = sch.alphas_cumprod.double()
    before = [sch.step_coefficients_ms(i) for i in range(n)]
    for i in range(n):
        t = int(sch.timesteps[i])
        tn = t - 1000 // n
        a_s, a_t = math.sqrt(float(ac[t])), math.sqrt(float(ac[tn] if tn >= 0 else ac[0]))
        s_s, s_t = math.sqrt(1 - a_s * a_s), math.sqrt(1 - a_t * a_t)
        h = math.log(a_t / s_t) - math.log(a_s / s_s)
        ax, am = {'epsilon': (1 / a_s, -s_s / a_s), 'v_prediction': (a_s, -s_s), 'sample': (0.0, 1.0)}[ptype]
        want = (ax, am, s_t / s_s, -a_t * math.expm1(-h), 0.0)
        got = sch.step_coefficients_ms(i, first=True)
        assert len(got) == 5 and got[4] == 0.0 and math.copysign(1.0, got[4]) == 1.0, (i, got)
        for a, b in zip(got, want):
            assert abs(a - b) <= 1e-12 * max(abs(b), 1.0), (ptype, n, i, got, want)
        # without `first` the row is what it was, and a second-order row differs from the override
        assert sch.step_coefficients_ms(i) == before[i] == sch.step_coefficients_ms(i, first=False)
        assert (before[i][4] != 0.0) == (0 < i < n - 1 or (i == n - 1 and n >= 15))
        if before[i][4] == 0.0:
            assert got == before[i]


@pytest.mark.parametrize('ptype', TYPES)
@pytest.mark.parametrize('n', (10, 20))   # 10: lower_order_final makes the last step first order
def test_stateful_step_from_mid_schedule(ptype, n):
    sch = DPMSolverMultistepScheduler(prediction_type=ptype)
    for start in (1, n // 2, n - 2, n - 1):
        sch.set_timesteps(n)
        sch.set_begin_index(start)
        g = torch.Generator().manual_seed(100 * n + start)
        xa = xb = torch.randn(2, 3, 4, 4, generator=g, dtype=torch.float64)
        hist = None
        for i in range(start, n):
            m = torch.randn(xa.shape, generator=g, dtype=torch.float64)
            ax, am, kx, k0, k1 = sch.step_coefficients_ms(i, first=i == start)
            assert (k1 != 0.0) == (i > start and not (n < 15 and i == n - 1)), (n, start, i, k1)
            x0 = ax * xb + am * m
            xb = kx * xb + k0 * x0 + (k1 * hist if k1 != 0.0 else 0.0)
            hist = x0
            xa = sch.step(m, sch.timesteps[i], xa)['prev_sample']
            _check(xa, xb, (ptype, n, start, i))
    # set_timesteps takes the schedule back to its first step
    sch.set_timesteps(n)
    x, m = torch.ones(3, dtype=torch.float64), torch.full((3,), 0.5, dtype=torch.float64)
    first = sch.step(m, sch.timesteps[0], x)['prev_sample']
    sch.set_begin_index(n - 1)
    sch.set_timesteps(n)
    assert torch.equal(sch.step(m, sch.timesteps[0], x)['prev_sample'], first)
    sch.step(m, sch.timesteps[1], x)
    sch.set_begin_index(0)   # and set_begin_index drops the history
    assert torch.equal(sch.step(m, sch.timesteps[0], x)['prev_sample'], first)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the whole masked loop in float64, on the Gaussian case of tests/test_dpm_host.py
# ---------------------------------------------------------------------------------------------------------------------
SIGMA_D2 = 4.0


def _model(sch, x, t):
    """Data N(0, sigma_d^2): the exact model output at timestep t in the scheduler's parameterisation."""
    a2 = float(sch.alphas_cumprod.double()[int(t)])
    a, s = math.sqrt(a2), math.sqrt(1 - a2)
    den = a2 * SIGMA_D2 + (1 - a2)
    eps, x0 = s * x / den, a * SIGMA_D2 * x / den
    return {'epsilon': eps, 'sample': x0, 'v_prediction': a * eps - s * x0}[sch.prediction_type]


def _reference_loop(sch, n, start, known, noise, mask):
    """The method itself with the scheduler's own add_noise / step: noise the known sample to timestep number `start`, run
    the tail; with a mask, after every step the state outside it is the known sample at the level of the next timestep."""
    sch.set_timesteps(n)
    ts = sch.timesteps
    if hasattr(sch, 'set_begin_index'):
        sch.set_begin_index(start)
    x = sch.add_noise(known, noise, ts[start:start + 1])
    for i in range(start, n):
        x = sch.step(_model(sch, x, ts[i]), ts[i], x)['prev_sample']
        if mask is not None:
            kn = sch.add_noise(known, noise, ts[i + 1:i + 2]) if i + 1 < n else known
            x = mask * x + (1 - mask) * kn
    return x


def _coefficient_loop(sch, n, start, known, noise, mask):
    """The same loop from the rows LatentSampler uploads (float64 here)."""
    sch.set_timesteps(n)
    ts = [int(t) for t in sch.timesteps]
    a0, s0 = sch.add_noise_coefficients(ts[start])
    x = a0 * known + s0 * noise
    hist = None
    for i in range(start, n):
        m = _model(sch, x, ts[i])
        if getattr(sch, 'multistep', False):
            ax, am, kx, k0, k1 = sch.step_coefficients_ms(i, first=i == start)
            d = ax * x + am * m
            v = kx * x + k0 * d + (k1 * hist if k1 != 0.0 else 0.0)
            hist = d
        else:
            cx, cm, cn = sch.step_coefficients(ts[i])
            assert cn == 0.0
            v = cx * x + cm * m
        if mask is not None:
            bA, bS = sch.add_noise_coefficients(ts[i + 1]) if i + 1 < n else (1.0, 0.0)
            v = mask * v + (1 - mask) * (bA * known + bS * noise)
        x = v
    return x


@pytest.mark.parametrize('ptype', TYPES)
@pytest.mark.parametrize('cls', (DDIMScheduler, DPMSolverMultistepScheduler))
@pytest.mark.parametrize('n,start', [(10, 0), (10, 4), (10, 9), (20, 7)])
def test_masked_loop_in_float64(cls, ptype, n, start):
    sch = cls(prediction_type=ptype)
    g = torch.Generator().manual_seed(n + start)
    known = 2.0 * torch.randn(2, 4, 6, 6, generator=g, dtype=torch.float64)
    noise = torch.randn(known.shape, generator=g, dtype=torch.float64)
    mixed = (torch.rand(2, 1, 6, 6, generator=g, dtype=torch.float64) * 1.5 - 0.25).clamp(0, 1)   # exact 0s, 1s, fractions
    assert (mixed == 0).any() and (mixed == 1).any() and ((mixed > 0) & (mixed < 1)).any()
    plain = _reference_loop(sch, n, start, known, noise, None)
    assert torch.equal(_reference_loop(sch, n, start, known, noise, torch.zeros_like(mixed)), known)
    assert torch.equal(_reference_loop(sch, n, start, known, noise, torch.ones_like(mixed)), plain)
    got = _reference_loop(sch, n, start, known, noise, mixed)
    keep, paint = (mixed == 0).expand_as(known), (mixed == 1).expand_as(known)
    assert torch.equal(got[keep], known[keep])
    assert not torch.equal(got[paint], known[paint])
    # the rows the sampler uploads are this loop
    for mask in (None, mixed):
        _check(_coefficient_loop(sch, n, start, known, noise, mask), _reference_loop(sch, n, start, known, noise, mask),
               (cls.__name__, ptype, n, start, mask is not None))
    if start == 0 and cls is DDIMScheduler:   # strength 1 still starts from the noised image, not from the noise
        assert not torch.equal(plain, _reference_loop(sch, n, 0, torch.zeros_like(known), noise, None))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the blended step kernel's arithmetic in fp32, contracted or not
# ---------------------------------------------------------------------------------------------------------------------
F32 = np.float32


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in float64 (one more rounding in the float64 sum, then to fp32)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _mac(a, b, c, fma):
    return _fma(a, b, c) if fma else (a * b + c).astype(F32)


def _blend_fp32(v, mk, kn, fma):
    """x_out = m v + (1 - m) kn as the compiler may emit it: no contraction, or either product folded into an FMA"""
    one_m = (F32(1) - mk).astype(F32)
    if fma == 0:
        return (mk * v + one_m * kn).astype(F32)
    if fma == 1:
        return _fma(mk, v, (one_m * kn).astype(F32))
    return _fma(one_m, kn, (mk * v).astype(F32))


def _rows():
    """(tag, first-order row (cx, cm), two-step row (ax, am, kx, k0, k1), (bA, bS)) of real schedules, float64"""
    out = []
    for ptype in TYPES:
        for n in (4, 20, 50):
            d, m = DDIMScheduler(prediction_type=ptype), DPMSolverMultistepScheduler(prediction_type=ptype)
            d.set_timesteps(n)
            m.set_timesteps(n)
            for i in sorted({0, 1, n // 2, n - 1}):
                t = int(d.timesteps[i])
                ren = d.add_noise_coefficients(int(d.timesteps[i + 1])) if i + 1 < n else (1.0, 0.0)
                out.append(((ptype, n, i), d.step_coefficients(t)[:2], m.step_coefficients_ms(i), ren))
    return out


def test_blended_step_in_fp32_against_float64():
    rng = np.random.default_rng(7)
    worst = {}
    count = 0
    for tag, (cx, cm), (ax, am, kx, k0, k1), (bA, bS) in _rows():
        for cfg, g in ((0, 0.0), (1, 1.5), (1, 7.5)):
            count += 1
            N = 4096
            x, pu, pt, hist, z0, e0 = (rng.standard_normal(N).astype(F32) for _ in range(6))
            z0 = (z0 * F32(3)).astype(F32)
            mk = np.clip(rng.random(N) * 1.5 - 0.25, 0, 1).astype(F32)
            X, PU, PT, H, Z0, E0, MK = (a.astype(np.float64) for a in (x, pu, pt, hist, z0, e0, mk))
            M = PU + g * (PT - PU) if cfg else PU
            Mmag = np.abs(PU) + g * (np.abs(PT) + np.abs(PU)) if cfg else np.abs(PU)
            KN = bA * Z0 + bS * E0
            K = np.abs(bA * Z0) + np.abs(bS * E0)
            # float64 references and the bounds Bv of the unblended values
            V1 = cx * X + cm * M
            B1 = 8 * U * (np.abs(cx * X) + abs(cm) * Mmag)
            D = ax * X + am * M
            V2 = kx * X + k0 * D + k1 * H
            B2 = 8 * U * (np.abs(kx * X) + abs(k0) * (np.abs(ax * X) + abs(am) * Mmag) + np.abs(k1 * H))
            f = lambda c: F32(c)   # noqa: E731  (a coefficient as the device table holds it)
            for fma in (0, 1, 2):
                c = bool(fma)
                m = _mac(np.full(N, f(g)), (pt - pu).astype(F32), pu, c) if cfg else pu
                v1 = _mac(np.full(N, f(cx)), x, (f(cm) * m).astype(F32), c)
                d = _mac(np.full(N, f(ax)), x, (f(am) * m).astype(F32), c)
                v2 = _mac(np.full(N, f(kx)), x, (f(k0) * d).astype(F32), c)
                if k1 != 0.0:
                    v2 = _mac(np.full(N, f(k1)), hist, v2, c)
                kn = _mac(np.full(N, f(bA)), z0, (f(bS) * e0).astype(F32), c)
                for name, v, V, Bv in (('first-order', v1, V1, B1), ('two-step', v2, V2, B2)):
                    out = _blend_fp32(v, mk, kn, fma)
                    REF = MK * V + (1 - MK) * KN
                    bound = MK * Bv + (1 - MK) * 6 * U * K + 4 * U * (np.abs(MK * V) + np.abs((1 - MK) * KN))
                    ratio = float(np.max(np.abs(out.astype(np.float64) - REF) / bound))
                    worst[(name, fma)] = max(worst.get((name, fma), 0.0), ratio)
                    assert ratio <= 1.0, (tag, cfg, g, name, fma, ratio)
                    # the form's exact properties, whichever way it is contracted
                    assert np.array_equal(out[mk == 1].view(np.int32), v[mk == 1].view(np.int32)), (tag, name, fma)
                    assert np.array_equal(out[mk == 0].view(np.int32), kn[mk == 0].view(np.int32)), (tag, name, fma)
                if (bA, bS) == (1.0, 0.0):
                    assert np.array_equal(kn.view(np.int32), z0.view(np.int32)), (tag, fma)
    assert count >= 100 and any(r[3] == (1.0, 0.0) for r in _rows())
    print('blended step, fp32 emulation: peak |got - ref| / bound per (form, contraction): '
          + ', '.join(f'{k[0]} {("none", "m v", "(1-m) kn")[k[1]]} {v:.3f}' for k, v in sorted(worst.items())))
    print(f'peak over all: {max(worst.values()):.3f}')


# ---------------------------------------------------------------------------------------------------------------------
# 5. every check comes before the device
# ---------------------------------------------------------------------------------------------------------------------
def test_generate_checks_raise_before_anything_touches_the_device(monkeypatch):
    """``generate`` is called with ``self`` None, so anything past the checks would fail with another exception (the
    convention of tests/test_dpm_host.py)."""
    from diffusion_amd.models.stable_diffusion import StableDiffusion
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: pytest.fail('looked for a device'))
    monkeypatch.delenv('DA_SAMPLER', raising=False)
    img, img1 = torch.rand(2, 3, 64, 128), torch.rand(1, 3, 64, 128)
    ok_mask = torch.zeros(64, 128)
    bad = [
        (dict(mask=ok_mask), 'init_image'),                                          # a mask needs an image
        (dict(init_image=img, strength=0.0), 'strength'),
        (dict(init_image=img, strength=1.5), 'strength'),
        (dict(init_image=img, strength=-0.1), 'strength'),
        (dict(init_image=img, strength=0.2, num_inference_steps=4), 'strength'),     # no step would run
        (dict(init_image=img, height=128), 'init_image'),                            # a size that is not the image's
        (dict(init_image=img, width=64), 'init_image'),
        (dict(init_image=torch.rand(3, 3, 64, 128)), 'init_image'),                  # neither 1 nor the batch
        (dict(init_image=torch.rand(2, 4, 64, 128)), 'init_image'),
        (dict(init_image=torch.rand(3, 64, 128)), 'init_image'),
        (dict(init_image=(img * 255).to(torch.uint8)), 'init_image'),
        (dict(init_image=img, mask=torch.zeros(64, 64)), 'mask'),
        (dict(init_image=img, mask=torch.zeros(3, 1, 64, 128)), 'mask'),
        (dict(init_image=img, mask=torch.zeros(2, 64, 128)), 'mask'),
        (dict(init_image=img, mask=torch.full((64, 128), 1.5)), 'mask'),
        (dict(init_image=img, mask=torch.full((64, 128), -0.5)), 'mask'),
        (dict(init_image=img, mask=torch.full((64, 128), float('nan'))), 'mask'),
        (dict(init_image=img, mask=torch.ones(64, 128, dtype=torch.bool)), 'mask'),
    ]
    for kw, what in bad:
        for sampler in ('hip', 'graph', 'torch'):
            with pytest.raises(ValueError, match=what):
                StableDiffusion.generate(None, prompt=['a cool doge', 'a hot cat'], sampler=sampler, **kw)
    # good arguments pass every check and only then fail on the missing model
    for kw in (dict(init_image=img), dict(init_image=img1, mask=ok_mask), dict(init_image=img, mask=ok_mask[None, None]),
               dict(init_image=img, mask=torch.ones(2, 1, 64, 128), height=64, width=128, strength=1.0)):
        with pytest.raises(AttributeError):
            StableDiffusion.generate(None, prompt=['a cool doge', 'a hot cat'], **kw)
    with pytest.raises(AttributeError):   # batch = prompts x images per prompt
        StableDiffusion.generate(None, prompt=['a cool doge'], num_images_per_prompt=2, init_image=img)


class _NoDevice:
    """A U-Net that has a shape and nothing else: reading its device fails the test."""

    class cfg:
        in_channels = 4

    def check_spatial(self, H, W):
        pass

    @property
    def device_(self):
        pytest.fail('looked for a device')


def test_sampler_checks_raise_before_anything_is_launched():
    from diffusion_amd.sampling import LatentSampler
    from diffusion_amd.schedulers.schedulers import ContinuousTimeScheduler
    smp = LatentSampler(_NoDevice(), DDIMScheduler())
    lat, cond = torch.zeros(2, 4, 8, 8), torch.zeros(2, 77, 16)
    kw = dict(num_inference_steps=6, guidance_scale=0.0)
    mask = torch.zeros(2, 64, 64)
    bad = [
        dict(mask_px=mask),                                               # a mask without the known sample
        dict(start_index=2),
        dict(known=lat, start_index=6), dict(known=lat, start_index=-1), dict(known=lat, start_index=60),
        dict(known=torch.zeros(2, 4, 8, 16)), dict(known=torch.zeros(1, 4, 8, 8)), dict(known=torch.zeros(4, 8, 8)),
        dict(known=lat, noise=torch.zeros(2, 4, 16, 8)),
        dict(known=lat, mask_px=torch.zeros(1, 64, 64)), dict(known=lat, mask_px=torch.zeros(2, 1, 64, 64)),
        dict(known=lat, mask_px=torch.zeros(2, 64, 32)), dict(known=lat, mask_px=torch.zeros(2, 24, 24)),
        dict(known=lat, mask_px=torch.zeros(2, 60, 60)), dict(known=lat, mask_px=torch.zeros(2, 256, 256)),
    ]
    for b in bad:
        with pytest.raises(ValueError):
            smp.sample(lat, cond, **kw, **b)
    with pytest.raises(ValueError):
        smp.sample(None, cond, known=lat, **kw)                            # nothing to noise it with
    with pytest.raises(ValueError, match='discrete-time'):
        LatentSampler(_NoDevice(), ContinuousTimeScheduler(t_max=1.56)).sample(lat, cond, known=lat, **kw)
    for multistep_ok in (dict(known=lat, start_index=5), dict(known=lat, mask_px=mask), dict(known=lat, noise=lat)):
        with pytest.raises(BaseException, match='looked for a device'):    # good arguments reach the device
            LatentSampler(_NoDevice(), DPMSolverMultistepScheduler()).sample(lat, cond, **kw, **multistep_ok)


# ---------------------------------------------------------------------------------------------------------------------
# 6. plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_documented():
    from diffusion_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'diffusion_amd.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name, arity in (('da_sampler_init', 16), ('da_sampler_step_blend', 15), ('da_sampler_step_ms_blend', 15)):
        assert f'int {name}(const float* ' in header, name
        assert len(_lib.SIGNATURES[name]) == arity, name
        assert f'`{name}`' in doc, name
        assert callable(getattr(ops, name[3:]))
    import inspect
    from diffusion_amd.models.stable_diffusion import StableDiffusion
    from diffusion_amd.sampling import LatentSampler
    names = list(inspect.signature(StableDiffusion.generate).parameters)
    assert names[-3:] == ['init_image', 'strength', 'mask'] and names[-5:-3] == ['sampler', 'inference_scheduler']
    p = inspect.signature(StableDiffusion.generate).parameters
    assert p['init_image'].default is None and p['strength'].default == 0.8 and p['mask'].default is None
    p = inspect.signature(LatentSampler.sample).parameters
    assert [p[k].default for k in ('known', 'noise', 'start_index', 'mask_px')] == [None, None, 0, None]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('known', 'noise', 'start_index', 'mask_px'))
