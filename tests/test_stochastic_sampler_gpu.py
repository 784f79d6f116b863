"""GPU tests of the stochastic samplers: ``da_randn_philox`` against the NumPy reference (words bit-exact, normals within 2e-5
of float64), the fused draw of ``da_sampler_step_rng`` against the unfused form bit for bit in every step form, batch
invariance at the kernel, a fresh draw per step (the second moment of ten DDIM eta = 1 steps against its float64
recursion), ``LatentSampler`` (eager, graph, masked, rescaled, zero terminal SNR) and ``generate()`` of both model families.

Tolerances.  Normals: 2e-5 absolute against float64, ten times the 1.6e-6 the same formula gives in NumPy fp32.  Second
moment: 5 sqrt(2 / N) relative over N = 2 x 4 x 64 x 64 values (3.9 %); correlations: 5 / sqrt(N).  ``LatentSampler`` against
the torch route: relative L2 3e-2, the bound of the deterministic comparison in test_sampler_gpu.py."""
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_reference as P  # noqa: E402
from parity_margins import record  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS = [0, 1, 2**64 - 1, 0x299f31d0a4093822]
NORMAL_TOL = 2e-5
SAMPLER_TOL = 3e-2


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-20)).item()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _corr(a, b):
    a, b = a.double().flatten() - a.double().mean(), b.double().flatten() - b.double().mean()
    return float((a * b).sum() / ((a * a).sum() * (b * b).sum()).sqrt())


# ---------------------------------------------------------------------------------------------------------------------
# 5. da_randn_philox against the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(3, 4, 5, 7), (2, 3, 8, 16), (1, 8, 5, 7), (2, 4, 64, 64)])
def test_randn_philox_matches_the_reference(dev, shape):
    from diffusion_amd import ops
    B, C, H, W = shape
    worst = 0.0
    for rot in range(len(SEEDS) if B < 3 else 2):     # every seed value appears in some slot
        sl = [(SEEDS + SEEDS)[rot + b] for b in range(B)]
        sd = ops.philox_seeds(sl, B, dev)
        for draw, stream in itertools.product((0, 1, 2**32 - 1), (0, 1)):
            got = ops.randn_philox(sd, draw, stream, shape).cpu().double().numpy()
            ref = P.randn(sl, draw, stream, C, H, W)
            err = float(np.abs(got - ref).max())
            worst = max(worst, err)
            assert err <= NORMAL_TOL, (shape, sl, draw, stream, err)
            if C % 4 == 0:
                w = ops.randn_philox(sd, draw, stream, shape, kind=1).cpu().view(torch.int32).numpy().view(np.uint32)
                want = np.stack([P.words(s, draw, stream, C, H, W) for s in sl])
                assert np.array_equal(w, want), (shape, sl, draw, stream)
    record(f'randn_philox {shape}', tolerances=dict(max_abs=NORMAL_TOL), max_abs=worst)
    print(f'randn_philox {shape}: worst |device - float64| = {worst:.3e} (tolerance {NORMAL_TOL})')


def test_randn_philox_rejects_bad_arguments(dev):
    """Every refusal is DA_ERR_SHAPE / ValueError before any launch."""
    from diffusion_amd import _lib, ops
    sd = ops.philox_seeds([1, 2, 3], 3, dev)
    out = torch.zeros(2, 4, 5, 7, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    f = _lib.load().da_randn_philox
    assert f(sd.data_ptr(), 0, 0, out.data_ptr(), 2, 4, 5, 7, 0, s) == 0
    for bad in ((None, 0, 0, out.data_ptr(), 2, 4, 5, 7, 0), (sd.data_ptr(), 0, 0, None, 2, 4, 5, 7, 0),
                (sd.data_ptr() + 4, 0, 0, out.data_ptr(), 2, 4, 5, 7, 0), (sd.data_ptr(), 0, 0, out.data_ptr() + 4, 2, 4, 5, 7, 0),
                (sd.data_ptr(), 0, 2, out.data_ptr(), 2, 4, 5, 7, 0), (sd.data_ptr(), 0, 0, out.data_ptr(), 2, 4, 5, 7, 2),
                (sd.data_ptr(), 0, 0, out.data_ptr(), 2, 3, 5, 7, 1), (sd.data_ptr(), 0, 0, out.data_ptr(), 0, 4, 5, 7, 0),
                (sd.data_ptr(), 0, 0, out.data_ptr(), 2, 9, 5, 7, 0), (sd.data_ptr(), 0, 0, out.data_ptr(), 2, 4, 0, 7, 0),
                (sd.data_ptr(), 0, 0, out.data_ptr(), 1, 4, 65536, 65536, 0)):
        assert f(*bad, s) == 1, bad
    for kw in (dict(draw=-1), dict(draw=2**32), dict(stream=2), dict(kind=2)):
        with pytest.raises(ValueError):
            ops.randn_philox(sd[:2].contiguous(), kw.get('draw', 0), kw.get('stream', 0), (2, 4, 5, 7), kind=kw.get('kind', 0))
    with pytest.raises(ValueError):
        ops.randn_philox(sd, 0, 0, (2, 4, 5, 7))                  # three seeds for two images
    with pytest.raises(ValueError):
        ops.randn_philox(sd[:2].contiguous(), 0, 0, (2, 3, 5, 7), kind=1)
    with pytest.raises(ValueError):
        ops.randn_philox(sd[:2].contiguous().view(torch.int64), 0, 0, (2, 4, 5, 7))


# ---------------------------------------------------------------------------------------------------------------------
# 6. fused equals unfused, bit for bit, in every form
# ---------------------------------------------------------------------------------------------------------------------
def _nhwc8(z):
    B, C, H, W = z.shape
    out = torch.zeros(B * H * W, 8, device=z.device)
    out[:, :C] = z.permute(0, 2, 3, 1).reshape(-1, C)
    return out


def _row(floats, slot, draw, dev):
    from diffusion_amd.sampling import stochastic_rows
    return stochastic_rows([floats], slot, [draw])[0].to(dev)


def _form_case(dev, shape, form, cfg, copies, gen, zero_coef=False):
    """One comparison: returns nothing, asserts bit equality of x_out, xt and hist between the fused entry and the unfused form."""
    from diffusion_amd import ops
    B, C, H, W = shape
    ms, blend, rs = bool(form & 1), bool(form & 2), bool(form & 4)
    npix, HW = B * H * W, H * W
    case = (shape, form, cfg, copies, zero_coef)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)   # noqa: E731
    pred, x = rnd((2 if cfg else 1) * npix, 8), rnd(npix, 8)
    pred[:, C:] = 1e30
    x[:, C:] = 1e30
    hist0 = rnd(npix, 8)
    known8, eps8 = rnd(npix, 8), rnd(npix, 8)
    mask = torch.rand(npix, generator=gen).to(dev)
    if ms:    # the two-step reference adds kn z after the blend, which equals the kernel's order where the mask is 0 or 1
        mask = (mask > 0.5).float()
    else:
        mask[::5], mask[1::5] = 0.0, 1.0
    factor = (0.5 + torch.rand(B, generator=gen)).to(dev)
    seeds = ops.philox_seeds([int(v) for v in torch.randint(0, 2**62, (B,), generator=gen)] if B != 3
                             else [2**64 - 1, 0, 0x299f31d0a4093822], B, dev)
    draw = int(torch.randint(0, 2**32, (1,), generator=gen))
    g = 3.5
    z = ops.randn_philox(seeds, draw, 0, shape)
    common = dict(C=C, cfg=bool(cfg), copies=copies)
    rkw = dict(factor=factor, HW=HW) if rs else {}
    bl = (known8, eps8, mask) if blend else ()
    mk = lambda: (torch.full((npix, 8), 7.0, device=dev),   # noqa: E731
                  torch.full((copies * npix, 8), 7.0, device=dev, dtype=torch.bfloat16))
    x_f, xt_f = mk()
    x_r, xt_r = mk()
    if not ms:
        cx, cm, cn, bA, bS = 0.9, -0.4, (0.0 if zero_coef else 0.37), 0.8, 0.6
        row = _row([cx, cm, cn, g, bA, bS, 0.0, 0.0], 6, draw, dev)
        ops.sampler_step_rng(pred, x, row, seeds, x_f, xt_f, HW=HW, **common, factor=factor if rs else None,
                             **(dict(known8=known8, eps8=eps8, mask=mask) if blend else {}))
        coef = torch.tensor([cx, cm, cn, g] + ([bA, bS, 0.0, 0.0] if blend else []), dtype=torch.float64).float().to(dev)
        noise = None if zero_coef else z
        if blend:
            ops.sampler_step_blend(pred, x, coef, *bl, x_r, xt_r, noise, **common, **rkw)
        else:
            ops.sampler_step(pred, x, coef, x_r, xt_r, noise, **common, **rkw)
        assert _same(x_f, x_r), case
        assert _same(xt_f, xt_r), case
    else:
        k1 = 0.0 if (form + cfg + copies) % 2 else -0.21     # first- and second-order steps
        ax, am, kx, k0, bA, bS, kn = 1.1, -0.5, 0.7, 0.35, 0.8, 0.6, (0.0 if zero_coef else 0.43)
        row = _row([ax, am, kx, k0, k1, g, bA, bS, kn, 0.0, 0.0, 0.0], 9, draw, dev)
        h_f, h_r = hist0.clone(), hist0.clone()
        ops.sampler_step_rng(pred, x, row, seeds, x_f, xt_f, HW=HW, **common, hist=h_f, factor=factor if rs else None,
                             **(dict(known8=known8, eps8=eps8, mask=mask) if blend else {}))
        coef = torch.tensor([ax, am, kx, k0, k1, g, bA, bS], dtype=torch.float64).float().to(dev)
        if blend:
            ops.sampler_step_ms_blend(pred, x, h_r, coef, *bl, x_r, xt_r, **common, **rkw)
        else:
            ops.sampler_step_ms(pred, x, h_r, coef, x_r, xt_r, **common, **rkw)
        if not zero_coef:      # x += kn z in torch: the product rounded, then the sum
            add = row[8] * _nhwc8(z)
            upd = x_r + add
            x_r = torch.where(mask[:, None] == 1.0, upd, x_r) if blend else upd
            want = torch.empty(npix, 8, device=dev, dtype=torch.bfloat16)
            ops.cast_f32_bf16(x_r, want)
            xt_r = torch.cat([want] * copies)
        assert _same(h_f, h_r), case
        assert _same(x_f, x_r), case
        assert _same(xt_f, xt_r), case
        if k1 == 0.0:
            assert not _same(h_f, hist0)
    assert (x_f[:, C:] == 0).all() and (xt_f[:, C:] == 0).all(), case
    if not zero_coef:
        assert not torch.equal(x_f[:, :C], x[:, :C])


@pytest.mark.parametrize('shape', [(2, 4, 8, 16), (3, 4, 5, 7), (2, 3, 5, 7)])
def test_fused_draw_equals_the_unfused_form_bit_for_bit(dev, shape):
    gen = torch.Generator().manual_seed(sum(shape))
    n = 0
    for form, cfg, copies in itertools.product(range(8), (0, 1), (1, 2)):
        _form_case(dev, shape, form, cfg, copies, gen)
        n += 1
    for form in range(8):    # a zero noise coefficient: the deterministic entry's bits, nothing drawn
        _form_case(dev, shape, form, 1, 2, gen, zero_coef=True)
    assert n == 32


def test_fused_draw_with_eight_channels(dev):
    """C = 8 makes the second Philox call (block 1)."""
    gen = torch.Generator().manual_seed(8)
    for form in (0, 1, 6):
        _form_case(dev, (2, 8, 5, 7), form, 1, 2, gen)


def test_sampler_step_rng_rejects_bad_arguments(dev):
    from diffusion_amd import _lib, ops
    npix, C, HW = 98, 4, 49
    pred, x = torch.zeros(2 * npix, 8, device=dev), torch.zeros(npix, 8, device=dev)
    hist, k8, e8 = torch.zeros(npix, 8, device=dev), torch.zeros(npix, 8, device=dev), torch.zeros(npix, 8, device=dev)
    mask, factor = torch.ones(npix + 4, device=dev)[:npix], torch.ones(2, device=dev)
    coef = torch.zeros(12, device=dev)
    xt = torch.zeros(2 * npix, 8, device=dev, dtype=torch.bfloat16)
    seeds = ops.philox_seeds([5, 6, 7], 3, dev)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t, off=0: t.data_ptr() + off   # noqa: E731

    def rc(form=7, seeds_=p(seeds), hist_=p(hist), k8_=p(k8), mask_=p(mask), factor_=p(factor), HW_=HW, C_=C, npix_=npix,
           coef_=p(coef)):
        return _lib.load().da_sampler_step_rng(p(pred), p(x), hist_, coef_, k8_, p(e8), mask_, factor_, seeds_, p(x), p(xt),
                                               npix_, HW_, C_, form, 1, 2, s)

    for form in range(8):
        assert rc(form) == 0
    assert rc(0, hist_=None, k8_=None, mask_=None, factor_=None) == 0        # operands of forms not selected may be NULL
    for bad in (dict(form=8), dict(form=-1), dict(seeds_=None), dict(seeds_=p(seeds, 4)), dict(form=1, hist_=None),
                dict(form=2, k8_=None), dict(form=2, mask_=None), dict(form=2, mask_=p(mask, 4)), dict(form=4, factor_=None),
                dict(form=4, factor_=p(factor) + 2), dict(HW_=48), dict(HW_=0), dict(C_=0), dict(C_=9), dict(npix_=0),
                dict(coef_=p(coef, 4)), dict(coef_=None)):
        assert rc(**bad) == 1, bad
    torch.cuda.synchronize()
    ok = dict(HW=HW, C=C, cfg=True, copies=2)
    s2 = seeds[:2].contiguous()
    ops.sampler_step_rng(pred, x, coef[:8], s2, x, xt, **ok)
    ops.sampler_step_rng(pred, x, coef, s2, x, xt, hist=hist, **ok)
    for bad in (lambda: ops.sampler_step_rng(pred, x, coef[:8], seeds, x, xt, **ok),                    # three seeds, two images
                lambda: ops.sampler_step_rng(pred, x, coef[:8], s2.view(torch.int64), x, xt, **ok),
                lambda: ops.sampler_step_rng(pred, x, coef[:8], None, x, xt, **ok),
                lambda: ops.sampler_step_rng(pred, x, coef[:4], s2, x, xt, **ok),                       # the narrow row
                lambda: ops.sampler_step_rng(pred, x, coef[:8], s2, x, xt, hist=hist, **ok),            # two-step needs 12
                lambda: ops.sampler_step_rng(pred, x, coef[:8], s2, x, xt, known8=k8, **ok),
                lambda: ops.sampler_step_rng(pred, x, coef[:8], s2, x, xt, **dict(ok, HW=48)),
                lambda: ops.sampler_step_rng(pred, x, coef[:8], s2.cpu(), x, xt, **ok)):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------------------------------
# 7. batch invariance at the kernel
# ---------------------------------------------------------------------------------------------------------------------
def test_an_images_noise_does_not_depend_on_its_batch(dev):
    from diffusion_amd import ops
    C, H, W = 4, 5, 7
    HW = H * W
    gen = torch.Generator().manual_seed(77)
    for ms in (False, True):
        pred3, x3, h3 = (torch.randn(3 * HW, 8, generator=gen).to(dev) for _ in range(3))
        for t in (pred3, x3):
            t[:, C:] = 0
        row = _row([0.9, -0.4, 0.37, 1.0, 0, 0, 0, 0], 6, 41, dev) if not ms else \
            _row([1.1, -0.5, 0.7, 0.35, -0.2, 1.0, 0, 0, 0.43, 0, 0, 0], 9, 41, dev)
        s3 = ops.philox_seeds([11, 2**63 + 5, 1138], 3, dev)
        out3, xt3 = torch.empty(3 * HW, 8, device=dev), torch.empty(3 * HW, 8, device=dev, dtype=torch.bfloat16)
        hk3 = h3.clone()
        ops.sampler_step_rng(pred3, x3, row, s3, out3, xt3, HW=HW, C=C, cfg=False, hist=hk3 if ms else None)
        # the third image alone, with its own seed
        sl = slice(2 * HW, 3 * HW)
        s1 = ops.philox_seeds([1138], 1, dev)
        out1, xt1 = torch.empty(HW, 8, device=dev), torch.empty(HW, 8, device=dev, dtype=torch.bfloat16)
        hk1 = h3[sl].clone()
        ops.sampler_step_rng(pred3[sl].contiguous(), x3[sl].contiguous(), row, s1, out1, xt1, HW=HW, C=C, cfg=False,
                             hist=hk1 if ms else None)
        assert _same(out1, out3[sl]) and _same(xt1, xt3[sl]), ms
        if ms:
            assert _same(hk1, hk3[sl])
        # the same image under another seed differs
        out1b = torch.empty(HW, 8, device=dev)
        ops.sampler_step_rng(pred3[sl].contiguous(), x3[sl].contiguous(), row, ops.philox_seeds([1139], 1, dev), out1b, None,
                             HW=HW, C=C, cfg=False, hist=h3[sl].clone() if ms else None)
        assert not _same(out1b, out1)
    # swapping two images' seeds swaps their noise: x = 0, m = 0, cn = 1 stores z itself
    zero = torch.zeros(2 * HW, 8, device=dev)
    row = _row([0.0, 0.0, 1.0, 1.0, 0, 0, 0, 0], 6, 3, dev)
    a, b = torch.empty(2 * HW, 8, device=dev), torch.empty(2 * HW, 8, device=dev)
    ops.sampler_step_rng(zero, zero, row, ops.philox_seeds([5, 9], 2, dev), a, None, HW=HW, C=C, cfg=False)
    ops.sampler_step_rng(zero, zero, row, ops.philox_seeds([9, 5], 2, dev), b, None, HW=HW, C=C, cfg=False)
    assert _same(a[:HW], b[HW:]) and _same(a[HW:], b[:HW]) and not _same(a[:HW], a[HW:])
    assert _same(a, _nhwc8(ops.randn_philox(ops.philox_seeds([5, 9], 2, dev), 3, 0, (2, C, H, W))))


# ---------------------------------------------------------------------------------------------------------------------
# 8. a fresh draw per step
# ---------------------------------------------------------------------------------------------------------------------
def test_every_step_draws_fresh_noise(dev):
    """Ten DDIM steps with eta = 1 under the 'model' pred = sqrt(1 - abar_t) x (epsilon prediction): every step is
    x <- (cx + cm s_t) x + cn z, so with independent unit draws the second moment follows var <- (cx + cm s_t)^2 var + cn^2
    from 1.  A draw number that is stuck or ignored adds the same z ten times and lands several hundred per cent away."""
    from diffusion_amd import ops
    from diffusion_amd.models.schedulers import DDIMScheduler
    B, C, H, W = 2, 4, 64, 64
    N, HW = B * C * H * W, H * W
    bound = 5 * math.sqrt(2 / N)
    sch = DDIMScheduler(eta=1.0, prediction_type='epsilon')
    sch.set_timesteps(10)
    ts = sch.timesteps.tolist()
    coefs = [sch.step_coefficients(t) for t in ts]
    s_t = [math.sqrt(1 - float(sch.alphas_cumprod[t])) for t in ts]
    var = 1.0
    for (cx, cm, cn), s in zip(coefs, s_t):
        var = (cx + cm * s) ** 2 * var + cn ** 2
    seeds = ops.philox_seeds([1138, 1139], B, dev)

    def run(stuck):
        x = _nhwc8(ops.randn_philox(seeds, 0, 1, (B, C, H, W)))      # the initial state: stream 1
        for i, ((cx, cm, cn), s) in enumerate(zip(coefs, s_t)):
            pred = torch.tensor(s, dtype=torch.float64).float().to(dev) * x
            row = _row([cx, cm, cn, 1.0, 0, 0, 0, 0], 6, 0 if stuck else i, dev)
            ops.sampler_step_rng(pred, x, row, seeds, x, None, HW=HW, C=C, cfg=False)
        return float((x[:, :C].double() ** 2).mean())

    got, stuck = run(False), run(True)
    rel, rel_stuck = abs(got / var - 1), abs(stuck / var - 1)
    record('ddim eta=1 second moment', tolerances=dict(rel=bound), rel=rel, rel_with_stuck_draw=rel_stuck, expected=var, got=got)
    print(f'second moment after 10 steps: {got:.5f}, recursion {var:.5f}, off by {rel:.3%} (bound {bound:.3%}); '
          f'with the draw number stuck at 0: off by {rel_stuck:.1%}')
    assert rel <= bound, (got, var)
    assert rel_stuck > 10 * bound, 'the check cannot tell a stuck draw number'
    n = C * H * W
    zs = [ops.randn_philox(seeds, d, 0, (B, C, H, W)) for d in range(4)]
    for d in range(3):
        for b in range(B):
            assert abs(_corr(zs[d][b], zs[d + 1][b])) < 5 / math.sqrt(n), (d, b)
    assert abs(_corr(zs[0][0], zs[0][1])) < 5 / math.sqrt(n)
    assert abs(_corr(zs[0], ops.randn_philox(seeds, 0, 1, (B, C, H, W)))) < 5 / math.sqrt(N)


# ---------------------------------------------------------------------------------------------------------------------
# 9. LatentSampler
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tiny(dev):
    from oracle import unet_oracle as O
    from diffusion_amd.models.models import stable_diffusion_2
    ocfg = O.UNetConfig.tiny()
    model = stable_diffusion_2(model_name='tiny', pretrained=False, precomputed_latents=True, fsdp=False)
    model.unet.load_state_dict(O.init_state_dict(ocfg, seed=17))
    return ocfg, model


def _inputs(ocfg, dev, seed=23, B=2, H=8, W=16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 4, H, W, generator=g).to(dev), torch.randn(B, 77, ocfg.cross_attention_dim, generator=g).to(dev),
            torch.randn(B, 77, ocfg.cross_attention_dim, generator=g).to(dev))


def _scheduler(name, **kw):
    from diffusion_amd.models.schedulers import make_inference_scheduler
    if name == 'eta1':
        return make_inference_scheduler('ddim', eta=1.0, **kw)
    return make_inference_scheduler('dpm++2m-sde', **kw)


def _torch_route(model, sch, lat0, txt, unc, steps, guidance, seeds, phi=0.0):
    """The same schedule in torch ops around unet(...), its noise from da_randn_philox as variance_noise."""
    from diffusion_amd import ops
    from diffusion_amd.sampling import rescale_noise_cfg
    sch.set_timesteps(steps)
    sd = ops.philox_seeds(seeds, lat0.shape[0], lat0.device)
    lat, emb = lat0, torch.cat([unc, txt])
    with torch.no_grad():
        for i, t in enumerate(sch.timesteps):
            pu, pt = model.unet(torch.cat([lat] * 2), t, encoder_hidden_states=emb).sample.chunk(2)
            pred = rescale_noise_cfg(pu + guidance * (pt - pu), pt, phi)
            lat = sch.step(pred, t, lat, variance_noise=ops.randn_philox(sd, i, 0, tuple(lat.shape)))['prev_sample']
    return lat


@pytest.mark.parametrize('name', ['eta1', 'dpm++2m-sde'])
def test_latent_sampler_stochastic_routes(tiny, dev, name):
    from diffusion_amd import ops
    from diffusion_amd.sampling import LatentSampler
    ocfg, model = tiny
    lat0, txt, unc = _inputs(ocfg, dev)
    sch = _scheduler(name)
    smp = LatentSampler(model.unet, sch)
    smp.graphs.clear()
    kw = dict(num_inference_steps=4, guidance_scale=3.0)
    seeds = [1138, 2**63 + 7]
    got = smp.sample(lat0, txt, unc, seeds=seeds, **kw)
    assert got.shape == lat0.shape and torch.isfinite(got).all()
    assert torch.equal(got, smp.sample(lat0, txt, unc, seeds=seeds, **kw))                    # run to run
    assert torch.equal(got, smp.sample(lat0, txt, unc, seeds=ops.philox_seeds(seeds, 2, dev), **kw))   # a tensor of seeds
    graphed = smp.sample(lat0, txt, unc, seeds=seeds, graph=True, **kw)
    assert len(smp.graphs) == 1 and torch.equal(graphed, got), _rel(graphed, got)
    other = smp.sample(lat0, txt, unc, seeds=[1138, 2**63 + 8], graph=True, **kw)             # the capture is reused
    assert len(smp.graphs) == 1 and not torch.equal(other[1], got[1])
    assert torch.equal(other, smp.sample(lat0, txt, unc, seeds=[1138, 2**63 + 8], **kw))
    ref = _torch_route(model, _scheduler(name), lat0, txt, unc, 4, 3.0, seeds)
    e = _rel(got, ref)
    record(f'LatentSampler {name} hip vs torch', tolerances=dict(rel_l2=SAMPLER_TOL), rel_l2=e)
    print(f'{name}: hip vs torch route on the same Philox noise, rel-L2 {e:.3e} (bound {SAMPLER_TOL})')
    assert e < SAMPLER_TOL, e
    # the noise matters: the deterministic twin of the schedule gives something else
    from diffusion_amd.models.schedulers import make_inference_scheduler
    det = LatentSampler(model.unet, make_inference_scheduler('ddim' if name == 'eta1' else 'dpm++2m'))
    plain = det.sample(lat0, txt, unc, **kw)
    assert _rel(got, plain) > SAMPLER_TOL
    assert torch.equal(plain, det.sample(lat0, txt, unc, seeds=seeds, **kw))      # a deterministic schedule reads no seeds
    with pytest.raises(ValueError, match='seeds'):
        smp.sample(lat0, txt, unc, **kw)
    smp.graphs.clear()


@pytest.mark.parametrize('name', ['eta1', 'dpm++2m-sde'])
def test_latent_sampler_stochastic_with_rescale_and_zero_snr(tiny, dev, name):
    from diffusion_amd.sampling import LatentSampler
    ocfg, model = tiny
    lat0, txt, unc = _inputs(ocfg, dev, seed=29)
    zkw = dict(prediction_type='v_prediction', rescale_betas_zero_snr=True, timestep_spacing='trailing')
    sch = _scheduler(name, **zkw)
    smp = LatentSampler(model.unet, sch)
    smp.graphs.clear()
    kw = dict(num_inference_steps=4, guidance_scale=3.0, guidance_rescale=0.7, seeds=[3, 4])
    got = smp.sample(lat0, txt, unc, **kw)
    assert int(sch.timesteps[0]) == 999 and torch.isfinite(got).all()
    assert torch.equal(got, smp.sample(lat0, txt, unc, graph=True, **kw))
    ref = _torch_route(model, _scheduler(name, **zkw), lat0, txt, unc, 4, 3.0, [3, 4], phi=0.7)
    e = _rel(got, ref)
    record(f'LatentSampler {name} zero-SNR rescale 0.7 hip vs torch', tolerances=dict(rel_l2=SAMPLER_TOL), rel_l2=e)
    print(f'{name}, zero terminal SNR, rescale 0.7: hip vs torch rel-L2 {e:.3e} (bound {SAMPLER_TOL})')
    assert e < SAMPLER_TOL, e
    smp.graphs.clear()


@pytest.mark.parametrize('name', ['eta1', 'dpm++2m-sde'])
def test_latent_sampler_stochastic_masked_sample_keeps_the_outside(tiny, dev, name):
    from diffusion_amd.sampling import LatentSampler
    ocfg, model = tiny
    lat0, txt, unc = _inputs(ocfg, dev, seed=31)
    known = torch.randn(2, 4, 8, 16, generator=torch.Generator().manual_seed(5)).to(dev)
    mask_px = torch.zeros(2, 64, 128, device=dev)
    mask_px[:, 16:48, 32:96] = 1.0
    smp = LatentSampler(model.unet, _scheduler(name))
    smp.graphs.clear()
    kw = dict(num_inference_steps=4, guidance_scale=3.0, known=known, noise=lat0, mask_px=mask_px, start_index=1, seeds=[8, 9])
    got = smp.sample(None, txt, unc, **kw)
    inside = torch.zeros(8, 16, dtype=torch.bool, device=dev)
    inside[2:6, 4:12] = True
    assert torch.equal(got[:, :, ~inside], known[:, :, ~inside])       # the last step's blend is (1, 0): the known bits
    assert not torch.equal(got[:, :, inside], known[:, :, inside]) and torch.isfinite(got).all()
    assert torch.equal(got, smp.sample(None, txt, unc, graph=True, **kw))
    other = smp.sample(None, txt, unc, **dict(kw, seeds=[8, 10]))
    assert torch.equal(other[0], got[0]) or _rel(other[0], got[0]) < SAMPLER_TOL     # image 0 keeps its seed
    assert not torch.equal(other[1][:, inside], got[1][:, inside])
    smp.graphs.clear()


# ---------------------------------------------------------------------------------------------------------------------
# 10. generate() of both families
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sd_model(dev):
    from diffusion_amd.models.models import stable_diffusion_2
    torch.manual_seed(11)
    return stable_diffusion_2(model_name='tiny', pretrained=False, fsdp=False)


def test_stable_diffusion_generate_stochastic(sd_model, dev, monkeypatch):
    monkeypatch.delenv('DA_SAMPLER', raising=False)
    model = sd_model
    kw = dict(prompt=['a cool doge', 'a hot cat'], height=64, width=64, num_inference_steps=3, progress_bar=False)
    base = model.generate(seed=3, **kw)
    assert torch.equal(model.generate(seed=3, eta=0.0, **kw), base)               # eta = 0 is the call without it
    assert torch.equal(model.generate(seed=3, eta=0.0, sampler='graph', **kw), base)
    for extra in (dict(eta=1.0), dict(inference_scheduler='dpm++2m-sde')):
        outs = {s: model.generate(seed=3, sampler=s, **extra, **kw) for s in ('hip', 'graph', 'torch')}
        assert torch.equal(outs['hip'], outs['graph']), extra
        assert torch.equal(outs['hip'], model.generate(seed=3, **extra, **kw))
        assert outs['hip'].shape == (2, 3, 64, 64) and torch.isfinite(outs['hip']).all()
        e = _rel(outs['hip'], outs['torch'])
        print(f'StableDiffusion.generate {extra}: hip vs torch image rel-L2 {e:.3e}')
        assert e < 8e-2, (extra, e)     # the decoder cap of test_vae_decoder_hip_gpu.py for image differences
        assert not torch.equal(outs['hip'], base)
        assert not torch.equal(model.generate(seed=4, **extra, **kw), outs['hip'])
        # per-image seeds: image 0 does not depend on who rides along (up to the U-Net's batch-dependent GEMM splits)
        a = model.generate(seed=[10, 11], **extra, **kw)
        b = model.generate(seed=[10, 12], **extra, **kw)
        e0 = _rel(a[0], b[0])
        record(f'generate {extra} image 0 under another neighbour', tolerances=dict(rel_l2=SAMPLER_TOL), rel_l2=e0)
        assert e0 < SAMPLER_TOL and not torch.equal(a[1], b[1]), (extra, e0)
        assert torch.equal(a, model.generate(seed=[10, 11], **extra, **kw))
    # per-image seeds with the deterministic sampler: the initial latents alone come from the streams
    a = model.generate(seed=[10, 11], **kw)
    b = model.generate(seed=[10, 12], **kw)
    assert _rel(a[0], b[0]) < SAMPLER_TOL and not torch.equal(a[1], b[1])
    c = model.generate(seed=[10, 11, 12, 13], num_images_per_prompt=2, eta=1.0, **kw)
    assert c.shape[0] == 4
    assert type(model.inference_scheduler).__name__ == 'DDIMScheduler' and model.inference_scheduler.eta == 0.0


def test_pixel_diffusion_generate_stochastic(dev, monkeypatch):
    from diffusion_amd.models.models import discrete_pixel_diffusion
    from diffusion_amd.models.unet import UNetConfig
    monkeypatch.delenv('DA_SAMPLER', raising=False)
    cfg = UNetConfig(in_channels=3, out_channels=3, block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4),
                     cross_attention_dim=768)
    torch.manual_seed(5)
    model = discrete_pixel_diffusion(unet_config=cfg, seed=3)
    kw = dict(prompt=['a cool doge', 'a hot cat'], height=8, width=8, num_inference_steps=3, guidance_scale=3.0,
              progress_bar=False)
    base = model.generate(seed=7, **kw)
    assert torch.equal(model.generate(seed=7, eta=0.0, **kw), base)
    for extra in (dict(eta=1.0), dict(inference_scheduler='dpm++2m-sde')):
        torch.manual_seed(19)
        outs = {s: model.generate(seed=7, sampler=s, **extra, **kw) for s in ('hip', 'graph', 'torch')}
        tail = torch.randn(1, device=dev).item()
        torch.manual_seed(19)
        assert tail == torch.randn(1, device=dev).item()          # nothing comes from the global generator
        assert torch.equal(outs['hip'], outs['graph']), extra
        assert outs['hip'].shape == (2, 3, 8, 8) and torch.isfinite(outs['hip']).all()
        e = _rel(outs['hip'], outs['torch'])
        print(f'PixelDiffusion.generate {extra}: hip vs torch image rel-L2 {e:.3e}')
        assert not torch.equal(outs['hip'], base)
        a = model.generate(seed=[10, 11], **extra, **kw)
        b = model.generate(seed=[10, 12], **extra, **kw)
        assert _rel(a[0], b[0]) < SAMPLER_TOL and not torch.equal(a[1], b[1]), extra
    torch.manual_seed(5)     # the random-init text encoder draws from the global generator: the same weights again
    hot = discrete_pixel_diffusion(unet_config=cfg, seed=3, inference_eta=1.0)
    assert hot.inference_scheduler.eta == 1.0
    assert torch.equal(hot.generate(seed=7, **kw), model.generate(seed=7, eta=1.0, **kw))


def test_trainer_eval_with_the_sde_solver_logs_a_clip_score(dev):
    import clip_reference as CR
    from diffusion_amd.metrics.clip_score import CLIPScore
    from diffusion_amd.models.composer_shim import MeanSquaredError
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.optim import FusedAdamW
    from diffusion_amd.trainer import Trainer
    clip = CR.tiny_clip(seed=5).to(dev)
    torch.manual_seed(11)
    model = stable_diffusion_2(model_name='tiny', pretrained=False, fsdp=False, encode_latents_in_fp16=False,
                               val_metrics=[MeanSquaredError(), CLIPScore(model=clip, device=dev)],
                               val_guidance_scales=[3.0], inference_scheduler='dpm++2m-sde')
    assert model.inference_scheduler.algorithm_type == 'sde-dpmsolver++'
    tok = model.tokenizer
    g = torch.Generator().manual_seed(4)
    evalset = [{'image': torch.randn(2, 3, 64, 64, generator=g),
                'captions': tok(['a red cube', 'a blue ball'], padding='max_length', max_length=77, truncation=True,
                                return_tensors='pt')['input_ids']}]
    tr = Trainer(model, train_dataloader=None, optimizers=FusedAdamW(lr=1e-3, weight_decay=0.01, unet=model.unet),
                 max_duration='1ba', eval_dataloader=evalset, log_every=1000)
    seen = []
    inner = model.generate
    model.generate = lambda **kw: seen.append(kw) or inner(**dict(kw, num_inference_steps=4))   # 4 steps, not eval's 50
    out = tr.eval()
    assert np.isfinite(out['metrics/eval/CLIPScore-scale-3p0'])
    assert len(seen) == 1 and seen[0]['seed'] == model.val_seed      # val_seed is the base of the per-image seeds
