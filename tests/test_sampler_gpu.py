"""GPU tests of the HIP sampling path: ``da_sampler_step`` against the schedulers' own ``step()`` in float64, the forward-only
U-Net walk against the recording one, ``LatentSampler`` (eager and graph replay) against the oracle sampler, and
``generate(sampler=...)`` of both models.

Bound of the kernel test, elementwise on |got - ref| with u = 2^-24:
    8u (|cx x| + |cm| (|pu| + g (|pt| + |pu|)) + |cn z|)        with guidance
    8u (|cx x| + |cm| |p| + |cn z|)                             without
It covers the six fp32 roundings of the arithmetic, the three coefficients rounded to fp32, and an FMA contraction either
way; a CPU simulation of the fp32 arithmetic peaked at 0.39 of it, a wrong coefficient misses it by orders of magnitude.
The reference is ``scheduler.step()`` on the float64 images of the same fp32 inputs, not the (cx, cm, cn) form."""
import dataclasses
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PAD = 1e30


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-20)).item()


# ---------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------
def _schedule_steps():
    """(scheduler, timestep) pairs from real schedules: first, middle and last steps, every prediction type; the second
    list is the SDE (the only steps with a noise term)."""
    from diffusion_amd.models.schedulers import DDIMScheduler
    from diffusion_amd.schedulers.schedulers import ContinuousTimeScheduler
    plain, sde = [], []
    for ptype in ('epsilon', 'v_prediction', 'sample'):
        d = DDIMScheduler(prediction_type=ptype)
        d.set_timesteps(50)
        plain += [(d, d.timesteps[0]), (d, d.timesteps[25]), (d, d.timesteps[-1])]
        o = ContinuousTimeScheduler(t_max=1.56, prediction_type=ptype, use_ode=True)
        o.set_timesteps(20)
        plain += [(o, o.timesteps[0]), (o, o.timesteps[-1])]
        s = ContinuousTimeScheduler(t_max=1.56, prediction_type=ptype, use_ode=False)
        s.set_timesteps(20)
        sde += [(s, s.timesteps[0]), (s, s.timesteps[7]), (s, s.timesteps[-1])]
    return plain, sde


def test_sampler_step_matches_scheduler_step_in_float64(dev, monkeypatch):
    from diffusion_amd import ops
    plain, sde = _schedule_steps()
    gen = torch.Generator().manual_seed(41)
    shapes = [(1, 1), (255, 1), (257, 1), (2 * 7 * 7, 1), (2 * 7 * 7, 49)]
    worst, count = 0.0, 0
    for (npix, HW), C, cfg, copies, with_noise, inplace in itertools.product(shapes, (3, 4, 8), (0, 1), (1, 2), (0, 1),
                                                                             (0, 1)):
        sch, t = (sde if with_noise else plain)[count % (len(sde) if with_noise else len(plain))]
        g = (1.5, 7.5)[(count // 3) % 2]
        count += 1
        B = npix // HW
        pred = torch.randn((2 if cfg else 1) * npix, 8, generator=gen)
        x = torch.randn(npix, 8, generator=gen)
        z = torch.randn(B, C, HW, 1, generator=gen)
        pred[:, C:] = PAD
        x[:, C:] = PAD
        cx, cm, cn = sch.step_coefficients(t)
        assert (cn != 0.0) == bool(with_noise)
        # float64 reference: guidance in the reference's order, then the scheduler's own step
        pu = pred[:npix, :C].double()
        pt = pred[npix:, :C].double() if cfg else pu
        m = pu + g * (pt - pu) if cfg else pu
        zz = z.double().view(B, C, HW).permute(0, 2, 1).reshape(npix, C)
        monkeypatch.setattr(torch, 'randn_like', lambda like, zz=zz: zz.clone())
        ref = sch.step(m, t, x[:, :C].double())['prev_sample']
        monkeypatch.undo()
        bound = 8 * U * ((cx * x[:, :C].double()).abs() + abs(cn) * zz.abs() * (1 if with_noise else 0)
                         + abs(cm) * ((pu.abs() + g * (pt.abs() + pu.abs())) if cfg else pu.abs()))
        # device
        coef = torch.tensor([cx, cm, cn, g], dtype=torch.float64).float().to(dev)
        dx, dpred = x.clone().to(dev), pred.to(dev)
        x_out = dx if inplace else torch.full((npix, 8), 7.0, device=dev)
        xt = torch.full((copies * npix, 8), 7.0, device=dev, dtype=torch.bfloat16)
        ops.sampler_step(dpred, dx, coef, x_out, xt, z.to(dev) if with_noise else None, C=C, cfg=cfg, copies=copies)
        got = x_out.cpu()
        err = (got[:, :C].double() - ref).abs()
        ratio = (err / bound).max().item()
        worst = max(worst, ratio)
        case = (npix, HW, C, cfg, copies, with_noise, inplace, type(sch).__name__, sch.prediction_type, float(t), g)
        assert ratio <= 1.0, (case, ratio)
        assert (got[:, C:] == 0).all(), case
        want_bf = torch.empty(npix, 8, device=dev, dtype=torch.bfloat16)
        ops.cast_f32_bf16(x_out, want_bf)
        for k in range(copies):
            assert torch.equal(xt[k * npix:(k + 1) * npix].view(torch.int16), want_bf.view(torch.int16)), (case, k)
        if not inplace:
            assert torch.equal(dx.cpu(), x), case   # the input is only read
        # last step: no next U-Net input
        x_last = torch.empty(npix, 8, device=dev)
        ops.sampler_step(dpred, dx if not inplace else x.to(dev), coef, x_last, None, z.to(dev) if with_noise else None,
                         C=C, cfg=cfg, copies=copies)
        assert torch.equal(x_last.cpu(), got), case
    print(f'sampler_step: {count} cases, worst |got - ref| / bound = {worst:.3f}')


def test_sampler_step_rejects_bad_arguments(dev):
    from diffusion_amd import _lib, ops
    npix, C = 98, 4
    pred = torch.zeros(2 * npix, 8, device=dev)
    x = torch.zeros(npix + 1, 8, device=dev)[:npix]
    coef = torch.zeros(8, device=dev)
    xt = torch.zeros(2 * npix + 1, 8, device=dev, dtype=torch.bfloat16)
    noise = torch.zeros(2, C, 7, 7, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t, off=0: t.data_ptr() + off   # noqa: E731

    def rc(pred_=p(pred), x_=p(x), noise_=p(noise), coef_=p(coef), xo=p(x), xt_=p(xt), npix_=npix, HW=49, C_=C, cfg=1,
           copies=2):
        return _lib.load().da_sampler_step(pred_, x_, noise_, coef_, xo, xt_, npix_, HW, C_, cfg, copies, s)

    assert rc() == 0 and rc(noise_=None, xt_=None) == 0
    for bad in (dict(C_=0), dict(C_=9), dict(copies=0), dict(copies=3), dict(HW=48), dict(HW=0), dict(npix_=0),
                dict(pred_=p(pred, 4)), dict(x_=p(x, 8)), dict(noise_=p(noise, 4)), dict(coef_=p(coef, 4)),
                dict(xo=p(x, 4)), dict(xt_=p(xt, 2)), dict(pred_=None), dict(x_=None), dict(coef_=None), dict(xo=None)):
        assert rc(**bad) == 1, bad
    torch.cuda.synchronize()
    # the wrapper
    ok = dict(C=C, cfg=True, copies=2)
    xc, c4 = x.contiguous(), coef[:4]
    ops.sampler_step(pred, xc, c4, xc, xt[:2 * npix], noise, **ok)
    with pytest.raises(ValueError):
        ops.sampler_step(pred, xc, c4, xc, xt[:2 * npix], noise, C=9, cfg=True, copies=2)
    with pytest.raises(ValueError):
        ops.sampler_step(pred, xc, c4, xc, xt[:2 * npix], noise, C=C, cfg=True, copies=3)
    with pytest.raises(ValueError):
        ops.sampler_step(pred[:npix], xc, c4, xc, None, None, **ok)            # half a guidance batch
    with pytest.raises(ValueError):
        ops.sampler_step(pred, xc, c4, xc, xt[:npix], None, **ok)              # one copy's room for two
    with pytest.raises(ValueError):
        ops.sampler_step(pred, xc, coef[1:5], xc, None, None, **ok)            # misaligned coefficients
    with pytest.raises(ValueError):
        ops.sampler_step(pred, xc, c4, xc, None, noise[:1], **ok)              # noise over half the pixels
    with pytest.raises(ValueError):
        ops.sampler_step(pred, xc.double(), c4, xc, None, None, **ok)
    with pytest.raises(ValueError):
        ops.sampler_step(pred.cpu(), xc, c4, xc, None, None, **ok)


# ---------------------------------------------------------------------------------------------------------------------
# the forward-only walk
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tiny(dev):
    from oracle import unet_oracle as O
    from diffusion_amd.models.models import stable_diffusion_2
    ocfg = O.UNetConfig.tiny()
    sd = O.init_state_dict(ocfg, seed=17)
    model = stable_diffusion_2(model_name='tiny', pretrained=False, precomputed_latents=True, fsdp=False)
    model.unet.load_state_dict(sd)
    return O, ocfg, sd, model


def _walk_inputs(unet, dev, B=4, S=8, seed=3):
    g = torch.Generator().manual_seed(seed)
    xt = unet.to_nhwc8(torch.randn(B, 4, S, S, generator=g).to(dev))
    t = torch.randint(0, 1000, (B,), generator=g).to(dev)
    ctx = unet.prepare_ctx(torch.randn(B, 77, unet.cfg.cross_attention_dim, generator=g).to(dev))
    return xt, t, ctx, B, S


def test_forward_only_walk_is_the_recording_walk_without_the_tape(tiny, dev):
    unet = tiny[3].unet
    xt, t, ctx, B, S = _walk_inputs(unet, dev)
    unet.forward_features(xt, t, ctx, B, S)   # scratch and workspaces exist before either peak is read
    unet._tape = unet._cats = unet._temb_saved = None

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base

    rec, peak_rec = peak(lambda: unet.forward_features(xt, t, ctx, B, S))
    assert unet._tape is not None
    unet._tape = unet._cats = unet._temb_saved = None
    kv = unet.project_context(ctx)
    assert len(kv) == 16
    got, peak_fwd = peak(lambda: unet.forward_features(xt, t, ctx, B, S, kv=kv, record=False))
    assert torch.equal(got, rec)
    assert unet._tape is None and unet._cats is None and unet._temb_saved is None
    assert unet._kv is None and unet._record is True
    print(f'forward walk peak above resident: recording {peak_rec} B, forward-only {peak_fwd} B')
    assert peak_fwd < peak_rec, (peak_fwd, peak_rec)
    # forward-only without the hoisted context: the same bits again
    assert torch.equal(unet.forward_features(xt, t, ctx, B, S, record=False), rec)
    with pytest.raises(ValueError):
        unet.forward_features(xt, t, ctx, B, S, kv=kv)   # a recording walk makes its own projections


def test_training_step_is_unchanged_by_a_sampler_call_in_between(tiny, dev):
    from diffusion_amd.sampling import LatentSampler
    model = tiny[3]
    unet = model.unet
    xt, t, ctx, B, S = _walk_inputs(unet, dev, seed=5)
    dpred = torch.randn(B * S * S, 8, generator=torch.Generator().manual_seed(6)).to(dev).to(torch.bfloat16)
    dpred[:, 4:] = 0

    def step(interleave):
        unet.zero_grad()
        pred = unet.forward_features(xt, t, ctx, B, S).clone()
        if interleave:   # between the recorded forward and its backward
            g = torch.Generator().manual_seed(8)
            LatentSampler(unet, model.inference_scheduler).sample(
                torch.randn(2, 4, S, S, generator=g).to(dev), torch.randn(2, 77, 128, generator=g).to(dev),
                torch.randn(2, 77, 128, generator=g).to(dev), num_inference_steps=2, guidance_scale=3.0)
        unet.backward_features(dpred)
        return pred, unet.grad.clone()

    p1, g1 = step(False)
    p2, g2 = step(True)
    assert torch.equal(p1, p2) and torch.equal(g1, g2)
    assert float(g1.abs().sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# LatentSampler against the oracle; graph replay
# ---------------------------------------------------------------------------------------------------------------------
def _parity_inputs(ocfg, seed=23, B=2, S=8):
    g = torch.Generator().manual_seed(seed)   # the draws of test_ddim_sampler_parity
    lat0 = torch.randn(B, 4, S, S, generator=g)
    txt = torch.randn(B, 77, ocfg.cross_attention_dim, generator=g)
    unc = torch.randn(B, 77, ocfg.cross_attention_dim, generator=g)
    return lat0, txt, unc


def _torch_loop(model, lat0, txt, unc, steps, guidance, dev):
    sch = model.inference_scheduler
    sch.set_timesteps(steps)
    lat = lat0.to(dev)
    emb = torch.cat([unc, txt]).to(dev) if guidance > 1.0 else txt.to(dev)
    with torch.no_grad():
        for t in sch.timesteps:
            x = torch.cat([lat] * 2) if guidance > 1.0 else lat
            pred = model.unet(x, t, encoder_hidden_states=emb).sample
            if guidance > 1.0:
                pu, pt = pred.chunk(2)
                pred = pu + guidance * (pt - pu)
            lat = sch.step(pred, t, lat)['prev_sample']
    return lat.cpu()


@pytest.fixture(scope='module')
def oracle_samples(tiny):
    """The float reference, computed once per (prediction type, guidance) and shared"""
    O, ocfg, sd, _ = tiny
    lat0, txt, unc = _parity_inputs(ocfg)
    out = {('epsilon', g): O.ddim_sample(sd, ocfg, txt, unc, lat0, 4, g) for g in (0.0, 3.0)}
    vcfg = dataclasses.replace(ocfg, prediction_type='v_prediction')
    out[('v_prediction', 3.0)] = O.ddim_sample(sd, vcfg, txt, unc, lat0, 4, 3.0)
    return out


@pytest.mark.parametrize('ptype,guidance', [('epsilon', 0.0), ('epsilon', 3.0), ('v_prediction', 3.0)])
def test_latent_sampler_matches_the_oracle(tiny, oracle_samples, dev, ptype, guidance):
    from diffusion_amd.sampling import LatentSampler
    O, ocfg, sd, model = tiny
    lat0, txt, unc = _parity_inputs(ocfg)
    ref = oracle_samples[(ptype, guidance)]
    sch = model.inference_scheduler
    old, sch.prediction_type = sch.prediction_type, ptype
    try:
        smp = LatentSampler(model.unet, sch)
        run = lambda **kw: smp.sample(lat0.to(dev), txt.to(dev), unc.to(dev), num_inference_steps=4,   # noqa: E731
                                      guidance_scale=guidance, **kw)
        got = run()
        assert got.shape == lat0.shape and got.dtype == torch.float32 and got.is_contiguous()
        assert [int(t) for t in sch.timesteps] == [int(t) for t in O.ddim_timesteps(4)]
        again = run()
        loop = _torch_loop(model, lat0, txt, unc, 4, guidance, dev)
    finally:
        sch.prediction_type = old
    e_hip, e_torch, d = _rel(got.cpu(), ref), _rel(loop, ref), _rel(got.cpu(), loop)
    print(f'{ptype} guidance {guidance}: rel-L2 to the oracle hip {e_hip:.3e}, torch loop {e_torch:.3e}; '
          f'hip vs torch {d:.3e}')
    assert torch.equal(got, again)
    assert e_hip < 3e-2, e_hip


@pytest.mark.parametrize('guidance', [0.0, 3.0])
def test_graph_replay_equals_the_eager_sampler(tiny, dev, guidance):
    from diffusion_amd.sampling import LatentSampler
    O, ocfg, sd, model = tiny
    smp = LatentSampler(model.unet, model.inference_scheduler)
    smp.graphs.clear()
    for n, seed in enumerate((23, 77)):   # the second call, other latents and context, reuses the capture
        lat0, txt, unc = _parity_inputs(ocfg, seed=seed)
        args = (lat0.to(dev), txt.to(dev), unc.to(dev))
        eager = smp.sample(*args, num_inference_steps=4, guidance_scale=guidance)
        graphed = smp.sample(*args, num_inference_steps=4, guidance_scale=guidance, graph=True)
        assert len(smp.graphs) == 1
        assert torch.equal(eager, graphed), (n, _rel(graphed, eager))
    smp.graphs.clear()


# ---------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------
def test_stable_diffusion_generate_hip_against_torch(dev, monkeypatch):
    from diffusion_amd.models.models import stable_diffusion_2
    monkeypatch.delenv('DA_SAMPLER', raising=False)
    torch.manual_seed(11)
    model = stable_diffusion_2(model_name='tiny', pretrained=False, fsdp=False)
    kw = dict(prompt=['a cool doge', 'a hot cat'], height=64, width=64, num_inference_steps=2, seed=3, progress_bar=False)
    ref = model.generate(sampler='torch', **kw)
    hip = model.generate(sampler='hip', **kw)
    assert torch.equal(hip, model.generate(**kw))   # the default
    assert hip.shape == ref.shape == (2, 3, 64, 64)
    assert torch.isfinite(hip).all() and hip.min() >= 0 and hip.max() <= 1
    e = _rel(hip, ref)
    print(f'StableDiffusion.generate: hip vs torch image rel-L2 {e:.3e}')
    assert e < 8e-2, e   # the decoder cap of test_vae_decoder_hip_gpu.py for image differences
    graph = model.generate(sampler='graph', **kw)
    assert torch.equal(graph, hip)
    with pytest.raises(ValueError):
        model.generate(sampler='nonsense', **kw)


def _pixel_cfg():
    from diffusion_amd.models.unet import UNetConfig
    return UNetConfig(in_channels=3, out_channels=3, block_out_channels=(64, 128, 256, 256),
                      attention_head_dim=(1, 2, 4, 4), cross_attention_dim=768)


@pytest.fixture(scope='module')
def pixel_models(dev):
    from diffusion_amd.models.models import continuous_pixel_diffusion, discrete_pixel_diffusion
    torch.manual_seed(5)
    return {'discrete': discrete_pixel_diffusion(unet_config=_pixel_cfg(), seed=3),
            'continuous': continuous_pixel_diffusion(unet_config=_pixel_cfg(), seed=3)}


@pytest.mark.parametrize('kind', ['discrete', 'ode', 'sde'])
def test_pixel_diffusion_generate(pixel_models, dev, kind, monkeypatch):
    model = pixel_models['discrete' if kind == 'discrete' else 'continuous']
    if kind != 'discrete':   # read at call time by step() and step_coefficients()
        monkeypatch.setattr(model.inference_scheduler, 'use_ode', kind == 'ode')
    kw = dict(prompt=['a cool doge'], height=8, width=8, num_inference_steps=3, guidance_scale=3.0, seed=7,
              progress_bar=False)
    tails = {}
    for sampler in ('torch', 'hip', 'graph'):
        torch.manual_seed(19)
        out = model.generate(sampler=sampler, **kw)
        tails[sampler] = torch.randn(1, device=dev).item()   # what the global generator gives next
        assert out.shape == (1, 3, 8, 8)
        assert torch.isfinite(out).all() and out.min() >= 0 and out.max() <= 1
    # the SDE draws exactly as many values from the global generator as step() does; the others draw none
    assert tails['hip'] == tails['torch'] and tails['graph'] == tails['torch'], tails
    torch.manual_seed(19)
    untouched = torch.randn(1, device=dev).item()
    assert (tails['torch'] == untouched) == (kind != 'sde')
