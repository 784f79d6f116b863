"""GPU end-to-end tests of zero-terminal-SNR training and sampling on the tiny U-Net: the Min-SNR-weighted loss and its
gradient through ``StableDiffusion``, ``LatentSampler`` with guidance rescale on the rescaled table with trailing spacing
against a float64 loop around the oracle's U-Net, and ``generate()`` on every ``sampler=`` route."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
STEPS, GUIDANCE, PHI = 4, 3.0, 0.7


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-20)).item()


def _vcfg():
    from diffusion_amd.models.unet import UNetConfig
    cfg = UNetConfig.tiny()
    cfg.prediction_type = 'v_prediction'
    return cfg


@pytest.fixture(scope='module')
def tiny_v(dev):
    """the tiny v-prediction model on the zero-terminal-SNR schedule with Min-SNR weighting, the oracle's weights loaded"""
    from oracle import unet_oracle as O
    from diffusion_amd.models.models import stable_diffusion_2
    ocfg = dataclasses.replace(O.UNetConfig.tiny(), prediction_type='v_prediction')
    sd = O.init_state_dict(ocfg, seed=17)
    model = stable_diffusion_2(model_name='tiny', pretrained=False, precomputed_latents=True, fsdp=False,
                               unet_config=_vcfg(), zero_terminal_snr=True, snr_gamma=5.0)
    model.unet.load_state_dict(sd)
    return O, ocfg, sd, model


# ---------------------------------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------------------------------
def _train_batch(dev, S=8):
    g = torch.Generator().manual_seed(31)
    return {'image_latents': torch.randn(4, 4, S, S, generator=g).to(dev),
            'caption_latents': torch.randn(4, 77, 128, generator=g).to(dev),
            '_timesteps': torch.tensor([0, 139, 500, 999]).to(dev), '_noise': torch.randn(4, 4, S, S, generator=g).to(dev)}


def test_min_snr_weighted_training_step(tiny_v, dev, monkeypatch):
    from diffusion_amd import ops
    from diffusion_amd.graph_step import GraphStepCache
    from diffusion_amd.models.schedulers import min_snr_weights
    model = tiny_v[3]
    assert model.snr_gamma == 5.0 and model.prediction_type == 'v_prediction'
    assert model.noise_scheduler.rescale_betas_zero_snr and float(model.noise_scheduler.alphas_cumprod[999]) == 0.0
    assert model.inference_scheduler.timestep_spacing == 'trailing' and model.inference_scheduler.rescale_betas_zero_snr
    batch = _train_batch(dev)
    B, HW = 4, 64
    npix = B * HW
    w64 = min_snr_weights(model.noise_scheduler.alphas_cumprod, 5.0, 'v_prediction')
    wtab = model.snr_weight_table(dev)
    assert wtab is model.snr_weight_table(dev) and torch.equal(wtab.cpu(), w64.float())     # built once, cached per device
    w = wtab.cpu().double()[batch['_timesteps'].cpu()]
    assert float(w[3]) == 0.0 and float(w[2]) == pytest.approx(0.241019, rel=1e-4)

    model.unet.zero_grad()
    out = model(batch)
    pred, target = out[0].double().cpu(), out[1].double().cpu()
    # at t = 999 the input is the noise and the target is -x0
    assert torch.equal(out[1][3].cpu(), -batch['image_latents'][3].cpu())
    pred8, target8 = model._pending[0].clone(), model._pending[1].clone()
    loss = model.loss(out, batch)
    dpred = model._dpred.clone()
    want = float((w[:, None, None, None] * (pred - target)**2).sum()) / (4 * npix)
    depth = 4 * 1 + 6 + 4 + 1 + 6 + 4 + 4 + 1       # mse_geometry(256, 4) of tests/test_pointwise_edges_gpu.py, plus w
    rel = abs(loss.item() - want) / (want * depth * U)
    unweighted = float(((pred - target)**2).mean())
    print(f'weighted loss {loss.item():.6f} vs float64 {want:.6f}: {rel:.3f} of (depth {depth}) x 2^-24; unweighted {unweighted:.6f}')
    assert rel <= 1.0 and abs(want - unweighted) > 1e-2 * unweighted
    # the t = 999 sample (weight 0) contributes exactly nothing to the gradient
    assert bool((dpred.view(B, HW, 8)[3] == 0).all()) and bool((dpred.view(B, HW, 8)[0, :, :4] != 0).any())
    assert bool((dpred[:, 4:] == 0).all())
    model.backward_from_loss()
    torch.cuda.synchronize()
    got = dict(model.unet.named_parameters())['conv_out.bias'].grad.double().cpu()
    d64 = dpred.double().cpu()[:, :4]
    ref = d64.sum(0)
    assert got.shape == ref.shape
    assert bool(((got - ref).abs() <= npix * U * d64.abs().sum(0)).all()), (got, ref)      # an fp32 sum of 256 terms
    assert float(ref.abs().max()) > 0

    # snr_gamma = None is the parent's launch: the bits of a direct ops.mse_loss call
    monkeypatch.setattr(model, 'snr_gamma', None)
    out = model(batch)
    assert torch.equal(model._pending[0], pred8) and torch.equal(model._pending[1], target8)
    plain = model.loss(out, batch)
    dp, lb = torch.empty(npix, 8, device=dev, dtype=torch.bfloat16), torch.zeros(1, device=dev)
    ops.mse_loss(pred8, target8, dp, lb, model.unet._scratch, npix, 2.0 / (4.0 * npix), 1.0, 0)
    assert torch.equal(plain.detach().view(1).view(torch.int32), lb.view(torch.int32))
    assert torch.equal(model._dpred.view(torch.int16), dp.view(torch.int16))
    assert abs(plain.item() - unweighted) < 1e-5
    model._run_backward(None)
    # the captured training step would drop the weighting, so with snr_gamma it is declined and the eager path runs
    cache = GraphStepCache(model)
    assert cache.usable(batch)
    monkeypatch.undo()
    assert model.snr_gamma == 5.0 and not cache.usable(batch)
    model.unet.zero_grad()


def test_trainer_step_with_graph_requested_keeps_the_weighting(tiny_v, dev, monkeypatch):
    """DA_GRAPH=1 asks for captured microbatches; with snr_gamma the cache declines, so the loss is the eager weighted one"""
    from diffusion_amd.graph_step import GraphStepCache
    model = tiny_v[3]
    monkeypatch.setenv('DA_GRAPH', '1')
    batch = _train_batch(dev)
    cache = GraphStepCache(model)
    assert not cache.usable(batch) and not cache.graphs
    model.unet.zero_grad()
    out = model(batch)
    eager = model.loss(out, batch)
    model.backward_from_loss()
    out2 = model(batch)
    again = model.loss(out2, batch)
    model.backward_from_loss()
    assert torch.equal(eager, again)
    model.unet.zero_grad()


# ---------------------------------------------------------------------------------------------------------------------
# sampling
# ---------------------------------------------------------------------------------------------------------------------
def _inputs(ocfg, seed=23, B=2, S=8):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 4, S, S, generator=g), torch.randn(B, 77, ocfg.cross_attention_dim, generator=g),
            torch.randn(B, 77, ocfg.cross_attention_dim, generator=g))


def _scheduler(name):
    from diffusion_amd.models.schedulers import make_inference_scheduler
    return make_inference_scheduler(name, prediction_type='v_prediction', rescale_betas_zero_snr=True,
                                    timestep_spacing='trailing')


def _rescale64(m, pt, phi):
    dims = (1, 2, 3)
    std = lambda z: ((z - z.mean(dim=dims, keepdim=True))**2).sum(dim=dims, keepdim=True).sqrt()   # noqa: E731
    return m * (phi * std(pt) / std(m) + 1 - phi)


def _loop64(O, ocfg, sd64, sch, lat0, txt, unc, phi):
    """the float64 sampler: the oracle's U-Net forward, guidance, rescale, and the step as the scheduler's coefficients"""
    sch.set_timesteps(STEPS)
    ts = sch.timesteps.tolist()
    x, emb, hist = lat0.double(), torch.cat([unc, txt]).double(), None
    for i, t in enumerate(ts):
        out = O.unet_forward(sd64, ocfg, torch.cat([x] * 2), torch.full((2 * x.shape[0],), t, dtype=torch.int64), emb)
        pu, pt = out.chunk(2)
        m = _rescale64(pu + GUIDANCE * (pt - pu), pt, phi)
        if getattr(sch, 'multistep', False):
            ax, am, kx, k0, k1 = sch.step_coefficients_ms(i)
            d = ax * x + am * m
            x = kx * x + k0 * d + (k1 * hist if k1 != 0.0 else 0.0)
            hist = d
        else:
            cx, cm, _ = sch.step_coefficients(t)
            x = cx * x + cm * m
    return x


def _torch_loop(unet, sch, lat0, txt, unc, phi, dev):
    from diffusion_amd.sampling import rescale_noise_cfg
    sch.set_timesteps(STEPS)
    lat, emb = lat0.to(dev), torch.cat([unc, txt]).to(dev)
    with torch.no_grad():
        for t in sch.timesteps:
            pu, pt = unet(torch.cat([lat] * 2), t, encoder_hidden_states=emb).sample.chunk(2)
            lat = sch.step(rescale_noise_cfg(pu + GUIDANCE * (pt - pu), pt, phi), t, lat)['prev_sample']
    return lat.cpu()


@pytest.fixture(scope='module')
def oracle64(tiny_v):
    """the float64 references, computed once per solver and shared"""
    O, ocfg, sd, _ = tiny_v
    sd64 = {k: v.double() for k, v in sd.items()}
    lat0, txt, unc = _inputs(ocfg)
    with torch.no_grad():
        return {name: _loop64(O, ocfg, sd64, _scheduler(name), lat0, txt, unc, PHI) for name in ('ddim', 'dpm++2m')}


@pytest.mark.parametrize('solver', ['ddim', 'dpm++2m'])
def test_rescaled_sampler_against_float64(tiny_v, oracle64, dev, solver):
    from diffusion_amd.sampling import LatentSampler
    O, ocfg, sd, model = tiny_v
    lat0, txt, unc = _inputs(ocfg)
    sch = _scheduler(solver)
    smp = LatentSampler(model.unet, sch)
    smp.graphs.clear()
    run = lambda **kw: smp.sample(lat0.to(dev), txt.to(dev), unc.to(dev), num_inference_steps=STEPS,   # noqa: E731
                                  guidance_scale=GUIDANCE, **kw)
    got = run(guidance_rescale=PHI)
    assert sch.timesteps.tolist() == [999, 749, 499, 249]
    assert got.shape == lat0.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    ref = oracle64[solver]
    loop = _torch_loop(model.unet, sch, lat0, txt, unc, PHI, dev)
    e_hip, e_loop, d = _rel(got.cpu(), ref), _rel(loop, ref), _rel(got.cpu(), loop)
    cap = 3e-2 if e_loop <= 3e-2 else 1.5 * e_loop
    print(f'{solver} zero-SNR trailing g {GUIDANCE} phi {PHI}: rel-L2 to float64 hip {e_hip:.3e}, torch loop {e_loop:.3e}; '
          f'hip vs torch {d:.3e}; cap {cap:.3e}')
    assert e_hip < cap, (e_hip, e_loop)
    plain = run()
    assert _rel(plain.cpu(), got.cpu()) > 1e-3                  # the rescale does something
    assert torch.equal(run(guidance_rescale=0.0), plain)        # phi = 0: today's launches
    assert torch.equal(got, run(guidance_rescale=PHI))          # two calls, the same bits
    graphed = run(guidance_rescale=PHI, graph=True)
    assert torch.equal(graphed, got), _rel(graphed, got)
    # another phi must not replay the capture made for phi = 0.7
    eager2 = run(guidance_rescale=0.2)
    graphed2 = run(guidance_rescale=0.2, graph=True)
    assert torch.equal(graphed2, eager2) and not torch.equal(eager2, got)
    assert torch.equal(run(guidance_rescale=PHI, graph=True), got)
    # without guidance there is nothing to rescale
    one = smp.sample(lat0.to(dev), txt.to(dev), None, num_inference_steps=STEPS, guidance_scale=1.0, guidance_rescale=PHI)
    assert torch.equal(one, smp.sample(lat0.to(dev), txt.to(dev), None, num_inference_steps=STEPS, guidance_scale=1.0))
    smp.graphs.clear()


# ---------------------------------------------------------------------------------------------------------------------
# generate()
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gen_models(dev):
    from diffusion_amd.models.models import stable_diffusion_2
    torch.manual_seed(11)
    v = stable_diffusion_2(model_name='tiny', pretrained=False, fsdp=False, unet_config=_vcfg(), zero_terminal_snr=True,
                           guidance_rescale=0.7)
    torch.manual_seed(11)
    eps = stable_diffusion_2(model_name='tiny', pretrained=False, fsdp=False)
    return v, eps


def _check_images(out, shape):
    assert out.shape == shape and out.dtype == torch.float32
    assert bool(torch.isfinite(out).all()) and out.min() >= 0 and out.max() <= 1


@pytest.mark.parametrize('solver', [None, 'dpm++2m'])
@pytest.mark.parametrize('inpaint', [False, True], ids=['text', 'inpaint'])
def test_generate_with_rescale_and_trailing(gen_models, dev, monkeypatch, solver, inpaint):
    monkeypatch.delenv('DA_SAMPLER', raising=False)
    model = gen_models[0]
    assert model.guidance_rescale == 0.7 and model.inference_scheduler.timestep_spacing == 'trailing'
    kw = dict(prompt=['a cool doge', 'a hot cat'], num_inference_steps=4, seed=3, progress_bar=False, inference_scheduler=solver,
              guidance_rescale=0.7, timestep_spacing='trailing')
    if inpaint:
        g = torch.Generator().manual_seed(9)
        mask = torch.zeros(64, 64)
        mask[:, 32:] = 1.0
        kw.update(init_image=torch.rand(2, 3, 64, 64, generator=g), mask=mask, strength=0.5)
    else:
        kw.update(height=64, width=64)
    hip = model.generate(sampler='hip', **kw)
    _check_images(hip, (2, 3, 64, 64))
    assert torch.equal(model.generate(sampler='graph', **kw), hip)
    ref = model.generate(sampler='torch', **kw)
    e = _rel(hip, ref)
    print(f'generate zero-SNR {solver or "ddim"} {"inpaint" if inpaint else "text"}: hip vs torch image rel-L2 {e:.3e}')
    assert e < 8e-2, e
    # the model's defaults are these keywords
    defaults = dict(kw)
    del defaults['guidance_rescale'], defaults['timestep_spacing']
    assert torch.equal(model.generate(sampler='hip', **defaults), hip)
    assert not torch.equal(model.generate(sampler='hip', **dict(kw, guidance_rescale=0.0)), hip)


def test_generate_defaults_keep_their_bits_and_bad_options_raise(gen_models, dev, monkeypatch):
    from diffusion_amd.models.schedulers import DDIMScheduler
    monkeypatch.delenv('DA_SAMPLER', raising=False)
    v, eps = gen_models
    kw = dict(prompt=['a cool doge', 'a hot cat'], height=64, width=64, num_inference_steps=2, seed=3, progress_bar=False)
    for sampler in ('hip', 'torch'):
        base = eps.generate(sampler=sampler, **kw)
        assert torch.equal(eps.generate(sampler=sampler, guidance_rescale=0.0, timestep_spacing='leading', **kw), base)
    for sampler in ('hip', 'graph', 'torch'):
        launches = []
        monkeypatch.setattr(eps, '_prepare_text_embeddings', lambda *a, **k: launches.append(1))
        monkeypatch.setattr(v, '_prepare_text_embeddings', lambda *a, **k: launches.append(1))
        with pytest.raises(ValueError, match='guidance_rescale'):
            eps.generate(sampler=sampler, guidance_rescale=1.5, **kw)
        with pytest.raises(ValueError, match='timestep_spacing'):
            eps.generate(sampler=sampler, timestep_spacing='linspace', **kw)
        bad = DDIMScheduler(prediction_type='epsilon', rescale_betas_zero_snr=True, timestep_spacing='trailing')
        with pytest.raises(ValueError, match='zero terminal SNR'):
            v.generate(sampler=sampler, inference_scheduler=bad, **kw)
        assert not launches                                     # raised before the first launch (the text encoder's)
        monkeypatch.undo()
        monkeypatch.delenv('DA_SAMPLER', raising=False)
