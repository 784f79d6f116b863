"""Rectangular inputs end to end on the MI355X: the U-Net walk on H != W against the CPU oracle (train step, forward, sampler),
the square walk unchanged, the divisibility rule, ``generate(height, width)`` of both model families, the VAE walks against
the torch ``AutoencoderKL`` and ``Trainer.eval`` on a rectangular batch.

Throughout (H, W) is rows x columns.  The tiny U-Net has 4 levels, so its inputs are multiples of 8.  Bounds are those of the
square tests next to which each case would sit (named at each use); an H / W mix-up is not a rounding matter - the walk on
the transposed input, transposed back, is at rel-L2 1.1 ... 1.2 from the straight call."""
import copy
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
sys.path.insert(0, HERE)

import clip_reference as CR  # noqa: E402
from parity_margins import record  # noqa: E402

pytestmark = pytest.mark.gpu

# tests/test_unet_parity_gpu.py's bounds for the tiny width (tiny_s16_b2 has the output count of the two train-step cases here)
TOL_TINY = {'pred_rel': 2.3e-2, 'loss_abs': 5.6e-4, 'grad_rel': 4e-2, 'matrix_cos': 0.9957, 'vector_rel': 2.3e-2}
VAE_CAP = 8e-2   # tests/test_vae_decoder_hip_gpu.py


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-20)).item()


def _inputs(B, H, W, ctx_dim, seed=17, C=4):
    g = torch.Generator().manual_seed(seed)
    latents = torch.randn(B, C, H, W, generator=g)
    ctx = torch.randn(B, 77, ctx_dim, generator=g)
    noise = torch.randn(B, C, H, W, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    return latents, ctx, noise, t


def _grad_margins(got, grads_ref):
    """global rel-L2, worst weight-matrix cosine, rel-L2 over the vectors: test_tiny_train_step_parity's three figures"""
    num = sum(((got[k] - grads_ref[k])**2).sum().item() for k in grads_ref)
    den = sum((grads_ref[k]**2).sum().item() for k in grads_ref)
    worst = (None, 1.0)
    for k, gr in grads_ref.items():
        if gr.dim() < 2 or gr.norm() == 0:
            continue
        cos = torch.nn.functional.cosine_similarity(got[k].flatten(), gr.flatten(), dim=0).item()
        if cos < worst[1]:
            worst = (k, cos)
    vk = [k for k in grads_ref if grads_ref[k].dim() == 1]
    numv = sum(((got[k] - grads_ref[k])**2).sum().item() for k in vk)
    denv = sum((grads_ref[k]**2).sum().item() for k in vk)
    return math.sqrt(num / den), worst, math.sqrt(numv / denv)


@pytest.fixture(scope='module')
def tiny(dev):
    """the tiny latent model on precomputed latents with the oracle's weights"""
    from oracle import unet_oracle as O
    from diffusion_amd.models.models import stable_diffusion_2
    ocfg = O.UNetConfig.tiny()
    sd = O.init_state_dict(ocfg, seed=17)
    model = stable_diffusion_2(model_name='tiny', pretrained=False, precomputed_latents=True, fsdp=False)
    model.unet.load_state_dict(sd)
    return O, ocfg, sd, model


@pytest.fixture(scope='module')
def tiny_images(dev):
    """the tiny latent model with its VAE and text encoder (random weights): generate(), eval"""
    from diffusion_amd.models.models import stable_diffusion_2
    torch.manual_seed(11)
    return stable_diffusion_2(model_name='tiny', pretrained=False, fsdp=False)


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: the walk against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', [(8, 32), (32, 8)])
def test_rect_train_step_parity(tiny, dev, H, W):
    """test_tiny_train_step_parity's procedure at B = 2 on 8 x 32 and 32 x 8 latents (bottom level 1 x 4 / 4 x 1)"""
    O, ocfg, sd, model = tiny
    B = 2
    latents, ctx, noise, t = _inputs(B, H, W, ocfg.cross_attention_dim)
    loss_ref, pred_ref, grads_ref = O.training_loss_and_grads(sd, ocfg, latents, t, ctx, noise)
    batch = {'image_latents': latents.to(dev), 'caption_latents': ctx.to(dev)}
    model.unet.zero_grad()
    out = model(batch, timesteps=t.to(dev), noise=noise.to(dev))
    pred, target, ts = out
    assert pred.shape == latents.shape and target.shape == latents.shape
    assert torch.equal(ts.cpu(), t)
    e = _rel(pred.cpu(), pred_ref)
    loss = model.loss(out, batch)
    dl = abs(loss.item() - loss_ref.item())
    loss.backward()
    torch.cuda.synchronize()
    got = {k: p.grad.detach().float().cpu() for k, p in model.unet.named_parameters()}
    grel, worst, vrel = _grad_margins(got, grads_ref)
    print(f'tiny_{H}x{W}_b2: pred rel-L2 {e:.3e}, |loss - oracle| {dl:.3e}, grad rel-L2 {grel:.3e}, worst matrix cosine '
          f'{worst[1]:.5f} ({worst[0]}), vector grads rel-L2 {vrel:.3e}')
    record(f'tiny_{H}x{W}_b2', tolerances=TOL_TINY, pred_rel_l2=e, loss_abs_delta=dl, grad_rel_l2=grel,
           worst_matrix_cosine=worst[1], worst_matrix=worst[0], vector_grads_rel_l2=vrel)
    assert e < TOL_TINY['pred_rel'], f'eps-prediction rel-L2 {e}'
    assert dl < TOL_TINY['loss_abs'], (loss.item(), loss_ref.item())
    assert grel < TOL_TINY['grad_rel'], f'global grad rel-L2 {grel}'
    assert worst[1] >= TOL_TINY['matrix_cos'], worst
    assert vrel < TOL_TINY['vector_rel'], vrel


def test_rect_forward_at_a_ratio_that_is_no_power_of_two(tiny, dev):
    """B = 1, 8 x 24 (bottom level 1 x 3), through the model's forward and through the diffusers-style call"""
    O, ocfg, sd, model = tiny
    latents, ctx, noise, t = _inputs(1, 8, 24, ocfg.cross_attention_dim, seed=5)
    pred_ref, _ = O.training_forward(sd, ocfg, latents, t, ctx, noise)
    batch = {'image_latents': latents.to(dev), 'caption_latents': ctx.to(dev)}
    pred, _, _ = model(batch, timesteps=t.to(dev), noise=noise.to(dev))
    e = _rel(pred.cpu(), pred_ref)
    model._pending = None
    model.unet._tape = None
    x = O.DDPMSchedule().add_noise(latents, noise, t)
    o = model.unet(x.to(dev), t.to(dev), ctx.to(dev))
    e2 = _rel(o.sample.cpu(), O.unet_forward(sd, ocfg, x, t, ctx))
    print(f'tiny_8x24_b1: pred rel-L2 {e:.3e} (forward), {e2:.3e} (UNetHIP.forward)')
    record('tiny_8x24_b1', tolerances={'pred_rel': TOL_TINY['pred_rel']}, pred_rel_l2=e, unet_call_rel_l2=e2)
    assert pred.shape == (1, 4, 8, 24) and o.sample.shape == (1, 4, 8, 24)
    assert e < TOL_TINY['pred_rel'], e
    assert e2 < TOL_TINY['pred_rel'], e2


# ---------------------------------------------------------------------------------------------------------------------
# 3: the square walk is what it was
# ---------------------------------------------------------------------------------------------------------------------
def test_int_side_and_square_pair_are_the_same_walk(tiny, dev):
    unet = tiny[3].unet
    B, S = 2, 16
    g = torch.Generator().manual_seed(3)
    xt = unet.to_nhwc8(torch.randn(B, 4, S, S, generator=g).to(dev))
    t = torch.randint(0, 1000, (B,), generator=g).to(dev)
    ctx = unet.prepare_ctx(torch.randn(B, 77, unet.cfg.cross_attention_dim, generator=g).to(dev))
    dpred = torch.randn(B * S * S, 8, generator=g).to(dev).to(torch.bfloat16)
    dpred[:, 4:] = 0
    res = []
    for side in (S, (S, S)):
        unet.zero_grad()
        pred = unet.forward_features(xt, t, ctx, B, side).clone()
        unet.backward_features(dpred)
        torch.cuda.synchronize()
        res.append((pred, unet.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float(res[0][1].abs().sum()) > 0
    kv = unet.project_context(ctx)
    assert torch.equal(unet.forward_features(xt, t, ctx, B, [S, S], kv=kv, record=False), res[0][0])


# ---------------------------------------------------------------------------------------------------------------------
# 4: the shape rule
# ---------------------------------------------------------------------------------------------------------------------
def test_extents_that_are_no_multiple_of_8_are_refused_before_any_launch(tiny, tiny_images, dev, monkeypatch):
    from diffusion_amd import _lib
    from diffusion_amd.sampling import LatentSampler
    O, ocfg, sd, model = tiny
    latents, ctx, noise, t = (z.to(dev) for z in _inputs(2, 8, 12, ocfg.cross_attention_dim))
    torch.cuda.synchronize()
    launched = []
    monkeypatch.setattr(_lib, 'call', lambda name, *a: launched.append(name))
    batch = {'image_latents': latents, 'caption_latents': ctx}
    with pytest.raises(ValueError, match='multiples of 8'):
        model(batch, timesteps=t, noise=noise)
    with pytest.raises(ValueError, match='multiples of 8'):
        model.unet(latents, t, ctx)
    with pytest.raises(ValueError, match='multiples of 8'):
        model.unet(latents.transpose(2, 3).contiguous(), t, ctx)      # 12 x 8
    with pytest.raises(ValueError, match='multiples of 8'):
        model.unet.forward_features(torch.zeros(2 * 8 * 12, 8, device=dev, dtype=torch.bfloat16), t, None, 2, (8, 12))
    with pytest.raises(ValueError, match='multiples of 8'):
        LatentSampler(model.unet, model.inference_scheduler).sample(latents, ctx, ctx, num_inference_steps=2, guidance_scale=3.0)
    with pytest.raises(ValueError, match='multiples of 8'):
        tiny_images.generate(prompt=['a cool doge'], height=64, width=96, num_inference_steps=1, progress_bar=False)
    with pytest.raises(ValueError):
        tiny_images.generate(prompt=['a cool doge'], height=64, width=132, num_inference_steps=1, progress_bar=False)
    assert launched == []
    assert model._pending is None and model.unet._tape is None


# ---------------------------------------------------------------------------------------------------------------------
# 5: the sampler
# ---------------------------------------------------------------------------------------------------------------------
def _sampler_inputs(ocfg, H, W, seed=23, B=2):
    g = torch.Generator().manual_seed(seed)
    lat0 = torch.randn(B, 4, H, W, generator=g)
    txt = torch.randn(B, 77, ocfg.cross_attention_dim, generator=g)
    unc = torch.randn(B, 77, ocfg.cross_attention_dim, generator=g)
    return lat0, txt, unc


@pytest.mark.parametrize('guidance', [0.0, 3.0])
def test_rect_latent_sampler_matches_the_oracle_and_its_graph_replay(tiny, dev, guidance):
    """2 x 4 x 8 x 16, 4 DDIM steps: rel-L2 < 3e-2 to ``O.ddim_sample`` (test_latent_sampler_matches_the_oracle's bound), run to
    run and graph replay bit for bit; a 16 x 8 call then captures a second graph and replays to the eager bits too"""
    from diffusion_amd.sampling import LatentSampler
    O, ocfg, sd, model = tiny
    smp = LatentSampler(model.unet, model.inference_scheduler)
    smp.graphs.clear()
    lat0, txt, unc = _sampler_inputs(ocfg, 8, 16)
    ref = O.ddim_sample(sd, ocfg, txt, unc, lat0, 4, guidance)
    args = (lat0.to(dev), txt.to(dev), unc.to(dev))
    kw = dict(num_inference_steps=4, guidance_scale=guidance)
    got = smp.sample(*args, **kw)
    assert got.shape == lat0.shape and got.dtype == torch.float32 and got.is_contiguous()
    e = _rel(got.cpu(), ref)
    print(f'sampler 2x4x8x16 guidance {guidance}: rel-L2 to the oracle {e:.3e}')
    record(f'sampler_8x16_g{guidance}', tolerances={'rel_l2': 3e-2}, rel_l2=e)
    assert torch.equal(got, smp.sample(*args, **kw))
    assert e < 3e-2, e
    graphed = smp.sample(*args, graph=True, **kw)
    assert len(smp.graphs) == 1
    assert torch.equal(graphed, got), _rel(graphed, got)
    lat1, txt1, unc1 = _sampler_inputs(ocfg, 16, 8, seed=77)
    args1 = (lat1.to(dev), txt1.to(dev), unc1.to(dev))
    eager1 = smp.sample(*args1, **kw)
    graphed1 = smp.sample(*args1, graph=True, **kw)
    assert len(smp.graphs) == 2
    assert eager1.shape == (2, 4, 16, 8) and torch.equal(graphed1, eager1), _rel(graphed1, eager1)
    assert torch.equal(smp.sample(*args, graph=True, **kw), got)   # the first capture is still there, and still right
    assert len(smp.graphs) == 2
    smp.graphs.clear()


# ---------------------------------------------------------------------------------------------------------------------
# 6: StableDiffusion.generate
# ---------------------------------------------------------------------------------------------------------------------
def test_stable_diffusion_generate_rectangular(tiny_images, dev, monkeypatch):
    monkeypatch.delenv('DA_SAMPLER', raising=False)
    model = tiny_images
    kw = dict(prompt=['a cool doge', 'a hot cat'], num_inference_steps=2, seed=3, progress_bar=False)
    ref = model.generate(sampler='torch', height=64, width=128, **kw)
    hip = model.generate(sampler='hip', height=64, width=128, **kw)
    assert hip.shape == ref.shape == (2, 3, 64, 128)
    assert torch.isfinite(hip).all() and hip.min() >= 0 and hip.max() <= 1
    e = _rel(hip, ref)
    print(f'StableDiffusion.generate 64x128: hip vs torch image rel-L2 {e:.3e}')
    record('generate_64x128', tolerances={'hip_vs_torch_rel_l2': 8e-2}, hip_vs_torch_rel_l2=e)
    assert e < 8e-2, e   # test_stable_diffusion_generate_hip_against_torch's bound
    assert torch.equal(model.generate(sampler='graph', height=64, width=128, **kw), hip)
    tall = model.generate(sampler='hip', height=128, width=64, **kw)
    assert tall.shape == (2, 3, 128, 64) and torch.isfinite(tall).all()
    assert not torch.equal(tall, hip.transpose(2, 3)) and _rel(tall, hip.transpose(2, 3)) > 1e-2
    model.unet._sampler_graphs.clear()


# ---------------------------------------------------------------------------------------------------------------------
# 7: PixelDiffusion
# ---------------------------------------------------------------------------------------------------------------------
def _pixel_cfg():
    from diffusion_amd.models.unet import UNetConfig
    return UNetConfig(in_channels=3, out_channels=3, block_out_channels=(64, 128, 256, 256),
                      attention_head_dim=(1, 2, 4, 4), cross_attention_dim=768)


class _FixedText(torch.nn.Module):
    """Stands in for the text encoder: ``enc(ids)[0]`` is a fixed embedding, so the U-Net step is compared alone."""

    def __init__(self, ctx):
        super().__init__()
        self.ctx = ctx

    def forward(self, ids):
        return (self.ctx[:ids.shape[0]],)


@pytest.mark.parametrize('continuous,prediction_type', [(True, 'epsilon'), (False, 'sample')])
def test_rect_pixel_train_step_vs_oracle(dev, continuous, prediction_type):
    """test_tiny_pixel_train_step_vs_oracle's fp64 route and bounds on 2 x 3 x 8 x 16 pixels"""
    from oracle import unet_oracle as O
    import make_golden_pixel as P
    from diffusion_amd.models.pixel_diffusion import PixelDiffusion
    from diffusion_amd.models.schedulers import DDPMScheduler
    from diffusion_amd.models.unet import UNetHIP
    from diffusion_amd.schedulers.schedulers import ContinuousTimeScheduler
    ocfg = P.tiny_pixel_config()
    sd = O.init_state_dict(ocfg, seed=23)
    unet = UNetHIP(_pixel_cfg(), device='cuda', init=False)
    unet.load_state_dict(sd)
    B, H, W = 2, 8, 16
    g = torch.Generator().manual_seed(5 + continuous)
    x0 = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    ctx = torch.randn(B, 77, 768, generator=g)
    noise = torch.randn(B, 3, H, W, generator=g)
    t = P.T_MAX * torch.rand(B, generator=g) if continuous else torch.randint(0, 1000, (B,), generator=g)
    loss_ref, pred_ref, target_ref, grads_ref = P.pixel_step(sd, ocfg, x0, t, ctx, noise, prediction_type, dtype=torch.float64)
    sched = ContinuousTimeScheduler(t_max=P.T_MAX) if continuous else DDPMScheduler(prediction_type=prediction_type)
    model = PixelDiffusion(unet, _FixedText(ctx.to(dev)), None, sched, continuous_time=continuous,
                           prediction_type=prediction_type)
    batch = {'image': x0.to(dev), 'captions': torch.zeros(B, 77, dtype=torch.int64, device=dev)}
    assert model.unet_input_side(batch) == (H, W)
    unet.zero_grad()
    out = model(batch, timesteps=t.to(dev), noise=noise.to(dev))
    assert out[0].shape == (B, 3, H, W) and out[1].shape == (B, 3, H, W)
    assert _rel(out[1].cpu(), target_ref) < 1e-5
    e = _rel(out[0].cpu(), pred_ref)
    loss = model.loss(out, batch)
    dl = abs(loss.item() - loss_ref.item())
    loss.backward()
    torch.cuda.synchronize()
    got = {k: p.grad.detach().double().cpu() for k, p in unet.named_parameters()}
    grel, worst, vrel = _grad_margins(got, grads_ref)
    case = f'pixel_tiny_8x16_b2_{"cont" if continuous else "disc"}_{prediction_type}'
    print(f'{case}: pred rel-L2 {e:.3e}, |loss - oracle| {dl:.3e}, grad rel-L2 {grel:.3e}, worst matrix cosine '
          f'{worst[1]:.5f} ({worst[0]}), vector grads rel-L2 {vrel:.3e}')
    record(case, tolerances=TOL_TINY, pred_rel_l2=e, loss_abs_delta=dl, grad_rel_l2=grel, worst_matrix_cosine=worst[1],
           worst_matrix=worst[0], vector_grads_rel_l2=vrel)
    assert e < TOL_TINY['pred_rel'], e
    assert dl < TOL_TINY['loss_abs'], (loss.item(), loss_ref.item())
    assert grel < TOL_TINY['grad_rel'], grel
    assert worst[1] >= TOL_TINY['matrix_cos'], worst
    assert vrel < TOL_TINY['vector_rel'], vrel


def test_pixel_diffusion_generate_rectangular(dev):
    from diffusion_amd.models.models import discrete_pixel_diffusion
    torch.manual_seed(5)
    model = discrete_pixel_diffusion(unet_config=_pixel_cfg(), seed=3)
    kw = dict(prompt=['a cool doge'], num_inference_steps=3, guidance_scale=3.0, seed=7, progress_bar=False)
    outs = {s: model.generate(sampler=s, height=8, width=16, **kw) for s in ('torch', 'hip', 'graph')}
    for out in outs.values():
        assert out.shape == (1, 3, 8, 16) and torch.isfinite(out).all() and out.min() >= 0 and out.max() <= 1
    assert torch.equal(outs['graph'], outs['hip'])
    with pytest.raises(ValueError, match='multiples of 8'):
        model.generate(height=8, width=12, **kw)
    model.unet._sampler_graphs.clear()


# ---------------------------------------------------------------------------------------------------------------------
# 8: the VAE walks
# ---------------------------------------------------------------------------------------------------------------------
def test_vae_walks_on_rectangular_images(dev):
    """encoder on 1 x 3 x 32 x 64 (rel-L2 < 2e-2 to the fp32 torch moments: tests/test_vae_hip_gpu.py), decoder on
    1 x 4 x 4 x 8 latents (e_hip <= 1.5 e_bf16 and < 8e-2: tests/test_vae_decoder_hip_gpu.py)"""
    from diffusion_amd.models.vae import AutoencoderKL
    from diffusion_amd.models.vae_hip import VAEDecoderHIP, VAEEncoderHIP
    torch.manual_seed(7)
    vae = AutoencoderKL().to(dev).eval()
    with torch.no_grad():   # non-trivial norm affines (torch default is gamma 1, beta 0)
        for n, p in vae.named_parameters():
            if 'norm' in n:
                p.add_(0.1 * torch.randn_like(p))
    enc, dec = VAEEncoderHIP(vae), VAEDecoderHIP(vae)
    g = torch.Generator().manual_seed(3264)
    x = (torch.rand(1, 3, 32, 64, generator=g) * 2 - 1).to(dev)
    with torch.no_grad():
        ref = vae.quant_conv(vae.encoder(x))
    got = enc.moments(x)
    assert got.shape == ref.shape == (1, 8, 4, 8)
    e_enc = _rel(got, ref)
    z = torch.randn(1, 4, 4, 8, generator=g).to(dev)
    vae_bf16 = copy.deepcopy(vae).to(torch.bfloat16)
    with torch.no_grad():
        dref = vae.decode(z).sample
        low = vae_bf16.decode(z.to(torch.bfloat16)).sample.float()
    dgot = dec.decode(z).sample
    assert dgot.shape == dref.shape == (1, 3, 32, 64) and dgot.dtype == torch.float32 and torch.isfinite(dgot).all()
    e_hip, e_bf16 = _rel(dgot, dref), _rel(low, dref)
    print(f'vae 32x64: encoder rel-L2 {e_enc:.3e}; decoder e_hip {e_hip:.3e}, e_bf16 {e_bf16:.3e}')
    record('vae_rect_32x64', tolerances={'encoder_rel_l2': 2e-2, 'e_hip_over_e_bf16': 1.5, 'e_hip': VAE_CAP},
           encoder_rel_l2=e_enc, e_hip=e_hip, e_bf16=e_bf16)
    assert e_enc < 2e-2, e_enc
    assert e_hip <= 1.5 * e_bf16, (e_hip, e_bf16)
    assert e_hip < VAE_CAP, e_hip


# ---------------------------------------------------------------------------------------------------------------------
# 9: eval
# ---------------------------------------------------------------------------------------------------------------------
def test_trainer_eval_on_a_rectangular_batch(dev):
    import numpy as np
    from diffusion_amd.metrics.clip_score import CLIPScore
    from diffusion_amd.models.composer_shim import MeanSquaredError
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.optim import FusedAdamW
    from diffusion_amd.trainer import Trainer
    clip = CR.tiny_clip(seed=5).to(dev)
    torch.manual_seed(11)
    model = stable_diffusion_2(model_name='tiny', pretrained=False, fsdp=False,
                               val_metrics=[MeanSquaredError(), CLIPScore(model=clip, device=dev)], val_guidance_scales=[3.0])
    assert model.vae_hip is not None and model.vae_dec_hip is not None
    g = torch.Generator().manual_seed(4)
    evalset = [{'image': torch.rand(2, 3, 64, 128, generator=g) * 2 - 1,
                'captions': model.tokenizer(['a red cube', 'a blue ball'], padding='max_length', max_length=77,
                                            truncation=True, return_tensors='pt')['input_ids']}]
    seen = []
    inner = model.eval_forward

    def recording(batch, outputs=None):
        out = inner(batch, outputs)
        seen.append(out)
        return out

    model.eval_forward = recording
    tr = Trainer(model, train_dataloader=None, optimizers=FusedAdamW(lr=1e-3, unet=model.unet), max_duration='1ba',
                 eval_dataloader=evalset, log_every=1000)
    torch.manual_seed(11)
    out = tr.eval()
    assert len(seen) == 1
    pred, target, _, images = seen[0]
    assert pred.shape == target.shape == (2, 4, 8, 16)
    assert images[3.0].shape == (2, 3, 64, 128) and torch.isfinite(images[3.0]).all()
    assert np.isfinite(out['metrics/eval/CLIPScore-scale-3p0'])
    mse = {k: v for k, v in out.items() if 'MeanSquaredError' in k}
    assert 'metrics/eval/MeanSquaredError' in mse and len(mse) >= 2
    assert all(np.isfinite(v) and v > 0 for v in mse.values())
