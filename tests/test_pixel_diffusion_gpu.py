"""The pixel-space model family on the MI355X: the new kernels (float timestep embedding, general noising, C-channel MSE,
quick-GELU) against torch, the 3-channel U-Net train step against the oracle (tiny width live in fp64, full width against
tests/golden/pixel_s32_b1.npz), generation through both factories, and the trainer on a continuous-time pixel model."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
sys.path.insert(0, GOLD)
sys.path.insert(0, HERE)

# the tiny-width bounds of tests/test_unet_parity_gpu.py (<= 2 x the margins measured there)
TOL_TINY = {'pred_rel': 2.3e-2, 'loss_abs': 5.6e-4, 'grad_rel': 4e-2, 'matrix_cos': 0.9957, 'vector_rel': 2.3e-2}
# full width at 32x32, B=1, continuous t (tests/golden/pixel_s32_b1.npz): every bound is 2 x the margin measured on MI355X
# (prediction rel-L2 1.005e-2 . |loss - oracle| 9.2e-6 . per-tensor gradient-norm ratio 0.99764 .. 1.00245 . whole-gradient
# norm ratio 0.99962 . worst slice cosine 0.99884 . rel-L2 over the slices 4.56e-3); the path is deterministic, so the margins
# repeat run to run for a given build
TOL_PIXEL = {'pred_rel': 2e-2, 'loss_abs': 1.9e-5, 'norm_lo': 0.9951, 'norm_hi': 1.0049, 'total_lo': 0.99924,
             'total_hi': 1.00076, 'slice_cos': 0.99768, 'slice_rel': 9.1e-3}


def _record(case, tol, **kv):
    from parity_margins import record
    record(case, tolerances=tol, **kv)


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-20)).item()


def _tiny_cfg():
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


def _pixel_model(unet, ctx, continuous, prediction_type):
    from diffusion_amd.models.pixel_diffusion import PixelDiffusion
    from diffusion_amd.models.schedulers import DDPMScheduler
    from diffusion_amd.schedulers.schedulers import ContinuousTimeScheduler
    sched = ContinuousTimeScheduler(t_max=1.570795) if continuous else DDPMScheduler(prediction_type=prediction_type)
    return PixelDiffusion(unet, _FixedText(ctx), None, sched, continuous_time=continuous, prediction_type=prediction_type)


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_timestep_embed_f32(dev):
    from oracle import unet_oracle as O
    from diffusion_amd import ops
    t = torch.cat([torch.linspace(0, 1.5708, 37), torch.tensor([0.0, 1e-3, 1.570795])])
    for dim in (64, 320):
        out = torch.empty(t.numel(), dim, device=dev, dtype=torch.bfloat16)
        ops.timestep_embed_f32(t.to(dev), out)
        ref = O.timestep_embedding(t, dim)
        assert (out.float().cpu() - ref).abs().max().item() <= 4e-3   # half a bf16 ulp at |x| <= 1
    # integer-valued t: the same bits as the int64 entry point
    ti = torch.tensor([0, 1, 2, 17, 500, 981, 999], dtype=torch.int64)
    a = torch.empty(ti.numel(), 320, device=dev, dtype=torch.bfloat16)
    b = torch.empty_like(a)
    ops.timestep_embed(ti.to(dev), a)
    ops.timestep_embed_f32(ti.float().to(dev), b)
    assert torch.equal(a, b)
    with pytest.raises(RuntimeError):   # odd dim: DA_ERR_SHAPE
        ops.timestep_embed_f32(t.to(dev), torch.empty(t.numel(), 63, device=dev, dtype=torch.bfloat16))


@pytest.mark.parametrize('C', [3, 4])
@pytest.mark.parametrize('continuous', [False, True])
@pytest.mark.parametrize('prediction_type', ['epsilon', 'v_prediction', 'sample'])
def test_add_noise_ex(dev, C, continuous, prediction_type):
    from diffusion_amd import ops
    from diffusion_amd.models.schedulers import DDPMScheduler
    g = torch.Generator().manual_seed(C + 7 * continuous)
    B, S = 3, 12
    x0, eps = torch.randn(B, C, S, S, generator=g), torch.randn(B, C, S, S, generator=g)
    sched = DDPMScheduler()
    sa, sb = sched.device_tables(dev)
    if continuous:
        t = 1.570795 * torch.rand(B, generator=g)
        c, s = torch.cos(t).view(-1, 1, 1, 1), torch.sin(t).view(-1, 1, 1, 1)
        xt_ref, v_ref = c * x0 + s * eps, -s * x0 + c * eps
    else:
        t = torch.randint(0, 1000, (B,), generator=g)
        xt_ref, v_ref = sched.add_noise(x0, eps, t), sched.get_velocity(x0, eps, t)
    tg_ref = {'epsilon': eps, 'v_prediction': v_ref, 'sample': x0}[prediction_type]
    xt = torch.full((B * S * S, 8), 7.0, device=dev, dtype=torch.bfloat16)
    tg = torch.full((B * S * S, 8), 7.0, device=dev, dtype=torch.float32)
    ops.add_noise_ex(x0.to(dev), eps.to(dev), t.to(dev), xt, tg, prediction_type, sa, sb)
    xt4, tg4 = xt.view(B, S, S, 8).cpu(), tg.view(B, S, S, 8).cpu()
    assert torch.all(xt4[..., C:] == 0) and torch.all(tg4[..., C:] == 0)
    got_xt, got_tg = xt4[..., :C].permute(0, 3, 1, 2).float(), tg4[..., :C].permute(0, 3, 1, 2)
    assert torch.allclose(got_xt, xt_ref, rtol=8e-3, atol=8e-3)       # bf16 rounding of x_t
    assert torch.allclose(got_tg, tg_ref, rtol=1e-5, atol=2e-6)
    if C == 4 and not continuous and prediction_type != 'sample':
        xt_old, tg_old = torch.empty_like(xt), torch.empty_like(tg)
        ops.add_noise(x0.to(dev), eps.to(dev), t.to(dev), sa, sb, xt_old, tg_old, prediction_type == 'v_prediction')
        assert torch.equal(xt, xt_old) and torch.equal(tg, tg_old)


def test_add_noise_ex_rejects(dev):
    from diffusion_amd import ops
    x = torch.zeros(1, 9, 8, 8, device=dev)
    buf8 = torch.zeros(64, 8, device=dev, dtype=torch.bfloat16)
    tg8 = torch.zeros(64, 8, device=dev)
    with pytest.raises(ValueError):   # 9 channels
        ops.add_noise_ex(x, x, torch.zeros(1, device=dev), buf8, tg8)
    x = torch.zeros(1, 3, 8, 8, device=dev)
    with pytest.raises(ValueError):   # discrete t without tables
        ops.add_noise_ex(x, x, torch.zeros(1, device=dev, dtype=torch.int64), buf8, tg8)
    with pytest.raises(ValueError):   # host tensors
        ops.add_noise_ex(x.cpu(), x.cpu(), torch.zeros(1), buf8, tg8)


def test_mse_loss_c(dev):
    from diffusion_amd import ops
    g = torch.Generator().manual_seed(3)
    C, npix = 3, 2 * 24 * 24
    pred = torch.randn(npix, 8, generator=g)
    target = torch.randn(npix, 8, generator=g)   # pad lanes hold garbage on purpose: they must not count
    scratch = torch.empty(4096, device=dev)
    dpred = torch.full((npix, 8), 5.0, device=dev, dtype=torch.bfloat16)
    loss = torch.zeros(1, device=dev)
    coef = 2.0 * 0.5 / (C * npix)
    ops.mse_loss_c(pred.to(dev), target.to(dev), dpred, loss, scratch, npix, C, coef, 1.0, 0)
    ref = torch.nn.functional.mse_loss(pred[:, :C].double(), target[:, :C].double()).item()
    assert abs(loss.item() - ref) < 1e-5 * ref
    d = dpred.cpu()
    assert torch.all(d[:, C:] == 0)
    assert torch.allclose(d[:, :C].float(), (coef * (pred[:, :C] - target[:, :C])), rtol=8e-3, atol=1e-9)
    # accumulate + weight
    ops.mse_loss_c(pred.to(dev), target.to(dev), dpred, loss, scratch, npix, C, coef, 0.25, 1)
    assert abs(loss.item() - 1.25 * ref) < 1e-5 * ref
    p, q = pred.to(dev), target.to(dev)
    for bad_c in (0, 9):   # the C ABI itself answers DA_ERR_SHAPE
        with pytest.raises(RuntimeError):
            ops._lib.call('da_mse_loss_c', p.data_ptr(), q.data_ptr(), dpred.data_ptr(), loss.data_ptr(),
                          scratch.data_ptr(), npix, bad_c, 1.0, 1.0, 0, ops._stream())


def test_quick_gelu_and_clip_l_text_encoder(dev):
    from diffusion_amd import ops
    from diffusion_amd.models.text import build_clip_text_encoder
    from diffusion_amd.models.text_hip import TextEncoderHIP
    x = (torch.randn(300, 128, generator=torch.Generator().manual_seed(1)) * 4).to(dev, torch.bfloat16)
    y = torch.empty_like(x)
    ops.quick_gelu_fwd(x, y)
    xf = x.float()
    assert torch.allclose(y.float(), xf * torch.sigmoid(1.702 * xf), rtol=8e-3, atol=1e-6)
    ops.quick_gelu_fwd(x, x)   # in place, as the encoder calls it
    assert torch.equal(x, y)
    torch.manual_seed(14)
    te = build_clip_text_encoder(None, num_hidden_layers=2).to(dev).eval()
    assert te.config.hidden_act == 'quick_gelu' and te.config.hidden_size == 768
    with torch.no_grad():
        for n, p in te.named_parameters():
            if 'norm' in n or n.endswith('bias'):
                p.add_(0.1 * torch.randn_like(p))
    hip = TextEncoderHIP(te)
    ids = torch.randint(0, 49408, (3, 77), generator=torch.Generator().manual_seed(3)).to(dev)
    with torch.no_grad():
        ref = te(ids)[0]
    got = hip(ids)[0]
    assert got.shape == ref.shape == (3, 77, 768)
    assert _rel(got, ref) < 2e-2, _rel(got, ref)


# ---------------------------------------------------------------------------------------------------------------------
# the U-Net train step against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tiny(dev):
    from oracle import unet_oracle as O
    import make_golden_pixel as P
    from diffusion_amd.models.unet import UNetHIP
    ocfg = P.tiny_pixel_config()
    sd = O.init_state_dict(ocfg, seed=23)
    unet = UNetHIP(_tiny_cfg(), device='cuda', init=False)
    unet.load_state_dict(sd)
    return O, P, ocfg, sd, unet


@pytest.mark.parametrize('continuous,prediction_type', [(True, 'epsilon'), (False, 'sample')])
def test_tiny_pixel_train_step_vs_oracle(tiny, dev, continuous, prediction_type):
    O, P, ocfg, sd, unet = tiny
    B, S = 2, 16
    x0, ctx, noise, t = P.inputs(B, S, 768, seed=5 + continuous, continuous=continuous)
    loss_ref, pred_ref, target_ref, grads_ref = P.pixel_step(sd, ocfg, x0, t, ctx, noise, prediction_type,
                                                             dtype=torch.float64)
    model = _pixel_model(unet, ctx.to(dev), continuous, prediction_type)
    batch = {'image': x0.to(dev), 'captions': torch.zeros(B, 77, dtype=torch.int64, device=dev)}
    unet.zero_grad()
    out = model(batch, timesteps=t.to(dev), noise=noise.to(dev))
    assert out[0].shape == (B, 3, S, S) and out[1].shape == (B, 3, S, S)
    assert out[2].dtype == t.dtype
    assert _rel(out[1].cpu(), target_ref) < 1e-5
    e = _rel(out[0].cpu(), pred_ref)
    loss = model.loss(out, batch)
    dl = abs(loss.item() - loss_ref.item())
    loss.backward()
    torch.cuda.synchronize()
    got = {k: p.grad.detach().double().cpu() for k, p in unet.named_parameters()}
    grel = math.sqrt(sum(((got[k] - g)**2).sum().item() for k, g in grads_ref.items()) /
                     sum((g**2).sum().item() for g in grads_ref.values()))
    worst = (None, 1.0)
    for k, g in grads_ref.items():
        if g.dim() >= 2 and g.norm() > 0:
            c = torch.nn.functional.cosine_similarity(got[k].flatten(), g.flatten(), dim=0).item()
            if c < worst[1]:
                worst = (k, c)
    vk = [k for k, g in grads_ref.items() if g.dim() == 1]
    vrel = math.sqrt(sum(((got[k] - grads_ref[k])**2).sum().item() for k in vk) /
                     sum((grads_ref[k]**2).sum().item() for k in vk))
    _record(f'pixel_tiny_s16_b2_{"cont" if continuous else "disc"}_{prediction_type}', TOL_TINY, pred_rel_l2=e,
            loss_abs_delta=dl, grad_rel_l2=grel, worst_matrix_cosine=worst[1], worst_matrix=worst[0],
            vector_grads_rel_l2=vrel)
    assert e < TOL_TINY['pred_rel'], e
    assert dl < TOL_TINY['loss_abs'], (loss.item(), loss_ref.item())
    assert grel < TOL_TINY['grad_rel'], grel
    assert worst[1] >= TOL_TINY['matrix_cos'], worst
    assert vrel < TOL_TINY['vector_rel'], vrel


def test_padded_conv_out_rows_stay_zero_under_adamw(tiny, dev):
    O, P, ocfg, sd, _ = tiny
    from diffusion_amd.models.unet import UNetHIP
    from diffusion_amd.optim import FusedAdamW
    unet = UNetHIP(_tiny_cfg(), device='cuda', init=False)
    unet.load_state_dict(sd)
    opt = FusedAdamW(lr=1e-2, weight_decay=0.01, unet=unet)
    x0, ctx, noise, t = P.inputs(2, 16, 768, seed=9)
    model = _pixel_model(unet, ctx.to(dev), True, 'v_prediction')
    batch = {'image': x0.to(dev), 'captions': torch.zeros(2, 77, dtype=torch.int64, device=dev)}
    w = unet.fp.storages['conv_out.weight']
    b = unet.fp.storages['conv_out.bias']
    ci = unet.fp.storages['conv_in.weight']
    for step in range(2):
        unet.zero_grad()
        loss = model.loss(model(batch, timesteps=t.to(dev), noise=noise.to(dev)), batch)
        loss.backward()
        assert torch.all(unet.grad[w.off:w.off + w.numel].view(w.shape)[3:] == 0)
        assert torch.all(unet.grad[b.off:b.off + b.numel][3:] == 0)
        opt.step()
    torch.cuda.synchronize()
    master = unet.master
    assert torch.all(master[w.off:w.off + w.numel].view(w.shape)[3:] == 0)
    assert torch.all(master[b.off:b.off + b.numel][3:] == 0)
    assert torch.all(master[ci.off:ci.off + ci.numel].view(ci.shape)[..., 3:] == 0)   # conv_in pad input channels
    assert torch.all(unet.shadow[w.off:w.off + w.numel].view(w.shape)[3:] == 0)
    assert master[w.off:w.off + w.numel].view(w.shape)[:3].abs().sum() > 0


def test_full_width_pixel_train_step_vs_fixture(dev):
    from oracle import unet_oracle as O
    import make_golden_full as G
    import make_golden_pixel as P
    from diffusion_amd.models.unet import UNetConfig, UNetHIP
    fx = np.load(os.path.join(GOLD, P.FNAME))
    ocfg = P.pixel_config()
    sd = O.init_state_dict(ocfg, seed=P.WSEED)
    x0, ctx, noise, t = P.inputs(P.B, P.S, 768, P.ISEED)
    if not np.allclose(G.checksum(sd, x0, ctx, noise), fx['checksum'], rtol=0, atol=1e-6):
        pytest.fail('seeded weight / input streams differ from the fixture: regenerate it with make_golden_pixel.py')
    unet = UNetHIP(UNetConfig.pixel(), device='cuda', init=False)
    unet.load_state_dict(sd)
    assert unet.num_params == O.param_count(ocfg)
    model = _pixel_model(unet, ctx.to(dev), True, 'epsilon')
    batch = {'image': x0.to(dev), 'captions': torch.zeros(P.B, 77, dtype=torch.int64, device=dev)}
    unet.zero_grad()
    out = model(batch, timesteps=torch.from_numpy(fx['t']).to(dev), noise=noise.to(dev))
    e = _rel(out[0].cpu(), torch.from_numpy(fx['pred']))
    assert _rel(out[1].cpu(), torch.from_numpy(fx['target'])) < 1e-5
    loss = model.loss(out, batch)
    dl = abs(loss.item() - float(fx['loss']))
    loss.backward()
    torch.cuda.synchronize()
    params = dict(unet.named_parameters())
    keys = [k for k, _ in O.param_manifest(ocfg)]
    ref_norms = fx['grad_norms']
    got_norms = np.array([float(params[k].grad.detach().double().norm()) for k in keys])
    big = ref_norms > 1e-3 * ref_norms.max()
    ratio = got_norms[big] / ref_norms[big]
    tot = math.sqrt((got_norms**2).sum() / (ref_norms**2).sum())
    num = den = 0.0
    worst_cos = (None, 1.0)
    for k, rows in P.SLICES:
        r = torch.from_numpy(fx['grad.' + k])
        g = params[k].grad.detach().float().cpu()
        g = g if rows is None else g[:rows]
        assert g.shape == r.shape, k
        num += ((g - r)**2).sum().item()
        den += (r**2).sum().item()
        if r.dim() >= 2 and r.norm() > 0:
            c = torch.nn.functional.cosine_similarity(g.flatten(), r.flatten(), dim=0).item()
            if c < worst_cos[1]:
                worst_cos = (k, c)
    srel = math.sqrt(num / den)
    _record('pixel_full_s32_b1_cont_eps', TOL_PIXEL, pred_rel_l2=e, loss_abs_delta=dl, norm_ratio_min=float(ratio.min()),
            norm_ratio_max=float(ratio.max()), total_norm_ratio=tot, worst_slice_cosine=worst_cos[1],
            worst_slice_tensor=worst_cos[0], slices_rel_l2=srel)
    print(f'pixel full-width margins: pred {e:.3e} loss {dl:.3e} norms {ratio.min():.5f}..{ratio.max():.5f} total {tot:.6f} '
          f'slice cos {worst_cos[1]:.5f} ({worst_cos[0]}) slice rel {srel:.3e}')
    assert e < TOL_PIXEL['pred_rel'], e
    assert dl < TOL_PIXEL['loss_abs'], (loss.item(), float(fx['loss']))
    assert np.all((ratio > TOL_PIXEL['norm_lo']) & (ratio < TOL_PIXEL['norm_hi'])), (ratio.min(), ratio.max())
    assert TOL_PIXEL['total_lo'] < tot < TOL_PIXEL['total_hi'], tot
    assert worst_cos[1] >= TOL_PIXEL['slice_cos'], worst_cos
    assert srel < TOL_PIXEL['slice_rel'], srel
    del unet, model
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# factories, generation, trainer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def factories(dev):
    from diffusion_amd.models.models import continuous_pixel_diffusion, discrete_pixel_diffusion
    return {'discrete': discrete_pixel_diffusion(unet_config=_tiny_cfg(), seed=3),
            'continuous': continuous_pixel_diffusion(unet_config=_tiny_cfg(), seed=3)}


@pytest.mark.parametrize('kind', ['discrete', 'continuous'])
@pytest.mark.parametrize('guidance_scale', [0.0, 3.0])
@pytest.mark.parametrize('negative_prompt', [None, 'so cool'])
def test_model_generate(factories, kind, guidance_scale, negative_prompt):
    model = factories[kind]
    output = model.generate(prompt='a cool doge', negative_prompt=negative_prompt, num_inference_steps=1,
                            num_images_per_prompt=1, height=8, width=8, guidance_scale=guidance_scale,
                            progress_bar=False)
    assert output.shape == (1, 3, 8, 8)
    assert torch.isfinite(output).all() and output.min() >= 0 and output.max() <= 1


@pytest.mark.parametrize('kind', ['discrete', 'continuous'])
def test_factory_model_forward_and_protocol(factories, dev, kind):
    model = factories[kind]
    assert model.unet is model.model and model.text_hip is not None
    assert all(not p.requires_grad for p in model.text_encoder.parameters())
    B = 2
    batch = {'image': torch.rand(B, 3, 16, 16, device=dev) * 2 - 1,
             'captions': torch.randint(0, 1000, (B, 77), device=dev)}
    out = model(batch)
    assert out[0].shape == out[1].shape == (B, 3, 16, 16)
    assert out[2].dtype == (torch.float32 if kind == 'continuous' else torch.int64)
    if kind == 'continuous':
        assert float(out[2].min()) >= 0 and float(out[2].max()) < 1.570795
    model.unet.zero_grad()
    loss = model.loss(out, batch)
    loss.backward()
    assert torch.isfinite(loss) and float(model.unet.grad.abs().sum()) > 0
    mets = model.get_metrics(is_train=True)
    assert list(mets) == ['MeanSquaredError']
    m = mets['MeanSquaredError']
    m.reset()
    model.update_metric(batch, out, m)
    assert abs(m.compute().item() - loss.item()) < 1e-4 * max(1.0, loss.item())
    # eval: seeded timesteps (val_seed), global-RNG noise
    e1 = model.eval_forward(batch)
    e2 = model.eval_forward(batch)
    assert torch.equal(e1[2], e2[2]) and e1[0].shape == (B, 3, 16, 16)


def test_continuous_ode_generate_matches_oracle_loop(factories, dev):
    from oracle import unet_oracle as O
    import make_golden_pixel as P
    from diffusion_amd.schedulers.schedulers import ContinuousTimeScheduler
    model = factories['continuous']
    sd = O.init_state_dict(P.tiny_pixel_config(), seed=29)
    model.unet.load_state_dict(sd)
    # v-prediction: the Euler ODE step is then x - dt * v, so the comparison sees the U-Net's error as it is.  (With eps from
    # t = 1.56 the first step multiplies x - eps by tan(1.56) * dt / 2 = 72 and the [0, 1] clamp turns the bf16 noise of
    # the prediction into flipped saturated pixels: 2.5e-2 image rel-L2 at 1.3e-2 prediction rel-L2.)
    sched = model.inference_scheduler
    old = sched.use_ode, sched.prediction_type
    sched.use_ode, sched.prediction_type = True, 'v_prediction'
    ctx = torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(2))
    try:
        got = model.generate(prompt_embeds=ctx.to(dev), height=16, width=16, num_inference_steps=2, guidance_scale=0.0,
                             seed=11, progress_bar=False).cpu()
    finally:
        sched.use_ode, sched.prediction_type = old
    # the same loop with the oracle U-Net in fp64 through the restated scheduler
    x = torch.randn((1, 3, 16, 16), device=dev, generator=torch.Generator(device=dev).manual_seed(11)).cpu().double()
    ref_sched = ContinuousTimeScheduler(t_max=1.56, use_ode=True, prediction_type='v_prediction')
    ref_sched.set_timesteps(2)
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        for t in ref_sched.timesteps:
            out = O.unet_forward(sd64, P.tiny_pixel_config(), x, torch.tensor([float(t)], dtype=torch.float32),
                                 ctx.double())
            x = ref_sched.step(out, t, x)['prev_sample']
    ref = (x / 2 + 0.5).clamp(0, 1)
    e = _rel(got, ref)
    _record('pixel_tiny_generate_ode_2step', TOL_TINY, image_rel_l2=e)
    assert e < TOL_TINY['pred_rel'], e


def test_trainer_on_continuous_pixel_model_is_deterministic(dev):
    from diffusion_amd.models.models import continuous_pixel_diffusion
    from diffusion_amd.optim import FusedAdamW
    from diffusion_amd.trainer import Trainer

    def run(use_graphs):
        torch.manual_seed(31)   # the random-init text encoder and every draw of the steps come from the global generator
        model = continuous_pixel_diffusion(unet_config=_tiny_cfg(), seed=4)
        opt = FusedAdamW(lr=1e-3, weight_decay=0.01, unet=model.unet)
        tr = Trainer(model, train_dataloader=None, optimizers=opt, max_duration='3ba',
                     device_train_microbatch_size='auto', use_graphs=use_graphs)
        g = torch.Generator().manual_seed(8)
        losses, grads = [], []
        for _ in range(3):
            batch = {'image': (torch.rand(4, 3, 16, 16, generator=g) * 2 - 1).to(dev),
                     'captions': torch.randint(0, 1000, (4, 77), generator=g).to(dev)}
            losses.append(tr.train_batch(batch))
            grads.append(model.unet.grad.clone())
        torch.cuda.synchronize()
        return tr, losses, grads, model.unet.master.clone()

    ta, la, ga, wa = run(False)
    tb, lb, gb, wb = run(True)   # graph replay asked for: the pixel model declines capture and runs eagerly
    assert list(ta._auto_mb) == [(4, 16)] and list(tb._auto_mb) == [(4, 16)]   # the pixel side, not side // 8
    assert tb._graph_cache is not None and not tb._graph_cache.graphs
    for step in range(3):
        assert torch.isfinite(la[step]) and torch.equal(la[step], lb[step]), step
        assert torch.isfinite(ga[step]).all() and torch.equal(ga[step], gb[step]), step
    assert torch.equal(wa, wb)


def test_hydra_config_node_builds_a_continuous_pixel_model(dev):
    from diffusion_amd import hydra_lite as h
    node = {'_target_': 'diffusion.models.models.continuous_pixel_diffusion', 'prediction_type': 'v_prediction',
            'use_ode': True,
            'unet_config': {'_target_': 'diffusion_amd.models.unet.UNetConfig', 'in_channels': 3, 'out_channels': 3,
                            'block_out_channels': [64, 128, 256, 256], 'attention_head_dim': [1, 2, 4, 4],
                            'cross_attention_dim': 768}}
    model = h.instantiate(node)
    assert type(model).__name__ == 'PixelDiffusion' and model.continuous_time
    assert model.inference_scheduler.use_ode and model.inference_scheduler.t_max == 1.56
    assert model.scheduler.t_max == 1.570795 and model.prediction_type == 'v_prediction'
    batch = {'image': torch.rand(1, 3, 16, 16, device=dev), 'captions': torch.randint(0, 1000, (1, 77), device=dev)}
    out = model(batch)
    loss = model.loss(out, batch)
    loss.backward()
    assert torch.isfinite(loss)
