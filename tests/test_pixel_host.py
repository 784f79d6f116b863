"""CPU tests of the pixel-space model family: the continuous-time scheduler against its closed forms, the DDIM x0
('sample') branch, the reference names resolving through hydra_lite with the reference signatures, the flat layout of the
pixel U-Net against the oracle manifest, and the factories refusing to run without a GPU."""
import inspect
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sched(**kw):
    from diffusion_amd.schedulers.schedulers import ContinuousTimeScheduler
    return ContinuousTimeScheduler(**kw)


def test_tangent_schedule_closed_form():
    from diffusion_amd.schedulers.schedulers import tangent_schedule
    for t in (0.0, 0.3, 1.2):
        beta, s, c = tangent_schedule(t)
        assert math.isclose(beta, 2 * math.tan(t)) and math.isclose(s, math.sin(t)) and math.isclose(c, math.cos(t))
        tb, ts, tc = tangent_schedule(torch.tensor([t], dtype=torch.float64))
        assert math.isclose(tb.item(), 2 * math.tan(t)) and math.isclose(ts.item(), math.sin(t))
        assert math.isclose(tc.item(), math.cos(t))


def test_continuous_add_noise_and_velocity():
    s = _sched()
    x = torch.tensor([[1.0, -2.0], [0.5, 3.0]], dtype=torch.float64)
    n = torch.tensor([[0.25, 1.5], [-1.0, 0.75]], dtype=torch.float64)
    t = torch.tensor([0.4, 1.1], dtype=torch.float64)
    xt = s.add_noise(x, n, t)
    v = s.get_velocity(x, n, t)
    for b in range(2):
        c, sn = math.cos(t[b].item()), math.sin(t[b].item())
        for j in range(2):
            assert math.isclose(xt[b, j].item(), c * x[b, j].item() + sn * n[b, j].item(), rel_tol=1e-12)
            assert math.isclose(v[b, j].item(), -sn * x[b, j].item() + c * n[b, j].item(), rel_tol=1e-12)
    # 4-D broadcasting over [B, C, H, W]
    x4, n4 = torch.ones(2, 3, 2, 2), torch.zeros(2, 3, 2, 2)
    assert torch.allclose(s.add_noise(x4, n4, torch.tensor([0.0, math.pi / 3]))[1], torch.full((3, 2, 2), 0.5))


def test_continuous_timesteps_and_defaults():
    s = _sched()
    assert s.t_max == 1.57 and s.num_inference_timesteps == 50 and s.prediction_type == 'epsilon'
    assert s.use_ode is False and s.init_noise_sigma == 1.0 and len(s) == 50
    assert s.timesteps.dtype == np.float64 and s.timesteps.shape == (50,) and s.timesteps[0] == 1.57
    s = _sched(t_max=1.5)
    s.set_timesteps(3)
    assert np.allclose(s.timesteps, [1.5, 1.0, 0.5]) and len(s) == 3
    x = torch.randn(2, 3, 4, 4)
    assert s.scale_model_input(x, 1.0) is x
    assert s.step(torch.randn_like(x), 0, x)['prev_sample'] is x   # t == 0 returns the input unchanged


@pytest.mark.parametrize('use_ode', [True, False])
@pytest.mark.parametrize('prediction_type', ['epsilon', 'v_prediction', 'sample'])
def test_continuous_step_closed_form(use_ode, prediction_type):
    s = _sched(t_max=1.5, prediction_type=prediction_type, use_ode=use_ode)
    s.set_timesteps(10)
    dt = 0.15
    t = 1.2
    x = torch.tensor([0.8, -0.4, 1.3], dtype=torch.float64)
    out = torch.tensor([0.3, 0.9, -0.2], dtype=torch.float64)
    torch.manual_seed(123)
    z = torch.randn_like(x)          # the SDE's noise draw, repeated below from the same global-generator state
    torch.manual_seed(123)
    got = s.step(out, t, x)['prev_sample']
    beta, sn, c = 2 * math.tan(t), math.sin(t), math.cos(t)
    for i in range(3):
        xi, oi = x[i].item(), out[i].item()
        x0 = {'sample': oi, 'epsilon': (xi - sn * oi) / c, 'v_prediction': c * xi - sn * oi}[prediction_type]
        score = -(xi - c * x0) / sn**2
        if use_ode:
            want = xi + 0.5 * (xi + score) * beta * dt
        else:
            want = xi + (0.5 * xi + score) * beta * dt + math.sqrt(beta * dt) * z[i].item()
        assert math.isclose(got[i].item(), want, rel_tol=1e-10, abs_tol=1e-12), (i, got[i].item(), want)


def test_continuous_step_rejects_unknown_prediction_type():
    s = _sched(prediction_type='noise')
    with pytest.raises(ValueError):
        s.step(torch.zeros(2), 1.0, torch.zeros(2))


def test_ddim_sample_branch_and_unchanged_eps_v():
    from diffusion_amd.models.schedulers import DDIMScheduler, DDPMScheduler
    s = DDPMScheduler()
    g = torch.Generator().manual_seed(0)
    x, n = torch.randn(3, 3, 8, 8, generator=g), torch.randn(3, 3, 8, 8, generator=g)
    d = DDIMScheduler(prediction_type='sample')
    d.set_timesteps(50)
    t0 = int(d.timesteps[0])
    xt = s.add_noise(x, n, torch.full((3,), t0))
    # with the true x0 as model output, the step lands on the less-noisy interpolation of the same (x0, eps)
    prev = d.step(x, t0, xt)['prev_sample']
    assert torch.allclose(prev, s.add_noise(x, n, torch.full((3,), t0 - 20)), atol=1e-4)
    # eps and v: the formulas of the existing branches, unchanged bit for bit
    ac_t, ac_p = s.alphas_cumprod[t0], s.alphas_cumprod[t0 - 20]
    out = torch.randn(3, 3, 8, 8, generator=g)
    for pt in ('epsilon', 'v_prediction'):
        d = DDIMScheduler(prediction_type=pt)
        d.set_timesteps(50)
        if pt == 'v_prediction':
            x0 = ac_t.sqrt() * xt - (1 - ac_t).sqrt() * out
            eps = ac_t.sqrt() * out + (1 - ac_t).sqrt() * xt
        else:
            eps = out
            x0 = (xt - (1 - ac_t).sqrt() * eps) / ac_t.sqrt()
        assert torch.equal(d.step(out, t0, xt)['prev_sample'], ac_p.sqrt() * x0 + (1 - ac_p).sqrt() * eps)


def test_reference_names_resolve_with_reference_signatures():
    from diffusion_amd import hydra_lite as h
    disc = h.resolve_target('diffusion.models.models.discrete_pixel_diffusion')
    cont = h.resolve_target('diffusion.models.models.continuous_pixel_diffusion')
    cts = h.resolve_target('diffusion.schedulers.schedulers.ContinuousTimeScheduler')
    assert disc.__module__ == cont.__module__ == 'diffusion_amd.models.models'
    assert cts.__module__ == 'diffusion_amd.schedulers.schedulers'
    assert h.resolve_target('diffusion.models.pixel_diffusion.PixelDiffusion').__name__ == 'PixelDiffusion'

    def head(fn, n):
        return [(p.name, p.default) for p in list(inspect.signature(fn).parameters.values())[:n]]

    # reference diffusion/models/models.py:115 and :175-179
    assert head(disc, 2) == [('clip_model_name', 'openai/clip-vit-large-patch14'), ('prediction_type', 'epsilon')]
    assert head(cont, 5) == [('clip_model_name', 'openai/clip-vit-large-patch14'), ('prediction_type', 'epsilon'),
                             ('use_ode', False), ('train_t_max', 1.570795), ('inference_t_max', 1.56)]
    # reference diffusion/schedulers/schedulers.py:43-48
    assert head(cts, 5) == [('t_max', 1.57), ('num_inference_timesteps', 50), ('prediction_type', 'epsilon'),
                            ('use_ode', False), ('schedule_function', h.resolve_target(
                                'diffusion.schedulers.schedulers.tangent_schedule'))]
    # reference diffusion/models/pixel_diffusion.py:38-50
    from diffusion_amd.models import PixelDiffusion
    assert head(PixelDiffusion.__init__, 13)[1:] == [
        ('model', inspect.Parameter.empty), ('text_encoder', inspect.Parameter.empty),
        ('tokenizer', inspect.Parameter.empty), ('scheduler', inspect.Parameter.empty), ('inference_scheduler', None),
        ('continuous_time', False), ('input_key', 'image'), ('conditioning_key', 'captions'),
        ('prediction_type', 'epsilon'), ('train_metrics', None), ('val_metrics', None), ('val_seed', 1138)]
    sched = h.instantiate({'_target_': 'diffusion.schedulers.schedulers.ContinuousTimeScheduler', 't_max': 1.56,
                           'use_ode': True, 'prediction_type': 'v_prediction'})
    assert isinstance(sched, cts) and sched.use_ode and sched.timesteps[0] == 1.56


def test_models_package_exports_the_reference_names():
    import diffusion_amd.models as m
    assert sorted(m.__all__) == sorted(['continuous_pixel_diffusion', 'discrete_pixel_diffusion', 'PixelDiffusion',
                                        'stable_diffusion_2', 'StableDiffusion'])
    for name in m.__all__:
        assert callable(getattr(m, name))


def test_pixel_config_and_validation():
    from diffusion_amd.models.unet import UNetConfig
    cfg = UNetConfig.pixel()
    assert (cfg.in_channels, cfg.out_channels, cfg.cross_attention_dim) == (3, 3, 768)
    assert cfg.block_out_channels == (320, 640, 1280, 1280) and cfg.attention_head_dim == (5, 10, 20, 20)
    cfg.validate()
    for c in (1, 8):
        UNetConfig(in_channels=c, out_channels=c).validate()
    for bad in (0, 9):
        with pytest.raises(ValueError):
            UNetConfig(in_channels=bad).validate()
        with pytest.raises(ValueError):
            UNetConfig(out_channels=bad).validate()


def test_flat_layout_covers_pixel_manifest():
    from oracle import unet_oracle as O
    from diffusion_amd.models.unet import UNetConfig, build_layout
    # full width: key set and every logical shape (shapes through meta tensors: nothing is materialised)
    fp, *_ = build_layout(UNetConfig.pixel())
    man = dict(O.param_manifest(O.UNetConfig(in_channels=3, out_channels=3, cross_attention_dim=768)))
    assert sorted(k for k, _, _ in fp.views) == sorted(man)
    for key, sname, fn in fp.views:
        st = fp.storages[sname]
        assert tuple(fn(torch.empty(st.shape, device='meta')).shape) == tuple(man[key]), key
    assert man['conv_in.weight'] == (320, 3, 3, 3) and man['conv_out.weight'] == (3, 320, 3, 3)
    # tiny width: views are disjoint and cover exactly the manifest's parameter count (pad channels stay outside)
    ocfg = O.UNetConfig(in_channels=3, out_channels=3, block_out_channels=(64, 128, 256, 256),
                        attention_head_dim=(1, 2, 4, 4), cross_attention_dim=768)
    cfg = UNetConfig(in_channels=3, out_channels=3, block_out_channels=(64, 128, 256, 256),
                     attention_head_dim=(1, 2, 4, 4), cross_attention_dim=768)
    fp, *_ = build_layout(cfg)
    flat = torch.arange(fp.total, dtype=torch.float64)
    seen = torch.zeros(fp.total, dtype=torch.int32)
    man = dict(O.param_manifest(ocfg))
    for key, sname, fn in fp.views:
        st = fp.storages[sname]
        v = fn(flat[st.off:st.off + st.numel].view(st.shape))
        assert tuple(v.shape) == tuple(man[key]), key
        seen[v.reshape(-1).long()] += 1
    assert int(seen.max()) == 1 and int(seen.sum()) == O.param_count(ocfg)


def test_clip_text_config_embedded():
    from diffusion_amd.models.text import CLIP_L14_TEXT
    want = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                hidden_act='quick_gelu', layer_norm_eps=1e-5, max_position_embeddings=77, vocab_size=49408)
    assert {k: CLIP_L14_TEXT[k] for k in want} == want


def test_pixel_factories_need_a_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from diffusion_amd.models.models import continuous_pixel_diffusion, discrete_pixel_diffusion
    with pytest.raises(RuntimeError):
        discrete_pixel_diffusion()
    with pytest.raises(RuntimeError):
        continuous_pixel_diffusion(use_ode=True)
    from diffusion_amd import ops
    a = torch.zeros(8, 8, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.quick_gelu_fwd(a, a)   # host tensors are rejected before any launch
    with pytest.raises(ValueError):
        ops.timestep_embed_f32(torch.zeros(2), torch.zeros(2, 8, dtype=torch.bfloat16))
