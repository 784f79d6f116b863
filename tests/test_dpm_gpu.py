"""GPU tests of the second-order multistep sampler (DPM-Solver++ 2M) on the HIP path: ``da_sampler_step_ms`` against float64,
its argument checks, ``LatentSampler`` with a ``DPMSolverMultistepScheduler`` (eager and graph replay) against the
``'torch'`` route of the same scheduler, and ``generate(inference_scheduler=...)`` of both discrete models.

Bound of the kernel test, elementwise on |got - ref| with u = 2^-24:
    8u (|kx x| + |k0| (|ax x| + |am| M) + |k1 hist|)        M = |pu| + g (|pt| + |pu|) with guidance, |p| without
and on the history, |hist - x0| <= 4u (|ax x| + |am| M).  They cover the kernel's fp32 roundings in its documented order
(guidance, x0 = ax x + am m, v = kx x + k0 x0, + k1 hist), the coefficients rounded to fp32 and an FMA contraction either
way.  The reference is the same expression in float64 with the float64 coefficients of ``step_coefficients_ms``, which
tests/test_dpm_host.py ties to the scheduler's ``step()`` and to the published update.

Measured on an MI355X: the worst kernel error is 0.45 of its bound and the history's 0.76 of its own over the 336 cases; the
'hip' route's distance to the 'torch' route is at most 2.02 times DDIM's on the same inputs (4 allowed)."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PAD = 1e30
TYPES = ('epsilon', 'v_prediction', 'sample')


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-20)).item()


# ---------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------
def _table_rows():
    """(first-order rows, second-order rows) of real 4-, 20- and 50-step tables, every prediction type."""
    from diffusion_amd.models.schedulers import DPMSolverMultistepScheduler
    first, second = [], []
    for ptype, n in itertools.product(TYPES, (4, 20, 50)):
        sch = DPMSolverMultistepScheduler(prediction_type=ptype)
        sch.set_timesteps(n)
        for i in sorted({0, 1, n // 2, n - 2, n - 1}):
            c = sch.step_coefficients_ms(i)
            (second if c[4] != 0.0 else first).append(((ptype, n, i), c))
    assert len(first) >= 9 and len(second) >= 18
    return first, second


def _step_ms(pred, x, hist, coef, x_out, xt, npix, HW, C, cfg, copies):
    """The entry itself, so that HW is the caller's (the wrapper passes npix)."""
    from diffusion_amd import _lib
    _lib.call('da_sampler_step_ms', pred.data_ptr(), x.data_ptr(), hist.data_ptr(), coef.data_ptr(), x_out.data_ptr(),
              xt.data_ptr() if xt is not None else None, npix, HW, C, int(cfg), copies,
              torch.cuda.current_stream().cuda_stream)


def _bf16_of(x_out, dev):
    from diffusion_amd import ops
    want = torch.empty(x_out.shape, device=dev, dtype=torch.bfloat16)
    ops.cast_f32_bf16(x_out, want)
    return want


SHAPES = [(1, 1), (2, 1), (63, 9), (64, 16), (255, 51), (256, 64), (257, 257)]   # (npix, HW): HW divides npix


def test_sampler_step_ms_matches_float64(dev):
    from diffusion_amd import ops
    first, second = _table_rows()
    gen = torch.Generator().manual_seed(43)
    worst = worst_hist = 0.0
    count = 0
    for (npix, HW), C, cfg, copies, inplace, order2 in itertools.product(SHAPES, (3, 4, 8), (0, 1), (1, 2), (0, 1), (0, 1)):
        rows = second if order2 else first
        tag, (ax, am, kx, k0, k1) = rows[count % len(rows)]
        g = (1.5, 7.5)[(count // 3) % 2]
        count += 1
        assert (k1 != 0.0) == bool(order2)
        pred = torch.randn((2 if cfg else 1) * npix, 8, generator=gen)
        x = torch.randn(npix, 8, generator=gen)
        hist = torch.randn(npix, 8, generator=gen)
        pred[:, C:] = PAD
        x[:, C:] = PAD
        hist[:, C:] = PAD
        if not order2:   # a first-order step does not read the history: whatever the allocator left must not reach the sample
            hist[:] = float('nan')
        # float64 reference in the entry's documented order
        pu = pred[:npix, :C].double()
        pt = pred[npix:, :C].double() if cfg else pu
        m = pu + g * (pt - pu) if cfg else pu
        M = (pu.abs() + g * (pt.abs() + pu.abs())) if cfg else pu.abs()
        xd = x[:, :C].double()
        x0 = ax * xd + am * m
        ref = kx * xd + k0 * x0
        x0_mag = (ax * xd).abs() + abs(am) * M
        bound = (kx * xd).abs() + abs(k0) * x0_mag
        if order2:
            ref = ref + k1 * hist[:, :C].double()
            bound = bound + (k1 * hist[:, :C].double()).abs()
        bound = 8 * U * bound
        # device
        coef = torch.tensor([ax, am, kx, k0, k1, g, 0.0, 0.0], dtype=torch.float64).float().to(dev)
        dx, dpred, dh = x.clone().to(dev), pred.to(dev), hist.clone().to(dev)
        x_out = dx if inplace else torch.full((npix, 8), 7.0, device=dev)
        xt = torch.full((copies * npix, 8), 7.0, device=dev, dtype=torch.bfloat16)
        if count % 2:
            _step_ms(dpred, dx, dh, coef, x_out, xt, npix, HW, C, cfg, copies)
        else:
            ops.sampler_step_ms(dpred, dx, dh, coef, x_out, xt, C=C, cfg=cfg, copies=copies)
        got, got_h = x_out.cpu(), dh.cpu()
        case = (npix, HW, C, cfg, copies, inplace, tag, g)
        ratio = ((got[:, :C].double() - ref).abs() / bound).max().item()
        ratio_h = ((got_h[:, :C].double() - x0).abs() / (4 * U * x0_mag)).max().item()
        worst, worst_hist = max(worst, ratio), max(worst_hist, ratio_h)
        assert ratio <= 1.0, (case, ratio)        # NaN (a history that leaked into a first-order step) fails here too
        assert ratio_h <= 1.0, (case, ratio_h)
        assert (got[:, C:] == 0).all() and (got_h[:, C:] == 0).all() and (xt.cpu()[:, C:] == 0).all(), case
        want_bf = _bf16_of(x_out, dev)
        for k in range(copies):
            assert torch.equal(xt[k * npix:(k + 1) * npix].view(torch.int16), want_bf.view(torch.int16)), (case, k)
        if not inplace:
            assert torch.equal(dx.cpu(), x), case   # the input is only read
        # last step: no next U-Net input; the same sample and history
        x_last, h_last = torch.empty(npix, 8, device=dev), hist.clone().to(dev)
        ops.sampler_step_ms(dpred, x.to(dev), h_last, coef, x_last, None, C=C, cfg=cfg, copies=copies)
        assert torch.equal(x_last.cpu(), got) and torch.equal(h_last.cpu(), got_h), case
    print(f'sampler_step_ms: {count} cases, worst |got - ref| / bound = {worst:.3f}, history {worst_hist:.3f}')


def test_sampler_step_ms_rejects_bad_arguments(dev):
    from diffusion_amd import _lib, ops
    npix, C = 98, 4
    pred = torch.zeros(2 * npix, 8, device=dev)
    x = torch.zeros(npix + 1, 8, device=dev)[:npix]
    hist = torch.zeros(npix + 1, 8, device=dev)[:npix]
    out = torch.full((npix + 1, 8), 7.0, device=dev)[:npix]
    coef = torch.zeros(16, device=dev)
    xt = torch.full((2 * npix + 1, 8), 7.0, device=dev, dtype=torch.bfloat16)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t, off=0: t.data_ptr() + off   # noqa: E731

    def rc(pred_=p(pred), x_=p(x), hist_=p(hist), coef_=p(coef), xo=p(out), xt_=p(xt), npix_=npix, HW=49, C_=C, cfg=1,
           copies=2):
        return _lib.load().da_sampler_step_ms(pred_, x_, hist_, coef_, xo, xt_, npix_, HW, C_, cfg, copies, s)

    for bad in (dict(hist_=None), dict(hist_=p(hist, 4)), dict(hist_=p(hist, 8)), dict(C_=0), dict(C_=9), dict(HW=48),
                dict(HW=0), dict(npix_=0), dict(copies=0), dict(copies=3), dict(pred_=p(pred, 4)), dict(x_=p(x, 8)),
                dict(coef_=p(coef, 4)), dict(xo=p(out, 4)), dict(xt_=p(xt, 2)), dict(pred_=None), dict(x_=None),
                dict(coef_=None), dict(xo=None)):
        assert rc(**bad) == 1, bad
    torch.cuda.synchronize()
    assert (out == 7).all() and (xt == 7).all() and (hist == 0).all()   # nothing was launched
    assert rc() == 0 and rc(xt_=None) == 0
    torch.cuda.synchronize()
    assert (out == 0).all()
    # the wrapper
    ok = dict(C=C, cfg=True, copies=2)
    xc, hc, c8 = x.contiguous(), hist.contiguous(), coef[:8]
    ops.sampler_step_ms(pred, xc, hc, c8, xc, xt[:2 * npix], **ok)
    with pytest.raises(ValueError):
        ops.sampler_step_ms(pred, xc, hc, c8, xc, None, C=9, cfg=True, copies=2)
    with pytest.raises(ValueError):
        ops.sampler_step_ms(pred, xc, hc, c8, xc, None, C=C, cfg=True, copies=3)
    with pytest.raises(ValueError):
        ops.sampler_step_ms(pred[:npix], xc, hc, c8, xc, None, **ok)           # half a guidance batch
    with pytest.raises(ValueError):
        ops.sampler_step_ms(pred, xc, hc[:npix - 1], c8, xc, None, **ok)       # a history over fewer pixels
    with pytest.raises(ValueError):
        ops.sampler_step_ms(pred, xc, xc, c8, xc, None, **ok)                  # the history is a buffer of its own
    with pytest.raises(ValueError):
        ops.sampler_step_ms(pred, xc, hc, coef[:4], xc, None, **ok)            # a four-float row
    with pytest.raises(ValueError):
        ops.sampler_step_ms(pred, xc, hc, coef[1:9], xc, None, **ok)           # misaligned coefficients
    with pytest.raises(ValueError):
        ops.sampler_step_ms(pred, xc, hc, c8, xc, xt[:npix], **ok)             # one copy's room for two
    with pytest.raises(ValueError):
        ops.sampler_step_ms(pred, xc, hc.double(), c8, xc, None, **ok)
    with pytest.raises(ValueError):
        ops.sampler_step_ms(pred, xc, hc.cpu(), c8, xc, None, **ok)


# ---------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tiny(dev):
    from oracle import unet_oracle as O
    from diffusion_amd.models.models import stable_diffusion_2
    ocfg = O.UNetConfig.tiny()
    model = stable_diffusion_2(model_name='tiny', pretrained=False, precomputed_latents=True, fsdp=False)
    model.unet.load_state_dict(O.init_state_dict(ocfg, seed=17))
    return ocfg, model


def _inputs(ocfg, seed=23, B=2, S=8):
    g = torch.Generator().manual_seed(seed)
    lat0 = torch.randn(B, 4, S, S, generator=g)
    txt = torch.randn(B, 77, ocfg.cross_attention_dim, generator=g)
    unc = torch.randn(B, 77, ocfg.cross_attention_dim, generator=g)
    return lat0, txt, unc


def _torch_loop(unet, sch, lat0, txt, unc, steps, guidance, dev):
    """generate()'s 'torch' route: the scheduler's own step() in torch ops around unet(...)"""
    sch.set_timesteps(steps)
    lat = lat0.to(dev)
    emb = torch.cat([unc, txt]).to(dev) if guidance > 1.0 else txt.to(dev)
    with torch.no_grad():
        for t in sch.timesteps:
            x = torch.cat([lat] * 2) if guidance > 1.0 else lat
            pred = unet(x, t, encoder_hidden_states=emb).sample
            if guidance > 1.0:
                pu, pt = pred.chunk(2)
                pred = pu + guidance * (pt - pu)
            lat = sch.step(pred, t, lat)['prev_sample']
    return lat


@pytest.mark.parametrize('ptype', ['epsilon', 'v_prediction'])
@pytest.mark.parametrize('guidance', [0.0, 3.0])
@pytest.mark.parametrize('n', [6, 20])
def test_hip_route_against_torch_route(tiny, dev, n, guidance, ptype):
    """The two routes differ only in the fp32 rounding of the step arithmetic (and what the U-Net makes of it).  The measuring
    stick is the same difference for DDIM on the same inputs; 2M has two more terms: 4x of it is allowed."""
    from diffusion_amd.models.schedulers import DDIMScheduler, DPMSolverMultistepScheduler
    from diffusion_amd.sampling import LatentSampler
    ocfg, model = tiny
    lat0, txt, unc = _inputs(ocfg)
    rel = {}
    for name, cls in (('ddim', DDIMScheduler), ('dpm++2m', DPMSolverMultistepScheduler)):
        sch = cls(prediction_type=ptype)
        hip = LatentSampler(model.unet, sch).sample(lat0.to(dev), txt.to(dev), unc.to(dev), num_inference_steps=n,
                                                    guidance_scale=guidance)
        loop = _torch_loop(model.unet, sch, lat0, txt, unc, n, guidance, dev)
        assert hip.shape == lat0.shape and hip.dtype == torch.float32 and torch.isfinite(hip).all()
        rel[name] = _rel(hip, loop)
        if name == 'dpm++2m':
            assert not torch.equal(hip, ddim_hip)   # another solver, another sample
        ddim_hip = hip
    print(f'{ptype} n {n} guidance {guidance}: hip vs torch rel-L2 DDIM {rel["ddim"]:.3e}, 2M {rel["dpm++2m"]:.3e}, '
          f'ratio {rel["dpm++2m"] / max(rel["ddim"], 1e-30):.2f}')
    assert rel['dpm++2m'] <= 4 * rel['ddim'], rel


@pytest.mark.parametrize('guidance', [0.0, 3.0])
def test_graph_replay_equals_eager_and_keeps_ddim_apart(tiny, dev, guidance):
    from diffusion_amd.models.schedulers import DDIMScheduler, DPMSolverMultistepScheduler
    from diffusion_amd.sampling import LatentSampler
    ocfg, model = tiny
    ms = LatentSampler(model.unet, DPMSolverMultistepScheduler())
    dd = LatentSampler(model.unet, DDIMScheduler())
    ms.graphs.clear()
    kw = dict(num_inference_steps=6, guidance_scale=guidance)
    args = [tuple(z.to(dev) for z in _inputs(ocfg, seed=seed)) for seed in (23, 77)]
    ddim_before = dd.sample(*args[0], graph=True, **kw)
    assert torch.equal(ddim_before, dd.sample(*args[0], **kw)) and len(ms.graphs) == 1
    for k, a in enumerate(args):   # the second call, other latents and context, reuses the capture
        eager = ms.sample(*a, **kw)
        graphed = ms.sample(*a, graph=True, **kw)
        assert len(ms.graphs) == 2, list(ms.graphs)   # its own capture, next to DDIM's of the same shape
        assert torch.equal(eager, graphed), (k, _rel(graphed, eager))
    assert not torch.equal(eager, dd.sample(*args[1], **kw))
    # DDIM's capture of the same shape is still DDIM's
    assert torch.equal(dd.sample(*args[0], graph=True, **kw), ddim_before) and len(ms.graphs) == 2
    # one capture serves both orders: the same graph with a first-order table
    o1 = LatentSampler(model.unet, DPMSolverMultistepScheduler(solver_order=1))
    assert torch.equal(o1.sample(*args[0], graph=True, **kw), o1.sample(*args[0], **kw)) and len(ms.graphs) == 2
    ms.graphs.clear()


# ---------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------
def _check_images(out, shape):
    assert out.shape == shape, out.shape
    assert torch.isfinite(out).all() and out.min() >= 0 and out.max() <= 1


def test_stable_diffusion_generate_with_dpm(dev, monkeypatch):
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.models.schedulers import DDIMScheduler, DPMSolverMultistepScheduler
    monkeypatch.delenv('DA_SAMPLER', raising=False)
    torch.manual_seed(11)
    model = stable_diffusion_2(model_name='tiny', pretrained=False, fsdp=False)
    assert type(model.inference_scheduler) is DDIMScheduler   # the default is what it was
    kw = dict(prompt=['a cool doge', 'a hot cat'], height=64, width=64, num_inference_steps=6, seed=3, progress_bar=False)
    ddim = model.generate(**kw)
    hip = model.generate(inference_scheduler='dpm++2m', **kw)
    _check_images(hip, (2, 3, 64, 64))
    assert not torch.equal(hip, ddim)
    assert torch.equal(model.generate(inference_scheduler='ddim', **kw), ddim)
    assert type(model.inference_scheduler) is DDIMScheduler   # for that call only
    assert torch.equal(model.generate(inference_scheduler='dpm++2m', sampler='graph', **kw), hip)
    obj = DPMSolverMultistepScheduler(prediction_type=model.inference_scheduler.prediction_type)
    assert torch.equal(model.generate(inference_scheduler=obj, **kw), hip)
    ref = model.generate(inference_scheduler='dpm++2m', sampler='torch', **kw)
    _check_images(ref, (2, 3, 64, 64))
    e = _rel(hip, ref)
    print(f'StableDiffusion.generate dpm++2m: hip vs torch image rel-L2 {e:.3e}')
    assert e < 8e-2, e   # the decoder cap of tests/test_sampler_gpu.py for image differences
    rect = model.generate(inference_scheduler='dpm++2m', **dict(kw, height=64, width=128))
    _check_images(rect, (2, 3, 64, 128))
    with pytest.raises(ValueError, match='inference_scheduler'):
        model.generate(inference_scheduler='euler', **kw)
    # the model's own scheduler: what eval_forward's generate() calls follow
    model.inference_scheduler = obj
    assert torch.equal(model.generate(**kw), hip)


def test_discrete_pixel_diffusion_built_with_dpm(dev, monkeypatch):
    from diffusion_amd.models.models import discrete_pixel_diffusion
    from diffusion_amd.models.schedulers import DPMSolverMultistepScheduler
    from diffusion_amd.models.unet import UNetConfig
    monkeypatch.delenv('DA_SAMPLER', raising=False)
    cfg = UNetConfig(in_channels=3, out_channels=3, block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4),
                     cross_attention_dim=768)
    torch.manual_seed(5)
    model = discrete_pixel_diffusion(unet_config=cfg, seed=3, inference_scheduler='dpm++2m', prediction_type='v_prediction')
    assert type(model.inference_scheduler) is DPMSolverMultistepScheduler
    assert model.inference_scheduler.prediction_type == 'v_prediction'
    kw = dict(prompt=['a cool doge'], height=8, width=8, num_inference_steps=6, guidance_scale=3.0, seed=7,
              progress_bar=False)
    outs = {s: model.generate(sampler=s, **kw) for s in ('hip', 'graph', 'torch')}
    for out in outs.values():
        _check_images(out, (1, 3, 8, 8))
    assert torch.equal(outs['graph'], outs['hip'])
    print(f'PixelDiffusion.generate dpm++2m: hip vs torch image rel-L2 {_rel(outs["hip"], outs["torch"]):.3e}')
    assert torch.equal(model.generate(inference_scheduler='dpm++2m', **kw), outs['hip'])
    assert not torch.equal(model.generate(inference_scheduler='ddim', **kw), outs['hip'])
    _check_images(model.generate(**dict(kw, height=8, width=16)), (1, 3, 8, 16))
