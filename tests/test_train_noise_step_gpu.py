"""GPU tests of the philox noise mode through the models, the trainer and the graphed step (tiny U-Net, latents 4x16x16, text
77x128): what a sample is trained on depends on its seed only - not on the batch it rides in, the microbatch split, graphs on
or off, or whether the run was resumed."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _sd(**kw):
    from diffusion_amd.models.models import stable_diffusion_2
    kw.setdefault('noise_source', 'philox')
    return stable_diffusion_2(model_name='tiny', pretrained=False, precomputed_latents=True, fsdp=False, seed=3, **kw)


def _trainer(model, mb, use_graphs=False, **kw):
    from diffusion_amd.optim import FusedAdamW
    from diffusion_amd.trainer import Trainer
    opt = FusedAdamW(lr=1e-3, weight_decay=0.01, unet=model.unet)
    return Trainer(model, train_dataloader=None, optimizers=opt, max_duration='4ba', device_train_microbatch_size=mb,
                   use_graphs=use_graphs, seed=11, **kw)


def _batch(dev, seed, n=6):
    g = torch.Generator().manual_seed(seed)
    return {'image_latents': torch.randn(n, 4, 16, 16, generator=g).half().to(dev),
            'caption_latents': torch.randn(n, 77, 128, generator=g).half().to(dev)}


def _record(model):
    """the hook: every forward's timesteps and target, in call order"""
    seen = []
    inner = model.forward

    def forward(batch, *a, **kw):
        out = inner(batch, *a, **kw)
        seen.append((out[2].clone(), out[1].clone()))
        return out
    model.forward = forward
    return seen


def _cat(seen):
    return torch.cat([t for t, _ in seen]).cpu(), torch.cat([g for _, g in seen]).cpu()


@pytest.mark.parametrize('kw', [{}, dict(noise_offset=0.1, input_perturbation=0.1, timestep_sampling='stratified',
                                         timestep_range=[100, 900])], ids=['plain', 'all-options'])
def test_forward_of_a_slice_is_the_slice_of_the_forward(dev, kw):
    from diffusion_amd import ops
    from diffusion_amd.train_noise import batch_entries
    model = _sd(**kw)
    batch = dict(_batch(dev, 1), **batch_entries(11, 0, 0, 1, 6, dev))
    with torch.no_grad():
        _, target, t = model(batch)
        target, t = target.clone(), t.clone()
        for s, e in ((0, 2), (2, 6)):
            sub = {k: (v[s:e] if torch.is_tensor(v) else v) for k, v in batch.items()}
            _, tg, ts = model(sub)
            assert torch.equal(ts, t[s:e]) and torch.equal(tg.contiguous().view(torch.int32), target[s:e].contiguous().view(torch.int32))
    model._pending = None
    assert t.dtype == torch.int64 and target.shape == (6, 4, 16, 16)
    if kw:
        for g, tt in enumerate(t.tolist()):   # stratified over the 6 places of the global batch, inside [100, 900)
            assert 100 + (g * 800) // 6 <= tt < 100 - (-(g + 1) * 800) // 6
    else:   # the epsilon target is the sample's own Philox stream
        n = ops.randn_philox(batch['_sample_seeds'], 0, 0, (6, 4, 16, 16))
        assert torch.equal(target.contiguous().view(torch.int32), n.view(torch.int32))
    # injected noise has no place in this mode; injected timesteps are honoured
    with pytest.raises(ValueError, match='philox'):
        model(dict(batch, _noise=torch.zeros(6, 4, 16, 16, device=dev)))
    inj = torch.tensor([0, 999, 5, 6, 7, 8], device=dev)
    with torch.no_grad():
        assert torch.equal(model(dict(batch, _timesteps=inj))[2], inj)
    model._pending = None
    # without seeds in the batch torch's generator governs
    bare = _batch(dev, 1)
    with torch.no_grad():
        torch.manual_seed(5); a = model(bare)
        torch.manual_seed(5); b = model(bare)
        c = model(bare)
    model._pending = None
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and not torch.equal(a[1], c[1])


def test_microbatch_split_does_not_change_the_draws(dev):
    small, whole = _trainer(_sd(), 2), _trainer(_sd(), 6)
    seen_s, seen_w = _record(small.model), _record(whole.model)
    for step in range(2):
        small.batch_idx = whole.batch_idx = step
        ls, lw = small.train_batch(_batch(dev, 20 + step)), whole.train_batch(_batch(dev, 20 + step))
        assert abs(ls.item() - lw.item()) < 1e-3, (step, ls.item(), lw.item())
    assert len(seen_s) == 6 and len(seen_w) == 2
    (ts, gs), (tw, gw) = _cat(seen_s), _cat(seen_w)
    assert torch.equal(ts, tw) and torch.equal(gs.view(torch.int32), gw.view(torch.int32))
    assert not torch.equal(tw[:6], tw[6:])   # the next optimizer step draws anew


@pytest.mark.parametrize('kw', [{}, dict(noise_offset=0.1, timestep_sampling='stratified')], ids=['plain', 'stratified-offset'])
def test_graph_replay_equals_eager_in_philox_mode(dev, kw):
    eager, graphed = _trainer(_sd(**kw), 2, False), _trainer(_sd(**kw), 2, True)
    for step in range(3):
        eager.batch_idx = graphed.batch_idx = step
        le, lg = eager.train_batch(_batch(dev, 30 + step)), graphed.train_batch(_batch(dev, 30 + step))
        torch.cuda.synchronize()
        assert torch.equal(le, lg), (step, le.item(), lg.item())
        assert torch.equal(eager.model.unet.grad, graphed.model.unet.grad), step
        assert torch.equal(eager.model.unet.master, graphed.model.unet.master), step
    assert len(graphed._graph_cache.graphs) == 1 and graphed._graph_cache.captures == 1
    assert eager._graph_cache is None or not eager._graph_cache.graphs


def test_resumed_run_draws_what_the_uninterrupted_run_drew(dev):
    full, resumed = _trainer(_sd(), 3), _trainer(_sd(), 3)
    seen_f, seen_r = _record(full.model), _record(resumed.model)
    for step in range(4):
        full.batch_idx = step
        full.train_batch(_batch(dev, 40 + step))
    for step in (2, 3):
        resumed.batch_idx = step
        resumed.train_batch(_batch(dev, 40 + step))
    (tf, gf), (tr, gr) = _cat(seen_f[4:]), _cat(seen_r)
    assert torch.equal(tf, tr) and torch.equal(gf.view(torch.int32), gr.view(torch.int32))


def test_min_snr_weights_read_the_drawn_timesteps(dev):
    from diffusion_amd import ops
    model = _sd(snr_gamma=5.0)
    batch = _batch(dev, 50, 4)
    torch.manual_seed(3)
    model.unet.zero_grad()
    pred, target, t = model(batch)
    loss = model.loss((pred, target, t), batch)
    npix = 4 * 16 * 16
    p8, g8 = (torch.zeros(npix, 8, device=dev) for _ in range(2))
    p8[:, :4], g8[:, :4] = pred.permute(0, 2, 3, 1).reshape(npix, 4), target.permute(0, 2, 3, 1).reshape(npix, 4)
    dpred = torch.empty(npix, 8, device=dev, dtype=torch.bfloat16)
    lossbuf = torch.zeros(1, device=dev)
    ops.mse_loss_w(p8, g8, dpred, lossbuf, model.unet._scratch, npix, 4, 256, t, model.snr_weight_table(dev),
                   2.0 / (4.0 * npix), 1.0, 0)
    assert torch.equal(loss.detach().view(torch.int32), lossbuf[0].view(torch.int32)), (loss.item(), lossbuf.item())
    assert len(set(t.tolist())) > 1
    loss.backward()
    assert float(model.unet.grad.abs().sum()) > 0


def test_trainer_eval_repeats_its_draws(dev):
    model = _sd()
    g = torch.Generator().manual_seed(9)
    evalset = [{'image_latents': torch.randn(4, 4, 16, 16, generator=g).half(),
                'caption_latents': torch.randn(4, 77, 128, generator=g).half()} for _ in range(2)]
    tr = _trainer(model, 4, eval_dataloader=evalset, log_every=1000)
    seen = _record(model)
    a = tr.eval()['metrics/eval/MeanSquaredError']
    torch.manual_seed(77)   # whatever the global generator does in between
    b = tr.eval()['metrics/eval/MeanSquaredError']
    assert a == b and a > 0
    assert torch.equal(seen[0][0], seen[2][0]) and torch.equal(seen[1][0], seen[3][0])
    assert not torch.equal(seen[0][0], seen[1][0])   # the second batch has its own seeds


@pytest.fixture(scope='module')
def pixel_models(dev):
    from diffusion_amd.models.models import continuous_pixel_diffusion, discrete_pixel_diffusion
    from diffusion_amd.models.unet import UNetConfig
    cfg = dict(in_channels=3, out_channels=3, block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4),
               cross_attention_dim=768)
    kw = dict(seed=3, noise_source='philox', noise_offset=0.05, input_perturbation=0.05, timestep_sampling='stratified')
    return {'discrete': discrete_pixel_diffusion(unet_config=UNetConfig(**cfg), **kw),
            'continuous': continuous_pixel_diffusion(unet_config=UNetConfig(**cfg), **kw)}


@pytest.mark.parametrize('prediction_type', ['sample', 'v_prediction'])
@pytest.mark.parametrize('kind', ['discrete', 'continuous'])
def test_pixel_models_train_in_philox_mode(dev, pixel_models, kind, prediction_type):
    from diffusion_amd.train_noise import batch_entries
    model = pixel_models[kind]
    model.prediction_type = prediction_type
    B = 4
    batch = {'image': torch.rand(B, 3, 16, 16, device=dev) * 2 - 1, 'captions': torch.randint(0, 1000, (B, 77), device=dev)}
    batch.update(batch_entries(11, 0, 0, 1, B, dev))
    model.unet.zero_grad()
    out = model(batch)
    loss = model.loss(out, batch)
    loss.backward()
    assert torch.isfinite(loss) and float(model.unet.grad.abs().sum()) > 0
    assert out[0].shape == out[1].shape == (B, 3, 16, 16)
    t = out[2].tolist()
    if kind == 'continuous':
        t_max = model.scheduler.t_max
        assert out[2].dtype == torch.float32 and all(0 <= v < t_max for v in t)
        for g, v in enumerate(t):   # sample g of 4 in the g-th quarter of [0, t_max), up to the roundings of the formula
            assert t_max * g / B - 1e-6 <= v <= t_max * (g + 1) / B + 1e-6
    else:
        assert out[2].dtype == torch.int64
        for g, v in enumerate(t):
            assert (g * 1000) // B <= v < -(-(g + 1) * 1000 // B)
    if prediction_type == 'sample':   # the target is the clean image, whatever was drawn
        assert torch.equal(out[1], batch['image'].float())
    with pytest.raises(ValueError, match='philox'):
        model(dict(batch, _noise=torch.zeros(B, 3, 16, 16, device=dev)))
