"""FrechetInceptionDistance (metrics/fid.py) on the GPU: the metric against numpy on the tower's own features, the two input
paths, and ``Trainer.eval()`` end to end.

The tower is random-init and 6 samples per side span 5 of 2048 dimensions, so Sigma_r Sigma_f is singular: the comparison
with numpy float64 on the tower's own fp32 features (means and traces from ``np.cov``) uses the absolute bound
1e-6 * (tr Sigma_r + tr Sigma_f), not a relative one.  The reference's square-root term is exact for such moments: the
non-zero eigenvalues of Sigma_r Sigma_f are the squared singular values of the 6 x 6 matrix Xr Xf^T / 5 of the centred
features.  ``np.linalg.eigvals(Sigma_r @ Sigma_f)`` is not used as the reference: it returns the 2043 zero eigenvalues as
+-1e-13, whose square roots sum to 1.2e-6 ... 1.4e-6 of the traces (measured with two LAPACK builds, differently on each) - more than the bound, in the reference alone."""
import warnings

import numpy as np
import pytest
import torch

import inception_reference as IR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def metric(dev):
    from diffusion_amd.metrics.fid import FrechetInceptionDistance
    with pytest.warns(UserWarning, match='RANDOM-INIT'):
        return FrechetInceptionDistance(device=dev)


def _numpy_fid(fr, ff):
    fr, ff = np.asarray(fr, np.float64), np.asarray(ff, np.float64)
    sr, sf = np.cov(fr, rowvar=False), np.cov(ff, rowvar=False)
    xr, xf = fr - fr.mean(0), ff - ff.mean(0)
    sv = np.linalg.svd(xr @ xf.T / np.sqrt((len(fr) - 1) * (len(ff) - 1)), compute_uv=False)
    return np.sum((fr.mean(0) - ff.mean(0)) ** 2) + np.trace(sr) + np.trace(sf) - 2 * sv.sum(), np.trace(sr) + np.trace(sf)


def test_metric_against_numpy_on_its_own_features(metric, dev):
    metric.reset()
    batches = [(IR.seeded_images(3, 40, 56, seed=s), s < 2) for s in range(4)]   # 2 real + 2 fake updates of B = 3
    feats = {True: [], False: []}
    for imgs, real in batches:
        metric.update(imgs, real=real)
        feats[real].append(metric.features(imgs).cpu().numpy())
    assert metric.state['real']['n'].item() == 6 and metric.state['fake']['n'].item() == 6
    got = float(metric.compute())
    want, traces = _numpy_fid(np.concatenate(feats[True]), np.concatenate(feats[False]))
    print(f'FID {got:.6e}, numpy {want:.6e}, traces {traces:.3e}, |diff| / traces {abs(got - want) / traces:.2e}')
    assert np.isfinite(got) and abs(got - want) <= 1e-6 * traces
    # the same images on both sides: zero within the same bound
    metric.reset()
    for imgs, _ in batches[:2]:
        metric.update(imgs, real=True)
        metric.update(imgs, real=False)
    assert abs(float(metric.compute())) <= 1e-6 * traces
    metric.reset()
    with pytest.raises(RuntimeError):
        metric.compute()


def test_normalize_true_on_floats_equals_uint8_of_the_floor(dev):
    from diffusion_amd.metrics.fid import FrechetInceptionDistance
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        as_u8 = FrechetInceptionDistance(device=dev)
        as_f = FrechetInceptionDistance(normalize=True, device=dev)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(3, 3, 48, 40, generator=g) * 1.2 - 0.1   # some values outside [0, 1]: they clamp
    u8 = torch.from_numpy(IR.levels_of_float(x.numpy()).astype(np.uint8))
    for real in (True, False):
        as_f.update(x, real=real)
        as_u8.update(u8, real=real)
    torch.cuda.synchronize()
    for side in ('real', 'fake'):
        for k in ('sum', 'cov', 'n'):
            assert torch.equal(as_f.state[side][k], as_u8.state[side][k]), (side, k)
    assert float(as_f.state['real']['cov'].abs().sum()) > 0
    with pytest.raises(ValueError):
        as_f.update(u8, real=True)
    with pytest.raises(ValueError):
        as_u8.update(x, real=True)


def test_trainer_eval_logs_fid_next_to_the_clip_score(dev):
    import clip_reference as CR
    from diffusion_amd.metrics.clip_score import CLIPScore
    from diffusion_amd.metrics.fid import FrechetInceptionDistance
    from diffusion_amd.models.composer_shim import MeanSquaredError
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.optim import FusedAdamW
    from diffusion_amd.trainer import Trainer
    clip = CR.tiny_clip(seed=5).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fid = FrechetInceptionDistance(normalize=True, device=dev)
    model = stable_diffusion_2(model_name='tiny', pretrained=False, fsdp=False, encode_latents_in_fp16=False,
                               val_metrics=[MeanSquaredError(), fid, CLIPScore(model=clip, device=dev)],
                               val_guidance_scales=[3.0])
    tok = model.tokenizer
    g = torch.Generator().manual_seed(4)
    evalset = [{'image': torch.rand(2, 3, 64, 64, generator=g),
                'captions': tok(['a red cube', 'a blue ball'], padding='max_length', max_length=77, truncation=True,
                                return_tensors='pt')['input_ids']}]
    opt = FusedAdamW(lr=1e-3, weight_decay=0.01, unet=model.unet)
    tr = Trainer(model, train_dataloader=None, optimizers=opt, max_duration='1ba', eval_dataloader=evalset, log_every=1000)
    inner = model.generate
    model.generate = lambda *a, **kw: inner(*a, **{**kw, 'num_inference_steps': 4})   # the routing is under test, not the sampler
    torch.manual_seed(11)
    try:
        out = tr.eval()
    finally:
        del model.generate
    key = 'metrics/eval/FrechetInceptionDistance-scale-3p0'
    assert key in out and 'metrics/eval/CLIPScore-scale-3p0' in out
    swept = model.val_metrics['FrechetInceptionDistance-scale-3p0']
    assert swept.state['real']['n'].item() == 2 and swept.state['fake']['n'].item() == 2
    print(f'{key} = {out[key]:.6e}')
    assert np.isfinite(out[key]) and out[key] >= 0   # measured 24.9: real images against a random U-Net's are far apart
    assert np.isfinite(out['metrics/eval/CLIPScore-scale-3p0'])
