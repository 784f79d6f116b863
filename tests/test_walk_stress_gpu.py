"""The HIP U-Net training step against the float64 CPU oracle at weights under which the walk's wiring carries weight
(tests/walk_stress.py): live norm affines (gamma 1 +- 0.5, beta +- 0.3), attention sharpened by doubled to_q / to_k (logit
standard deviation 1.2 ... 1.9), a width whose C = 320 levels take the fused-GEGLU forward and backward, head counts 1 / 2 / 5,
t = 0 and t = 999 - and with EVERY gradient tensor of the manifest held to a bound of its own.  The model is driven as in
test_unet_parity_gpu.py::test_tiny_train_step_parity (model forward, ``model.loss``, ``backward``), so the noising, v-target
and MSE kernels are in the loop.

``walk_stress.BOUNDS`` holds what is asserted; test_walk_stress_host.py shows on the CPU that the reference alone under our
number format stays inside those bounds and that each of seven wiring slips breaks them.  Measured on MI355X
(profiles/walk_stress_margins.json), HIP / bf16 emulation of the oracle / bound:

  case                  pred rel-L2        |loss - oracle|      global grad rel-L2   worst tensor rel-L2   worst matrix cosine
  stress-eps-b3-16x16   0.0110 / 0.0100    2.6e-4 / 2.2e-4      0.0211 / 0.0174      0.0642 / 0.0510       0.99795 / 0.99875
  stress-v-b2-8x24      0.0105 / 0.0095    3.9e-5 / 3.6e-4      0.0254 / 0.0207      0.0615 / 0.0538       0.99813 / 0.99855
  tiny-eps-b2-16x16     0.0124 / 0.0107    1.5e-4 / 1.5e-4      0.0234 / 0.0200      0.0617 / 0.0666       0.99817 / 0.99785
  bound                 0.024              5.6e-4               0.040                0.12                  0.9959

The worst tensors are the mid block's attn1.to_q / to_k weights and norm vectors in every case, for the HIP path and for the
emulation alike: number-format noise, not a block that stands out.  The tests found no defect in the walk.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import walk_stress as ws  # noqa: E402
from parity_margins import record  # noqa: E402

pytestmark = pytest.mark.gpu

CASE_NAMES = list(ws.CASES)
REPEAT_CASE = 'stress-v-b2-8x24'
_RUNS = {}


def _model(width, ptype):
    from diffusion_amd.models.models import stable_diffusion_2
    model = stable_diffusion_2(model_name='tiny', unet_config=ws.stress_config('hip', width, ptype), pretrained=False,
                               precomputed_latents=True, fsdp=False)
    assert model.prediction_type == ptype
    model.unet.load_state_dict(ws.state_dict64(width))
    return model


def _step(model, inputs, dev):
    latents, ctx, noise, t = inputs
    batch = {'image_latents': latents.to(dev), 'caption_latents': ctx.to(dev)}
    model.unet.zero_grad()
    out = model(batch, timesteps=t.to(dev), noise=noise.to(dev))
    pred8 = model._pending[0].clone()
    loss = model.loss(out, batch)
    loss.backward()
    torch.cuda.synchronize()
    return out[0].detach().float().cpu(), pred8.cpu(), loss.item(), model.unet.grad.clone()


def _run(name, dev):
    """One HIP training step of the case (once per process) and its figures against the fp64 oracle."""
    if name not in _RUNS:
        width, ptype = ws.CASES[name][:2]
        d = ws.case_data(name)
        model = _model(width, ptype)
        if width == 'stress':
            assert model.unet.num_params == ws.STRESS_PARAMS
        pred, pred8, loss, flat = _step(model, d['inputs'], dev)
        grads = {k: p.grad.detach().float().cpu() for k, p in model.unet.named_parameters()}
        assert set(grads) == set(d['grads'])
        m = ws.metrics(pred, grads, d['pred'], d['grads'], loss, d['loss'])
        s = ws.summary(m)
        e = ws.summary(d['emu'])
        record('walk_stress/' + name, tolerances=ws.BOUNDS, **s, **{'emulation_' + k: v for k, v in e.items()})
        print(f'\n{name}: HIP {s}\n{name}: emulation {e}')
        _RUNS[name] = {'model': model, 'data': d, 'pred': pred, 'pred8': pred8, 'loss': loss, 'flat': flat, 'grads': grads,
                       'm': m}
    return _RUNS[name]


def _worst_table(m, emu, key, n=5, reverse=True):
    order = sorted(m[key], key=m[key].get, reverse=reverse)[:n]
    return '\n' + '\n'.join(f'  {k}: HIP {m[key][k]:.4g}, emulation {emu[key][k]:.4g}' for k in order)


@pytest.mark.parametrize('name', CASE_NAMES)
def test_outputs_are_finite_and_pad_channels_zero(dev, name):
    r = _run(name, dev)
    assert torch.isfinite(r['pred8']).all() and torch.isfinite(r['flat']).all() and r['loss'] == r['loss']
    assert r['pred8'].shape[1] == 8 and torch.equal(r['pred8'][:, 4:], torch.zeros_like(r['pred8'][:, 4:]))
    assert r['pred'].shape == r['data']['pred'].shape


@pytest.mark.parametrize('name', CASE_NAMES)
def test_aggregates_within_bounds(dev, name):
    m = _run(name, dev)['m']
    assert m['pred_rel'] < ws.BOUNDS['pred_rel'], f"prediction rel-L2 {m['pred_rel']}"
    assert m['loss_abs'] < ws.BOUNDS['loss_abs'], f"|loss - oracle| {m['loss_abs']}"
    assert m['grad_rel'] < ws.BOUNDS['grad_rel'], f"global gradient rel-L2 {m['grad_rel']}"


@pytest.mark.parametrize('name', CASE_NAMES)
def test_every_gradient_tensor_on_its_own(dev, name):
    """No tensor of the manifest is excluded: the smallest fp64 gradient rms over the cases is 2.2e-6 and none is zero."""
    r = _run(name, dev)
    m, emu = r['m'], r['data']['emu']
    assert len(m['tensor_rel']) == len(r['data']['grads']) and all(g.norm() > 0 for g in r['data']['grads'].values())
    bad = [k for k, v in m['tensor_rel'].items() if not v < ws.BOUNDS['tensor_rel']]
    assert not bad, f"{len(bad)} gradient tensors at or above rel-L2 {ws.BOUNDS['tensor_rel']}; the five worst:" + \
        _worst_table(m, emu, 'tensor_rel')
    bad = [k for k, v in m['matrix_cos'].items() if not v >= ws.BOUNDS['matrix_cos']]
    assert not bad, f"{len(bad)} weight-matrix gradients below cosine {ws.BOUNDS['matrix_cos']}; the five worst:" + \
        _worst_table(m, emu, 'matrix_cos', reverse=False)


def test_second_identical_step_gives_equal_gradients(dev):
    r = _run(REPEAT_CASE, dev)
    pred, pred8, loss, flat = _step(r['model'], r['data']['inputs'], dev)
    assert loss == r['loss'] and torch.equal(pred8, r['pred8'])
    assert torch.equal(flat, r['flat'])


def test_forward_only_walk(dev):
    """The stressed width as sampling runs it: B = 2 doubled to 4 as under guidance (unconditional | conditional context),
    t = 999 and 0.  The diffusers-style call matches the fp64 oracle, and the forward-only walk on the context K/V projected
    once equals the recording walk bit for bit."""
    O = ws.oracle()
    r = _run(ws.SQUARE_CASE, dev)
    unet, cfg = r['model'].unet, r['data']['cfg']
    g = torch.Generator().manual_seed(41)
    B, H, W = 4, 16, 16
    x = torch.randn(2, 4, H, W, generator=g).repeat(2, 1, 1, 1)
    t = torch.tensor([999, 0, 999, 0])
    ctx = torch.randn(B, 77, cfg.cross_attention_dim, generator=g)
    ref = O.unet_forward(r['data']['sd'], cfg, x.double(), t, ctx.double())
    with torch.no_grad():
        got = unet(x.to(dev), t.to(dev), ctx.to(dev)).sample.float().cpu()
        xt, c = unet.to_nhwc8(x.to(dev)), unet.prepare_ctx(ctx.to(dev))
        rec = unet.forward_features(xt, t.to(dev), c, B, (H, W)).clone()
        unet._tape = None
        fwd = unet.forward_features(xt, t.to(dev), c, B, (H, W), kv=unet.project_context(c), record=False)
    e = ((got.double() - ref).norm() / ref.norm()).item()
    record('walk_stress/forward-only-b4-16x16', tolerances=ws.BOUNDS, pred_rel_l2=e)
    assert torch.isfinite(got).all()
    assert e < ws.BOUNDS['pred_rel'], f'prediction rel-L2 {e}'
    assert torch.equal(rec.view(B, H, W, 8)[..., :4].permute(0, 3, 1, 2).float().cpu(), got)
    assert torch.equal(fwd, rec)
