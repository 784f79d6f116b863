"""LoRA training steps on the MI355X against the float64 oracle with adapters (tests/lora_reference.py): the merged shadows in
the forward and dgrad, the projected adapter gradients, the adapter AdamW step, the frozen master, reproducibility and
checkpoint / resume.  Cases ``tiny-eps-b2-16x16`` and ``stress-v-b2-8x24`` of walk_stress (the stress width takes the
fused-GEGLU and grouped-wgrad paths), ranks 4 and 16, the default attention targets plus one 3x3 convolution.

Measured on MI355X (profiles/lora_margins.json), HIP / bf16 emulation of the oracle / bound:

  case               r    pred rel-L2        |loss - oracle|      worst adapter-gradient rel-L2   worst cosine
  tiny-eps-b2-16x16  4    0.0123 / 0.0112    2.0e-4 / 2.2e-4      0.1105 / 0.0891                 0.99401 / 0.99613
  tiny-eps-b2-16x16  16   0.0124 / 0.0106    1.2e-4 / 4.0e-5      0.0754 / 0.0696                 0.99725 / 0.99769
  stress-v-b2-8x24   4    0.0116 / 0.0107    2.5e-4 / 6.3e-4      0.0831 / 0.0702                 0.99664 / 0.99788
  stress-v-b2-8x24   16   0.0112 / 0.0093    3.7e-4 / 2.4e-4      0.0890 / 0.0754                 0.99604 / 0.99735
  bound                   0.024              5.6e-4               0.19                            0.9929
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import lora_reference as lr  # noqa: E402
import walk_stress as ws  # noqa: E402
from parity_margins import record  # noqa: E402

pytestmark = pytest.mark.gpu

COMBOS = [(n, r) for n in lr.CASES for r in lr.RANKS]
SEQ = ('stress-v-b2-8x24', 4)      # the optimizer sequence: the width with the fused-GEGLU / grouped-wgrad paths
LR = 1e-3
_RUNS = {}


def _model(name, r, via_algorithm=False):
    """The case's model with the test's adapters attached (A as initialised, B from lora_reference.adapter_tensors)."""
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.optim import FusedAdamW
    width, ptype = ws.CASES[name][:2]
    model = stable_diffusion_2(model_name='tiny', unet_config=ws.stress_config('hip', width, ptype), pretrained=False,
                               precomputed_latents=True, fsdp=False)
    model.unet.load_state_dict(ws.state_dict64(width))
    opt = FusedAdamW(unet=model.unet, lr=LR, weight_decay=0.01)
    if via_algorithm:
        from diffusion_amd.algorithms.lora import LoRA
        LoRA(rank=r, target_modules=list(lr.TARGETS), seed=lr.ADAPTER_SEED).configure_optimizer(opt)
    else:
        model.unet.add_lora(r, target_modules=lr.TARGETS, seed=lr.ADAPTER_SEED)
        opt.attach_lora()
    ad = model.unet.lora
    assert [it.module for it in ad.items] == [it.module for it in lr.layout(name, r).items]
    ad.load_state_dict({k: v.float() for k, v in lr.adapter_tensors(name, r).items()})
    model.unet.sync_shadows()
    return model, opt


def _fwd_bwd(model, inputs, dev):
    latents, ctx, noise, t = inputs
    batch = {'image_latents': latents.to(dev), 'caption_latents': ctx.to(dev)}
    model.unet.zero_grad()
    out = model(batch, timesteps=t.to(dev), noise=noise.to(dev))
    loss = model.loss(out, batch)
    loss.backward()
    return out[0].detach().float().cpu(), loss.item()


def _adapter_grads(ad):
    from diffusion_amd.lora import to_file_tensors
    g = ad.grad.cpu()
    out = {}
    for it in ad.items:
        out.update(to_file_tensors(it, ad.A(it, g), ad.B(it, g)))
    return out


def _run(name, r, dev):
    if (name, r) not in _RUNS:
        from diffusion_amd import ops
        d = lr.case_data(name, r)
        model, opt = _model(name, r)
        pred, loss = _fwd_bwd(model, d.inputs, dev)
        ops.lora_project(model.unet.grad, model.unet.lora)
        torch.cuda.synchronize()
        grads = _adapter_grads(model.unet.lora)
        m = ws.metrics(pred, grads, d.pred, d.grads, loss, d.loss)
        tr, mc = m['tensor_rel'], m['matrix_cos']
        kw, kc = max(tr, key=tr.get), min(mc, key=mc.get)
        etr, emc = d.emu['tensor_rel'], d.emu['matrix_cos']
        fig = {'pred_rel_l2': m['pred_rel'], 'loss_abs_delta': m['loss_abs'], 'worst_tensor_rel_l2': tr[kw], 'worst_tensor': kw,
               'worst_cosine': mc[kc], 'worst_cosine_tensor': kc, 'emulation_pred_rel_l2': d.emu['pred_rel'],
               'emulation_loss_abs_delta': d.emu['loss_abs'], 'emulation_worst_tensor_rel_l2': max(etr.values()),
               'emulation_worst_cosine': min(emc.values())}
        record(f'lora/{name}-r{r}', tolerances={**{k: ws.BOUNDS[k] for k in ('pred_rel', 'loss_abs')}, **lr.BOUNDS}, **fig)
        print(f'\n{name} r={r}: {fig}')
        _RUNS[name, r] = {'model': model, 'opt': opt, 'd': d, 'm': m, 'pred': pred, 'loss': loss,
                          'flat': model.unet.lora.grad.clone()}
    return _RUNS[name, r]


@pytest.mark.parametrize('name,r', COMBOS)
def test_prediction_and_loss_follow_the_merged_weights(dev, name, r):
    m = _run(name, r, dev)['m']
    assert m['pred_rel'] < ws.BOUNDS['pred_rel'], f"prediction rel-L2 {m['pred_rel']}"
    assert m['loss_abs'] < ws.BOUNDS['loss_abs'], f"|loss - oracle| {m['loss_abs']}"


@pytest.mark.parametrize('name,r', COMBOS)
def test_every_adapter_gradient_tensor(dev, name, r):
    run = _run(name, r, dev)
    m, d = run['m'], run['d']
    assert len(m['tensor_rel']) == len(d.grads) == 2 * len(d.ad.items) and len(m['matrix_cos']) == len(d.grads)
    assert torch.isfinite(run['flat']).all()
    bad = sorted((v, k) for k, v in m['tensor_rel'].items() if not v < lr.BOUNDS['tensor_rel'])
    assert not bad, f"{len(bad)} adapter gradients at or above rel-L2 {lr.BOUNDS['tensor_rel']}; worst {bad[-3:]}"
    bad = sorted((v, k) for k, v in m['matrix_cos'].items() if not v >= lr.BOUNDS['matrix_cos'])
    assert not bad, f"{len(bad)} adapter gradients below cosine {lr.BOUNDS['matrix_cos']}; worst {bad[:3]}"


def test_frozen_matrices_get_no_weight_gradient_and_a_repeated_step_is_bit_identical(dev):
    from diffusion_amd import ops
    run = _run(*SEQ, dev)
    unet = run['model'].unet
    adapted = set(unet.lora.storages)
    for name, mat in unet._mats.items():
        if name in adapted:
            assert mat.gw.abs().max() > 0, name
        else:
            assert not mat.gw.any(), name          # skipped: the zero fill of zero_grad() is still there
    pred, loss = _fwd_bwd(run['model'], run['d'].inputs, dev)
    ops.lora_project(unet.grad, unet.lora)
    assert loss == run['loss'] and torch.equal(pred, run['pred'])
    assert torch.equal(unet.lora.grad.view(torch.int32), run['flat'].view(torch.int32))


def _train(model, opt, inputs, dev, steps, hook=None):
    for i in range(steps):
        _fwd_bwd(model, inputs, dev)
        if hook:
            hook(i)
        opt.step()
    torch.cuda.synchronize()


def test_three_steps_adamw_frozen_master_and_resume(dev):
    O = ws.oracle()
    name, r = SEQ
    d = lr.case_data(name, r)
    model, opt = _model(name, r, via_algorithm=True)
    unet, ad = model.unet, model.unet.lora
    master0, shadow0, params0 = unet.master.clone(), unet.shadow.clone(), ad.params.clone()
    # step 1: the adapter update is AdamW applied to the HIP path's own adapter gradient
    _train(model, opt, d.inputs, dev, 1)
    assert unet.opt_step == 1
    g = ad.grad.double().cpu()
    ref, m1, v1 = O.adamw_step(params0.double().cpu(), g, torch.zeros_like(g), torch.zeros_like(g), 1, LR, weight_decay=0.01)
    tol = 2.0 ** -20 * LR + 2.0 ** -23 * ref.abs()     # ~12 fp32 roundings on the update (<= lr at step 1), 2 on the parameter
    assert ((ad.params.double().cpu() - ref).abs() <= tol).all()
    assert ((ad.exp_avg.double().cpu() - m1).abs() <= 2.0 ** -20 * m1.abs() + 1e-30).all()   # 1 - 0.9f is 2^-22 off 0.1
    assert (ad.params != params0).any()
    _train(model, opt, d.inputs, dev, 1)
    ckpt = {'opt': opt.state_dict(), 'master': unet.master.clone()}
    assert ckpt['opt']['step'] == 2 and ckpt['opt']['lora']['rank'] == r
    _train(model, opt, d.inputs, dev, 1)
    # the base is frozen: the master and its moments keep their bits, the adapter buffers and the shadows moved
    assert torch.equal(unet.master.view(torch.int32), master0.view(torch.int32))
    assert not unet.exp_avg.any() and not unet.exp_avg_sq.any()
    moved = unet.shadow.view(torch.int16) != shadow0.view(torch.int16)
    own = torch.zeros_like(moved)
    for it in ad.items:
        own[it.w_off:it.w_off + it.N * it.K] = True
    assert moved[own].any() and not moved[~own].any()
    # checkpoint after step 2 -> resume in a fresh model -> step 3 bit for bit
    model2, opt2 = _model(name, r, via_algorithm=True)
    opt2.load_state_dict(ckpt['opt'])
    assert model2.unet.opt_step == 2
    _train(model2, opt2, d.inputs, dev, 1)
    ad2 = model2.unet.lora
    for a, b in ((ad.params, ad2.params), (ad.exp_avg, ad2.exp_avg), (ad.exp_avg_sq, ad2.exp_avg_sq)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(unet.shadow.view(torch.int16), model2.unet.shadow.view(torch.int16))
    assert torch.equal(unet.shadow_t.view(torch.int16), model2.unet.shadow_t.view(torch.int16))
    # a checkpoint with adapter state does not load into an optimizer without adapters, nor the other way round
    model2.unet.remove_lora()
    assert torch.equal(model2.unet.master.view(torch.int32), master0.view(torch.int32))
    cast = torch.empty_like(shadow0)
    from diffusion_amd import ops
    ops.cast_f32_bf16(master0, cast)
    assert torch.equal(model2.unet.shadow.view(torch.int16), cast.view(torch.int16))     # remove_lora: bf16(master) again


def test_clipping_measures_the_adapter_gradient(dev):
    name, r = SEQ
    d = lr.case_data(name, r)
    model, opt = _model(name, r)
    opt.clip_max_norm, opt.guard_nonfinite = 0.05, True
    ad = model.unet.lora
    params0 = ad.params.clone()
    seen = {}

    def hook(i):
        opt.compute_grad_stats()          # the monitor's pass: projects, measures; step() reuses the record
        seen['stats'] = opt.last_grad_stats()
        seen['norm64'] = ad.grad.double().norm().item()
        seen['segs'] = opt.last_segment_norms()
    _train(model, opt, d.inputs, dev, 1, hook)
    s = seen['stats']
    assert s['finite'] and abs(s['norm'] - seen['norm64']) <= 1e-6 * seen['norm64'], (s, seen['norm64'])
    assert s['norm'] > 0.05 and abs(s['grad_mult'] - 0.05 / (seen['norm64'] + 1e-6)) <= 1e-5 * s['grad_mult']
    names = ad.segments()[0]
    assert set(seen['segs']) == set(names) | {'global'} and all(seen['segs'][n] > 0 for n in names)
    it = ad.items[0]
    assert abs(seen['segs'][names[0]] - ad.A(it, ad.grad).double().norm().item()) <= 1e-5 * seen['segs'][names[0]]
    # the clipped update: AdamW on grad_mult * g
    O = ws.oracle()
    g = ad.grad.double().cpu() * s['grad_mult']
    ref, _, _ = O.adamw_step(params0.double().cpu(), g, torch.zeros_like(g), torch.zeros_like(g), 1, LR, weight_decay=0.01)
    assert ((ad.params.double().cpu() - ref).abs() <= 2.0 ** -20 * LR + 2.0 ** -23 * ref.abs()).all()


def test_trainer_with_the_algorithm_runs_eagerly_and_refuses_ema(dev):
    """The YAML route: Trainer(algorithms=[LoRA]) attaches the adapters and switches the optimizer; with use_graphs the step
    runs eagerly (a captured microbatch would replay the skipped weight gradients); EMA is a ValueError."""
    from diffusion_amd.algorithms.ema import EMA
    from diffusion_amd.algorithms.lora import LoRA
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.optim import FusedAdamW
    from diffusion_amd.trainer import Trainer
    model = stable_diffusion_2(model_name='tiny', pretrained=False, precomputed_latents=True, fsdp=False)
    unet = model.unet
    opt = FusedAdamW(unet=unet, lr=LR, weight_decay=0.01)
    ema = EMA(half_life=None, smoothing=0.99)
    with pytest.raises(ValueError, match='EMA'):
        Trainer(model, None, optimizers=opt, max_duration='1ba', algorithms=[ema, LoRA(rank=4)])
    assert unet.lora is not None and opt.lora is unet.lora      # the algorithm had attached them before the check
    tr = Trainer(model, None, optimizers=opt, max_duration='2ba', device_train_microbatch_size=2, use_graphs=True,
                 algorithms=[LoRA(rank=4)])
    assert tr.sliced_optimizer is False
    g = torch.Generator().manual_seed(3)
    batch = {'image_latents': torch.randn(4, 4, 16, 16, generator=g).half().to(dev),
             'caption_latents': torch.randn(4, 77, 128, generator=g).half().to(dev)}
    master0, params0 = unet.master.clone(), unet.lora.params.clone()
    losses = [float(tr.train_batch(batch)) for _ in range(2)]
    torch.cuda.synchronize()
    assert all(math.isfinite(x) for x in losses) and unet.opt_step == 2
    assert tr._graph_cache is None or not tr._graph_cache.graphs            # declined: nothing was captured
    assert torch.equal(unet.master, master0) and not torch.equal(unet.lora.params, params0)
    b_moved = [unet.lora.B(it).abs().max().item() > 0 for it in unet.lora.items]
    assert all(b_moved)                                                     # B = 0 at the start: every adapter got a gradient
