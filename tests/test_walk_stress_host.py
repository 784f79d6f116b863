"""The power of test_walk_stress_gpu.py as a tested property, on the CPU (tests/walk_stress.py holds the shared pieces).

  * the stressed setup is what it claims: 49,997,380 parameters, fused GEGLU at the C = 320 levels, every norm with a gamma
    that is not 1 and a beta that is not 0, attention logits with a standard deviation of 1.2 ... 1.9 in every block;
  * the oracle under our number format (``emulate_bf16``) stays inside every entry of ``BOUNDS`` on each GPU case: the
    bounds leave room for the reference alone;
  * each entry of ``MUTATIONS`` - a wiring slip of the walk, applied to the fp64 oracle - breaks at least one entry of
    ``BOUNDS`` on the square case, on a gradient tensor the slip does not name.  Loosening a bound until such a slip passes
    fails here, without a GPU.

What the same slips look like to the figures test_unet_parity_gpu.py asserts (tiny width, ``init_state_dict`` weights, the
inputs of test_tiny_train_step_parity, fp64 oracle against itself; recorded, not asserted - this is the gap the stressed
weights close).  TOL_TINY: prediction 0.023, global gradient 0.040, worst matrix cosine 0.9957, vector gradients 0.023.

  slip at default weights                          pred rel-L2  global grad  worst cosine  vectors  worst tensor  caught
  cross-attention scale x 1.1                      0.0031       0.0059       0.99895       0.0033   0.12          no
  self-attention scale x 1.1                       0.0041       0.0088       0.99939       0.0052   0.11          no
  one GroupNorm's gamma taken as 1                 0            0            1             0        0             no
  one LayerNorm's beta taken as 0                  0            0            1             0        0             no
  two GroupNorm gammas swapped                     0            0            1             0        0             no
  the 2-head level run as one head of width 128    0.0203       0.0569       0.641         0.0281   1.31          yes
  transformer GroupNorm fed the next norm1 affine  0            0            1             0        0             no

(The four affine slips are bit-identical to the correct step there: every gamma is 1 and every beta 0.  "worst tensor" is the
per-tensor rel-L2 that test_unet_parity_gpu.py records but does not assert; the gradient tensors a slip names itself,
``MUTATION_OWN``, are left out as they are below.)  At the stressed weights every one of the seven breaks ``tensor_rel``.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import walk_stress as ws  # noqa: E402


def test_stress_config_and_weights():
    from diffusion_amd import ops
    O = ws.oracle()
    ocfg, cfg = ws.stress_config('oracle'), ws.stress_config('hip')
    cfg.validate()
    assert O.param_count(ocfg) == ws.STRESS_PARAMS
    for f in ('block_out_channels', 'attention_head_dim', 'cross_attention_dim', 'prediction_type'):
        assert getattr(ocfg, f) == getattr(cfg, f)
    assert ws.stress_config('oracle', 'tiny') == O.UNetConfig.tiny()
    assert [ops.geglu_fusable(4 * c, c) and ops.geglu_bwd_fusable(4 * c, c) for c in cfg.block_out_channels] == \
        [False, False, True, True]
    sd, base = ws.state_dict64('stress'), O.init_state_dict(ocfg, ws.SEED, dtype=torch.float64)
    assert list(sd) == [k for k, _ in O.param_manifest(ocfg)]
    norms = [k for k in sd if ws.is_norm_key(k)]
    assert len(norms) == 2 * (22 * 2 + 16 * 4 + 1)
    for k, v in sd.items():
        assert v.dtype == torch.float64 and v.shape == base[k].shape
        if k in norms:
            centre, half = (1.0, 0.5) if k.endswith('.weight') else (0.0, 0.3)
            assert ((v - centre).abs() <= half).all() and (v != centre).all(), k
            assert (v - centre).abs().mean() > 0.3 * half, k       # U(-1, 1) has mean |u| = 0.5: the vector carries weight
        elif k.endswith(('.to_q.weight', '.to_k.weight')):
            assert torch.equal(v, base[k] * 2), k
        else:
            assert torch.equal(v, base[k]), k


def test_attention_logits_are_sharp_but_not_saturated():
    """Standard deviation of the scaled logits per attention call of the fp64 oracle on the square case: 1.2 ... 1.9
    everywhere (default weights: 0.31 ... 0.35).  Above about 3 bf16 noise alone breaks any usable gradient bound."""
    O = ws.oracle()
    d = ws.case_data(ws.SQUARE_CASE)
    latents, ctx, noise, t = d['inputs']
    stds = {}
    lin = O._lin

    def _lin(x, sd, p, bias=True):
        y = lin(x, sd, p, bias=bias)
        if p.endswith(('.to_q', '.to_k')):
            stds.setdefault(p.rsplit('.', 1)[0], []).append(y)
        return y

    heads = {}
    attention = O.attention

    def att(x, c, sd, p, h):
        heads[p] = h
        return attention(x, c, sd, p, h)

    with ws.patched(O, _lin=_lin, attention=att), torch.no_grad():
        O.training_forward(d['sd'], d['cfg'], latents.double(), t, ctx.double(), noise.double())
    assert len(stds) == 32
    out = {}
    for p, (q, k) in stds.items():
        b, h = q.shape[0], heads[p]
        sp = lambda z: z.reshape(b, -1, h, 64).permute(0, 2, 1, 3)
        out[p] = (sp(q) @ sp(k).transpose(-1, -2) * 0.125).std().item()
    lo, hi = min(out, key=out.get), max(out, key=out.get)
    print(f'\nlogit standard deviation: {out[lo]:.3f} ({lo}) ... {out[hi]:.3f} ({hi})')
    assert 1.2 <= out[lo] and out[hi] <= 1.9, (lo, out[lo], hi, out[hi])


@pytest.mark.parametrize('name', list(ws.CASES))
def test_emulation_stays_inside_the_bounds(name):
    d = ws.case_data(name)
    assert all(g.norm() > 0 for g in d['grads'].values())
    s = ws.summary(d['emu'])
    print(f'\n{name}: {s}')
    assert ws.violations(d['emu']) == []


@pytest.mark.parametrize('mutation', list(ws.MUTATIONS))
def test_mutation_breaks_a_bound(mutation):
    O = ws.oracle()
    d = ws.case_data(ws.SQUARE_CASE)
    latents, ctx, noise, t = d['inputs']
    loss, pred, grads = ws.oracle_step(O, d['sd'], d['cfg'], latents.double(), t, ctx.double(), noise.double(), mutation)
    m = ws.metrics(pred, grads, d['pred'], d['grads'], loss, d['loss'], exclude=ws.MUTATION_OWN.get(mutation, ()))
    bad = ws.violations(m)
    print(f'\n{mutation}: ' + ('breaks nothing' if not bad else '; '.join(
        f'{key} {val:.4g} against {bound:g} ({val / bound if key != "matrix_cos" else (1 - val) / (1 - bound):.1f} x'
        + (f', {k}' if k else '') + ')' for key, val, bound, k in bad)))
    assert bad, ws.summary(m)
    assert any(key == 'tensor_rel' for key, *_ in bad), 'the per-tensor bound is the one meant to catch every slip'
    # the patches are gone again
    assert O.attention.__module__ == O.__name__ and O._gn.__module__ == O.__name__
