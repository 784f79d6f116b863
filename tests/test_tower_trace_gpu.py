"""The frozen towers launch by launch on the MI355X: ``TextEncoderHIP``, ``VAEEncoderHIP`` and ``VAEDecoderHIP`` run under the
recorder of tests/tower_trace.py at stressed weights, and every launch is held against the table built from the torch module.

Per case (``tower_trace.CASES``; the stresses, the table and the bounds are proved on the CPU by test_tower_trace_host.py):
  * sequence, flow, parameters and numerics of every launch (``check_trace``): the kinds in order (the wide kernel for the
    512-wide head, the causal kernel for the text tower, quick-GELU only where the config says so, torch SDPA only in the two
    fallbacks), each data input the very tensor an earlier launch wrote, each weight / affine / eps / scale / Geom the module's,
    each output within the kernel suite's own bound of the float64 operation on the launch's recorded inputs;
  * the value the tower returns is the last launch's output, bit for bit, in the module's layout;
  * final output against the float64 walk with fp32 weights: e_hip <= 1.5 x e_emul (the bf16 emulation of the same walk,
    computed here) and e_hip < ``CAPS[case]`` over the whole tensor and per image / sequence;
  * a second run gives a bit-identical final output and an identical launch sequence.
DA_PARITY_MARGINS=<path> writes each case's worst per-launch value by kind and its e_hip / e_emul pair
(tests/parity_margins.py; profiles/tower_trace_margins.json holds the MI355X run).
"""
import pytest
import torch

import tower_trace as T
from parity_margins import record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops(dev):
    from diffusion_amd import ops as o
    return o


def build(case, dev):
    """the HIP tower of a case and the call that runs it on the case's input"""
    import copy
    from diffusion_amd.models.text_hip import TextEncoderHIP
    from diffusion_amd.models.vae_hip import VAEDecoderHIP, VAEEncoderHIP
    d = T.case_data(case)
    m = copy.deepcopy(d['module']).to(dev)
    x = d['x'].to(dev)
    if d['tower'] == 'text':
        hip = TextEncoderHIP(m, device=dev)
        return lambda: hip(x)[0]
    if d['tower'] == 'enc':
        hip = VAEEncoderHIP(m, device=dev)
        return lambda: hip.moments(x)
    hip = VAEDecoderHIP(m, device=dev)
    return lambda: hip.decode(x).sample


def run_recorded(ops, call):
    from diffusion_amd.models import text_hip, vae_hip
    with T.recording(ops, (text_hip, vae_hip)) as trace:
        out = call()
        torch.cuda.synchronize()
    return trace, out


@pytest.mark.parametrize('case', list(T.CASES))
def test_tower_launch_by_launch(dev, ops, case):
    d = T.case_data(case)
    call = build(case, dev)
    trace, out = run_recorded(ops, call)
    fails, worst = T.check_trace(trace, d['rows'], d['x0k'], native=True)
    final = out.detach().float().cpu()
    e_hip, e_emul = T.rel_l2(final, d['ref']), d['e_emul']
    items = T.per_item(final, d['ref'])
    print(f'{case}: {len(trace)} launches, worst per kind {worst}; e_hip {e_hip:.3e} (worst item {max(items):.3e}), '
          f'e_emul {e_emul:.3e}')
    record('tower_trace_' + case, tolerances={**T.NUMERIC_BOUNDS, 'e_hip_over_e_emul': 1.5, 'e_hip': T.CAPS[case]},
           e_hip=e_hip, e_emul=e_emul, e_hip_worst_item=max(items), **{'launch.' + k: v for k, v in worst.items()})
    T.assert_clean(fails, case)
    assert out.dtype == torch.float32 and final.shape == d['ref'].shape
    assert torch.equal(final, d['finish'](trace[-1]['out'].float().cpu())), 'the returned tensor is not the last launch\'s output'
    assert e_hip <= 1.5 * e_emul, (e_hip, e_emul)
    assert e_hip < T.CAPS[case] and max(items) < T.CAPS[case], (e_hip, items, T.CAPS[case])
    trace2, out2 = run_recorded(ops, call)
    assert torch.equal(out2, out), 'a second run of the same input differs'
    assert [(e['kind'], e['s']) for e in trace2] == [(e['kind'], e['s']) for e in trace], 'the launch sequence changed'


def test_text_tower_takes_one_unbatched_sequence(dev, ops):
    """``ids.dim() == 1``: one sequence, the same launches and bits as the batch of one"""
    import copy
    from diffusion_amd.models.text_hip import TextEncoderHIP
    d = T.case_data('text-l14-t33')
    hip = TextEncoderHIP(copy.deepcopy(d['module']).to(dev), device=dev)
    ids = d['x'][0].to(dev)
    a, b = hip(ids)[0], hip(ids[None])[0]
    assert a.shape == (1, ids.numel(), d['module'].config.hidden_size) and torch.equal(a, b)
