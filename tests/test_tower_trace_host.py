"""The tower-trace checker proved on the CPU (tests/tower_trace.py; the GPU cases are in test_tower_trace_gpu.py).

  * the float64 walks equal ``transformers.CLIPTextModel`` / ``models/vae.AutoencoderKL`` run in float64 (rel-L2 <= 1e-10):
    the expected launch table IS the module;
  * every stress is a property of the float64 reference: attention-logit standard deviation 2 +- 0.5 with a mean largest
    softmax probability >= 0.3, fc1 pre-activations of standard deviation 0.5 ... 2, first-GroupNorm group variances of
    1e-7 ... 1e-5 in the low-variance case, LayerNorm row variances of the order of eps where eps = 1e-3;
  * the emulation of our number format (bf16 weights and launch outputs, float64 maths) passes every per-launch check of every
    case: the imported bounds leave room for the number format itself;
  * every entry of ``MUTATIONS`` is caught: the first failed check of the mutated emulation is at the launch the entry names,
    its numeric check there (where the slip leaves the launch's operation applicable) fails by >= 2 x the bound;
  * ``CAPS`` (the GPU tests' cap on the final output) is at most half the smallest whole-output effect of the case's
    mutations, and the emulation alone stays below it, over the whole tensor and per image / sequence.
With DA_PARITY_MARGINS set, the effect of every mutation on the final output at the EXISTING tower tests' weights
(test_text_hip_gpu.py, test_vae_hip_gpu.py, test_vae_decoder_hip_gpu.py: default init, norm affines + 0.1 N(0, 1)) is
recorded next to those tests' bounds ("Tower traces"); nothing is asserted on it.
"""
import os

import pytest
import torch

import tower_trace as T
from parity_margins import record

CASE_NAMES = list(T.CASES)
PAIRS = [(m, c) for m, e in T.MUTATIONS.items() for c in e['cases']]


@pytest.fixture(scope='module', autouse=True)
def threads():
    old = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    yield
    torch.set_num_threads(old)


@pytest.mark.parametrize('case', CASE_NAMES)
def test_float64_walk_equals_the_torch_module(case):
    import copy
    d = T.case_data(case)
    m, x = copy.deepcopy(d['module']).double(), d['x']
    with torch.no_grad():
        if d['tower'] == 'text':
            ref = m(x)[0]
        elif d['tower'] == 'enc':
            ref = m.quant_conv(m.encoder(x.double()))
        else:
            ref = m.decode(x.double()).sample
    assert d['ref'].shape == ref.shape
    e = T.rel_l2(d['ref'], ref)
    print(f'{case}: float64 walk against the torch module {e:.3e}, {len(d["rows"])} launches')
    assert e <= 1e-10, e


@pytest.mark.parametrize('case', CASE_NAMES)
def test_stress_is_what_it_claims(case):
    d = T.case_data(case)
    std, maxp, per = T.attention_figures(d['ref_trace'])
    print(f'{case}: logit std {std:.3f}, mean max softmax {maxp:.3f}, per launch {per}')
    assert 1.5 <= std <= 2.5, std
    assert maxp >= 0.3, maxp
    for e, r in zip(d['ref_trace'], d['rows']):
        if r['key'].endswith('mlp.fc1'):
            s = e['out'].std().item()
            print(f'  {r["key"]}: pre-activation std {s:.3f}')
            assert 0.5 <= s <= 2, (r['key'], s)
    if case == 'enc-lowvar':
        e = d['ref_trace'][1]
        assert e['kind'] == 'groupnorm_fwd' and d['module'].encoder.conv_in.bias.abs().max() == 0
        s = e['s']
        v = e['ins']['X'].reshape(s['B'], s['HW'], s['G'], -1).var((1, 3), unbiased=False)
        print(f'  first GroupNorm group variances {v.min().item():.3e} ... {v.max().item():.3e}')
        assert 1e-7 <= v.min() and v.max() <= 1e-5
        # eps 1e-5 for 1e-6 there: sqrt((v + 1e-5) / (v + 1e-6)) - 1 = 25 % ... 60 % of every normalised value
        ratio = ((v + 1e-5) / (v + 1e-6)).sqrt() - 1
        assert 0.25 <= ratio.min() and ratio.max() <= 2.2
    if case.startswith('text-l14'):
        e = d['ref_trace'][0]
        eps = d['module'].config.layer_norm_eps
        v = e['ins']['X'].var(1, unbiased=False)
        print(f'  first LayerNorm row variances {v.min().item():.3e} ... {v.max().item():.3e}, eps {eps}')
        assert eps == 1e-3 and e['s']['eps'] == 1e-3 and eps / 10 <= v.min() and v.max() <= 10 * eps


@pytest.mark.parametrize('case', CASE_NAMES)
def test_emulation_passes_every_launch_check(case):
    d = T.case_data(case)
    fails, worst = T.check_trace(d['emu_trace'], d['rows'], d['x0k'])
    print(f'{case}: emulation worst per kind {worst}')
    T.assert_clean(fails, case)
    assert set(worst) == {r['kind'] for r in d['rows']}   # every launch kind was compared


@pytest.fixture(scope='module')
def mutated():
    """{(mutation, case): (failures up to the named launch, its index, whole-output effect, per-item effects)}, once"""
    out = {}
    for name, case in PAIRS:
        d = T.case_data(case)
        at = T._find(d['rows'], T.MUTATIONS[name]['at'])
        trace, final = T.WALKS[d['tower']](d['module'], d['x'], fmt='bf16', mutate=name)
        fails, _ = T.check_trace(trace, d['rows'], d['x0k'], upto=at + 1)
        _, exact = T.WALKS[d['tower']](d['module'], d['x'], mutate=name)   # the slip alone, without the number format
        out[name, case] = (fails, at, T.rel_l2(exact, d['ref']), T.per_item(exact, d['ref']))
    return out


@pytest.mark.parametrize('name,case', PAIRS, ids=[f'{m}@{c}' for m, c in PAIRS])
def test_mutation_is_caught_at_its_launch(mutated, name, case):
    fails, at, effect, items = mutated[name, case]
    d = T.case_data(case)
    assert fails, f'{name} on {case}: not caught'
    here = [f for f in fails if f['launch'] == at]
    print(f'{name} on {case}: launch {at} ({d["rows"][at]["kind"]}, {d["rows"][at]["key"]}): '
          f'{sorted({f["check"] for f in here})}; whole-output effect {effect:.3e}')
    for f in here:
        print('   ', f['msg'])
    assert fails[0]['launch'] == at and here, f'{name} on {case}: first failure {fails[0]["msg"]}, expected at launch {at}'
    numeric = [f for f in here if f['check'] == 'numerics' and f['value'] is not None]
    for f in numeric:
        assert f['value'] >= 2 * f['bound'], f'{name} on {case}: numeric failure by less than 2 x the bound: {f["msg"]}'
    if all(f['check'] == 'numerics' for f in here):
        assert numeric, f'{name} on {case}: {here[0]["msg"]}'
    if T.MUTATIONS[name].get('numeric'):
        assert numeric, f'{name} on {case}: the numeric check at launch {at} did not fail'


@pytest.mark.parametrize('case', CASE_NAMES)
def test_caps_separate_emulation_from_mutations(mutated, case):
    d = T.case_data(case)
    for (m, c), v in mutated.items():
        if c == case and T.MUTATIONS[m].get('whole') is False:
            print(f'{case}: {m} moves the whole output by {v[2]:.3e} (left out of the cap: see MUTATIONS)')
    effects = {m: mutated[m, c] for (m, c) in mutated if c == case and T.MUTATIONS[m].get('whole') is not False}
    assert effects, f'{case}: no mutation is shown on it'
    weakest = min(effects, key=lambda m: min([effects[m][2]] + effects[m][3]))
    smallest = min([effects[weakest][2]] + effects[weakest][3])
    worst_item = max(T.per_item(d['emu'], d['ref']))
    print(f'{case}: cap {T.CAPS[case]:.3e}; emulation {d["e_emul"]:.3e} (worst item {worst_item:.3e}); smallest mutation effect '
          f'{smallest:.3e} ({weakest})')
    assert T.CAPS[case] <= 0.5 * smallest, (weakest, smallest)
    assert d['e_emul'] < T.CAPS[case] and worst_item < T.CAPS[case]
    assert 1.5 * d['e_emul'] < T.CAPS[case]   # the calibrated bound of the GPU test is the tighter of the two


def test_record_mutation_effects_at_the_existing_tests_weights():
    """Not an assertion: with DA_PARITY_MARGINS set, what each slip does to the ONE number the existing tower tests assert,
    at their weights (default init, norm affines + 0.1 N(0, 1)) and this suite's shapes."""
    if not os.environ.get('DA_PARITY_MARGINS'):
        return
    from diffusion_amd.models.text import build_clip_text_encoder, build_text_encoder
    from diffusion_amd.models.vae import AutoencoderKL

    def plain(m):
        with torch.no_grad():
            for n, p in m.named_parameters():
                if 'norm' in n:
                    p.add_(0.1 * torch.randn_like(p))
        return m.eval().requires_grad_(False)

    torch.manual_seed(7)
    vae = plain(AutoencoderKL())
    torch.manual_seed(130)
    sd2 = plain(build_text_encoder(None, torch.float32, num_hidden_layers=3, hidden_size=128))
    l14 = plain(build_clip_text_encoder(hidden_size=128, num_attention_heads=2, intermediate_size=512, num_hidden_layers=2,
                                        layer_norm_eps=1e-3))
    existing_bound = {'text': 2e-2, 'enc': 2e-2, 'dec': 8e-2}
    for name, case in PAIRS:
        tower, kw = T.CASES[case][:2]
        if kw.get('block_out_channels') or kw.get('hidden_size') == 96:
            continue   # widths the existing tests do not build
        m = vae if tower != 'text' else (sd2 if kw['kind'] == 'sd2' else l14)
        x = T.case_input(case)
        if kw.get('lowvar'):
            x = x / T.LOWVAR_IMAGE_SCALE
        _, ref = T.WALKS[tower](m, x)
        _, mut = T.WALKS[tower](m, x, mutate=name)
        record('tower_trace_existing_weights', tolerances=existing_bound, **{f'{name}@{case}': T.rel_l2(mut, ref)})
