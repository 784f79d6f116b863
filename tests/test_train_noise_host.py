"""CPU-only tests of the per-sample training noise: the package's Philox and seed derivation against the NumPy reference, the
invariance of seeds and slots to the world and microbatch split, the integer timestep formulas, option validation, and the YAML
route to the factories."""
import inspect
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_reference as PR  # noqa: E402
import train_noise_reference as TR  # noqa: E402

from diffusion_amd import train_noise as TN  # noqa: E402
from diffusion_amd.train_noise import TrainNoise  # noqa: E402


def test_philox_matches_known_answers_and_reference():
    for counter, key, want in PR.KAT:
        assert TN.philox4x32_10(counter, key) == want
    for counter, key in (((1, 2, 3, 4), (5, 6)), ((7, 0, 2**32 - 1, 0x7472616e), (0xdeadbeef, 17))):
        assert TN.philox4x32_10(counter, key) == tuple(int(w) for w in PR.philox4x32_10(counter, key))


def test_train_noise_does_not_import_tests():
    src = inspect.getsource(TN)
    assert 'philox_reference' not in src and 'import tests' not in src and 'from tests' not in src


@pytest.mark.parametrize('run_seed,batch_idx', [(0, 0), (17, 3), (2**64 - 1, 2**40 + 5)])
def test_sample_seeds_match_reference(run_seed, batch_idx):
    got = TN.sample_seeds(run_seed, batch_idx, 3, 5)
    assert got == TR.sample_seeds(run_seed, batch_idx, 3, 5)
    assert all(0 <= s < 2**64 for s in got) and len(set(got)) == 5


def test_seeds_and_slots_do_not_depend_on_world_or_microbatch():
    """world 1 x batch 8 == world 2 x batch 4 == world 4 x batch 2, position by position; slots are 0..7 in each case"""
    whole = TN.sample_seeds(17, 5, 0, 8)
    for world in (1, 2, 4):
        n = 8 // world
        seeds, slots = [], []
        for rank in range(world):
            seeds += TN.sample_seeds(17, 5, rank * n, n)
            slots += list(range(rank * n, rank * n + n))
        assert seeds == whole and slots == list(range(8))
    assert TN.sample_seeds(17, 6, 0, 8) != whole and TN.sample_seeds(18, 5, 0, 8) != whole
    # a microbatch is a slice of the rank's entries
    assert TN.sample_seeds(17, 5, 0, 8)[2:6] == TN.sample_seeds(17, 5, 2, 4)


R0S = (0, 1, 2**31, 2**32 - 1)


@pytest.mark.parametrize('R,n_slots', [(1000, 1), (1000, 7), (1000, 2048), (1, 5), (3, 8)])
def test_integer_timesteps_stay_in_range_and_stratum(R, n_slots):
    for t_lo in (0, 13):
        t_hi = t_lo + R
        for r0 in R0S:
            t = TN.discrete_timestep(r0, t_lo, t_hi)
            assert t == TR.discrete_t(r0, t_lo, t_hi) and t_lo <= t < t_hi
            for slot in sorted({0, 1 % n_slots, n_slots // 2, n_slots - 1}):
                ts = TN.discrete_timestep(r0, t_lo, t_hi, slot, n_slots)
                assert ts == TR.discrete_t(r0, t_lo, t_hi, slot, n_slots)
                lo, hi = TR.stratum(t_lo, t_hi, slot, n_slots)
                assert t_lo <= lo <= ts < hi <= t_hi, (ts, lo, hi)
                # the kernel's form of the same floor: shift by 32 first, then a 32-bit division
                assert ts == t_lo + ((((slot << 32) | r0) * R) >> 32) // n_slots
        if R == 1:
            assert all(TN.discrete_timestep(r0, t_lo, t_hi, s, n_slots) == t_lo for r0 in R0S for s in range(n_slots))


def test_option_validation():
    assert not TrainNoise().philox and TrainNoise(noise_source='philox').philox
    for kw in (dict(noise_offset=0.1), dict(input_perturbation=0.1), dict(timestep_range=(0, 500)),
               dict(timestep_sampling='stratified')):
        with pytest.raises(ValueError, match='philox'):
            TrainNoise(**kw)
        TrainNoise(noise_source='philox', **kw)
    for bad in (-0.1, float('nan'), float('inf'), '0.1', True):
        with pytest.raises(ValueError):
            TrainNoise(noise_source='philox', noise_offset=bad)
        with pytest.raises(ValueError):
            TrainNoise(noise_source='philox', input_perturbation=bad)
    for bad in ((5, 5), (7, 3), (-1, 4), (0,), 'ab0', (0, float('nan'))):
        with pytest.raises(ValueError):
            TrainNoise(noise_source='philox', timestep_range=bad)
    with pytest.raises(ValueError):
        TrainNoise(noise_source='philox', timestep_range=(0, 1001)).discrete_range(1000)
    with pytest.raises(ValueError):
        TrainNoise(noise_source='philox', timestep_range=(0.5, 10.5)).discrete_range(1000)
    with pytest.raises(ValueError):
        TrainNoise(noise_source='philox', timestep_range=(0.0, 1.5)).continuous_range(1.57)
    assert TrainNoise(noise_source='philox', timestep_range=(999, 1000)).discrete_range(1000) == (999, 1000)
    assert TrainNoise(noise_source='philox').discrete_range(1000) == (0, 1000)
    with pytest.raises(ValueError):
        TrainNoise(noise_source='philox', timestep_sampling='sobol')
    with pytest.raises(ValueError):
        TrainNoise(noise_source='cuda')
    with pytest.raises(ValueError, match='philox'):
        TN.check_injected(TrainNoise(noise_source='philox'), object())
    TN.check_injected(TrainNoise(), object())
    TN.check_injected(TrainNoise(noise_source='philox'), None)


FACTORIES = ('stable_diffusion_2', 'discrete_pixel_diffusion', 'continuous_pixel_diffusion')


@pytest.mark.parametrize('factory', FACTORIES)
def test_factories_refuse_bad_options_before_the_device(factory):
    from diffusion_amd.models import models
    f = getattr(models, factory)
    for kw in (dict(noise_offset=0.1), dict(noise_source='philox', noise_offset=-1.0),
               dict(noise_source='philox', timestep_sampling='sobol'), dict(noise_source='philox', timestep_range=[0, 1001]),
               dict(noise_source='philox', timestep_range=[4, 4])):
        with pytest.raises(ValueError):
            f(**kw)


@pytest.mark.parametrize('factory', FACTORIES)
def test_yaml_keys_reach_the_factory(tmp_path, factory):
    from diffusion_amd import hydra_lite
    frac = factory == 'continuous_pixel_diffusion'
    p = tmp_path / 'cfg.yaml'
    p.write_text(f'''
model:
  _target_: diffusion.models.models.{factory}
  _partial_: true
  noise_source: philox
  noise_offset: 0.1
  input_perturbation: 0.05
  timestep_range: {'[0.25, 1.0]' if frac else '[20, 980]'}
  timestep_sampling: stratified
bad:
  _target_: diffusion.models.models.{factory}
  noise_source: torch
  timestep_sampling: stratified
''')
    cfg = hydra_lite.load_config(str(p), ['model.noise_offset=0.2'])
    part = hydra_lite.instantiate(cfg.model)
    assert part.func.__name__ == factory
    kw = part.keywords
    assert set(kw) <= set(inspect.signature(part.func).parameters)
    assert (kw['noise_source'], kw['noise_offset'], kw['input_perturbation'], kw['timestep_sampling']) == \
        ('philox', 0.2, 0.05, 'stratified')
    from diffusion_amd.models.models import _train_noise_options
    tn = _train_noise_options(kw['noise_source'], kw['noise_offset'], kw['input_perturbation'], kw['timestep_range'],
                              kw['timestep_sampling'])
    assert tn.timestep_range == ((0.25, 1.0) if frac else (20, 980)) and tn.stratified
    with pytest.raises(ValueError, match='philox'):   # the call itself: refused by the factory before any device is looked for
        hydra_lite.instantiate(cfg.bad)
