"""CPU-only tests of metrics/inception_score.py, metrics/kid.py and what they stand on: the two host float64 functions against
the NumPy restatement (tests/inception_metrics_reference.py) within 1e-12, the hydra targets, constructor validation, the
trainer's log entries for (mean, std) metrics, the random head, the unchanged random tower, the state-dict check with
``fc.weight``, the "MI355X only" error, and ``gather_rows`` under gloo with unequal counts."""
import copy
import os
import socket
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import inception_metrics_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(got, want, tol=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.all(np.abs(got - want) <= tol * np.maximum(np.abs(want), 1e-300)), (got, want)


@pytest.mark.parametrize('N,C,splits,scale', [(23, 1008, 10, 3.0), (5, 8, 10, 1.0), (64, 100, 1, 80.0), (40, 16, 4, 5.0)])
def test_inception_score_from_logits_against_numpy(N, C, splits, scale):
    from diffusion_amd.metrics.inception_score import inception_score_from_logits, inception_scores_per_split
    rng = np.random.default_rng(N)
    logits = (rng.normal(0, scale, (N, C))).astype(np.float32)
    perm = rng.permutation(N)
    want = R.inception_scores(logits, perm, splits)
    assert len(want) == len(R.chunk_bounds(N, splits)) == -(-N // -(-N // splits))
    _close(inception_scores_per_split(torch.from_numpy(logits), torch.from_numpy(perm), splits), want)
    mean, std = inception_score_from_logits(torch.from_numpy(logits), torch.from_numpy(perm).to(torch.int32), splits)
    wm, ws = R.inception_score(logits, perm, splits)
    _close(mean, wm)
    if len(want) == 1:   # torch.std of one chunk is NaN, and so is the unbiased convention here
        assert np.isnan(float(std)) and np.isnan(ws)
    else:
        _close(std, ws)
        assert abs(float(std) - want.std(ddof=0)) > 1e-9 * float(std) or float(std) == 0.0   # unbiased, not the biased one
    if N < splits:   # one row per chunk: p == m, every score is 1
        assert len(want) == N and np.all(np.abs(want - 1.0) <= 1e-15)


def test_inception_score_zero_probabilities_contribute_zero():
    from diffusion_amd.metrics.inception_score import inception_scores_per_split
    logits = np.zeros((4, 6), np.float32)
    logits[:, 0] = [0, 2000, -2000, 5]   # exp underflows to an exact 0 next to these
    perm = np.array([2, 0, 3, 1])
    got = inception_scores_per_split(torch.from_numpy(logits), torch.from_numpy(perm), 2)
    assert torch.isfinite(got).all()
    _close(got, R.inception_scores(logits, perm, 2))


@pytest.mark.parametrize('m,D,degree,gamma,coef', [(2, 8, 3, None, 1.0), (5, 8, 1, 0.37, 0.0), (33, 64, 3, None, 1.0),
                                                   (7, 12, 4, 0.01, 2.5)])
def test_kid_from_features_against_numpy(m, D, degree, gamma, coef):
    from diffusion_amd.metrics.kid import kid_from_features, kid_values
    rng = np.random.default_rng(m)
    fr, ff = rng.normal(0, 1, (m + 4, D)).astype(np.float32), rng.normal(0.2, 1.1, (m + 9, D)).astype(np.float32)
    ir, jf = R.subset_indices(rng, 3, m, m + 4), R.subset_indices(rng, 3, m, m + 9)
    want, scale = R.poly_mmd(fr, ff, ir, jf, degree, gamma, coef)
    got = kid_values(torch.from_numpy(fr), torch.from_numpy(ff), torch.from_numpy(ir), torch.from_numpy(jf), degree, gamma, coef)
    assert np.all(np.abs(got.numpy() - want) <= 1e-12 * scale)
    mean, std = kid_from_features(fr, ff, ir, jf, degree, gamma, coef)
    wm, ws = R.kid(fr, ff, ir, jf, degree, gamma, coef)
    assert abs(float(mean) - wm) <= 1e-12 * scale.max() and abs(float(std) - ws) <= 1e-12 * scale.max()
    assert abs(ws - want.std(ddof=0)) == 0.0 and ws != want.std(ddof=1)   # the biased convention
    if m == 2:   # the diagonal is skipped: only the two mirrored off-diagonal entries of each square block remain
        x, y = fr[ir[0]].astype(np.float64), ff[jf[0]].astype(np.float64)
        k = lambda a, b: (a @ b / D + coef) ** degree
        hand = (2 * k(x[0], x[1]) + 2 * k(y[0], y[1])) / 2 - 2 * sum(k(a, b) for a in x for b in y) / 4
        assert abs(want[0] - hand) <= 1e-12 * scale[0]


def test_hydra_targets_resolve():
    from diffusion_amd import hydra_lite
    from diffusion_amd.metrics.inception_score import InceptionScore
    from diffusion_amd.metrics.kid import KernelInceptionDistance
    assert hydra_lite.resolve_target('torchmetrics.image.inception.InceptionScore') is InceptionScore
    assert hydra_lite.resolve_target('torchmetrics.image.InceptionScore') is InceptionScore
    assert hydra_lite.resolve_target('torchmetrics.image.kid.KernelInceptionDistance') is KernelInceptionDistance
    assert hydra_lite.resolve_target('torchmetrics.image.KernelInceptionDistance') is KernelInceptionDistance
    assert InceptionScore.__name__ == 'InceptionScore' and KernelInceptionDistance.__name__ == 'KernelInceptionDistance'


@pytest.fixture(scope='module')
def metrics():
    from diffusion_amd.metrics.inception_score import InceptionScore
    from diffusion_amd.metrics.kid import KernelInceptionDistance
    with pytest.warns(UserWarning, match='RANDOM-INIT'):
        a = InceptionScore(device='cpu')
    with pytest.warns(UserWarning, match='meaningless'):
        b = KernelInceptionDistance(device='cpu', subsets=2, subset_size=3)
    return a, b


def test_constructor_validation():
    from diffusion_amd.metrics.inception_score import InceptionScore
    from diffusion_amd.metrics.kid import KernelInceptionDistance
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for kw in (dict(feature=2048), dict(feature='logits'), dict(feature=None), dict(splits=0), dict(splits=2.0),
                   dict(splits=True), dict(normalize='yes'), dict(seed=1.5)):
            with pytest.raises(ValueError):
                InceptionScore(device='cpu', **kw)
        for kw in (dict(feature=64), dict(feature='2048'), dict(subsets=0), dict(subsets=1.5), dict(subset_size=0),
                   dict(subset_size=-3), dict(degree=0), dict(degree=2.0), dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=1),
                   dict(coef=-0.5), dict(coef='1'), dict(reset_real_features=1), dict(normalize=None), dict(seed='0')):
            with pytest.raises(ValueError):
                KernelInceptionDistance(device='cpu', **kw)
        k = KernelInceptionDistance(device='cpu', gamma=0.5, coef=0, degree=1)
    assert (k.gamma, k.coef, k.degree, k.subsets, k.subset_size) == (0.5, 0.0, 1, 100, 1000)


def test_argument_errors_come_first_and_there_is_no_cpu_path(metrics):
    score, kid = metrics
    u8 = torch.zeros(2, 3, 8, 8, dtype=torch.uint8)
    for bad in (u8[0], u8[:, :2], u8.float(), [u8]):
        with pytest.raises(ValueError, match='InceptionScore'):
            score.update(bad)
        with pytest.raises(ValueError, match='KernelInceptionDistance'):
            kid.update(bad, real=True)
    with pytest.raises(RuntimeError, match='MI355X only'):
        score.update(u8)
    with pytest.raises(RuntimeError, match='MI355X only'):
        kid.update(u8, real=False)
    assert score.store.n == 0 and kid.stores['real'].n == 0 and kid.stores['fake'].n == 0
    with pytest.raises(ValueError, match='`subset_size` should be smaller than the number of samples'):
        kid.compute()


def test_permutations_are_owned_and_reseeded(metrics):
    score, kid = metrics
    torch.manual_seed(1)
    a, (ir, jf) = score.permutation(50), kid.subset_indices(10, 12)
    torch.manual_seed(2)   # the global generator plays no part
    b, (ir2, jf2) = score.permutation(50), kid.subset_indices(10, 12)
    assert torch.equal(a, b) and torch.equal(ir, ir2) and torch.equal(jf, jf2)
    assert a.dtype == torch.int32 and sorted(a.tolist()) == list(range(50)) and a.tolist() != list(range(50))
    assert ir.shape == jf.shape == (2, 3) and ir.dtype == torch.int32
    assert int(ir.max()) < 10 and int(jf.max()) < 12 and all(len(set(r)) == 3 for r in ir.tolist() + jf.tolist())
    g = torch.Generator().manual_seed(0)   # real first, then fake, per subset
    assert ir[0].tolist() == torch.randperm(10, generator=g)[:3].tolist()
    assert jf[0].tolist() == torch.randperm(12, generator=g)[:3].tolist()
    assert ir[1].tolist() == torch.randperm(10, generator=g)[:3].tolist()


def test_deepcopy_clones_the_state_and_reset_honours_reset_real_features(metrics):
    from diffusion_amd.metrics.kid import KernelInceptionDistance
    score, kid = metrics
    c = copy.deepcopy(kid)
    c.stores['real'].append(torch.ones(70, 2048))   # grows past the first allocation of 64 rows
    c.stores['fake'].append(torch.ones(3, 2048))
    assert (c.stores['real'].n, kid.stores['real'].n) == (70, 0) and c.stores['real'].buf.shape[0] == 128
    assert c.weights_path is kid.weights_path and list(c.parameters()) == []
    cap = c.stores['real'].buf.data_ptr()
    c.reset()
    assert c.stores['real'].n == 0 and c.stores['fake'].n == 0 and c.stores['real'].buf.data_ptr() == cap   # allocation kept
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        keep = KernelInceptionDistance(device='cpu', reset_real_features=False)
    keep.stores['real'].append(torch.ones(2, 2048))
    keep.stores['fake'].append(torch.ones(2, 2048))
    keep.reset()
    assert keep.stores['real'].n == 2 and keep.stores['fake'].n == 0
    s = copy.deepcopy(score)
    s.store.append(torch.zeros(5, 1008))
    assert s.store.n == 5 and score.store.n == 0


def test_metric_log_entries():
    from diffusion_amd.trainer import _metric_log_entries
    assert _metric_log_entries('FID', torch.tensor(3.5, dtype=torch.float64)) == {'metrics/eval/FID': 3.5}
    assert _metric_log_entries('mse', 0.25) == {'metrics/eval/mse': 0.25}
    pair = (torch.tensor(2.0, dtype=torch.float64), torch.tensor(0.5, dtype=torch.float64))
    assert _metric_log_entries('InceptionScore-scale-3p0', pair) == {'metrics/eval/InceptionScore-scale-3p0': 2.0,
                                                                   'metrics/eval/InceptionScore-scale-3p0-std': 0.5}


def test_stable_diffusion_sweeps_both_metrics_over_guidance_scales(metrics):
    from diffusion_amd.models.stable_diffusion import StableDiffusion
    model = StableDiffusion(unet=None, vae=None, text_encoder=None, tokenizer=None, noise_scheduler=None,
                            inference_noise_scheduler=None, val_metrics=[copy.deepcopy(m) for m in metrics],
                            val_guidance_scales=[1.0, 3.0])
    for name in ('InceptionScore', 'KernelInceptionDistance'):
        a, b = (model.val_metrics[f'{name}-scale-{s}'] for s in ('1p0', '3p0'))
        assert (a.guidance_scale, b.guidance_scale) == (1.0, 3.0) and a is not b


def test_random_fc_weight_is_seeded_and_leaves_random_state_dict_alone(tmp_path):
    from diffusion_amd.models.inception_hip import random_fc_weight, random_state_dict
    w = random_fc_weight(0)
    assert tuple(w.shape) == (1008, 2048) and w.dtype == torch.float32
    assert torch.equal(w, random_fc_weight(0)) and not torch.equal(w, random_fc_weight(1))
    assert 0.9 < float(w.std()) * 2048 ** 0.5 < 1.1
    after = random_state_dict(0)
    # the dict of a process in which the fc function is never called
    code = ('import sys, torch; sys.path.insert(0, sys.argv[1]); from diffusion_amd.models.inception_hip import random_state_dict; '
            'torch.save(random_state_dict(0), sys.argv[2])')
    path = str(tmp_path / 'random_state_dict.pt')
    subprocess.run([sys.executable, '-c', code, ROOT, path], check=True, capture_output=True)
    before = torch.load(path, weights_only=True)
    assert list(before) == list(after) and 'fc.weight' not in after
    assert all(torch.equal(before[k], after[k]) for k in before)


def test_check_state_dict_checks_the_shape_of_fc_weight():
    from diffusion_amd.models.inception_hip import check_state_dict, random_fc_weight, random_state_dict
    sd = random_state_dict(0)
    check_state_dict(sd)   # without the head
    sd['fc.weight'], sd['fc.bias'] = random_fc_weight(0), torch.zeros(1008)
    check_state_dict(sd)
    for bad in (torch.zeros(1000, 2048), torch.zeros(2048, 1008), torch.zeros(1008)):
        sd['fc.weight'] = bad
        with pytest.raises(RuntimeError, match='fc.weight'):
            check_state_dict(sd)


def test_wrappers_reject_bad_indices_before_any_device_use():
    """the index checks read the host copies; on this machine reaching the library's launch would fail differently"""
    from diffusion_amd import ops
    x = torch.zeros(4, 8)
    with pytest.raises(TypeError):
        ops.inception_score(x.double(), torch.arange(4, dtype=torch.int32), 2)
    with pytest.raises(TypeError):
        ops.poly_mmd(x.half(), x, torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32))


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def test_gather_rows_gloo_world2_unequal_counts(tmp_path):
    from inception_gather_worker import store_of
    from diffusion_amd.metrics._inception_shared import gather_rows
    st = store_of(1)   # world 1: the [:n] view
    v = gather_rows(st, 5)
    assert v.data_ptr() == st.data_ptr() and tuple(v.shape) == (5, 4)
    counts, port, prefix = (3, 5), _free_port(), str(tmp_path / 'rows')
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE='2')
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, 'tests', 'inception_gather_worker.py'), prefix, '3,5'],
                              env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=120)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    want = torch.cat([store_of(r)[:c] for r, c in enumerate(counts)])
    for r in range(2):
        got = torch.load(f'{prefix}.{r}.pt', weights_only=True)
        assert torch.equal(got, want), (r, got)
