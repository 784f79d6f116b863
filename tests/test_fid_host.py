"""CPU-only tests of metrics/fid.py: ``fid_from_moments`` against closed forms and scipy, and the metric's host logic (hydra
targets, argument errors before any device use, deepcopy, reset_real_features, the guidance-scale sweep).

``fid_from_moments`` takes torchmetrics' state (sum, sum of outer products, n) and evaluates its formula in float64.
  * diagonal covariances at D = 2048: |dmu|^2 + sum (sqrt a - sqrt b)^2;
  * D = 64, SPD pairs with condition <= 1e3: scipy.linalg.sqrtm of Sigma_r Sigma_f.  Rel 1e-6 is what two float64 routes
    should agree to; the sqrtm route is first checked against itself (sqrtm(S)^2 reproduces S to 1e-9 relative, and the
    symmetric form tr sqrtm(A^1/2 B A^1/2) gives the same trace to 1e-8) before it is used as the reference;
  * identical moments: within 1e-6 of 0 (relative to the traces).
Also here, because they need no GPU: the float64 gather of tests/conv_rect_reference.py against F.conv2d, and its case
tables against what tests/test_conv_rect_gpu.py says they cover."""
import copy
import warnings

import numpy as np
import pytest
import torch


def _moments(mu, sigma, n):
    """the state n samples with exactly this mean and (unbiased) covariance would leave: sum = n mu, cov_sum = (n - 1) Sigma +
    n mu mu^T"""
    mu, sigma = np.asarray(mu, np.float64), np.asarray(sigma, np.float64)
    return torch.from_numpy(n * mu), torch.from_numpy((n - 1) * sigma + n * np.outer(mu, mu)), n


def test_fid_from_moments_diagonal_closed_form():
    from diffusion_amd.metrics.fid import fid_from_moments
    rng = np.random.default_rng(0)
    D = 2048
    a, b = rng.uniform(0.1, 4.0, D), rng.uniform(0.1, 4.0, D)
    m1, m2 = rng.normal(0, 1, D), rng.normal(0, 1, D)
    want = np.sum((m1 - m2) ** 2) + np.sum((np.sqrt(a) - np.sqrt(b)) ** 2)
    got = float(fid_from_moments(*_moments(m1, np.diag(a), 1000), *_moments(m2, np.diag(b), 777)))
    assert got == pytest.approx(want, rel=1e-6)


def _spd(rng, D, cond):
    q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    ev = np.exp(rng.uniform(0, np.log(cond), D))
    return (q * ev) @ q.T


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_fid_from_moments_against_scipy_sqrtm(seed):
    from scipy.linalg import sqrtm
    from diffusion_amd.metrics.fid import fid_from_moments
    rng = np.random.default_rng(seed)
    D = 64
    A, B = _spd(rng, D, 1e3), _spd(rng, D, 1e3)
    m1, m2 = rng.normal(0, 1, D), rng.normal(0, 1, D)
    # the reference route is stable first: sqrtm squares back, and the symmetric form gives the same trace
    S = sqrtm(A @ B)
    assert np.linalg.norm(S @ S - A @ B) <= 1e-9 * np.linalg.norm(A @ B)
    rA = sqrtm(A)
    tr_sym = np.trace(sqrtm(rA @ B @ rA)).real
    assert np.trace(S).real == pytest.approx(tr_sym, rel=1e-8)
    want = np.sum((m1 - m2) ** 2) + np.trace(A) + np.trace(B) - 2 * np.trace(S).real
    got = float(fid_from_moments(*_moments(m1, A, 500), *_moments(m2, B, 300)))
    assert got == pytest.approx(want, rel=1e-6)


def test_fid_from_moments_identical_is_zero_and_needs_two_samples():
    from diffusion_amd.metrics.fid import fid_from_moments
    rng = np.random.default_rng(4)
    A, m = _spd(rng, 64, 1e3), rng.normal(0, 1, 64)
    st = _moments(m, A, 100)
    assert abs(float(fid_from_moments(*st, *st))) <= 1e-6 * 2 * np.trace(A)
    one = _moments(m, A, 1)
    with pytest.raises(RuntimeError):
        fid_from_moments(*one, *st)
    with pytest.raises(RuntimeError):
        fid_from_moments(*st, *one)


def test_fid_from_moments_matches_numpy_cov_of_samples():
    from diffusion_amd.metrics.fid import fid_from_moments
    from scipy.linalg import sqrtm
    rng = np.random.default_rng(5)
    X, Y = rng.normal(0, 1, (200, 32)) @ rng.normal(0, 1, (32, 32)), rng.normal(0.3, 1.2, (150, 32))
    sx, sy = np.cov(X, rowvar=False), np.cov(Y, rowvar=False)
    want = np.sum((X.mean(0) - Y.mean(0)) ** 2) + np.trace(sx) + np.trace(sy) - 2 * np.trace(sqrtm(sx @ sy)).real
    got = float(fid_from_moments(torch.from_numpy(X.sum(0)), torch.from_numpy(X.T @ X), len(X), torch.from_numpy(Y.sum(0)),
                                 torch.from_numpy(Y.T @ Y), len(Y)))
    assert got == pytest.approx(want, rel=1e-6)


def test_hydra_targets_resolve():
    from diffusion_amd import hydra_lite
    from diffusion_amd.metrics.fid import FrechetInceptionDistance
    assert hydra_lite.resolve_target('torchmetrics.image.fid.FrechetInceptionDistance') is FrechetInceptionDistance
    assert hydra_lite.resolve_target('torchmetrics.image.FrechetInceptionDistance') is FrechetInceptionDistance
    assert FrechetInceptionDistance.__name__ == 'FrechetInceptionDistance'


@pytest.fixture(scope='module')
def metric():
    from diffusion_amd.metrics.fid import FrechetInceptionDistance
    with pytest.warns(UserWarning, match='RANDOM-INIT'):
        return FrechetInceptionDistance(device='cpu')


def test_argument_errors_before_any_device_use(metric):
    from diffusion_amd.metrics.fid import FrechetInceptionDistance
    for feature in (64, 192, 768, '2048', None):
        with pytest.raises(ValueError):
            FrechetInceptionDistance(feature=feature, device='cpu')
    with pytest.raises(ValueError):
        FrechetInceptionDistance(normalize='yes', device='cpu')
    u8 = torch.zeros(2, 3, 8, 8, dtype=torch.uint8)
    # the metric lives on the CPU, where reaching the tower is a RuntimeError: a ValueError shows the check came first
    for bad in (u8[0], u8[:, :2], torch.zeros(2, 3, 8), u8.float(), u8.to(torch.int32), [u8]):
        with pytest.raises(ValueError):
            metric.update(bad, real=True)
    norm = copy.deepcopy(metric)
    norm.normalize = True
    with pytest.raises(ValueError):
        norm.update(u8, real=False)
    with pytest.raises(RuntimeError, match='MI355X'):
        metric.update(u8, real=True)
    with pytest.raises(RuntimeError, match='MI355X'):
        norm.update(u8.float(), real=True)
    assert all(float(v.abs().sum()) == 0 for st in metric.state.values() for v in st.values())


def test_random_init_is_seeded_and_warns_and_a_missing_file_is_not_fetched(tmp_path):
    from diffusion_amd.metrics.fid import FrechetInceptionDistance
    with pytest.warns(UserWarning, match='meaningless'):
        a = FrechetInceptionDistance(weights_path=str(tmp_path / 'absent.pth'), device='cpu')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        b = FrechetInceptionDistance(device='cpu')
    sa, sb = a._shared['state_dict'], b._shared['state_dict']
    assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_weights_file_is_loaded_strictly(tmp_path):
    from diffusion_amd.metrics.fid import FrechetInceptionDistance
    from diffusion_amd.models.inception_hip import random_state_dict
    sd = random_state_dict(9)
    sd['fc.weight'], sd['fc.bias'] = torch.zeros(1008, 2048), torch.zeros(1008)   # present in the real file, ignored
    path = tmp_path / 'w.pth'
    torch.save(sd, path)
    with warnings.catch_warnings():
        warnings.simplefilter('error')   # a real file: no warning
        m = FrechetInceptionDistance(weights_path=str(path), device='cpu')
    assert torch.equal(m._shared['state_dict']['Mixed_7c.branch_pool.conv.weight'], sd['Mixed_7c.branch_pool.conv.weight'])
    del sd['Mixed_5b.branch1x1.bn.bias']
    torch.save(sd, path)
    with pytest.raises(RuntimeError):
        FrechetInceptionDistance(weights_path=str(path), device='cpu')


def test_deepcopy_shares_the_tower_and_not_the_state(metric):
    m = copy.deepcopy(metric)
    m.state['real']['sum'] += 1.0
    c = copy.deepcopy(m)
    c.guidance_scale = 3.0
    assert c._shared is m._shared and m._shared is metric._shared
    assert c.state['real']['sum'].data_ptr() != m.state['real']['sum'].data_ptr()
    assert torch.equal(c.state['real']['sum'], m.state['real']['sum'])
    c.reset()
    assert float(m.state['real']['sum'].sum()) == 2048.0 and float(c.state['real']['sum'].sum()) == 0.0
    assert float(metric.state['real']['sum'].sum()) == 0.0 and not hasattr(m, 'guidance_scale')
    assert list(m.parameters()) == []


def test_reset_real_features_semantics_and_compute_on_hand_set_state():
    from diffusion_amd.metrics.fid import FrechetInceptionDistance, fid_from_moments
    rng = np.random.default_rng(6)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        keep = FrechetInceptionDistance(reset_real_features=False, device='cpu')
        drop = FrechetInceptionDistance(device='cpu')
    X, Y = rng.normal(0, 1, (5, 2048)), rng.normal(0.1, 1, (4, 2048))
    for m in (keep, drop):
        for side, Z in (('real', X), ('fake', Y)):
            m.state[side]['sum'] += torch.from_numpy(Z.sum(0))
            m.state[side]['cov'] += torch.from_numpy(Z.T @ Z)
            m.state[side]['n'] += len(Z)
    want = float(fid_from_moments(X.sum(0), X.T @ X, 5, Y.sum(0), Y.T @ Y, 4))
    assert np.isfinite(want) and want > 0
    assert float(keep.compute()) == want
    assert all(torch.equal(keep.state[s][k], drop.state[s][k]) for s in ('real', 'fake') for k in ('sum', 'cov', 'n'))
    keep.reset()
    drop.reset()
    assert keep.state['real']['n'].item() == 5 and float(keep.state['real']['cov'].abs().sum()) > 0
    assert keep.state['fake']['n'].item() == 0 and float(keep.state['fake']['cov'].abs().sum()) == 0
    assert drop.state['real']['n'].item() == 0 and float(drop.state['real']['sum'].abs().sum()) == 0
    with pytest.raises(RuntimeError):
        keep.compute()   # no fake samples left


def test_stable_diffusion_sweeps_the_metric_over_guidance_scales(metric):
    """the class itself (the factory needs a GPU for the U-Net): the metric list is all this constructor looks at here"""
    from diffusion_amd.models.stable_diffusion import StableDiffusion
    model = StableDiffusion(unet=None, vae=None, text_encoder=None, tokenizer=None, noise_scheduler=None,
                            inference_noise_scheduler=None, val_metrics=[copy.deepcopy(metric)], val_guidance_scales=[1.0, 3.0])
    keys = ['FrechetInceptionDistance-scale-1p0', 'FrechetInceptionDistance-scale-3p0']
    assert all(k in model.val_metrics for k in keys)
    a, b = (model.val_metrics[k] for k in keys)
    assert (a.guidance_scale, b.guidance_scale) == (1.0, 3.0)
    assert a._shared is b._shared and a.state['fake']['cov'].data_ptr() != b.state['fake']['cov'].data_ptr()


def test_conv_rect_case_tables_cover_what_they_claim():
    from conv_rect_reference import CINS, COUTS, EXACT_CASES, FORMS, LARGE_CASE, TILE_CASES, out_size
    assert {c[2] for c in EXACT_CASES} == set(CINS) and {c[3] for c in EXACT_CASES} == set(COUTS)
    assert {c[1][0] for c in EXACT_CASES} == {1, 3} and {c[5] for c in EXACT_CASES} == {0, 32, 64, 96}
    for name, *_ in FORMS:   # every form meets ReLU on and off, a straddling Cin (48 or 80) and the K tail (K % 64 != 0)
        mine = [c for c in EXACT_CASES if c[0].startswith(name + '-')]
        assert {c[4] for c in mine} == {True, False}, name
        assert any(c[2] in (48, 80) for c in mine) and any((c[1][3] * c[1][4] * c[2]) % 64 for c in mine), name
    for _, (B, H, W, kh, kw, s, ph, pw), *_ in EXACT_CASES + TILE_CASES + LARGE_CASE:
        assert H != W
    B, H, W, kh, kw, s, ph, pw = LARGE_CASE[0][1]
    Ho, Wo = out_size(H, W, kh, kw, s, ph, pw)
    assert 50000 <= B * Ho * Wo <= 51000


def test_conv_rect_reference_gather_matches_conv2d():
    """the float64 gather the GPU tests compare against is F.conv2d, for every form and size of the exact cases"""
    import torch.nn.functional as F
    from conv_rect_reference import FORMS, reference
    g = torch.Generator().manual_seed(0)
    for name, kh, kw, s, ph, pw, sizes in FORMS:
        for H, W in sizes:
            B, Cin, Cout = 2, 8, 16
            X, Wt = torch.randn(B * H * W, Cin, generator=g), torch.randn(Cout, kh * kw * Cin, generator=g)
            bias = torch.randn(Cout, generator=g)
            ref, absprod = reference(X, Wt, bias, (B, H, W, kh, kw, s, ph, pw), True)
            y = F.conv2d(X.double().view(B, H, W, Cin).permute(0, 3, 1, 2), Wt.double().view(Cout, kh, kw, Cin).permute(0, 3, 1, 2),
                         bias.double(), stride=s, padding=(ph, pw)).clamp(min=0)
            assert torch.allclose(ref, y.permute(0, 2, 3, 1).reshape(-1, Cout), rtol=0, atol=1e-12), (name, H, W)
            assert bool((absprod >= ref.abs() - 1e-12).all())
