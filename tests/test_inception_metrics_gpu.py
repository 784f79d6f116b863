"""The Inception-score / KID kernels (csrc/inception_metrics.hip) and metrics on the MI355X against the NumPy float64
restatement of tests/inception_metrics_reference.py.

Every comparison first asserts on the CPU that the float64 reference and the same code in ``np.longdouble`` agree to 1e-13
on the very inputs used, so what is measured afterwards is the kernel and not the conditioning of the input.  (For the one
call at m = 1000 the longdouble side, which has no BLAS, runs on every 8th row of the same stores.)  ``da_inception_score``
and ``da_poly_mmd`` are held to the smaller of the cap 1e-11 and twice the worst deviation measured on an MI355X
(profiles/inception_metrics_margins.json, written through DA_PARITY_MARGINS): relative to the score, and for the MMD relative
to mean|k_xx| + mean|k_yy| + 2 mean|k_xy| (the value is a small difference of those).  Measured: 2.7e-15 and 8.8e-16, so
5.3e-15 and 1.8e-15 are asserted.  The metrics' ``compute()`` against their own host functions is held to the cap.  ``da_fc_logits_f32`` is held to a
derived bound, 2^-24 |ref| + (K + 1) 2^-53 sum_k |F W|.
"""
import copy
import warnings

import numpy as np
import pytest
import torch

import inception_metrics_reference as R
import inception_reference as IR
from parity_margins import record

pytestmark = pytest.mark.gpu

# worst deviation of each kernel measured on an MI355X over the cases of this file, in the units described above: the score
# at (N, C, splits, scale) = (64, 1008, 1, 80), the MMD at m = 1000; every other case is 2 to 100 times closer
MEASURED = {'inception_score': 2.67e-15, 'poly_mmd': 8.77e-16}


def _tol(kind):
    """the two kernels: min(cap, 2 x measured); the metrics against their own host functions ('end_to_end'): the cap"""
    return min(R.CAP, 2.0 * MEASURED[kind]) if kind in MEASURED else R.CAP


def _agree(a, b, scale=None):
    """float64 and longdouble evaluations of the reference, relative to the value (or to ``scale``)"""
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    return float(np.max(np.abs(a - b) / (np.abs(b) if scale is None else np.asarray(scale, np.longdouble))))


def _strided(x, dev, extra):
    """the matrix as a column slice of a wider device buffer (row stride = columns + extra)"""
    x = torch.as_tensor(x)
    buf = torch.full((x.shape[0], x.shape[1] + extra), float('nan'), dtype=x.dtype, device=dev)
    buf[:, :x.shape[1]] = x.to(dev)
    return buf[:, :x.shape[1]]


# ------------------------------------------------------------------------------------------------------------- the head
@pytest.mark.parametrize('B,K,C', [(1, 8, 1), (3, 2048, 1008), (32, 2048, 1008), (5, 64, 17)])
def test_fc_logits_against_the_derived_bound(dev, B, K, C):
    from diffusion_amd import ops
    rng = np.random.default_rng(B * 1000 + C)
    F, W = rng.normal(0, 1, (B, K)).astype(np.float32), rng.normal(0, K ** -0.5, (C, K)).astype(np.float32)
    ref, bound = R.fc_bound(F, W)
    dF = _strided(F, dev, 4)
    out = torch.full((B, C + 3), -7.0, device=dev)
    got = ops.fc_logits_f32(dF, torch.from_numpy(W).to(dev), out[:, :C])
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    print(f'fc_logits B={B} K={K} C={C}: worst err / bound = {float((err / bound).max()):.3f}')
    assert np.all(err <= bound)
    assert bool((out[:, C:] == -7.0).all())   # nothing written past the C columns
    again = ops.fc_logits_f32(dF, torch.from_numpy(W).to(dev), torch.empty(B, C, device=dev))
    assert torch.equal(again, got)


def test_fc_logits_integers_are_exact_and_bad_arguments_launch_nothing(dev):
    from diffusion_amd import _lib, ops
    rng = np.random.default_rng(3)
    B, K, C = 5, 64, 17
    F, W = rng.integers(-8, 9, (B, K)).astype(np.float32), rng.integers(-8, 9, (C, K)).astype(np.float32)
    dF, dW = torch.from_numpy(F).to(dev), torch.from_numpy(W).to(dev)
    got = ops.fc_logits_f32(dF, dW, torch.empty(B, C, device=dev))
    assert np.array_equal(got.cpu().numpy().astype(np.int64), F.astype(np.int64) @ W.astype(np.int64).T)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    out = torch.full((B, C), -7.0, device=dev)
    p = (dF.data_ptr(), dW.data_ptr(), out.data_ptr())
    assert lib.da_fc_logits_f32(None, K, p[1], p[2], C, B, K, C, st) == 1      # null pointer
    assert lib.da_fc_logits_f32(p[0], K, None, p[2], C, B, K, C, st) == 1
    assert lib.da_fc_logits_f32(p[0], K, p[1], None, C, B, K, C, st) == 1
    assert lib.da_fc_logits_f32(p[0], K, p[1], p[2], C, B, K - 2, C, st) == 1  # K % 4 != 0
    assert lib.da_fc_logits_f32(p[0], K - 4, p[1], p[2], C, B, K, C, st) == 1  # ldf < K
    assert lib.da_fc_logits_f32(p[0], K, p[1], p[2], C - 1, B, K, C, st) == 1  # ldo < C
    assert lib.da_fc_logits_f32(p[0] + 4, K, p[1], p[2], C, B, K, C, st) == 1  # F not 16-byte aligned
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    with pytest.raises(ValueError):
        ops.fc_logits_f32(dF[:, :62], dW[:, :62].contiguous(), out)
    with pytest.raises(TypeError):
        ops.fc_logits_f32(dF.double(), dW, out)


# ------------------------------------------------------------------------------------------------------ Inception score
def _logits(N, C, scale):
    rng = np.random.default_rng(N * 7 + C)
    return (rng.normal(0, scale, (N, C))).astype(np.float32), rng.permutation(N).astype(np.int32)


@pytest.mark.parametrize('N,C,splits,scale', [(23, 1008, 10, 3.0), (5, 8, 10, 1.0), (64, 1008, 1, 80.0), (1000, 1008, 10, 5.0)])
def test_inception_score_kernel(dev, N, C, splits, scale):
    from diffusion_amd import ops
    logits, perm = _logits(N, C, scale)
    assert not np.array_equal(perm, np.arange(N))
    ref = R.inception_scores(logits, perm, splits)
    agree = _agree(ref, R.inception_scores(logits, perm, splits, np.longdouble))
    assert agree <= R.REF_AGREEMENT, agree
    chunks = len(R.chunk_bounds(N, splits))
    if (N, splits) == (23, 10):
        assert chunks == 8 and R.chunk_bounds(N, splits)[-1] == (21, 23)
    if N < splits:
        assert chunks == N and np.all(np.abs(ref - 1.0) <= 1e-15)
    if scale == 80.0:   # the case that shows float64 and the subtracted maximum: the same formulas in float32 are not finite
        with np.errstate(all='ignore'):
            assert np.isinf(np.exp(logits.max())) and not np.isfinite(R.inception_scores(logits, perm, splits, np.float32)).all()
    d = torch.from_numpy(logits).to(dev)
    buf = torch.full((splits,), -7.0, dtype=torch.float64, device=dev)
    got = ops.inception_score(d, torch.from_numpy(perm), splits, buf)
    assert got.shape[0] == chunks and bool((buf[chunks:] == -7.0).all())   # the reported chunk count, nothing past it
    rel = float(np.max(np.abs(got.cpu().numpy() - ref) / np.abs(ref)))
    record('inception_score', {'rel': _tol('inception_score')}, **{f'N{N}_C{C}_s{splits}_x{scale:g}': rel})
    print(f'inception_score N={N} C={C} splits={splits} scale={scale}: rel {rel:.3e} (reference vs longdouble {agree:.1e})')
    assert np.isfinite(got.cpu().numpy()).all() and rel <= _tol('inception_score')
    again = ops.inception_score(d, torch.from_numpy(perm), splits)
    assert torch.equal(again, got)   # the same bits
    wide = ops.inception_score(_strided(logits, dev, 5), torch.from_numpy(perm), splits)   # ld > C
    assert torch.equal(wide, got)


# ------------------------------------------------------------------------------------------------------- polynomial MMD
_STORES = {}


def _stores(m, D):
    """per (m, D): the two fp32 stores and the index sets (3 subsets, overlapping, unsorted), shared by the kernel
    parameters run on them"""
    if (m, D) not in _STORES:
        rng = np.random.default_rng(m * 31 + D)
        nr, nf = m + 7, m + 11
        fr, ff = rng.normal(0, 1, (nr, D)).astype(np.float32), rng.normal(0.1, 1.1, (nf, D)).astype(np.float32)
        _STORES[m, D] = (fr, ff, R.subset_indices(rng, 3, m, nr), R.subset_indices(rng, 3, m, nf))
    return _STORES[m, D]


def _mmd_case(dev, name, fr, ff, ir, jf, degree, gamma, coef, agree_on=None):
    """``agree_on``: the (fr, ff, idx_r, idx_f) the float64 / longdouble agreement is checked on, when not the inputs"""
    from diffusion_amd import ops
    ref, scale = R.poly_mmd(fr, ff, ir, jf, degree, gamma, coef)
    small = (fr, ff, ir, jf) if agree_on is None else agree_on
    lref, lscale = (ref, scale) if agree_on is None else R.poly_mmd(*small, degree, gamma, coef)
    agree = _agree(lref, R.poly_mmd(*small, degree, gamma, coef, np.longdouble)[0], lscale)
    assert agree <= R.REF_AGREEMENT, agree
    dr, df = _strided(fr, dev, 4), _strided(ff, dev, 8)
    got = ops.poly_mmd(dr, df, torch.from_numpy(ir), torch.from_numpy(jf), degree, gamma, coef)
    rel = float(np.max(np.abs(got.cpu().numpy() - ref) / scale))
    record('poly_mmd', {'rel_to_kernel_scale': _tol('poly_mmd')}, **{name: rel})
    print(f'poly_mmd {name}: {rel:.3e} of the kernel scale (reference vs longdouble {agree:.1e})')
    assert rel <= _tol('poly_mmd')
    again = ops.poly_mmd(dr, df, torch.from_numpy(ir), torch.from_numpy(jf), degree, gamma, coef)
    assert torch.equal(again, got)   # the same bits


@pytest.mark.parametrize('degree,gamma,coef', [(3, None, 1.0), (1, 0.013, 0.0)])
@pytest.mark.parametrize('m,D', [(2, 8), (5, 8), (33, 2048), (257, 2048)])
def test_poly_mmd_kernel(dev, m, D, degree, gamma, coef):
    fr, ff, ir, jf = _stores(m, D)
    assert any(set(ir[0]) & set(ir[s]) for s in (1, 2))   # the subsets overlap
    assert m == 2 or any(not np.array_equal(np.sort(i), i) for i in ir)   # and are not sorted
    _mmd_case(dev, f'm{m}_D{D}_deg{degree}_g{gamma}_c{coef:g}', fr, ff, ir, jf, degree, gamma, coef)


def test_poly_mmd_kernel_at_the_default_subset_size(dev):
    """m = 1000, D = 2048, 2 subsets; the longdouble agreement runs on every 8th row of the same stores (m = 125)"""
    rng = np.random.default_rng(1000)
    fr, ff = rng.normal(0, 1, (1030, 2048)).astype(np.float32), rng.normal(0.1, 1.1, (1050, 2048)).astype(np.float32)
    ir, jf = R.subset_indices(rng, 2, 1000, 1030), R.subset_indices(rng, 2, 1000, 1050)
    sr, sf = fr[::8], ff[::8]
    si, sj = R.subset_indices(rng, 2, 125, len(sr)), R.subset_indices(rng, 2, 125, len(sf))
    _mmd_case(dev, 'm1000_D2048_deg3_gNone_c1', fr, ff, ir, jf, 3, None, 1.0, agree_on=(sr, sf, si, sj))


def test_poly_mmd_bad_arguments_launch_nothing(dev):
    from diffusion_amd import _lib, ops
    fr, ff, ir, jf = _stores(5, 8)
    dr, df = torch.from_numpy(fr).to(dev), torch.from_numpy(ff).to(dev)
    di, dj = torch.from_numpy(ir).to(dev), torch.from_numpy(jf).to(dev)
    need = ops.poly_mmd_workspace(3, 5)
    assert need == 3 * 3 and ops.poly_mmd_workspace(100, 1000) == 100 * (16 * 16 + 16 * 17)
    assert ops.poly_mmd_workspace(3, 1) == 0 and ops.poly_mmd_workspace(0, 5) == 0 and ops.poly_mmd_workspace(70000, 5) == 0
    out = torch.full((3,), -7.0, dtype=torch.float64, device=dev)
    ws = torch.full((need,), -7.0, dtype=torch.float64, device=dev)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream

    def raw(m=5, D=8, degree=3, gamma=0.125, coef=1.0, ws_n=need, fr_ptr=dr.data_ptr(), ldr=8):
        return lib.da_poly_mmd(fr_ptr, ldr, dr.shape[0], df.data_ptr(), 8, df.shape[0], di.data_ptr(), dj.data_ptr(), 3, m, D,
                               degree, gamma, coef, out.data_ptr(), ws.data_ptr(), ws_n, st)
    assert raw(m=1) == 1 and raw(degree=0) == 1 and raw(degree=9) == 1 and raw(D=6) == 1 and raw(ws_n=need - 1) == 1
    assert raw(fr_ptr=None) == 1 and raw(ldr=4) == 1 and raw(gamma=0.0) == 1 and raw(coef=-1.0) == 1
    assert raw(fr_ptr=dr.data_ptr() + 4) == 1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((ws == -7.0).all())
    assert raw() == 0
    torch.cuda.synchronize()
    assert bool((out != -7.0).all())


def test_wrapper_guards_raise_before_any_launch(dev):
    from diffusion_amd import ops
    fr, ff, ir, jf = _stores(5, 8)
    dr, df = torch.from_numpy(fr).to(dev), torch.from_numpy(ff).to(dev)
    out = torch.full((3,), -7.0, dtype=torch.float64, device=dev)
    for bad_r, bad_f in ((np.where(ir == ir[1, 2], len(fr), ir), jf), (ir, np.where(jf == jf[0, 0], -1, jf))):
        with pytest.raises(ValueError, match=r'must lie in'):
            ops.poly_mmd(dr, df, torch.from_numpy(bad_r.astype(np.int32)), torch.from_numpy(bad_f.astype(np.int32)), out=out)
    with pytest.raises(TypeError):
        ops.poly_mmd(dr, df, torch.from_numpy(ir).long(), torch.from_numpy(jf), out=out)
    with pytest.raises(TypeError):
        ops.poly_mmd(dr.double(), df, torch.from_numpy(ir), torch.from_numpy(jf), out=out)
    with pytest.raises(ValueError):
        ops.poly_mmd(dr, df, torch.from_numpy(ir).to(dev), torch.from_numpy(jf).to(dev), out=out)   # device indices: unchecked
    with pytest.raises(ValueError):
        ops.poly_mmd(dr, df, torch.from_numpy(ir), torch.from_numpy(jf), out=out, ws=torch.empty(8, dtype=torch.float64, device=dev))
    logits, perm = _logits(23, 8, 1.0)
    d = torch.from_numpy(logits).to(dev)
    scores = torch.full((4,), -7.0, dtype=torch.float64, device=dev)
    twice = perm.copy()
    twice[3] = twice[4]
    for bad in (twice, np.where(perm == 0, 23, perm).astype(np.int32), perm[:-1]):
        with pytest.raises(ValueError, match='permutation'):
            ops.inception_score(d, torch.from_numpy(bad), 4, scores)
    with pytest.raises(TypeError):
        ops.inception_score(d, torch.from_numpy(perm).long(), 4, scores)
    with pytest.raises(TypeError):
        ops.inception_score(d.half(), torch.from_numpy(perm), 4, scores)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((scores == -7.0).all())


def test_row_offsets_past_2_and_4_gib(dev):
    """one store with rows of 2^20 floats: rows 511 | 512 and 1023 | 1024 put idx * ld * 4 bytes on both sides of 2 GiB and
    4 GiB.  torch.empty: only the columns written are ever read."""
    from diffusion_amd import ops
    free, _ = torch.cuda.mem_get_info()
    if free < 6 * 2 ** 30:
        pytest.skip(f'needs 6 GiB of free device memory, {free / 2 ** 30:.1f} GiB are free')
    LD, N, D = 2 ** 20, 1100, 8
    rows = np.array([0, 511, 512, 1023, 1024, 1099])
    rng = np.random.default_rng(64)
    small = rng.normal(0, 1, (N, D)).astype(np.float32)
    store = torch.empty(N, LD, device=dev)
    assert store.stride(0) * 4 * 512 == 2 ** 31
    view = store[:, :D]
    view.copy_(torch.from_numpy(small).to(dev))
    # MMD: m = 3 per side, real rows below | fake rows above each boundary and the ends
    ir, jf = np.array([[1024, 0, 511]], np.int32), np.array([[512, 1099, 1023]], np.int32)
    assert set(ir[0]) | set(jf[0]) == set(rows)
    ref, scale = R.poly_mmd(small, small, ir, jf)
    assert _agree(ref, R.poly_mmd(small, small, ir, jf, dtype=np.longdouble)[0], scale) <= R.REF_AGREEMENT
    got = ops.poly_mmd(view, view, torch.from_numpy(ir), torch.from_numpy(jf))
    rel = float(np.max(np.abs(got.cpu().numpy() - ref) / scale))
    record('poly_mmd', {'rel_to_kernel_scale': _tol('poly_mmd')}, large_offsets=rel)
    assert rel <= _tol('poly_mmd')
    # score: all 1100 rows in a shuffled order, 4 chunks
    perm = rng.permutation(N).astype(np.int32)
    sref = R.inception_scores(small, perm, 4)
    assert _agree(sref, R.inception_scores(small, perm, 4, np.longdouble)) <= R.REF_AGREEMENT
    sgot = ops.inception_score(view, torch.from_numpy(perm), 4)
    srel = float(np.max(np.abs(sgot.cpu().numpy() - sref) / sref))
    record('inception_score', {'rel': _tol('inception_score')}, large_offsets=srel)
    assert srel <= _tol('inception_score')
    # a row that is wrong only past 4 GiB shows: swap what rows 0 and 1024 hold and the numbers move
    moved = small.copy()
    moved[[0, 1024]] = moved[[1024, 0]] * 1.5
    assert np.max(np.abs(R.poly_mmd(moved, moved, ir, jf)[0] - ref) / scale) > 1e-3
    del store, view


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope='module')
def fed(dev):
    """both metrics on the shared random-init tower after two batches of two 64 x 96 images per side"""
    from diffusion_amd.metrics.inception_score import InceptionScore
    from diffusion_amd.metrics.kid import KernelInceptionDistance
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        score = InceptionScore(splits=2, device=dev, max_batch=2)
        kid = KernelInceptionDistance(subsets=4, subset_size=3, device=dev, max_batch=2)
    batches = [IR.seeded_images(2, 64, 96, seed=s) for s in (7, 8, 9, 10)]
    for b in batches[:2]:
        kid.update(b, real=True)
    for b in batches[2:]:
        kid.update(b.to(dev), real=False)
        score.update(b)
    return score, kid, batches


def test_logits_head_of_the_tower_on_its_own_features(dev, fed):
    score, kid, batches = fed
    tower = score._tower()
    assert tower is kid._tower()
    feats = tower(batches[0].to(dev))
    got = tower.logits_unbiased(feats)
    assert tuple(got.shape) == (2, 1008) and got.dtype == torch.float32
    ref, bound = R.fc_bound(feats.cpu().numpy(), tower.fc_weight.cpu().numpy())
    assert np.all(np.abs(got.cpu().numpy().astype(np.float64) - ref) <= bound)
    assert float(np.abs(ref).max()) > 0
    from diffusion_amd.models.inception_hip import InceptionV3HIP, random_state_dict
    with pytest.raises(RuntimeError, match='fc.weight'):
        InceptionV3HIP(random_state_dict(0), dev, max_batch=1).logits_unbiased(feats)


def test_metrics_equal_their_host_functions_on_their_own_stores(dev, fed):
    from diffusion_amd.metrics.inception_score import inception_score_from_logits
    from diffusion_amd.metrics.kid import kid_from_features
    score, kid, _ = fed
    assert score.logits().shape == (4, 1008) and kid.features(True).shape == (4, 2048) and kid.features(False).shape == (4, 2048)
    mean, std = score.compute()
    wm, ws = inception_score_from_logits(score.logits(), score.permutation(4), 2)
    e1 = max(abs(float(mean) - float(wm)) / float(wm), abs(float(std) - float(ws)) / float(wm))
    kmean, kstd = kid.compute()
    ir, jf = kid.subset_indices(4, 4)
    km, ks = kid_from_features(kid.features(True), kid.features(False), ir, jf, 3, None, 1.0)
    _, scale = R.poly_mmd(kid.features(True).cpu().numpy(), kid.features(False).cpu().numpy(), ir.numpy(), jf.numpy())
    e2 = max(abs(float(kmean) - float(km)), abs(float(kstd) - float(ks))) / float(scale.max())
    record('end_to_end', {'rel': _tol('end_to_end')}, inception_score=e1, kid=e2)
    print(f'end to end: InceptionScore {float(mean):.6f} +- {float(std):.6f} (rel {e1:.3e}), KID {float(kmean):.6e} +- '
          f'{float(kstd):.6e} ({e2:.3e} of the kernel scale)')
    assert float(std) > 0 and float(kstd) > 0   # the images differ in kind: the numbers are not degenerate
    assert e1 <= _tol('end_to_end') and e2 <= _tol('end_to_end')
    again, kagain = score.compute(), kid.compute()
    assert again[0].equal(mean) and again[1].equal(std) and kagain[0].equal(kmean) and kagain[1].equal(kstd)


def test_reset_deepcopy_and_too_few_samples(dev, fed):
    from diffusion_amd.metrics.kid import KernelInceptionDistance
    score, kid, batches = fed
    c, s = copy.deepcopy(kid), copy.deepcopy(score)
    assert c._tower() is kid._tower() and s._tower() is score._tower()
    assert c.stores['real'].buf.data_ptr() != kid.stores['real'].buf.data_ptr()
    assert torch.equal(c.features(False), kid.features(False)) and torch.equal(s.logits(), score.logits())
    c.reset()
    s.reset()
    assert c.stores['real'].n == 0 and c.stores['fake'].n == 0 and s.store.n == 0
    assert kid.stores['real'].n == 4 and kid.stores['fake'].n == 4 and score.store.n == 4
    keep = copy.deepcopy(kid)
    keep.reset_real_features = False
    keep.reset()
    assert keep.stores['real'].n == 4 and keep.stores['fake'].n == 0
    big = copy.deepcopy(kid)
    big.subset_size = 5
    with pytest.raises(ValueError, match='`subset_size` should be smaller than the number of samples'):
        big.compute()
    with pytest.raises(ValueError, match='`subset_size` should be smaller than the number of samples'):
        keep.compute()


def test_through_the_model(dev, fed):
    from diffusion_amd.metrics.inception_score import InceptionScore
    from diffusion_amd.metrics.kid import KernelInceptionDistance
    from diffusion_amd.models.stable_diffusion import StableDiffusion
    _, _, batches = fed
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        metrics = [InceptionScore(splits=2, normalize=True, device=dev, max_batch=2),
                   KernelInceptionDistance(subset_size=2, subsets=2, normalize=True, device=dev, max_batch=2)]
    model = StableDiffusion(unet=None, vae=None, text_encoder=None, tokenizer=None, noise_scheduler=None,
                            inference_noise_scheduler=None, val_metrics=metrics, val_guidance_scales=[1.0, 3.0])
    names = [f'{n}-scale-{s}' for n in ('InceptionScore', 'KernelInceptionDistance') for s in ('1p0', '3p0')]
    assert all(n in model.val_metrics for n in names)
    real = batches[0].float().div(255).to(dev)
    gen = {1.0: batches[2].float().div(255).to(dev), 3.0: batches[3].float().div(255).to(dev)}
    outputs = (None, None, None, gen)
    for n in names:
        model.update_metric({model.image_key: real}, outputs, model.val_metrics[n])
    for s, g in (('1p0', 1.0), ('3p0', 3.0)):
        sc, kd = model.val_metrics[f'InceptionScore-scale-{s}'], model.val_metrics[f'KernelInceptionDistance-scale-{s}']
        assert sc.store.n == 2 and kd.stores['real'].n == 2 and kd.stores['fake'].n == 2
        tower = kd._tower()
        assert tower is sc._tower()
        assert torch.equal(kd.features(True), tower(real)) and torch.equal(kd.features(False), tower(gen[g]))
        assert torch.equal(sc.logits(), tower.logits_unbiased(tower(gen[g])))
        mean, std = kd.compute()
        assert np.isfinite(float(mean)) and np.isfinite(float(std))
        assert np.isfinite(float(sc.compute()[0]))


def test_trainer_eval_logs_mean_and_std_of_both_metrics(dev):
    from diffusion_amd.metrics.inception_score import InceptionScore
    from diffusion_amd.metrics.kid import KernelInceptionDistance
    from diffusion_amd.models.composer_shim import MeanSquaredError
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.optim import FusedAdamW
    from diffusion_amd.trainer import Trainer
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        score = InceptionScore(splits=2, normalize=True, device=dev, max_batch=2)
        kid = KernelInceptionDistance(subsets=3, subset_size=2, normalize=True, device=dev, max_batch=2)
    model = stable_diffusion_2(model_name='tiny', pretrained=False, fsdp=False, encode_latents_in_fp16=False,
                               val_metrics=[MeanSquaredError(), score, kid], val_guidance_scales=[3.0])
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
    for name in ('InceptionScore', 'KernelInceptionDistance'):
        key = f'metrics/eval/{name}-scale-3p0'
        assert key in out and key + '-std' in out, sorted(out)
        print(f'{key} = {out[key]:.6e} +- {out[key + "-std"]:.6e}')
        assert np.isfinite(out[key]) and np.isfinite(out[key + '-std'])
    swept = model.val_metrics['KernelInceptionDistance-scale-3p0']
    assert swept.stores['real'].n == 2 and swept.stores['fake'].n == 2
    assert model.val_metrics['InceptionScore-scale-3p0'].store.n == 2
