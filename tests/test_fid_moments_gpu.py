"""da_feature_moments (csrc/inception.hip): the float64 FID state update.

Exact case: integer-valued fp32 features (|.| <= 64) give sums of integers far below 2^53, so ``sum``, ``cov`` and ``n`` after
two updates must equal numpy int64 arithmetic; D in {8, 2048}, B in {1, 3, 67}; F is a column view with NaN surroundings
and the three state tensors sit between NaN sentinels that must keep their bits.
Float case: N(0, 1) features.  A product of two fp32 values is exact in float64 and each output element is one thread's
running sum in batch order, B_total additions onto the stored value, each with relative error 2^-53 of a partial sum that
is at most sum_b |F_bd F_be|; so |cov - ref| <= (B_total + 1) * 2^-53 * sum_b |F_bd F_be| per element (derived, not
measured), the same form for ``sum``.  The reference is numpy in 80-bit long double (64-bit significand), whose own error
is 2^-11 of that bound: the + 1 covers it.  Two runs give identical bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float('nan')


@pytest.fixture(scope='module')
def ops(dev):
    from diffusion_amd import ops as o
    return o


def state(D, dev):
    """(buffer, sum, cov, n): the three float64 state tensors as zeroed slices of one NaN buffer, 16 NaN between them"""
    buf = torch.full((16 + D + 16 + D * D + 16 + 1 + 16,), NAN, device=dev, dtype=torch.float64)
    s = buf[16:16 + D]
    c = buf[32 + D:32 + D + D * D].view(D, D)
    n = buf[48 + D + D * D:49 + D + D * D]
    for t in (s, c, n):
        t.zero_()
    return buf, s, c, n


def feature_view(F, dev):
    B, D = F.shape
    buf = torch.full((B + 2, 8 + D + 8), NAN, device=dev, dtype=torch.float32)
    buf[:B, 8:8 + D] = F.to(dev)
    return buf[:B, 8:8 + D]


@pytest.mark.parametrize('B', [1, 3, 67])
@pytest.mark.parametrize('D', [8, 2048])
def test_moments_exact_on_integers(ops, dev, D, B):
    g = torch.Generator().manual_seed(D + B)
    F1 = torch.randint(-64, 65, (B, D), generator=g).float()
    F2 = torch.randint(-64, 65, (2, D), generator=g).float()
    buf, s, c, n = state(D, dev)
    ops.feature_moments(feature_view(F1, dev), s, c, n)
    ops.feature_moments(feature_view(F2, dev), s, c, n)   # two updates accumulate
    torch.cuda.synchronize()
    A = np.concatenate([F1.numpy(), F2.numpy()]).astype(np.int64)
    assert np.array_equal(s.cpu().numpy(), A.sum(0).astype(np.float64))
    assert np.array_equal(c.cpu().numpy(), (A.T @ A).astype(np.float64))
    assert n.item() == B + 2
    outside = torch.ones(buf.shape, dtype=torch.bool, device=dev)
    outside[16:16 + D] = outside[32 + D:32 + D + D * D] = outside[48 + D + D * D] = False
    assert bool(torch.isnan(buf[outside]).all())


def test_moments_float_bound_and_determinism(ops, dev):
    D, Bs = 2048, (33, 31)
    g = torch.Generator().manual_seed(5)
    Fs = [torch.randn(B, D, generator=g) for B in Bs]
    runs = []
    for _ in range(2):
        _, s, c, n = state(D, dev)
        for F in Fs:
            ops.feature_moments(feature_view(F, dev), s, c, n)
        torch.cuda.synchronize()
        runs.append((s.cpu().numpy().copy(), c.cpu().numpy().copy(), n.item()))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    assert np.finfo(np.longdouble).nmant >= 63
    A = torch.cat(Fs).numpy().astype(np.longdouble)
    Bt = A.shape[0]
    s, c, n = runs[0]
    assert n == Bt
    cov_err, cov_bound = np.abs(c - A.T @ A), (Bt + 1) * np.longdouble(2.0 ** -53) * (np.abs(A).T @ np.abs(A))
    sum_err, sum_bound = np.abs(s - A.sum(0)), (Bt + 1) * np.longdouble(2.0 ** -53) * np.abs(A).sum(0)
    print(f'cov: worst err / bound {float(np.max(cov_err / cov_bound)):.3f}; sum: {float(np.max(sum_err / sum_bound)):.3f}')
    assert (cov_err <= cov_bound).all() and (sum_err <= sum_bound).all()


def test_moments_rejects(ops, dev):
    _, s, c, n = state(8, dev)
    F = torch.zeros(2, 8, device=dev)
    with pytest.raises(ValueError):
        ops.feature_moments(torch.zeros(2, 12, device=dev), s, c, n)
    with pytest.raises(ValueError):
        ops.feature_moments(F, s.float(), c, n)
    with pytest.raises(ValueError):
        ops.feature_moments(F, s, c[:, :4], n)
    with pytest.raises(ValueError):
        ops.feature_moments(F.double(), s, c, n)
