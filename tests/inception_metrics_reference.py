"""Shared by the Inception-score / KID tests: the two metrics' formulas restated in NumPy, independent of the product's host
functions (metrics/inception_score.py, metrics/kid.py).  Every function takes the working ``dtype``: the tests evaluate it in
float64 (the reference) and in ``np.longdouble`` (the reference's own error on the very inputs used), and hold the kernels
to the float64 values.  Written from torchmetrics' documented behaviour; that package is not needed."""
import numpy as np

CAP = 1e-11          # kernels vs the float64 reference: 3+ orders above fp64 rounding, 3 orders below fp32 accumulation
REF_AGREEMENT = 1e-13   # float64 vs longdouble evaluation of the reference on the inputs of each comparison


def chunk_bounds(n, splits):
    """torch.chunk: chunks of ceil(n / splits) rows; the last may be short and there may be fewer than ``splits``"""
    c = -(-n // splits)
    return [(i, min(i + c, n)) for i in range(0, n, c)]


def inception_scores(logits, perm, splits, dtype=np.float64):
    """per chunk of rows ``perm``: exp(mean_i sum_c p_ic (log p_ic - log m_c)), p = softmax(row) through a log-softmax with
    the maximum subtracted, m = mean_i p_i; terms with p_ic == 0 are 0"""
    x = np.asarray(logits).astype(dtype)[np.asarray(perm, np.int64)]
    out = []
    for a, b in chunk_bounds(len(x), splits):
        z = x[a:b] - x[a:b].max(axis=1, keepdims=True)
        lp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
        p = np.exp(lp)
        with np.errstate(divide='ignore', invalid='ignore'):
            t = np.where(p > 0, p * (lp - np.log(p.mean(axis=0, keepdims=True))), dtype(0))
        out.append(np.exp(t.sum(axis=1).mean()))
    return np.array(out, dtype)


def inception_score(logits, perm, splits, dtype=np.float64):
    """(mean, unbiased std) over the chunks, as torch.mean / torch.std give them (one chunk: NaN)"""
    s = inception_scores(logits, perm, splits, dtype)
    with np.errstate(divide='ignore', invalid='ignore'):
        return s.mean(), (s.std(ddof=1) if len(s) > 1 else dtype(np.nan))


_GRAMS = {}


def grams(fr, ff, dtype=np.float64):
    """every dot product the subsets can ask for, once per pair of stores and dtype: (fr fr^T, ff ff^T, fr ff^T).  The
    subsets overlap, so this is cheaper than a product per subset (np.longdouble has no BLAS); the arrays are kept for the
    other kernel parameters run on the same stores."""
    key = (id(fr), id(ff), np.dtype(dtype).name)
    if key not in _GRAMS:
        a, b = np.asarray(fr).astype(dtype), np.asarray(ff).astype(dtype)
        _GRAMS[key] = (fr, ff, a @ a.T, b @ b.T, a @ b.T)   # fr, ff: the ids stay taken while the entry lives
    return _GRAMS[key][2:]


def poly_mmd(fr, ff, idx_r, idx_f, degree=3, gamma=None, coef=1.0, dtype=np.float64):
    """per subset s, with x = fr[idx_r[s]], y = ff[idx_f[s]], k(a, b) = (gamma <a, b> + coef)^degree:
    value = (sum_{i != j} k_xx + sum_{i != j} k_yy) / (m (m - 1)) - 2 sum_ij k_xy / m^2 and the scale the value's error is
    measured against, mean|k_xx| + mean|k_yy| + 2 mean|k_xy| (the value is a small difference of those terms).
    Returns (values [subsets], scales [subsets])."""
    grr, gff, grf = grams(fr, ff, dtype)
    gamma = dtype(1) / dtype(np.asarray(fr).shape[1]) if gamma is None else dtype(gamma)
    vals, scales = [], []
    for ir, jf in zip(np.asarray(idx_r, np.int64), np.asarray(idx_f, np.int64)):
        m = len(ir)
        dots = (grr[np.ix_(ir, ir)], gff[np.ix_(jf, jf)], grf[np.ix_(ir, jf)])
        kxx, kyy, kxy = ((gamma * d + dtype(coef)) ** degree for d in dots)
        off = ~np.eye(m, dtype=bool)
        vals.append((kxx[off].sum() + kyy[off].sum()) / dtype(m * (m - 1)) - 2 * kxy.sum() / dtype(m * m))
        scales.append(np.abs(kxx).mean() + np.abs(kyy).mean() + 2 * np.abs(kxy).mean())
    return np.array(vals, dtype), np.array(scales, dtype)


def kid(fr, ff, idx_r, idx_f, degree=3, gamma=None, coef=1.0, dtype=np.float64):
    """(mean, biased std) over the subsets"""
    v, _ = poly_mmd(fr, ff, idx_r, idx_f, degree, gamma, coef, dtype)
    return v.mean(), v.std(ddof=0)


def fc_bound(F, W):
    """the float64 head and its derived bound: ref = F W^T in float64 and
    |out - ref| <= 2^-24 |ref| + (K + 1) 2^-53 sum_k |F_bk W_ck| (one fp32 rounding of a float64 sum of exact products)"""
    F, W = np.asarray(F, np.float64), np.asarray(W, np.float64)
    ref = F @ W.T
    return ref, 2.0 ** -24 * np.abs(ref) + (F.shape[1] + 1) * 2.0 ** -53 * (np.abs(F) @ np.abs(W).T)


def subset_indices(rng, subsets, m, n):
    """[subsets, m] int32 rows of range(n): unsorted, and overlapping across subsets"""
    return np.stack([rng.permutation(n)[:m] for _ in range(subsets)]).astype(np.int32)
