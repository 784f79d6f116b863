"""``KernelInceptionDistance``: torchmetrics' ``image.kid.KernelInceptionDistance`` on the HIP path.

``update(imgs, real)`` enqueues ``da_inception_preprocess`` -> ``InceptionV3HIP`` and appends the fp32 ``pool3`` features
to the real or the fake device-resident store; it never synchronises the host.  ``compute`` gathers the stores of all ranks,
draws ``subsets`` pairs of ``subset_size`` row indices, and ``da_poly_mmd`` evaluates per subset the unbiased
polynomial-kernel MMD^2 in float64 straight from the stores (rows gathered through the indices, no copy); the result is
(mean, biased std) over the subsets.  ``kid_from_features`` is the same number in plain float64 torch on the CPU.

One deliberate departure from torchmetrics - determinism: the subsets come from a generator this metric owns and re-seeds
with ``seed`` on every ``compute()``, not from the global RNG.  ``compute()`` is idempotent and every rank gets the same
number.

The distances mean something only with torch-fidelity's ``pt_inception-2015-12-05`` weights in ``weights_path``; otherwise
the tower is random-init with a warning, and nothing is fetched.  Agreement with torchmetrics'
``KernelInceptionDistance`` is UNVERIFIED: neither that package nor the weights file is available to the tests; the
formulas are written from the package's documented behaviour.
"""
from __future__ import annotations

import copy

import torch

from ..models.composer_shim import Metric
from . import _inception_shared as shared

FEATURES = 2048


def kid_values(fr, ff, idx_r, idx_f, degree=3, gamma=None, coef=1.0) -> torch.Tensor:
    """float64 [subsets]: with x = fr[idx_r[s]], y = ff[idx_f[s]] and k(a, b) = (gamma <a, b> + coef)^degree,
    (sum_{i != j} k_xx + sum_{i != j} k_yy) / (m (m - 1)) - 2 sum_ij k_xy / m^2 (torchmetrics' ``poly_mmd``)"""
    fr = torch.as_tensor(fr).detach().to('cpu', torch.float64)
    ff = torch.as_tensor(ff).detach().to('cpu', torch.float64)
    idx_r, idx_f = (torch.as_tensor(i).to('cpu', torch.int64) for i in (idx_r, idx_f))
    gamma = 1.0 / fr.shape[1] if gamma is None else float(gamma)
    out = []
    for ir, jf in zip(idx_r, idx_f):
        x, y = fr[ir], ff[jf]
        m = x.shape[0]
        kxx, kyy, kxy = ((a @ b.T * gamma + coef) ** degree for a, b in ((x, x), (y, y), (x, y)))
        off = ~torch.eye(m, dtype=torch.bool)
        out.append((kxx[off].sum() + kyy[off].sum()) / (m * (m - 1)) - 2 * kxy.sum() / (m * m))
    return torch.stack(out)


def kid_from_features(fr, ff, idx_r, idx_f, degree=3, gamma=None, coef=1.0):
    """torchmetrics' ``compute`` on CPU tensors in float64: (mean, std) of the per-subset values; the std is the biased
    one (``unbiased=False``)"""
    v = kid_values(fr, ff, idx_r, idx_f, degree, gamma, coef)
    return v.mean(), v.std(unbiased=False)


def _positive_int(v, name):
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError(f'KernelInceptionDistance: Argument `{name}` expected to be integer larger than 0')


class KernelInceptionDistance(Metric):
    """``update(imgs, real)`` / ``compute() -> (mean, std)`` / ``reset()`` of torchmetrics' KID at ``feature=2048``.
    ``weights_path``, ``normalize``, ``device``, ``max_batch``: as for ``FrechetInceptionDistance``; ``seed`` fixes the
    subsets (see the module docstring).  ``copy.deepcopy`` shares the frozen tower and clones the state."""

    def __init__(self, feature=FEATURES, subsets: int = 100, subset_size: int = 1000, degree: int = 3, gamma=None,
                 coef: float = 1.0, reset_real_features: bool = True, normalize: bool = False, weights_path=None,
                 seed: int = 0, device=None, max_batch: int = 32):
        super().__init__()
        if isinstance(feature, bool) or feature != FEATURES:
            raise ValueError(f'KernelInceptionDistance: feature must be {FEATURES} (the pool3 tap), got {feature!r}')
        _positive_int(subsets, 'subsets')
        _positive_int(subset_size, 'subset_size')
        _positive_int(degree, 'degree')
        if gamma is not None and not (isinstance(gamma, float) and gamma > 0):
            raise ValueError('KernelInceptionDistance: Argument `gamma` expected to be `None` or float larger than 0')
        if isinstance(coef, bool) or not isinstance(coef, (int, float)) or not coef >= 0:
            raise ValueError('KernelInceptionDistance: Argument `coef` expected to be float larger or equal to 0')
        if not isinstance(reset_real_features, bool) or not isinstance(normalize, bool):
            raise ValueError('KernelInceptionDistance: reset_real_features and normalize must be bool')
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f'KernelInceptionDistance: seed must be an int, got {seed!r}')
        shared.get_state_dict(weights_path, 'KernelInceptionDistance')   # strict check of a file, the warning without one
        self.subsets, self.subset_size, self.degree, self.gamma, self.coef = subsets, subset_size, degree, gamma, float(coef)
        self.reset_real_features, self.normalize, self.seed, self.max_batch = reset_real_features, normalize, seed, int(max_batch)
        self.weights_path = weights_path
        self.dev = torch.device(device if device is not None else ('cuda' if torch.cuda.is_available() else 'cpu'))
        self.stores = {side: shared.RowStore(FEATURES, self.dev) for side in ('real', 'fake')}

    def __deepcopy__(self, memo):
        new = copy.copy(self)
        for k in ('_parameters', '_buffers', '_modules'):
            setattr(new, k, copy.copy(getattr(self, k)))
        new.stores = {side: st.clone() for side, st in self.stores.items()}
        memo[id(self)] = new
        return new

    def _tower(self):
        return shared.get_tower(self.weights_path, self.dev, self.max_batch, 'KernelInceptionDistance')

    @torch.no_grad()
    def update(self, imgs: torch.Tensor, real: bool):
        shared.check_images(imgs, self.normalize, 'KernelInceptionDistance')
        tower = self._tower()
        imgs = imgs.to(self.dev, non_blocking=True)
        if self.normalize:
            imgs = imgs.float()
        self.stores['real' if real else 'fake'].append(tower(imgs.contiguous()))

    def features(self, real: bool) -> torch.Tensor:
        """this rank's stored features of one side, fp32 [n, 2048]"""
        return self.stores['real' if real else 'fake'].rows()

    def subset_indices(self, n_real: int, n_fake: int):
        """the subsets ``compute`` uses: two int32 [subsets, subset_size] CPU tensors; per subset a ``randperm`` prefix of
        the real rows, then one of the fake rows, from a fresh generator seeded with ``seed``"""
        g = torch.Generator().manual_seed(self.seed)
        m = self.subset_size
        ir, jf = [], []
        for _ in range(self.subsets):
            ir.append(torch.randperm(int(n_real), generator=g)[:m])
            jf.append(torch.randperm(int(n_fake), generator=g)[:m])
        return torch.stack(ir).to(torch.int32), torch.stack(jf).to(torch.int32)

    @torch.no_grad()
    def compute(self):
        from .. import ops
        fr = shared.gather_rows(self.stores['real'].buf, self.stores['real'].n)
        ff = shared.gather_rows(self.stores['fake'].buf, self.stores['fake'].n)
        if fr.shape[0] < self.subset_size or ff.shape[0] < self.subset_size:
            raise ValueError('Argument `subset_size` should be smaller than the number of samples')
        if fr.device.type != 'cuda':
            raise RuntimeError('KernelInceptionDistance runs on an MI355X only (there is no CPU path)')
        idx_r, idx_f = self.subset_indices(fr.shape[0], ff.shape[0])
        v = ops.poly_mmd(fr, ff, idx_r, idx_f, self.degree, self.gamma, self.coef).cpu()
        return v.mean(), v.std(unbiased=False)

    def reset(self):
        self.stores['fake'].reset()
        if self.reset_real_features:
            self.stores['real'].reset()
