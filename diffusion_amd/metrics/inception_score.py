"""``InceptionScore``: torchmetrics' ``image.inception.InceptionScore`` on the HIP path.

``update`` enqueues ``da_inception_preprocess`` -> ``InceptionV3HIP`` -> ``da_fc_logits_f32`` (torch-fidelity's
``logits_unbiased``: the 1008 logits without the bias) and appends the fp32 logits to a device-resident store; it never
synchronises the host.  ``compute`` gathers the stores of all ranks, permutes the rows, and ``da_inception_score`` evaluates
per ``torch.chunk`` split exp(mean_i KL(p_i || mean_i p_i)) in float64; the result is (mean, unbiased std) over the splits.
``inception_score_from_logits`` is the same number in plain float64 torch on the CPU: the definition.

One deliberate departure from torchmetrics - determinism: the permutation comes from a generator this metric owns and
re-seeds with ``seed`` on every ``compute()``, not from the global RNG.  ``compute()`` is idempotent and every rank gets the
same number.

The scores mean something only with torch-fidelity's ``pt_inception-2015-12-05`` weights in ``weights_path`` (tower and
``fc.weight``); otherwise tower AND head are random-init with a warning, and nothing is fetched.  Agreement with
torchmetrics' ``InceptionScore`` is UNVERIFIED: neither that package nor the weights file is available to the tests; the
formulas are written from the package's documented behaviour.
"""
from __future__ import annotations

import copy

import torch

from ..models.composer_shim import Metric
from . import _inception_shared as shared

CLASSES = 1008


def inception_scores_per_split(logits, perm, splits) -> torch.Tensor:
    """float64 [chunks]: rows ``perm`` of ``logits``, cut as ``torch.chunk(splits)`` cuts them; per chunk
    exp(mean_i sum_c p_ic (log p_ic - log m_c)) with p = softmax and m = mean_i p_i; terms with p_ic == 0 are 0"""
    x = torch.as_tensor(logits).detach().to('cpu', torch.float64)
    x = x[torch.as_tensor(perm).to('cpu', torch.int64)]
    lp = torch.log_softmax(x, dim=1)
    p = lp.exp()
    out = []
    for pc, lpc in zip(p.chunk(int(splits), dim=0), lp.chunk(int(splits), dim=0)):
        log_m = pc.mean(dim=0, keepdim=True).log()
        kl = torch.where(pc > 0, pc * (lpc - log_m), torch.zeros_like(pc)).sum(dim=1)
        out.append(kl.mean().exp())
    return torch.stack(out)


def inception_score_from_logits(logits, perm, splits):
    """torchmetrics' ``compute`` on CPU tensors in float64: (mean, std) of the per-split scores; the std is the unbiased
    one of ``torch.std`` (NaN for a single split)"""
    return _mean_std(inception_scores_per_split(logits, perm, splits))


def _mean_std(s: torch.Tensor):
    """(mean, unbiased std) of a float64 CPU vector; one element gives NaN, as ``torch.std`` does (without its warning)"""
    return s.mean(), (s.std() if s.numel() > 1 else torch.full((), float('nan'), dtype=s.dtype))


class InceptionScore(Metric):
    """``update(imgs)`` / ``compute() -> (mean, std)`` / ``reset()`` of torchmetrics' Inception score at
    ``feature='logits_unbiased'``.  ``weights_path``, ``normalize``, ``device``, ``max_batch``: as for
    ``FrechetInceptionDistance``; ``seed`` fixes the row permutation (see the module docstring).  ``copy.deepcopy`` shares
    the frozen tower and clones the state."""

    def __init__(self, feature='logits_unbiased', splits: int = 10, normalize: bool = False, weights_path=None, seed: int = 0,
                 device=None, max_batch: int = 32):
        super().__init__()
        if feature != 'logits_unbiased':
            raise ValueError(f"InceptionScore: feature must be 'logits_unbiased', got {feature!r}")
        if isinstance(splits, bool) or not isinstance(splits, int) or splits < 1:
            raise ValueError(f'InceptionScore: splits must be a positive int, got {splits!r}')
        if not isinstance(normalize, bool):
            raise ValueError('InceptionScore: normalize must be bool')
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f'InceptionScore: seed must be an int, got {seed!r}')
        shared.get_state_dict(weights_path, 'InceptionScore')   # strict check of a file, the warning without one
        self.splits, self.normalize, self.seed, self.max_batch = splits, normalize, seed, int(max_batch)
        self.weights_path = weights_path
        self.dev = torch.device(device if device is not None else ('cuda' if torch.cuda.is_available() else 'cpu'))
        self.store = shared.RowStore(CLASSES, self.dev)

    def __deepcopy__(self, memo):
        new = copy.copy(self)
        for k in ('_parameters', '_buffers', '_modules'):
            setattr(new, k, copy.copy(getattr(self, k)))
        new.store = self.store.clone()
        memo[id(self)] = new
        return new

    def _tower(self):
        return shared.get_tower(self.weights_path, self.dev, self.max_batch, 'InceptionScore')

    @torch.no_grad()
    def update(self, imgs: torch.Tensor):
        shared.check_images(imgs, self.normalize, 'InceptionScore')
        tower = self._tower()
        imgs = imgs.to(self.dev, non_blocking=True)
        if self.normalize:
            imgs = imgs.float()
        self.store.append(tower.logits_unbiased(tower(imgs.contiguous())))

    def logits(self) -> torch.Tensor:
        """this rank's stored logits, fp32 [n, 1008]"""
        return self.store.rows()

    def permutation(self, n: int) -> torch.Tensor:
        """the row order ``compute`` uses for n rows: int32 [n] on the CPU, from a fresh generator seeded with ``seed``"""
        return torch.randperm(int(n), generator=torch.Generator().manual_seed(self.seed)).to(torch.int32)

    @torch.no_grad()
    def compute(self):
        from .. import ops
        rows = shared.gather_rows(self.store.buf, self.store.n)
        if rows.shape[0] < 1:
            raise RuntimeError('InceptionScore.compute: no samples')
        if rows.device.type != 'cuda':
            raise RuntimeError('InceptionScore runs on an MI355X only (there is no CPU path)')
        return _mean_std(ops.inception_score(rows, self.permutation(rows.shape[0]), self.splits).cpu())

    def reset(self):
        self.store.reset()
