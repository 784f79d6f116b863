"""``FrechetInceptionDistance``: torchmetrics' ``image.fid.FrechetInceptionDistance`` on the HIP path.

The reference evaluates a trained model with ``val_metrics=[FrechetInceptionDistance(normalize=True), CLIPScore()]``
(scripts/fid-clip-evaluation.py).  Here ``update`` enqueues ``da_inception_preprocess`` -> ``InceptionV3HIP`` ->
``da_feature_moments`` and never synchronises the host; the state is torchmetrics': per side the float64 feature sum, the
float64 sum of outer products and the sample count, in device memory.  ``compute`` all-reduces the state, moves it to the
host and evaluates ``fid_from_moments`` in float64.  The class is named ``FrechetInceptionDistance`` because
``StableDiffusion`` routes and sweeps metrics by class name.

The distances mean something only with torch-fidelity's ``pt_inception-2015-12-05`` weights in ``weights_path``; agreement
with torchmetrics on those weights has NOT been verified (neither the file nor the package is available to the tests).
"""
from __future__ import annotations

import copy
import os
import warnings

import torch

from ..models.composer_shim import Metric

FEATURES = 2048


def _psd_sqrt(s: torch.Tensor) -> torch.Tensor:
    """the symmetric square root of a covariance matrix: eigenvalues below zero (rounding of a rank-deficient matrix) count
    as zero"""
    w, v = torch.linalg.eigh((s + s.T) / 2)
    return (v * w.clamp(min=0).sqrt()) @ v.T


def fid_from_moments(sum_r, cov_r, n_r, sum_f, cov_f, n_f) -> torch.Tensor:
    """torchmetrics' ``compute``: mu = sum / n, Sigma = (cov_sum - n mu mu^T) / (n - 1) per side and
    |mu_r - mu_f|^2 + tr Sigma_r + tr Sigma_f - 2 sum(sqrt(eigvals(Sigma_r Sigma_f)).real), on CPU tensors in float64.

    The eigenvalues of Sigma_r Sigma_f are the squared singular values of Sigma_r^1/2 Sigma_f^1/2, and that is how the last
    term is evaluated: ``eigvals`` of the unsymmetric product returns every zero eigenvalue of a rank-deficient covariance
    (fewer samples than 2048, or collinear features) as +-eps |Sigma_r Sigma_f|, whose square roots add up: with 6 samples
    per side 1.4e-6 (tr Sigma_r + tr Sigma_f) was measured, different from one LAPACK build to the next.  Singular values
    carry no square-root amplification (1e-8 of the traces on the same moments)."""
    n_r, n_f = float(n_r), float(n_f)
    if n_r < 2 or n_f < 2:
        raise RuntimeError('More than one sample is required for both the real and fake distributed to compute FID')
    sum_r, sum_f = (torch.as_tensor(s).detach().to('cpu', torch.float64) for s in (sum_r, sum_f))
    cov_r, cov_f = (torch.as_tensor(c).detach().to('cpu', torch.float64) for c in (cov_r, cov_f))
    mu_r, mu_f = sum_r / n_r, sum_f / n_f
    sig_r = (cov_r - n_r * torch.outer(mu_r, mu_r)) / (n_r - 1)
    sig_f = (cov_f - n_f * torch.outer(mu_f, mu_f)) / (n_f - 1)
    a = (mu_r - mu_f).square().sum()
    b = sig_r.trace() + sig_f.trace()
    c = torch.linalg.svdvals(_psd_sqrt(sig_r) @ _psd_sqrt(sig_f)).sum()
    return a + b - 2 * c


def _check_images(imgs, normalize):
    if not torch.is_tensor(imgs) or imgs.dim() != 4 or imgs.shape[1] != 3 or imgs.shape[0] < 1:
        shape = tuple(imgs.shape) if torch.is_tensor(imgs) else type(imgs).__name__
        raise ValueError(f'FrechetInceptionDistance.update: images must be [B, 3, H, W], got {shape}')
    if normalize and not imgs.is_floating_point():
        raise ValueError(f'FrechetInceptionDistance.update: normalize=True takes float images in [0, 1], got {imgs.dtype}')
    if not normalize and imgs.dtype != torch.uint8:
        raise ValueError(f'FrechetInceptionDistance.update: normalize=False takes uint8 images, got {imgs.dtype}')


class FrechetInceptionDistance(Metric):
    """``update(imgs, real)`` / ``compute()`` / ``reset()`` of torchmetrics' FID at ``feature=2048``.

    ``weights_path``: a local file holding the FID Inception state dict, loaded strictly with ``weights_only=True``; any
    other value gives a RANDOM-INIT tower from a fixed seed (every rank and copy agrees) with a warning - nothing is ever
    fetched.  ``copy.deepcopy`` shares the frozen tower and clones the state."""

    def __init__(self, feature=FEATURES, reset_real_features: bool = True, normalize: bool = False, weights_path=None,
                 device=None, max_batch: int = 32):
        super().__init__()
        if isinstance(feature, bool) or feature != FEATURES:
            raise ValueError(f'FrechetInceptionDistance: feature must be {FEATURES} (the pool3 tap), got {feature!r}')
        if not isinstance(reset_real_features, bool) or not isinstance(normalize, bool):
            raise ValueError('FrechetInceptionDistance: reset_real_features and normalize must be bool')
        from ..models import inception_hip
        if weights_path is not None and os.path.isfile(str(weights_path)):
            sd = inception_hip.load_state_dict_file(str(weights_path))
        else:
            warnings.warn(f'FrechetInceptionDistance: {weights_path!r} is not a local weights file; the Inception tower is '
                          'RANDOM-INIT (nothing is downloaded), the distances are meaningless', stacklevel=2)
            sd = inception_hip.random_state_dict(0)
        self.reset_real_features, self.normalize, self.max_batch = reset_real_features, normalize, int(max_batch)
        self._shared = {'state_dict': sd, 'tower': None}   # what deepcopy shares
        self.dev = torch.device(device if device is not None else ('cuda' if torch.cuda.is_available() else 'cpu'))
        self.state = {side: self._zero_state() for side in ('real', 'fake')}

    def _zero_state(self):
        f64 = dict(dtype=torch.float64, device=self.dev)
        return {'sum': torch.zeros(FEATURES, **f64), 'cov': torch.zeros(FEATURES, FEATURES, **f64),
                'n': torch.zeros(1, **f64)}

    def __deepcopy__(self, memo):
        new = copy.copy(self)   # every attribute shared, the tower among them ...
        for k in ('_parameters', '_buffers', '_modules'):
            setattr(new, k, copy.copy(getattr(self, k)))
        new.state = {side: {k: v.clone() for k, v in st.items()} for side, st in self.state.items()}   # ... except the state
        memo[id(self)] = new
        return new

    def _tower(self):
        if self.dev.type != 'cuda':
            raise RuntimeError('FrechetInceptionDistance runs on an MI355X only (there is no CPU path)')
        if self._shared['tower'] is None:
            from ..models.inception_hip import InceptionV3HIP
            self._shared['tower'] = InceptionV3HIP(self._shared['state_dict'], self.dev, max_batch=self.max_batch)
        return self._shared['tower']

    @torch.no_grad()
    def features(self, imgs: torch.Tensor) -> torch.Tensor:
        """the tower's fp32 [B, 2048] features of one ``update`` input"""
        _check_images(imgs, self.normalize)
        tower = self._tower()
        imgs = imgs.to(self.dev, non_blocking=True)
        if self.normalize:
            imgs = imgs.float()
        return tower(imgs.contiguous())

    @torch.no_grad()
    def update(self, imgs: torch.Tensor, real: bool):
        from .. import ops
        _check_images(imgs, self.normalize)
        feats = self.features(imgs)
        st = self.state['real' if real else 'fake']
        ops.feature_moments(feats, st['sum'], st['cov'], st['n'])

    def compute(self):
        import torch.distributed as dist
        world = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        host = {}
        for side, st in self.state.items():
            for k, v in st.items():
                if world:
                    v = v.clone()
                    dist.all_reduce(v)
                host[side, k] = v.cpu()
        return fid_from_moments(host['real', 'sum'], host['real', 'cov'], host['real', 'n'].item(), host['fake', 'sum'],
                                host['fake', 'cov'], host['fake', 'n'].item())   # float64: the host's own precision

    def reset(self):
        for side, st in self.state.items():
            if side == 'real' and not self.reset_real_features:
                continue
            for v in st.values():
                v.zero_()
