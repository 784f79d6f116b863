"""What ``InceptionScore`` and ``KernelInceptionDistance`` share: one Inception tower per weights file, the device-resident row
store their per-image outputs go to, and the gather of such stores over the ranks."""
from __future__ import annotations

import os
import warnings

import torch

from .fid import _check_images

_STATE_DICTS = {}   # weights key -> state dict (with 'fc.weight')
_TOWERS = {}        # (weights key, device, max_batch) -> InceptionV3HIP


def _key(weights_path):
    return os.path.abspath(str(weights_path)) if weights_path is not None and os.path.isfile(str(weights_path)) else None


def get_state_dict(weights_path, who='metric'):
    """the FID Inception state dict of a local file (checked strictly), else the seeded RANDOM-INIT tower and head with a
    warning; nothing is ever fetched.  Cached per file."""
    from ..models import inception_hip
    key = _key(weights_path)
    if key is None:
        warnings.warn(f'{who}: {weights_path!r} is not a local weights file; the Inception tower and its logits head are '
                      'RANDOM-INIT (nothing is downloaded), the values are meaningless', stacklevel=3)
    if key not in _STATE_DICTS:
        if key is None:
            sd = inception_hip.random_state_dict(0)
            sd['fc.weight'] = inception_hip.random_fc_weight(0)
        else:
            sd = inception_hip.load_state_dict_file(key)
        _STATE_DICTS[key] = sd
    return _STATE_DICTS[key]


def get_tower(weights_path, device, max_batch: int = 32, who='metric'):
    """the one ``InceptionV3HIP`` of (weights file, device, max_batch): the two metrics and their deep copies across
    guidance scales walk the same weights and buffers"""
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError(f'{who} runs on an MI355X only (there is no CPU path)')
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    k = (_key(weights_path), str(device), int(max_batch))
    if k not in _TOWERS:
        from ..models.inception_hip import InceptionV3HIP
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')   # the constructor of the metric has warned already
            sd = get_state_dict(weights_path, who)
        _TOWERS[k] = InceptionV3HIP(sd, device, max_batch=int(max_batch))
    return _TOWERS[k]


def check_images(imgs, normalize, who):
    """``fid._check_images`` under this metric's name"""
    try:
        _check_images(imgs, normalize)
    except ValueError as e:
        raise ValueError(str(e).replace('FrechetInceptionDistance', who)) from None


class RowStore:
    """fp32 rows [n, width] in device memory; the allocation doubles when it is full and is kept by ``reset``.  The row
    count is host state (batch sizes are known on the host), so appending never synchronises."""

    def __init__(self, width, device, capacity=64):
        self.width, self.dev = int(width), torch.device(device)
        self.buf = torch.empty(int(capacity), self.width, device=self.dev, dtype=torch.float32)
        self.n = 0

    def append(self, rows):
        b = rows.shape[0]
        if self.n + b > self.buf.shape[0]:
            cap = self.buf.shape[0]
            while cap < self.n + b:
                cap *= 2
            new = torch.empty(cap, self.width, device=self.dev, dtype=torch.float32)
            new[:self.n] = self.buf[:self.n]
            self.buf = new
        self.buf[self.n:self.n + b] = rows
        self.n += b

    def rows(self):
        return self.buf[:self.n]

    def reset(self):
        self.n = 0

    def clone(self):
        new = RowStore(self.width, self.dev, self.buf.shape[0])
        new.buf[:self.n] = self.buf[:self.n]
        new.n = self.n
        return new


def gather_rows(store: torch.Tensor, n: int) -> torch.Tensor:
    """rows [:n] of every rank's ``store``, concatenated rank-major: the counts are all-gathered, each rank pads to the
    largest, one ``all_gather``, then the padding is trimmed.  At world size 1 this is the ``[:n]`` view."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return store[:n]
    world = dist.get_world_size()
    counts = [torch.zeros(1, dtype=torch.int64, device=store.device) for _ in range(world)]
    dist.all_gather(counts, torch.tensor([int(n)], dtype=torch.int64, device=store.device))
    counts = [int(c.item()) for c in counts]
    padded = torch.zeros(max(max(counts), 1), store.shape[1], dtype=store.dtype, device=store.device)
    padded[:n] = store[:n]
    parts = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(parts, padded)
    return torch.cat([p[:c] for p, c in zip(parts, counts)])
