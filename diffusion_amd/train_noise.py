"""Per-sample training noise: the options of the noising step, and the seeds its in-kernel draws are keyed by.

With ``noise_source='philox'`` a training step draws nothing from torch's generator.  Every sample of the global batch gets a
64-bit seed that is a function of (the run's seed, the optimizer step, the sample's place in the global batch), and the noising
launch (``ops.add_noise_rng`` / ``da_add_noise_rng``) draws the sample's timestep, noise, offset and perturbation from the
Philox stream under that seed.  So what a sample is trained on does not depend on how the batch is split into microbatches or
over ranks, a resumed run reproduces the draws from the batch index alone, and the draw sits inside a captured microbatch.

The options, the Philox restatement and the seed derivation are host code; ``add_noise`` (the models' one launch) and
``batch_entries`` (the trainer's upload of seeds and strata) are the two places that touch the device.
"""
from __future__ import annotations

import math
import numbers
from dataclasses import dataclass
from typing import List, Optional, Tuple

M0, M1 = 0xD2511F53, 0xCD9E8D57     # the round multipliers of Philox4x32 (csrc/philox.hpp)
W0, W1 = 0x9E3779B9, 0xBB67AE85     # the Weyl constants the key is bumped by
MASK = 0xFFFFFFFF
SEED_DOMAIN = 0x7472616e            # 'tran': the fourth counter word of the seed derivation

NOISE_SOURCES = ('torch', 'philox')
TIMESTEP_SAMPLINGS = ('uniform', 'stratified')


def philox4x32_10(counter, key) -> Tuple[int, int, int, int]:
    """Philox4x32-10 (Salmon et al., SC'11) on Python integers: ``counter`` four and ``key`` two 32-bit words."""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def _uint64(v, name) -> int:
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= int(v) < 2**64:
        raise ValueError(f'{name} must be an integer in [0, 2^64), got {v!r}')
    return int(v)


def sample_seeds(run_seed: int, batch_idx: int, first_position: int, n: int) -> List[int]:
    """The seeds of positions ``first_position .. first_position + n - 1`` of global batch ``batch_idx``: for position g,
    ``r0 | r1 << 32`` of Philox with counter (g, batch_idx & 0xffffffff, batch_idx >> 32, 'tran') and the run's seed as the
    key.  A function of the run's seed, the optimizer step and the sample's place in the GLOBAL batch, and of nothing else."""
    run_seed, batch_idx = _uint64(run_seed, 'run_seed'), _uint64(batch_idx, 'batch_idx')
    first_position, n = int(first_position), int(n)
    if first_position < 0 or n < 0 or first_position + n > 2**32:
        raise ValueError(f'positions {first_position} .. {first_position + n} must lie in [0, 2^32]')
    key = (run_seed & MASK, run_seed >> 32)
    out = []
    for g in range(first_position, first_position + n):
        r = philox4x32_10((g, batch_idx & MASK, batch_idx >> 32, SEED_DOMAIN), key)
        out.append(r[0] | r[1] << 32)
    return out


def discrete_timestep(r0: int, t_lo: int, t_hi: int, slot: Optional[int] = None, n_slots: int = 0) -> int:
    """The integer timestep ``da_add_noise_rng`` makes of the Philox word ``r0`` (host restatement, exact)."""
    R = t_hi - t_lo
    if slot is None:
        return t_lo + ((r0 * R) >> 32)
    return t_lo + ((slot << 32 | r0) * R) // (n_slots << 32)


@dataclass(frozen=True)
class TrainNoise:
    """The noising options of a model.  ``noise_source='torch'`` (the default) is the reference's: timesteps and noise from
    torch's generator, once per microbatch; every other knob needs ``'philox'``.

    ``noise_offset``: n += offset * randn(B, C, 1, 1) (diffusers ``--noise_offset``), part of the target.
    ``input_perturbation``: x_t is made from n + gamma * randn_like(n), the target keeps n (Ning et al., arXiv:2301.11706).
    ``timestep_range``: (lo, hi), timesteps drawn from [lo, hi): integers inside the table for a discrete schedule, fractions of
    ``t_max`` in [0, 1] for continuous time.  ``timestep_sampling='stratified'``: sample g of a global batch of N draws from the
    g-th of N equal strata of the range."""
    noise_source: str = 'torch'
    noise_offset: float = 0.0
    input_perturbation: float = 0.0
    timestep_range: Optional[Tuple] = None
    timestep_sampling: str = 'uniform'

    def __post_init__(self):
        if self.noise_source not in NOISE_SOURCES:
            raise ValueError(f'noise_source must be one of {NOISE_SOURCES}, got {self.noise_source!r}')
        if self.timestep_sampling not in TIMESTEP_SAMPLINGS:
            raise ValueError(f'timestep_sampling must be one of {TIMESTEP_SAMPLINGS}, got {self.timestep_sampling!r}')
        for name in ('noise_offset', 'input_perturbation'):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v < 0:
                raise ValueError(f'{name} must be a finite number >= 0, got {v!r}')
            object.__setattr__(self, name, float(v))
        r = self.timestep_range
        if r is not None:
            try:
                lo, hi = r
            except (TypeError, ValueError):
                raise ValueError(f'timestep_range must be (lo, hi), got {r!r}') from None
            if any(isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) for v in (lo, hi)) \
                    or not 0 <= lo < hi:
                raise ValueError(f'timestep_range must be (lo, hi) with 0 <= lo < hi, got {r!r}')
            object.__setattr__(self, 'timestep_range', (lo, hi))
        if not self.philox and (self.noise_offset or self.input_perturbation or r is not None
                                or self.timestep_sampling != 'uniform'):
            raise ValueError("noise_offset, input_perturbation, timestep_range and timestep_sampling are drawn in the noising "
                             "kernel: they need noise_source='philox'")

    @property
    def philox(self) -> bool:
        return self.noise_source == 'philox'

    @property
    def stratified(self) -> bool:
        return self.timestep_sampling == 'stratified'

    def key(self) -> Tuple:
        """what a captured microbatch depends on"""
        return (self.noise_source, self.noise_offset, self.input_perturbation, self.timestep_range, self.timestep_sampling)

    def discrete_range(self, table_len: int) -> Tuple[int, int]:
        """(lo, hi) inside a table of ``table_len`` timesteps; ``ValueError`` for a fractional or out-of-table range."""
        if self.timestep_range is None:
            return 0, int(table_len)
        lo, hi = self.timestep_range
        if any(not isinstance(v, numbers.Integral) for v in (lo, hi)) or hi > table_len:
            raise ValueError(f'timestep_range {self.timestep_range} must be integers inside [0, {table_len}]')
        return int(lo), int(hi)

    def continuous_range(self, t_max: float) -> Tuple[float, float]:
        """(lo, hi) as fp32 values: the range's fractions (at most 1) of ``t_max``, rounded to fp32 like ``t_max`` itself."""
        import numpy as np
        lo, hi = (0.0, 1.0) if self.timestep_range is None else self.timestep_range
        if hi > 1:
            raise ValueError(f'timestep_range {self.timestep_range} of a continuous-time model is in fractions of t_max: '
                             'it must lie inside [0, 1]')
        lo, hi = float(np.float32(np.float32(t_max) * np.float32(lo))), float(np.float32(np.float32(t_max) * np.float32(hi)))
        if not lo < hi:
            raise ValueError(f'timestep_range {self.timestep_range} is empty at t_max = {t_max}')
        return lo, hi


def check_injected(options: TrainNoise, noise) -> None:
    """An injected noise tensor has no place in philox mode: the kernel would draw its own."""
    if options.philox and noise is not None:
        raise ValueError("an injected noise tensor ('_noise' / noise=) cannot be combined with noise_source='philox': "
                         'the noising kernel draws the noise itself (inject _sample_seeds instead)')


def generator_seeds(B: int, device, generator=None):
    """B seeds (uint64 on ``device``) from torch's generator there: what a batch without '_sample_seeds' is noised with"""
    import torch
    w = torch.randint(0, 2**32, (2, B), device=device, dtype=torch.int64, generator=generator)
    return ((w[0] << 32) | w[1]).view(torch.uint64)


def add_noise(options: TrainNoise, batch, x0, timesteps, prediction_type, tables=None, t_max=None, generator=None):
    """The one fused noising launch of a philox-mode ``forward``: returns ``(xt, target8, t)``, all device tensors.  ``x0``
    fp32 NCHW on the device; ``tables`` = (sqrt_ac, sqrt_1mac) for a discrete schedule, else ``t_max`` for continuous time.
    Seeds come from ``batch['_sample_seeds']``, else B of them are drawn from torch's generator on the device (so
    ``torch.manual_seed`` still governs a bare ``forward``); strata from ``batch['_sample_slots']`` / ``['_n_slots']``, else
    the batch is its own global batch.  ``timesteps`` given: read, not drawn."""
    import torch
    from . import ops
    dev = x0.device
    B, _, H, W = x0.shape
    seeds = batch.get('_sample_seeds')
    if seeds is None:
        seeds = generator_seeds(B, dev, generator)
    seeds = ops.philox_seeds(seeds, B, dev)
    slots, n_slots = None, 0
    if options.stratified:
        slots, n_slots = batch.get('_sample_slots'), batch.get('_n_slots')
        if (slots is None) != (n_slots is None):
            raise ValueError("stratified timesteps: '_sample_slots' and '_n_slots' go together")
        if slots is None:
            slots, n_slots = torch.arange(B, dtype=torch.int32, device=dev), B
        slots = slots.to(dev, torch.int32).contiguous()
    continuous = tables is None
    t_range = options.continuous_range(t_max) if continuous else options.discrete_range(int(tables[0].numel()))
    dtype = torch.float32 if continuous else torch.int64
    draw = timesteps is None
    t = torch.empty(B, device=dev, dtype=dtype) if draw else timesteps.to(dev, dtype).contiguous()
    xt = torch.empty(B * H * W, 8, device=dev, dtype=torch.bfloat16)
    target8 = torch.empty(B * H * W, 8, device=dev, dtype=torch.float32)
    sa, sb = (None, None) if continuous else tables
    ops.add_noise_rng(x0, seeds, t, xt, target8, prediction_type, sa, sb, draw_t=draw, t_range=t_range, slots=slots,
                      n_slots=int(n_slots), noise_offset=options.noise_offset, perturbation=options.input_perturbation)
    return xt, target8, t


def batch_entries(run_seed: int, batch_idx: int, rank: int, world: int, n: int, device=None) -> dict:
    """What the trainer puts into a per-rank batch of ``n`` samples before it slices microbatches: the seeds and the global
    positions of the rank's samples.  Tensors sliced by ``[s:s + mb]`` carry them along."""
    import torch
    from . import ops
    first = int(rank) * int(n)
    return {'_sample_seeds': ops.philox_seeds(sample_seeds(run_seed, batch_idx, first, n), n, device),
            '_sample_slots': torch.arange(first, first + n, dtype=torch.int32, device=device),
            '_n_slots': int(n) * int(world)}
