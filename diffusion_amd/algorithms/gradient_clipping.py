"""Gradient clipping by global norm (composer.algorithms.GradientClipping with ``clipping_type: norm``, i.e.
torch.nn.utils.clip_grad_norm_ over all parameters), on the device.

The algorithm only sets FusedAdamW's ``clip_max_norm`` (and turns the non-finite guard on): the optimizer step then runs
the segmented sum-of-squares pass over the flat gradient buffer and AdamW reads its gradient multiplier
grad_scale * min(1, threshold / (norm + 1e-6)) from device memory - the gradient buffer itself is never rescaled and
nothing returns to the host.  A step whose gradient holds an inf or NaN is skipped (FusedAdamW.step)."""
from __future__ import annotations

from ..trainer import Callback


class GradientClipping(Callback):

    def __init__(self, clipping_type: str = 'norm', clipping_threshold: float = 1.0, **kw):
        if clipping_type in ('value', 'adaptive'):
            raise NotImplementedError(f"GradientClipping: clipping_type={clipping_type!r} is not implemented (only 'norm')")
        if clipping_type != 'norm':
            raise ValueError(f"GradientClipping: unknown clipping_type {clipping_type!r} ('norm', 'value', 'adaptive')")
        clipping_threshold = float(clipping_threshold)
        if not clipping_threshold >= 0:
            raise ValueError(f'GradientClipping: clipping_threshold must be >= 0, got {clipping_threshold}')
        self.clipping_type = clipping_type
        self.clipping_threshold = clipping_threshold

    def configure_optimizer(self, optimizer):
        """Called by the trainer at construction (it has to know then that AdamW cannot run in slices) and before every
        optimizer step."""
        optimizer.clip_max_norm = self.clipping_threshold
        optimizer.guard_nonfinite = True

    def before_optimizer_step(self, trainer):
        self.configure_optimizer(trainer.optimizer)

    def state_dict(self):
        return {'clipping_type': self.clipping_type, 'clipping_threshold': self.clipping_threshold}

    def load_state_dict(self, sd):
        pass   # the YAML's threshold wins over a checkpoint's
