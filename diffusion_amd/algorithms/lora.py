"""LoRA fine-tuning as a trainer algorithm: low-rank adapters on a frozen U-Net (diffusion_amd/lora.py).

From YAML: ``algorithms: {lora: {_target_: diffusion.algorithms.lora.LoRA, rank: 16}}``.  The algorithm attaches the
adapters to the optimizer's U-Net (fresh ones, or those of ``load_path``) and switches FusedAdamW to its adapter mode: the
step then projects the dense weight gradient onto the adapters, updates them and re-merges the bf16 weight shadows.  Multi-GPU
runs keep the dense gradient exchange (the projection is linear in dW and runs after it); exchanging only the adapter
gradients is not implemented.  Not with EMA, which averages the frozen master; with ``use_graphs`` the step runs eagerly."""
from __future__ import annotations

from typing import Optional, Sequence

from ..trainer import Callback


class LoRA(Callback):

    def __init__(self, rank: int = 16, alpha: Optional[float] = None, target_modules: Optional[Sequence[str]] = None,
                 seed: int = 17, load_path: Optional[str] = None, **kw):
        from ..lora import MAX_RANK
        if isinstance(rank, bool) or int(rank) != rank or not 1 <= int(rank) <= MAX_RANK:
            raise ValueError(f'LoRA: rank must be an integer in 1..{MAX_RANK}, got {rank!r}')
        self.rank, self.alpha, self.seed, self.load_path = int(rank), alpha, int(seed), load_path
        self.target_modules = list(target_modules) if target_modules else None

    def configure_optimizer(self, optimizer):
        """Called by the trainer at construction: attach the adapters (once) and put the optimizer in adapter mode."""
        unet = optimizer.unet
        if getattr(optimizer, 'ema', None) is not None:
            raise ValueError('LoRA cannot be combined with EMA: the average is over the frozen master')
        if unet.lora is None:
            if self.load_path:
                unet.load_lora(self.load_path)
            else:
                unet.add_lora(self.rank, self.alpha, self.target_modules, self.seed)
        if optimizer.lora is not unet.lora:
            optimizer.attach_lora()

    def before_optimizer_step(self, trainer):
        if trainer.optimizer.ema is not None:
            raise ValueError('LoRA cannot be combined with EMA: the average is over the frozen master')

    def state_dict(self):
        return {'rank': self.rank, 'alpha': self.alpha, 'target_modules': self.target_modules}

    def load_state_dict(self, sd):
        pass   # the adapter tensors and their moments travel in the optimizer's state
