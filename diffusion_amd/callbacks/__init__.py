"""Callbacks (the reference's ``diffusion.callbacks`` exports)."""
from .log_diffusion_images import LogDiffusionImages

__all__ = ['LogDiffusionImages']
