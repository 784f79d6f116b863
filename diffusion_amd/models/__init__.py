"""Diffusion models (the reference's ``diffusion.models`` exports)."""
from .models import continuous_pixel_diffusion, discrete_pixel_diffusion, stable_diffusion_2
from .pixel_diffusion import PixelDiffusion
from .stable_diffusion import StableDiffusion

__all__ = [
    'continuous_pixel_diffusion',
    'discrete_pixel_diffusion',
    'PixelDiffusion',
    'stable_diffusion_2',
    'StableDiffusion',
]
