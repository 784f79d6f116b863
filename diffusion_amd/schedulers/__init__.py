"""Custom schedulers for diffusion models (the reference's ``diffusion.schedulers`` package)."""
from .schedulers import ContinuousTimeScheduler, tangent_schedule

__all__ = ['ContinuousTimeScheduler', 'tangent_schedule']
