"""Dataloader builders (the reference's ``diffusion.datasets`` exports)."""
from .coco.coco_captions import build_streaming_cocoval_dataloader
from .laion.laion import build_streaming_laion_dataloader

__all__ = ['build_streaming_cocoval_dataloader', 'build_streaming_laion_dataloader']
