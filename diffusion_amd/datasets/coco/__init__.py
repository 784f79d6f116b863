from .coco_captions import StreamingCOCOCaption, build_streaming_cocoval_dataloader

__all__ = ['StreamingCOCOCaption', 'build_streaming_cocoval_dataloader']
