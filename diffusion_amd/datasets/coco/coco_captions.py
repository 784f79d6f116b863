"""COCO-val evaluation dataloader - the reference's diffusion/datasets/coco/coco_captions.py on the raw-image route.

``build_streaming_cocoval_dataloader`` keeps the reference's signature (coco_captions.py:93-103).  It reads a local MDS
directory (``datasets/mds.py``) with an ``image`` column (``jpeg``, ``png``, ``pil`` or ``bytes``) and a ``captions`` column (a
``json`` list, or a single ``str``): what scripts/convert_coco.py:55 writes.  As on the training route
(``datasets/image_ingest.py``) a worker only decodes; the packed ``uint8`` pixels go to the device and one kernel
(``ops.image_resize``) does the reference's transform there.  The reference has two (:105-108), neither with a ``Normalize``:

  ``use_crop=True``   LargestCenterSquare(R) -> ToTensor: the training geometry and filter, output in [0, 1];
  ``use_crop=False``  ToTensor -> Resize((R, R)), the default: torchvision's tensor resize, which stretches to R x R on the
                      float values with ``F.interpolate(mode='bilinear', align_corners=False)``.  The torchvision of the
                      reference's era (0.14 / 0.15: ``antialias=None`` / ``'warn'``) resolves that to ``antialias=False``, a
                      two-tap filter, so that is the default here; ``antialias=True`` gives what current torchvision computes.

A batch carries the transform as plain data next to ``image_size``: ``batch['image_transform'] = {'geometry', 'filter',
'range'}`` (the ``ops.image_resize`` switches), which ``StableDiffusion.ingest_raw`` turns into the reference's fp32
``image`` tensor.

Partition.  ``drop_last=False`` as in the reference, and over the ranks of a data-parallel job rank ``r`` reads samples
``r, r + world, ...`` of the (optionally shuffled) order with NO padding sample: an evaluation metric must not count an image
twice.  The ranks may therefore differ by one sample and by one batch; ``Trainer.eval()`` has no collective before the
final reduction of the metric states, so unequal batch counts are safe there."""
from __future__ import annotations

import os
import random
from typing import Optional

import torch
from torch.utils.data import Dataset

from ..image_ingest import collate_raw_images, decode_rgb
from ..laion.laion import EpochDataLoader, EpochRandomSampler, ResumableBatchSampler, _as_list

CAPTION_SELECTIONS = ('random', 'first')


class StreamingCOCOCaption(Dataset):
    """One local MDS directory of COCO samples (coco_captions.py:17-90) without the image transform: yields
    ``{'image_u8': uint8 [h, w, 3], 'captions': int64 [77]}``; batches are built by ``collate_raw_images``."""

    def __init__(self, local: str, tokenizer, caption_selection: str = 'first'):
        from ..mds import MDSDirectory
        self.caption_selection = str(caption_selection).lower()
        if self.caption_selection not in CAPTION_SELECTIONS:
            raise ValueError(f'caption selection {caption_selection!r}: one of {CAPTION_SELECTIONS} expected')
        self.mds = MDSDirectory(local)
        self.tokenizer = tokenizer

    def __len__(self):
        return len(self.mds)

    def __getitem__(self, index):
        smp = self.mds.get(index, columns=('image', 'captions'))
        image = smp['image']
        if isinstance(image, (bytes, bytearray, memoryview)):   # jpeg / png / bytes: the encoded file; pil is decoded already
            image = decode_rgb(bytes(image))
        captions = smp['captions']
        if isinstance(captions, str):
            captions = [captions]
        caption = captions[0] if self.caption_selection == 'first' else random.sample(list(captions), k=1)[0]
        ids = self.tokenizer(caption, padding='max_length', max_length=77, truncation=True)['input_ids']
        return {'image_u8': torch.from_numpy(image), 'captions': torch.as_tensor(ids, dtype=torch.int64)}


class StridedSampler(torch.utils.data.Sampler):
    """Rank ``rank`` of ``world``: elements ``rank, rank + world, ...`` of the order ``sampler`` gives, unpadded - the ranks'
    indices are disjoint and jointly exhaustive, and their counts differ by at most one."""

    def __init__(self, sampler, rank: int, world: int):
        if not 0 <= rank < world:
            raise ValueError(f'rank {rank} outside 0..{world - 1}')
        self.sampler, self.rank, self.world = sampler, int(rank), int(world)

    def set_epoch(self, epoch: int):
        if hasattr(self.sampler, 'set_epoch'):
            self.sampler.set_epoch(epoch)

    def __iter__(self):
        return iter(list(self.sampler)[self.rank::self.world])

    def __len__(self):
        return len(range(self.rank, len(self.sampler), self.world))


def build_streaming_cocoval_dataloader(
    batch_size: int,
    remote: str,
    local: str = '/tmp/mds-cache/mds-coco-val/',
    shuffle: bool = False,
    resize_size: int = 512,
    use_crop: bool = False,
    caption_selection='first',
    num_canonical_nodes: Optional[int] = None,
    **dataloader_kwargs,
):
    """Builds the dataloader for the COCO validation set (module docstring).  Popped from ``dataloader_kwargs``:
    ``antialias`` (default False, the stretch route's filter), ``tokenizer_name_or_path`` (a local directory, else the built-in
    tokenizer - nothing is fetched), ``seed`` (the shuffle's), ``rank`` / ``world`` (default: the process group's)."""
    antialias = bool(dataloader_kwargs.pop('antialias', False))
    tokenizer_name_or_path = dataloader_kwargs.pop('tokenizer_name_or_path', None)
    seed = int(dataloader_kwargs.pop('seed', 17))
    rank, world = dataloader_kwargs.pop('rank', None), dataloader_kwargs.pop('world', None)
    local = _as_list(local)
    if len(local) != 1:
        if _as_list(remote) and not local:
            raise ValueError('a remote without a local cache directory cannot be read here: mosaicml-streaming (download-on-'
                             'miss) is not available; point `local` at a directory that already holds the shards')
        raise ValueError(f'the COCO loader reads one local MDS directory, got local={local!r}')
    if not os.path.isdir(local[0]):   # never anything but the named data
        raise FileNotFoundError(f'local dataset directory not found: {local[0]}')
    from ...models.text import build_tokenizer
    tok = build_tokenizer(tokenizer_name_or_path if os.path.isdir(str(tokenizer_name_or_path)) else None)
    dataset = StreamingCOCOCaption(local[0], tok, caption_selection)
    # use_crop: LargestCenterSquare's antialiased filter whatever `antialias` says (it is PIL's resize there)
    transform = {'geometry': 0, 'filter': 0, 'range': 1} if use_crop else \
        {'geometry': 1, 'filter': 0 if antialias else 1, 'range': 1}
    if dataloader_kwargs.get('num_workers', 0) == 0:
        dataloader_kwargs.pop('prefetch_factor', None)
        dataloader_kwargs.pop('persistent_workers', None)
    dataloader_kwargs.setdefault('collate_fn', collate_raw_images(
        int(resize_size), pin_memory=bool(dataloader_kwargs.get('pin_memory')) and not dataloader_kwargs.get('num_workers'),
        image_transform=transform))
    if world is None:
        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        rank = dist.get_rank() if world > 1 else 0
    sampler = EpochRandomSampler(dataset, seed=seed) if shuffle else torch.utils.data.SequentialSampler(dataset)
    if world > 1:
        sampler = StridedSampler(sampler, int(rank or 0), int(world))
    return EpochDataLoader(dataset=dataset, batch_sampler=ResumableBatchSampler(sampler, batch_size, drop_last=False),
                           **dataloader_kwargs)
