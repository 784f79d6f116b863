"""Raw images through the dataloader: the host half of the HIP resize-crop ingest (``ops.image_ingest``).

The reference decodes each JPEG in a worker, runs ``LargestCenterSquare(R)`` -> ``ToTensor`` -> ``Normalize(0.5, 0.5)`` on
the PIL image there (diffusion/datasets/laion/transforms.py:9-21, laion.py:159-164) and ships an fp32 3xRxR tensor.  Here
a worker only decodes: the ``uint8`` pixels of a batch travel packed into one 1-D tensor (one byte per value instead of
four), and one kernel does the transform on the device into the layout the VAE encoder reads.

``ingest_geometry`` is the one place the resize / crop rule is written for humans and tests; the kernel restates it in
integers (csrc/image.hip)."""
from __future__ import annotations

import io
from typing import List, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset
from torch.utils.data._utils.collate import default_collate

RAW_KEYS = ('image_raw', 'image_off', 'image_hw')
TRANSFORM_KEYS = ('geometry', 'filter', 'range')   # batch['image_transform']: the ops.image_resize switches


def target_hw(R) -> Tuple[int, int]:
    """The ingest target as ``(Rh, Rw)`` rows x columns: an int is the square ``(R, R)``, a pair is taken as it is."""
    if isinstance(R, (tuple, list)) or (hasattr(R, '__len__') and not isinstance(R, str)):
        if len(R) != 2:
            raise ValueError(f'an image size is an int or an (Rh, Rw) pair, got {R!r}')
        return int(R[0]), int(R[1])
    return int(R), int(R)


def ingest_geometry(w: int, h: int, R) -> Tuple[int, int, int, int]:
    """``(nw, nh, top, left)`` of the resize and centre crop of a ``w x h`` image to ``R``, an int or an ``(Rh, Rw)`` pair.

    An int is LargestCenterSquare(R): the shorter side is resized to R and the longer one to ``floor(R * long / short)``
    (torchvision ``resize`` with an int size).  A pair resizes to cover ``Rh`` rows x ``Rw`` columns the same way: with
    ``w * Rh <= h * Rw`` the width goes to ``Rw`` and the height to ``floor(Rw * h / w)``, else the height to ``Rh`` and the
    width to ``floor(Rh * w / h)``; at ``Rh == Rw`` that is the square rule.  Then the centre crop takes the window whose
    origin per axis is ``round((n - R) / 2)``, halves rounded to even (Python ``round``, torchvision ``CenterCrop``)."""
    Rh, Rw = target_hw(R)
    if w < 1 or h < 1 or Rh < 1 or Rw < 1:
        raise ValueError(f'ingest_geometry: w, h, R must be positive, got {(w, h, R)}')
    if w * Rh <= h * Rw:
        nw, nh = Rw, (Rw * h) // w
    else:
        nw, nh = (Rh * w) // h, Rh

    def origin(n, r):
        d = n - r
        q = d // 2
        return q if d % 2 == 0 else q + (q & 1)

    return nw, nh, origin(nh, Rh), origin(nw, Rw)


def decode_rgb(data: bytes) -> np.ndarray:
    """Encoded image bytes (JPEG, PNG, ...) -> ``uint8 [h, w, 3]``; non-RGB modes are converted (laion.py:92-94)."""
    from PIL import Image
    img = Image.open(io.BytesIO(data))
    if img.mode != 'RGB':
        img = img.convert('RGB')
    return np.array(img, dtype=np.uint8)   # a writable, contiguous copy


class MDSImageDataset(Dataset):
    """The reference's raw LAION shards (columns ``jpg`` + ``caption``, laion.py:81-100) without the transform: yields
    ``{'image_u8': uint8 [h, w, 3], 'captions': int64 [77]}``; batches are built by ``collate_raw_images``."""

    def __init__(self, directory: str, tokenizer=None, caption_drop_prob: float = 0.0):
        from .mds import MDSDirectory
        self.mds = MDSDirectory(directory)
        self.tokenizer, self.caption_drop_prob = tokenizer, caption_drop_prob

    def __len__(self):
        return len(self.mds)

    def __getitem__(self, index):
        smp = self.mds.get(index, columns=('jpg', 'caption'))
        out = {'image_u8': torch.from_numpy(decode_rgb(smp['jpg']))}
        caption = '' if torch.rand(1) < self.caption_drop_prob else smp.get('caption', '')
        if self.tokenizer is not None:
            ids = self.tokenizer(caption, padding='max_length', max_length=self.tokenizer.model_max_length,
                                 truncation=True)['input_ids']
            out['captions'] = torch.tensor(ids)
        else:
            out['captions'] = torch.zeros(77, dtype=torch.int64)
        return out


def pack_images(images: List[torch.Tensor], pin_memory: bool = False):
    """``uint8 [h, w, 3]`` tensors of any sizes -> ``(image_raw uint8 [sum 3hw], image_off int64 [B], image_hw int32
    [B, 2])``: the images back to back with no padding, so an image starts at whatever byte the previous one ended."""
    for im in images:
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
            raise ValueError(f'pack_images: uint8 [h, w, 3] images expected, got {im.dtype} {tuple(im.shape)}')
    sizes = [int(im.numel()) for im in images]
    off = torch.tensor([0] + sizes[:-1], dtype=torch.int64).cumsum(0)
    hw = torch.tensor([[im.shape[0], im.shape[1]] for im in images], dtype=torch.int32)
    raw = torch.empty(sum(sizes), dtype=torch.uint8, pin_memory=pin_memory)
    torch.cat([im.reshape(-1) for im in images], out=raw)
    return raw, off, hw


class collate_raw_images:
    """Collate function for samples carrying ``image_u8``: packs the images (``pack_images``), default-collates every
    other key, and records the target as ``image_size`` when one was given: the Python int it was given, or an
    ``(Rh, Rw)`` tuple for a rectangular target.  The packed tensor is allocated pinned when ``pin_memory`` is set (and a
    device is present), so the training step's upload is asynchronous without a second host copy.  ``image_transform``
    (the COCO evaluation loader's) rides along as ``batch['image_transform']``: a dict of the ``ops.image_resize`` switches
    ``geometry`` / ``filter`` / ``range``; without one the key is absent and the batch means the training transform.
    Samples of a bucketed run (``datasets/buckets.py``) carry ``image_target``, their bucket: the batch's one bucket becomes
    its ``image_size``; their ``image_aug`` draws are stacked to int32 ``[B, 3]`` like any other key."""

    def __init__(self, image_size=0, pin_memory: bool = False, image_transform=None):
        self.image_size = target_hw(image_size) if hasattr(image_size, '__len__') else int(image_size)
        self.pin_memory = bool(pin_memory)
        self.image_transform = None if image_transform is None else {k: int(image_transform[k]) for k in TRANSFORM_KEYS}

    def __call__(self, samples):
        pin = self.pin_memory and torch.cuda.is_available()
        raw, off, hw = pack_images([s['image_u8'] for s in samples], pin)
        batch = default_collate([{k: v for k, v in s.items() if k != 'image_u8'} for s in samples])
        batch['image_raw'], batch['image_off'], batch['image_hw'] = raw, off, hw
        if self.image_size:
            batch['image_size'] = self.image_size
        if 'image_target' in batch:   # a bucketed run (datasets/buckets.py): the batch's one bucket is its target
            t = batch.pop('image_target')
            if not bool((t == t[0]).all()):
                raise ValueError(f'a batch mixes the targets {sorted({tuple(r) for r in t.tolist()})}: bucketed samples '
                                 'need AspectBucketBatchSampler')
            batch['image_size'] = (int(t[0, 0]), int(t[0, 1]))
        if self.image_transform is not None:
            batch['image_transform'] = dict(self.image_transform)
        return batch


def is_raw_image_directory(directory: str, resize_size) -> bool:
    """An MDS directory whose ``index.json`` lists a ``jpg`` column and no ``latents_{resize_size}`` column.  Latent columns
    exist for square sizes only, so for an ``(Rh, Rw)`` pair the ``jpg`` column alone decides."""
    import json
    import os
    with open(os.path.join(directory, 'index.json')) as f:
        shards = json.load(f)['shards']
    names = set().union(*[set(s['column_names']) for s in shards]) if shards else set()
    if hasattr(resize_size, '__len__'):
        return 'jpg' in names
    return 'jpg' in names and f'latents_{resize_size}' not in names


def ingest_batch(batch, R, kind: int, device, transform=None):
    """Upload a raw batch (non-blocking) and run the ingest kernel for the target ``R``, an int or an ``(Rh, Rw)`` pair:
    kind 0 -> bf16 [B*Rh*Rw, 8], kind 1 -> fp32 [B,3,Rh,Rw].  An int runs the square entry, a pair the rectangular one;
    with a ``transform`` (a batch's ``image_transform``) ``ops.image_resize`` runs with its switches instead, and a batch
    that carries ``image_aug`` (int32 [B, 3]: crop origin and flip per image) goes through ``ops.image_ingest_aug``."""
    from .. import ops
    raw, off, hw = (batch[k] for k in RAW_KEYS)
    if off.is_cuda or hw.is_cuda:
        raise ValueError('ingest_batch: image_off / image_hw must still be host tensors (ingest before moving the batch to '
                         'the device): the bounds of the packed buffer are checked on them')
    B = off.numel()
    Rh, Rw = target_hw(R)
    d_raw, d_off, d_hw = (z.to(device, non_blocking=True) for z in (raw, off, hw))
    if kind == 0:
        out = torch.empty(B * Rh * Rw, 8, device=device, dtype=torch.bfloat16)
    else:
        out = torch.empty(B, 3, Rh, Rw, device=device, dtype=torch.float32)
    aug = batch.get('image_aug')
    if aug is not None:   # per-image crop origin and flip (datasets/buckets.py draws them): the augmenting entry
        if transform is not None:
            raise ValueError('ingest_batch: image_aug and image_transform cannot be combined')
        if aug.is_cuda:
            raise ValueError('ingest_batch: image_aug must still be a host tensor (its origins are checked on it)')
        aug = aug.to(torch.int32).contiguous()
        ops.image_ingest_aug(d_raw, d_off, d_hw, aug.to(device, non_blocking=True), Rh, Rw, out, kind, host=(off, hw, aug))
    elif transform is not None:
        ops.image_resize(d_raw, d_off, d_hw, Rh, Rw, out, kind, *(int(transform[k]) for k in TRANSFORM_KEYS), host=(off, hw))
    elif isinstance(R, int):
        ops.image_ingest(d_raw, d_off, d_hw, R, out, kind, host=(off, hw))
    else:
        ops.image_ingest_rect(d_raw, d_off, d_hw, Rh, Rw, out, kind, host=(off, hw))
    return out
