"""LAION dataloader surface - mirrors /root/reference diffusion/datasets/laion/laion.py:115-194.

``build_streaming_laion_dataloader`` keeps the reference signature (:115-130) and the batch-dict contract of
``StreamingLAIONDataset.__getitem__`` (:81-112): ``image`` 3xRxR fp32 in [-1,1], ``captions`` 77 int64,
``caption_latents`` 77x1024 fp16, ``image_latents`` 4x(R/8)x(R/8) fp16.  mosaicml-streaming (MDS) is not available
here, so two backends exist:
  * ``local`` pointing at an MDS directory (``index.json`` + ``shard.*.mds``, read by ``datasets/mds.py`` - the
    reference's own precomputed-latent format) or at a directory of ``*.npz`` shards with raw-fp16 columns ``caption_latents``,
    ``latents_256`` / ``latents_512`` (the column names scripts/precompute_latents.py:252-272 writes) and
    optional ``captions``;
  * no ``remote``/``local`` (the YAML default: both empty) -> a seeded synthetic dataset of the same shapes
    (N(0,1) latents / text embeddings), which is what bench.py and the tests use.
JPEG decode (:83) is skipped when latents are present: the reference decodes images it never uses.  A
``local`` MDS directory with a ``jpg`` column and no ``latents_{resize_size}`` column is read as raw images instead
(``datasets/image_ingest.py``): batches then carry ``image_raw`` / ``image_off`` / ``image_hw`` / ``image_size``.
``resize_size`` may be an ``(Rh, Rw)`` pair for such directories (a rectangular target, ``image_size`` is then the tuple);
latent columns, latent shards and the synthetic data are square, so a pair anywhere else is a ``ValueError``.
``aspect_buckets`` turns one target shape into a table of them, one per batch (``datasets/buckets.py``): raw-image
directories, or latent directories with the ``latents_ar{R}`` / ``latents_ar{R}_hw`` columns of
``tools/precompute_latents.py --aspect-buckets``; ``random_crop`` / ``flip_prob`` augment raw images in the ingest kernel."""
from __future__ import annotations

import glob
import os
from typing import List, Optional, Sequence, Union

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset, DistributedSampler, SequentialSampler


class SyntheticLAIONDataset(Dataset):

    def __init__(self, num_samples: int = 1 << 20, image_size: int = 256, caption_drop_prob: float = 0.0, seed: int = 17,
                 text_dim: int = 1024, with_images: bool = False):
        self.n, self.image_size, self.seed = num_samples, image_size, seed
        self.text_dim, self.with_images, self.caption_drop_prob = text_dim, with_images, caption_drop_prob

    def __len__(self):
        return self.n

    def __getitem__(self, index):
        g = torch.Generator().manual_seed(self.seed * 1_000_003 + index)
        s = self.image_size // 8
        out = {
            'captions': torch.randint(0, 49408, (77,), generator=g),
            'caption_latents': torch.randn(77, self.text_dim, generator=g).half(),
            'image_latents': torch.randn(4, s, s, generator=g).half(),
        }
        if self.with_images:
            out['image'] = torch.rand(3, self.image_size, self.image_size, generator=g) * 2 - 1
        return out


class MDSLatentDataset(Dataset):
    """Precomputed-latent MDS shards (the reference's training data format).  Yields the reference's sample dict
    (laion.py:102-112) minus the decoded JPEG: with latents present the image is never used by ``forward``
    (stable_diffusion.py:157-158), and decoding it is the dominant host cost of the reference loader."""

    def __init__(self, directory: str, image_size: int, tokenizer=None, caption_drop_prob: float = 0.0,
                 aspect_buckets: bool = False):
        from ..mds import MDSDirectory
        self.mds = MDSDirectory(directory)
        self.image_size, self.tokenizer, self.caption_drop_prob = image_size, tokenizer, caption_drop_prob
        self.col = f'latents_{image_size}'
        self.skipped = 0
        self.bucket_hw = None
        if aspect_buckets:
            # the columns tools/precompute_latents.py --aspect-buckets writes: each image encoded at its bucket, and the
            # bucket's (Rh, Rw); the second one is this dataset's bucket index (int64 [N, 2]), read once
            self.col = f'latents_ar{image_size}'
            names = set().union(*[set(s.names) for s in self.mds.shards]) if self.mds.shards else set()
            if self.col not in names or self.col + '_hw' not in names:
                raise ValueError(f'{directory}: no {self.col} / {self.col}_hw columns; write them with '
                                 f'tools/precompute_latents.py --aspect-buckets {image_size}')
            self.bucket_hw = np.stack([np.frombuffer(self.mds.get(i, columns=(self.col + '_hw',))[self.col + '_hw'],
                                                     dtype=np.int32) for i in range(len(self.mds))]).astype(np.int64)
            if self.bucket_hw.shape[1:] != (2,) or (self.bucket_hw < 8).any() or (self.bucket_hw % 8).any():
                raise ValueError(f'{directory}: {self.col}_hw must hold two int32 (Rh, Rw), multiples of 8')

    MAX_SKIP = 4096

    def __len__(self):
        return len(self.mds)

    def _tokens(self, smp):
        caption = '' if torch.rand(1) < self.caption_drop_prob else smp.get('caption', '')
        if self.tokenizer is None:
            return torch.zeros(77, dtype=torch.int64)
        return torch.tensor(self.tokenizer(caption, padding='max_length', max_length=self.tokenizer.model_max_length,
                                           truncation=True)['input_ids'])

    def __getitem__(self, index):
        if self.bucket_hw is not None:
            Rh, Rw = (int(v) for v in self.bucket_hw[index])
            smp = self.mds.get(index, columns=('caption', 'caption_latents', self.col))
            lat = np.frombuffer(smp[self.col], dtype=np.float16)
            if lat.size != 4 * (Rh // 8) * (Rw // 8):
                raise RuntimeError(f'sample {index}: {self.col} holds {lat.size} values, its bucket {Rh} x {Rw} needs '
                                   f'{4 * (Rh // 8) * (Rw // 8)}')
            return {'caption_latents': torch.from_numpy(np.frombuffer(smp['caption_latents'], dtype=np.float16).copy()).reshape(77, -1),
                    'image_latents': torch.from_numpy(lat.copy()).reshape(4, Rh // 8, Rw // 8), 'captions': self._tokens(smp)}
        s = self.image_size // 8
        n = len(self.mds)
        # the writer stores b'' when the source image is smaller than the resolution (precompute_latents.py:303-306):
        # such a sample cannot be trained on at this resolution - take the next one that can (deterministic in index)
        for probe in range(self.MAX_SKIP):
            smp = self.mds.get((index + probe) % n, columns=('caption', 'caption_latents', self.col))
            lat = np.frombuffer(smp[self.col], dtype=np.float16)
            if lat.size == 4 * s * s:
                break
            self.skipped += 1
        else:
            raise RuntimeError(f'{self.MAX_SKIP} consecutive samples from index {index} have no {self.col}: '
                               f'this MDS directory holds no latents for {self.image_size} px')
        out = {'caption_latents': torch.from_numpy(np.frombuffer(smp['caption_latents'], dtype=np.float16).copy()).reshape(77, -1),
               'image_latents': torch.from_numpy(lat.copy()).reshape(4, s, s)}
        caption = '' if torch.rand(1) < self.caption_drop_prob else smp.get('caption', '')
        if self.tokenizer is not None:
            ids = self.tokenizer(caption, padding='max_length', max_length=self.tokenizer.model_max_length,
                                 truncation=True)['input_ids']
            out['captions'] = torch.tensor(ids)
        else:
            out['captions'] = torch.zeros(77, dtype=torch.int64)
        return out


class LocalLatentShards(Dataset):
    """*.npz shards: arrays ``caption_latents`` [n,77*1024] fp16 bytes-equivalent, ``latents_{res}`` [n,4*s*s]."""

    def __init__(self, directory: str, image_size: int):
        self.files = sorted(glob.glob(os.path.join(directory, '*.npz')))
        if not self.files:
            raise FileNotFoundError(f'no *.npz latent shards under {directory}')
        self.image_size = image_size
        self.index = []
        for fi, f in enumerate(self.files):
            with np.load(f) as z:
                n = z['caption_latents'].shape[0]
            self.index += [(fi, i) for i in range(n)]
        self._cache = (None, None)

    def __len__(self):
        return len(self.index)

    def __getitem__(self, index):
        fi, i = self.index[index]
        if self._cache[0] != fi:
            self._cache = (fi, dict(np.load(self.files[fi])))
        z = self._cache[1]
        s = self.image_size // 8
        out = {
            'caption_latents': torch.from_numpy(z['caption_latents'][i].astype(np.float16).copy()).reshape(77, -1),
            'image_latents': torch.from_numpy(z[f'latents_{self.image_size}'][i].astype(np.float16).copy()).reshape(4, s, s),
        }
        out['captions'] = torch.from_numpy(z['captions'][i].astype(np.int64)) if 'captions' in z else torch.zeros(
            77, dtype=torch.int64)
        return out


def build_streaming_laion_dataloader(
    remote: Union[str, List, None] = None,
    local: Union[str, List, None] = None,
    batch_size: int = 1,
    tokenizer_name_or_path: str = 'stabilityai/stable-diffusion-2-base',
    caption_drop_prob: float = 0.0,
    resize_size: Union[int, Sequence[int]] = 256,
    num_samples: Optional[int] = None,
    predownload: int = 100_000,
    download_retry: int = 2,
    download_timeout: float = 120,
    drop_last: bool = True,
    shuffle: bool = True,
    num_canonical_nodes: Optional[int] = None,
    aspect_buckets=None,
    random_crop: bool = False,
    flip_prob: float = 0.0,
    **dataloader_kwargs,
):
    """``aspect_buckets`` / ``random_crop`` / ``flip_prob`` do not exist in the reference (datasets/buckets.py).
    ``aspect_buckets``: ``None`` (one target shape, the behaviour without it), ``True`` (``bucket_table(resize_size)``), a
    dict of ``step`` / ``min_side`` / ``max_side``, or a list of ``[Rh, Rw]`` pairs; every batch then holds one bucket.
    ``random_crop`` / ``flip_prob`` augment raw-image directories in the ingest kernel, with or without buckets."""
    remote, local = _as_list(remote), _as_list(local)
    if remote and local and len(remote) != len(local):
        raise ValueError(f'remote and local Sequences must be the same length, got lengths {len(remote)} and {len(local)}')
    if remote and not local:
        raise ValueError('a remote without a local cache directory cannot be read here: mosaicml-streaming (download-on-'
                         'miss) is not available; point `local` at a directory that already holds the shards')
    text_dim = dataloader_kwargs.pop('text_dim', 1024)
    with_images = dataloader_kwargs.pop('synthetic_images', False)
    seed = int(dataloader_kwargs.pop('seed', 17))
    # an (Rh, Rw) pair: a rectangular target, which only the raw-image ingest can produce (latent columns, latent shards and
    # the synthetic data are square)
    rect = hasattr(resize_size, '__len__')
    if rect:
        from ..image_ingest import target_hw
        resize_size = target_hw(resize_size)
        if min(resize_size) < 1:
            raise ValueError(f'resize_size must be positive, got {resize_size}')
    # aspect-ratio buckets and the in-kernel augmentation: everything that can be refused is refused before a shard is opened
    flip_prob = float(flip_prob)
    if not 0.0 <= flip_prob <= 1.0:
        raise ValueError(f'flip_prob must be in [0, 1], got {flip_prob}')
    augment = bool(random_crop) or flip_prob > 0.0
    table = None
    if aspect_buckets is not None and aspect_buckets is not False:
        from ..buckets import resolve_table
        table = resolve_table(aspect_buckets, resize_size)   # a rectangular resize_size, a step the U-Net cannot take: ValueError
        if not local:
            raise ValueError('aspect_buckets: the synthetic dataset is square; buckets need MDS directories of raw images or '
                             'of latents written by tools/precompute_latents.py --aspect-buckets')
        npz = [d for d in local if os.path.isdir(d) and not os.path.exists(os.path.join(d, 'index.json'))]
        if npz:
            raise ValueError(f'aspect_buckets: {npz} hold *.npz latent shards, which are square; buckets need MDS directories')
    if augment and not local:
        raise ValueError('random_crop / flip_prob augment raw images in the ingest kernel; the synthetic dataset has none')
    if augment and dataloader_kwargs.get('persistent_workers') and dataloader_kwargs.get('num_workers'):
        raise ValueError('random_crop / flip_prob: persistent workers keep the epoch they were started in, the draws of '
                         '(seed, epoch, index) need fresh workers per epoch')
    if local:
        missing = [d for d in local if not os.path.isdir(d)]
        if missing:  # never fall through to synthetic noise because of a mistyped path
            raise FileNotFoundError(f'local dataset director{"ies" if len(missing) > 1 else "y"} not found: {missing}')
        from ...models.text import build_tokenizer
        tok = build_tokenizer(tokenizer_name_or_path if os.path.isdir(str(tokenizer_name_or_path)) else None)
        # an MDS directory of raw images (a `jpg` column and no latents for this resolution - the reference's own LAION
        # shards, laion.py:81-100): the workers decode, the packed uint8 pixels go to the device and the HIP ingest kernel
        # does the reference's transform there (datasets/image_ingest.py)
        from ..image_ingest import MDSImageDataset, collate_raw_images, is_raw_image_directory
        raw = [os.path.exists(os.path.join(d, 'index.json')) and is_raw_image_directory(d, resize_size) for d in local]
        if table is not None:   # a directory that already holds the bucketed latent columns is trained from those
            raw = [r and f'latents_ar{resize_size}' not in _mds_columns(d) for d, r in zip(local, raw)]
        if any(raw) and not all(raw):
            raise ValueError('raw-image and latent directories cannot be mixed in one dataloader: '
                             f'{[d for d, r in zip(local, raw) if r]} hold images only')
        if rect and not all(raw):
            raise ValueError(f'resize_size={list(resize_size)}: a rectangular size needs raw-image MDS directories (a `jpg` '
                             f'column); {[d for d, r in zip(local, raw) if not r]} hold latents, which are square')
        if augment and not all(raw):
            raise ValueError('random_crop / flip_prob augment raw images in the ingest kernel; '
                             f'{[d for d, r in zip(local, raw) if not r]} hold latents, which were encoded without them')
        bucket_of_index = None
        if all(raw):
            parts = [MDSImageDataset(d, tok, caption_drop_prob) for d in local]
            dataloader_kwargs.setdefault('collate_fn', collate_raw_images(
                resize_size, pin_memory=bool(dataloader_kwargs.get('pin_memory')) and not dataloader_kwargs.get('num_workers')))
            if table is not None:   # the bucket of every image from its recorded size: no pixel is decoded for this
                from ..buckets import assign_bucket, scan_image_sizes
                sizes = np.concatenate([scan_image_sizes(d) for d in local])
                bucket_of_index = np.array([assign_bucket(int(w), int(h), table) for w, h in sizes], dtype=np.int64)
        elif table is not None:   # bucketed latent columns: the shapes found in the `_hw` column are the table
            parts = [MDSLatentDataset(d, resize_size, tok, caption_drop_prob, aspect_buckets=True) for d in local]
            hw = np.concatenate([p.bucket_hw for p in parts])
            table = sorted({(int(a), int(b)) for a, b in hw})
            lookup = {s: i for i, s in enumerate(table)}
            bucket_of_index = np.array([lookup[(int(a), int(b))] for a, b in hw], dtype=np.int64)
        else:
            parts = [MDSLatentDataset(d, resize_size, tok, caption_drop_prob) if os.path.exists(os.path.join(d, 'index.json'))
                     else LocalLatentShards(d, resize_size) for d in local]
        dataset = torch.utils.data.ConcatDataset(parts)
    else:  # both remote and local empty (the shipped YAML): seeded synthetic data of the same shapes
        if rect:
            raise ValueError(f'resize_size={list(resize_size)}: the synthetic dataset is square; a rectangular size needs '
                             'raw-image MDS directories')
        dataset = SyntheticLAIONDataset(image_size=resize_size, caption_drop_prob=caption_drop_prob, text_dim=text_dim,
                                        with_images=with_images, seed=seed)
    if num_samples is not None:
        dataset = torch.utils.data.Subset(dataset, range(num_samples))
    if table is not None:
        bucket_of_index = bucket_of_index[:len(dataset)]
    if local and all(raw) and (table is not None or augment):
        # each sample learns its target (its bucket) and, with augmentation on, its (top, left, flip) draw of
        # (seed, epoch, index); the collate function turns the former into the batch's `image_size`
        from ..buckets import BucketedImages
        dataset = BucketedImages(dataset, bucket_of_index if table is not None else resize_size, table, seed,
                                 random_crop, flip_prob)
    if dataloader_kwargs.get('num_workers', 0) == 0:
        dataloader_kwargs.pop('prefetch_factor', None)
        dataloader_kwargs.pop('persistent_workers', None)
    # The reference gets shuffling and the per-rank partition from StreamingDataset (laion.py:167-180: shuffle=...,
    # batch_size=..., num_canonical_nodes=...) with train.py:40 dividing the batch by the world size.  Here: a
    # rank-strided partition of a per-epoch seeded permutation (torch DistributedSampler), so the ranks of a data-
    # parallel job read disjoint, jointly exhaustive samples; single process: a seeded RandomSampler.
    import torch.distributed as dist
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank() if world > 1 else 0
    new_keys = table is not None or augment
    if new_keys:   # the iterator's base seed from (seed, epoch), not from the global stream: see EpochDataLoader.__iter__
        dataloader_kwargs.setdefault('generator', torch.Generator())
    if table is not None:   # one bucket per batch, the same bucket on every rank at the same step (datasets/buckets.py)
        from ..buckets import AspectBucketBatchSampler
        loader = EpochDataLoader(dataset=dataset, batch_sampler=AspectBucketBatchSampler(
            bucket_of_index, batch_size, world, rank, seed, shuffle, drop_last), **dataloader_kwargs)
        loader.bucket_table = table
        loader.epoch_seed = seed
        return loader
    if world > 1:
        sampler = DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=shuffle, seed=seed,
                                     drop_last=drop_last)
    elif shuffle:
        sampler = EpochRandomSampler(dataset, seed=seed)
    else:
        sampler = SequentialSampler(dataset)
    loader = EpochDataLoader(dataset=dataset, batch_sampler=ResumableBatchSampler(sampler, batch_size, drop_last),
                             **dataloader_kwargs)
    if new_keys:
        loader.epoch_seed = seed
    return loader


def _mds_columns(directory: str) -> set:
    """the column names an MDS directory's ``index.json`` lists"""
    import json
    with open(os.path.join(directory, 'index.json')) as f:
        shards = json.load(f)['shards']
    return set().union(*[set(s['column_names']) for s in shards]) if shards else set()


def _as_list(x) -> List[str]:
    """None / '' -> [], 'path' -> ['path'], sequences -> list without empty entries."""
    if x is None:
        return []
    if isinstance(x, (str, os.PathLike)):
        return [str(x)] if str(x) else []
    return [str(d) for d in x if d]


class EpochRandomSampler(torch.utils.data.Sampler):
    """Single-process shuffle: the permutation of epoch e is a pure function of (seed, e) - like DistributedSampler's -
    so a resumed run reproduces the epoch it stopped in instead of continuing a generator it no longer has."""

    def __init__(self, data_source, seed: int = 0):
        self.n = len(data_source)
        self.seed = int(seed)
        self.epoch = 0

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed + self.epoch)
        return iter(torch.randperm(self.n, generator=g).tolist())

    def __len__(self):
        return self.n


class ResumableBatchSampler(torch.utils.data.Sampler):
    """torch's BatchSampler plus ``skip``: the next iterator drops its first ``skip`` batches at INDEX level (no sample is
    loaded for them) - how a resumed run continues in the middle of an epoch (streaming's StreamingDataset resumes
    mid-epoch from its state dict; reference laion.py:167-180 / SD-2-base-256.yaml:91-94 autoresume)."""

    def __init__(self, sampler, batch_size: int, drop_last: bool):
        self.sampler, self.batch_size, self.drop_last = sampler, int(batch_size), bool(drop_last)
        self.skip = 0

    def __iter__(self):
        skip, self.skip = self.skip, 0
        batch, nb = [], 0
        for idx in self.sampler:
            batch.append(idx)
            if len(batch) == self.batch_size:
                if nb >= skip:
                    yield batch
                nb += 1
                batch = []
        if batch and not self.drop_last and nb >= skip:
            yield batch

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)


class EpochDataLoader(DataLoader):
    """DataLoader that advances its sampler's epoch each time a new iterator is made (the samplers reshuffle only when
    told the epoch).  ``set_epoch(e, skip_batches=k)`` lets a resumed run continue the sequence: the next iterator is
    epoch e without its first k batches."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._next_epoch = 0
        self.epoch_seed = None   # set with a `generator`: the iterator's base seed becomes a function of (seed, epoch)

    @property
    def index_sampler(self):
        return self.batch_sampler.sampler if self._resumable else self.sampler

    @property
    def _resumable(self):
        """a ResumableBatchSampler, or a batch sampler with its ``skip`` contract (AspectBucketBatchSampler)"""
        from ..buckets import AspectBucketBatchSampler
        return isinstance(self.batch_sampler, (ResumableBatchSampler, AspectBucketBatchSampler))

    def set_epoch(self, epoch: int, skip_batches: int = 0):
        self._next_epoch = int(epoch)
        if self._resumable:
            self.batch_sampler.skip = int(skip_batches)
        elif skip_batches:
            raise ValueError('skip_batches needs a ResumableBatchSampler')

    def __iter__(self):
        smp = self.index_sampler
        if hasattr(smp, 'set_epoch'):
            smp.set_epoch(self._next_epoch)
        if hasattr(self.dataset, 'set_epoch'):   # BucketedImages: the augmentation draws are a function of the epoch
            self.dataset.set_epoch(self._next_epoch)
        if self.epoch_seed is not None:
            # torch draws every iterator's base seed (the workers' seeds) from the loader's generator, or from the GLOBAL
            # one without it: a resumed run makes an iterator the uninterrupted run did not, and everything drawn from the
            # global stream afterwards (the caption drops) would shift.  Here it is a function of (seed, epoch) instead
            self.generator.manual_seed((self.epoch_seed * 1_000_003 + self._next_epoch) % (1 << 63))
        self._next_epoch += 1
        return super().__iter__()
