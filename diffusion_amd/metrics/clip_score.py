"""``CLIPScore``: torchmetrics' ``multimodal.clip_score.CLIPScore`` on the HIP path.

The reference evaluates generated images this way (scripts/fid-clip-evaluation.py:52-53, yamls/mosaic-yamls/eval.yaml:
``CLIPScore()`` with its default ``openai/clip-vit-large-patch14``): 100 x the cosine between CLIP's image embedding of the
generated image and its text embedding of the caption, averaged over all samples and clamped at 0.  Here the processor is
``da_clip_preprocess``, the towers are ``CLIPVisionHIP`` and ``TextEncoderHIP`` + ``text_projection``, and the score and
its running sum are ``da_clip_score``: ``update`` enqueues kernels and never synchronises the host.  The class is named
``CLIPScore`` because ``StableDiffusion`` routes and sweeps metrics by class name.
"""
from __future__ import annotations

import copy
import json
import os
import warnings
from typing import List, Sequence, Union

import torch

from ..models.composer_shim import Metric

DEFAULT_MODEL = 'openai/clip-vit-large-patch14'


def _load_local(path: str):
    """strictly: every weight of the checkpoint directory, its tokenizer and its preprocessor settings"""
    from transformers import CLIPModel, CLIPTokenizer
    model, info = CLIPModel.from_pretrained(path, torch_dtype=torch.float32, local_files_only=True, output_loading_info=True)
    missing = [k for k in info.get('missing_keys', []) if 'position_ids' not in k]
    if missing or info.get('mismatched_keys'):
        raise RuntimeError(f'{path}: incomplete CLIP weights (missing {missing[:5]}, mismatched '
                           f'{info.get("mismatched_keys", [])[:5]})')
    tokenizer = CLIPTokenizer.from_pretrained(path, local_files_only=True)
    with open(os.path.join(path, 'preprocessor_config.json')) as f:
        pc = json.load(f)
    size = pc['size']
    size = size['shortest_edge'] if isinstance(size, dict) else int(size)
    crop = pc.get('crop_size', size)
    crop = crop['height'] if isinstance(crop, dict) else int(crop)
    if crop != size or size != model.config.vision_config.image_size or pc.get('resample', 3) != 3 \
            or not pc.get('do_center_crop', True):
        raise RuntimeError(f'{path}: preprocessor settings outside what da_clip_preprocess computes (shortest edge = crop = '
                           f'image_size, bicubic, centre crop): {pc}')
    return model, tokenizer, dict(image_mean=tuple(pc['image_mean']), image_std=tuple(pc['image_std']))


def _random_init():
    from transformers import CLIPConfig, CLIPModel
    from ..models.text import CLIP_L14_TEXT, CLIP_L14_VISION, ByteTokenizer
    cfg = CLIPConfig(text_config=dict(CLIP_L14_TEXT), vision_config=dict(CLIP_L14_VISION),
                     projection_dim=CLIP_L14_VISION['projection_dim'])
    return CLIPModel(cfg).float(), ByteTokenizer()


class CLIPScore(Metric):
    """``update(images, text)`` / ``compute()`` / ``reset()`` of torchmetrics' CLIPScore.

    ``model_name_or_path``: a local checkpoint directory is loaded strictly (weights, tokenizer, preprocessor settings);
    any other value, a hub name included, gives a RANDOM-INIT ViT-L/14 on the embedded configuration with a warning -
    nothing is ever fetched.  ``model`` (a ``transformers.CLIPModel``) and ``tokenizer`` inject ready objects.  The state is
    two device floats, (sum of scores, samples); the frozen towers are shared by ``copy.deepcopy``."""

    def __init__(self, model_name_or_path: str = DEFAULT_MODEL, model=None, tokenizer=None, device=None):
        super().__init__()
        from ..models.text import CLIP_L14_PREPROCESS
        pre = dict(CLIP_L14_PREPROCESS)
        if model is None:
            if model_name_or_path and os.path.isdir(model_name_or_path):
                model, tok, pre = _load_local(model_name_or_path)
            else:
                warnings.warn(f'CLIPScore: {model_name_or_path!r} is not a local directory; the towers are RANDOM-INIT '
                              'ViT-L/14 (nothing is downloaded), the scores are meaningless', stacklevel=2)
                model, tok = _random_init()
            tokenizer = tokenizer or tok
        elif tokenizer is None:
            from ..models.text import ByteTokenizer
            tokenizer = ByteTokenizer()
        self.mean, self.std = tuple(pre['image_mean']), tuple(pre['image_std'])
        # what deepcopy shares: the torch module, the tokenizer and the towers built from it at the first update
        self._shared = {'model': model.eval().requires_grad_(False), 'tokenizer': tokenizer, 'towers': None}
        self.dev = torch.device(device if device is not None else ('cuda' if torch.cuda.is_available() else 'cpu'))
        self.state = torch.zeros(2, dtype=torch.float32, device=self.dev)

    def __deepcopy__(self, memo):
        new = copy.copy(self)   # every attribute shared, the towers among them ...
        for k in ('_parameters', '_buffers', '_modules'):
            setattr(new, k, copy.copy(getattr(self, k)))
        new.state = self.state.clone()   # ... except the state
        memo[id(self)] = new
        return new

    @property
    def tokenizer(self):
        return self._shared['tokenizer']

    def _towers(self):
        if self.dev.type != 'cuda':
            raise RuntimeError('CLIPScore runs on an MI355X only (there is no CPU path)')
        if self._shared['towers'] is None:
            from ..models.clip_vision_hip import CLIPTextEmbedHIP, CLIPVisionHIP
            model = self._shared['model']
            self._shared['towers'] = (CLIPVisionHIP(model, self.dev), CLIPTextEmbedHIP(model, self.dev))
        return self._shared['towers']

    @torch.no_grad()
    def update(self, images: Union[torch.Tensor, Sequence[torch.Tensor]], text: Union[str, List[str], torch.Tensor]):
        from .. import ops
        vision, text_tower = self._towers()
        if not torch.is_tensor(images):
            images = list(images)
            if len({tuple(i.shape) for i in images}) != 1:
                raise ValueError('CLIPScore.update: all images of one call must have the same size')
            images = torch.stack(images)
        if images.dim() == 3:
            images = images[None]
        if images.dim() != 4 or images.shape[1] != 3 or images.dtype != torch.uint8:
            raise ValueError(f'CLIPScore.update: images must be uint8 [B, 3, H, W], got {tuple(images.shape)} {images.dtype}')
        if torch.is_tensor(text):
            ids = text if text.dim() == 2 else text[None]
        else:
            text = [text] if isinstance(text, str) else list(text)
            ids = self.tokenizer(text, padding='max_length', max_length=text_tower.max_length, truncation=True,
                                 return_tensors='pt')['input_ids']
        if ids.shape[0] != images.shape[0]:
            raise ValueError(f'CLIPScore.update: {images.shape[0]} images, {ids.shape[0]} captions')
        img = vision(images.to(self.dev, non_blocking=True).contiguous(), self.mean, self.std)
        txt = text_tower(ids.to(self.dev, non_blocking=True))
        scores = torch.empty(img.shape[0], device=self.dev, dtype=torch.float32)
        ops.clip_score(img, txt, scores, self.state)
        return scores

    def compute(self):
        import torch.distributed as dist
        st = self.state
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            st = st.clone()
            dist.all_reduce(st)
        return torch.clamp(st[0] / st[1], min=0.0)

    def reset(self):
        self.state.zero_()
