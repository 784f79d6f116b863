"""Frozen OpenCLIP-H (SD-2) / CLIP ViT-L/14 (pixel models) text encoders + tokenizer on stock PyTorch-ROCm / transformers (no hub access).

Stands where diffusion/models/models.py:82,85,87 load ``CLIPTextModel`` / ``CLIPTokenizer`` by hub NAME.  Here the
SD-2 text-encoder config is embedded (hidden 1024, 23 layers, 16 heads, 77 positions, vocab 49408 - the published
stabilityai/stable-diffusion-2-base text_encoder/config.json) and the model is random-init unless ``local_dir``
points at a local checkpoint directory.  Without vocabulary files the real BPE tokenizer cannot be built; the
``ByteTokenizer`` below keeps the call surface (``__call__``, ``model_max_length``, ``decode``) for synthetic runs."""
from __future__ import annotations

import os
from typing import List, Optional, Union

import torch


def build_text_encoder(local_dir: Optional[str] = None, dtype=torch.float32, num_hidden_layers: int = 23,
                       hidden_size: int = 1024):
    from transformers import CLIPTextConfig, CLIPTextModel
    if local_dir and os.path.isdir(local_dir):
        return CLIPTextModel.from_pretrained(local_dir, torch_dtype=dtype, local_files_only=True)
    cfg = CLIPTextConfig(vocab_size=49408, hidden_size=hidden_size, intermediate_size=4 * hidden_size,
                         num_hidden_layers=num_hidden_layers, num_attention_heads=max(1, hidden_size // 64),
                         max_position_embeddings=77, hidden_act='gelu', projection_dim=512, pad_token_id=1,
                         bos_token_id=0, eos_token_id=2)
    return CLIPTextModel(cfg).to(dtype)


# openai/clip-vit-large-patch14's published text configuration (the encoder of the pixel models, reference
# models.py:136,197 load it by hub name): 768 hidden, 12 layers, 12 heads, 3072 intermediate, quick_gelu, eps 1e-5
CLIP_L14_TEXT = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                     max_position_embeddings=77, hidden_act='quick_gelu', layer_norm_eps=1e-5, projection_dim=768,
                     pad_token_id=1, bos_token_id=0, eos_token_id=2)

# its published vision configuration (the image tower of the CLIP score): ViT-L/14 at 224, 257 tokens of width 1024
CLIP_L14_VISION = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224,
                       patch_size=14, hidden_act='quick_gelu', layer_norm_eps=1e-5, projection_dim=768)
# CLIPImageProcessor's published per-channel mean and std for it (the shortest edge / crop is the image_size above)
CLIP_L14_PREPROCESS = dict(image_mean=(0.48145466, 0.4578275, 0.40821073), image_std=(0.26862954, 0.26130258, 0.27577711))


def build_clip_text_encoder(local_dir: Optional[str] = None, dtype=torch.float32, **overrides):
    """CLIP ViT-L/14 text encoder: strictly loaded from ``local_dir`` when it is a directory (every weight must be
    present), else random-init on the embedded configuration (``overrides`` narrow it for tests).  Never fetches."""
    from transformers import CLIPTextConfig, CLIPTextModel
    if local_dir and os.path.isdir(local_dir):
        model, info = CLIPTextModel.from_pretrained(local_dir, torch_dtype=dtype, local_files_only=True,
                                                    output_loading_info=True)
        missing = [k for k in info.get('missing_keys', []) if 'position_ids' not in k]
        if missing or info.get('mismatched_keys'):
            raise RuntimeError(f'{local_dir}: incomplete CLIP text encoder weights (missing {missing[:5]}, '
                               f'mismatched {info.get("mismatched_keys", [])[:5]})')
        return model
    return CLIPTextModel(CLIPTextConfig(**dict(CLIP_L14_TEXT, **overrides))).to(dtype)


class ByteTokenizer:
    model_max_length = 77
    bos, eos = 49406, 49407

    def __call__(self, text: Union[str, List[str]], padding='max_length', max_length: Optional[int] = None,
                 truncation=True, return_tensors: Optional[str] = None):
        max_length = max_length or self.model_max_length
        texts = [text] if isinstance(text, str) else list(text)
        ids = []
        for t in texts:
            body = [b + 256 for b in t.encode('utf-8')][:max_length - 2]
            row = [self.bos] + body + [self.eos]
            row += [self.eos] * (max_length - len(row))
            ids.append(row)
        if isinstance(text, str) and return_tensors is None:
            ids = ids[0]

        class _Enc(dict):
            pass

        out = _Enc(input_ids=torch.tensor(ids) if return_tensors == 'pt' else ids)
        out.input_ids = out['input_ids']
        return out

    def decode(self, ids, skip_special_tokens=True):
        bs = bytes(int(i) - 256 for i in ids if 256 <= int(i) < 512)
        return bs.decode('utf-8', errors='ignore')


def build_tokenizer(local_dir: Optional[str] = None):
    if local_dir and os.path.isdir(local_dir):
        from transformers import CLIPTokenizer
        return CLIPTokenizer.from_pretrained(local_dir, local_files_only=True)
    return ByteTokenizer()
