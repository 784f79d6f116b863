"""CLIP's image tower (``transformers.CLIPVisionModelWithProjection`` / the vision half of ``CLIPModel``) on the hand-written
gfx950 kernels, forward only: the counterpart of models/text_hip.py for the CLIP score (metrics/clip_score.py).

The tower is a pre-LN ViT: patch embedding (a stride-P convolution without bias, i.e. one GEMM over the patch matrix
``da_clip_preprocess`` writes), class token and position embeddings, a LayerNorm (``pre_layrnorm``, as transformers spells it),
L layers of the text tower's op set with non-causal 64-wide heads (``da_attn_fwd``), a LayerNorm of the class rows and
``visual_projection``.  The patch matrix carries one all-zero row per image in the class-token slot, so the embedding GEMM
with a residual table (row 0: class embedding + position 0, row j: position j) produces all ``Np + 1`` tokens in one launch.
``text_embeds`` below is the text side of the score: the last hidden state of ``TextEncoderHIP`` at the EOS position through
``text_projection``.  tests/test_clip_score_gpu.py bounds both embeddings against the fp32 torch module.
"""
from __future__ import annotations

import torch

from .. import ops
from ..ops import BF16, F32
from .text_hip import layernorm, linear, load_layers, run_layers


def eos_index(input_ids: torch.Tensor, eos_token_id: int) -> torch.Tensor:
    """Row of the last hidden state ``CLIPTextModel`` pools, per sequence: the argmax of the ids for the legacy configuration
    (``eos_token_id == 2``: the EOS token has the largest id of the vocabulary), else the first position holding
    ``eos_token_id``.  int64 [B]; no host synchronisation."""
    if eos_token_id == 2:
        return input_ids.to(torch.int).argmax(dim=-1)
    return (input_ids.to(torch.int) == eos_token_id).int().argmax(dim=-1)


class CLIPVisionHIP:
    """``tower(images_uint8)`` -> ``image_embeds`` fp32 [B, projection_dim].  ``model``: a ``CLIPModel`` or
    ``CLIPVisionModelWithProjection`` (fp32 weights are read, the module is not kept)."""

    def __init__(self, model, device='cuda'):
        self.dev = torch.device(device)
        if self.dev.type != 'cuda':
            raise RuntimeError('CLIPVisionHIP runs on an MI355X only')
        cfg = getattr(model.config, 'vision_config', model.config)
        self.C, self.H, self.L = cfg.hidden_size, cfg.num_attention_heads, cfg.num_hidden_layers
        self.R, self.P = cfg.image_size, cfg.patch_size
        self.eps, self.act = float(cfg.layer_norm_eps), cfg.hidden_act
        if self.C % self.H or self.C // self.H != 64 or self.act not in ('gelu', 'quick_gelu'):
            raise ValueError(f'CLIPVisionHIP: unsupported config (hidden {self.C}, heads {self.H}: head_dim must be 64; '
                             f'act {self.act})')
        if self.R % self.P or self.P > ops.CLIP_MAX_PATCH or self.R > ops.CLIP_MAX_SIZE:
            raise ValueError(f'CLIPVisionHIP: image {self.R}, patch {self.P}')
        pre = 'vision_model.'
        sd = {(k[len(pre):] if k.startswith(pre) else k): v.detach().to(self.dev, F32)
              for k, v in model.state_dict().items() if k.startswith(pre) or k == 'visual_projection.weight'}
        self.Np = (self.R // self.P) ** 2
        self.Kp = ops.clip_patch_cols(self.P)
        wp = torch.zeros(self.C, self.Kp, device=self.dev, dtype=F32)   # conv weight [C, 3, P, P] -> [C, Kp], zero pad columns
        wp[:, :3 * self.P * self.P] = sd['embeddings.patch_embedding.weight'].reshape(self.C, -1)
        self.w_patch = wp.to(BF16).contiguous()
        tok = sd['embeddings.position_embedding.weight'].clone()
        tok[0] += sd['embeddings.class_embedding']
        self.tok = tok.to(BF16).contiguous()   # [Np + 1, C]; tiled per image on demand
        self._tok_tiled = {}
        self.ln_pre = (sd['pre_layrnorm.weight'].contiguous(), sd['pre_layrnorm.bias'].contiguous())
        self.layers = load_layers(sd, self.L)
        self.ln_post = (sd['post_layernorm.weight'].contiguous(), sd['post_layernorm.bias'].contiguous())
        self.w_proj = sd['visual_projection.weight'].to(BF16).contiguous()

    def patch_matrix(self, images: torch.Tensor, mean, std) -> torch.Tensor:
        B = images.shape[0]
        out = torch.empty(B * (self.Np + 1), self.Kp, device=self.dev, dtype=BF16)
        return ops.clip_preprocess(images, self.R, self.P, out, 0, mean, std)

    @torch.no_grad()
    def forward_patches(self, patches: torch.Tensor, B: int) -> torch.Tensor:
        """the kind-0 patch matrix of ``B`` images -> ``image_embeds``"""
        T, C = self.Np + 1, self.C
        M = B * T
        if ops.SPLITK_WS is None:
            ops.SPLITK_WS = torch.empty(32 * 1024 * 1024, device=self.dev, dtype=F32)
        if B not in self._tok_tiled:
            self._tok_tiled = {B: self.tok.repeat(B, 1).contiguous()}
        stats = torch.empty(2 * M, device=self.dev, dtype=F32)
        h = linear(patches, self.w_patch, None, residual=self._tok_tiled[B])
        h = layernorm(h, self.ln_pre, stats, self.eps)
        h = run_layers(self.layers, h, B, T, self.H, self.act, self.eps, stats, causal=False)
        cls = h.view(B, T * C)[:, :C]   # the class rows: leading dimension T * C
        pooled = layernorm(cls, self.ln_post, stats, self.eps)
        return linear(pooled, self.w_proj, None, dtype=F32)

    def __call__(self, images: torch.Tensor, mean, std) -> torch.Tensor:
        images = images.to(self.dev)
        return self.forward_patches(self.patch_matrix(images, mean, std), images.shape[0])


class CLIPTextEmbedHIP:
    """``text(input_ids)`` -> ``text_embeds`` fp32 [B, projection_dim]: ``TextEncoderHIP`` on the model's text tower, the EOS
    row of its last hidden state, ``text_projection``."""

    def __init__(self, model, device='cuda'):
        from .text_hip import TextEncoderHIP
        self.dev = torch.device(device)
        if self.dev.type != 'cuda':
            raise RuntimeError('CLIPTextEmbedHIP runs on an MI355X only')
        cfg = model.config.text_config
        if cfg.hidden_size // cfg.num_attention_heads != 64:
            raise ValueError(f'CLIPTextEmbedHIP: head_dim {cfg.hidden_size // cfg.num_attention_heads} (must be 64)')
        self.encoder = TextEncoderHIP(model.text_model, device)
        self.eos_token_id = cfg.eos_token_id
        self.max_length = cfg.max_position_embeddings
        self.w_proj = model.text_projection.weight.detach().to(self.dev, BF16).contiguous()

    @torch.no_grad()
    def __call__(self, input_ids: torch.Tensor) -> torch.Tensor:
        ids = input_ids.to(self.dev)[:, :self.max_length]
        last = self.encoder(ids)[0]
        rows = last[torch.arange(ids.shape[0], device=self.dev), eos_index(ids, self.eos_token_id)]
        return linear(rows.to(BF16).contiguous(), self.w_proj, None, dtype=F32)
