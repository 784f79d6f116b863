"""Frozen SD-2 text encoder (OpenCLIP-H as ``transformers.CLIPTextModel``) on the hand-written gfx950 kernels, forward only.

The reference encodes captions inside the training step when text latents are not precomputed (/root/reference
diffusion/models/stable_diffusion.py:168,172: ``self.text_encoder(conditioning)[0]``, the last hidden state after the
final LayerNorm; ``CLIPTextModel.from_pretrained(..., subfolder='text_encoder')`` at models.py:82).  The encoder is a
pre-LN transformer - LayerNorm, q|k|v projection, 77-token causal attention, output projection + residual, LayerNorm,
fc1, GELU, fc2 + residual - i.e. the op set the U-Net's transformer blocks already run on ``da_layernorm_fwd`` and
``da_gemm_nt`` (bias / residual epilogues).  This module walks the weights of the torch module through those kernels
(bf16 activations, fp32 accumulation / statistics), the causal self-attention through ``da_attn_fwd_causal`` (the flash
forward kernel with a per-query key limit; heads are 64-column slices of the fused q|k|v buffer, so nothing is transposed)
and the MLP activation through ``da_gelu_fwd`` (``da_quick_gelu_fwd`` for CLIP ViT-L/14, the pixel models' encoder).  Only the embedding gather is a torch op.
tests/test_text_hip_gpu.py bounds the difference of the last hidden state against the fp32 torch module.
"""
from __future__ import annotations

from typing import List

import torch
import torch.nn.functional as F

from .. import ops
from ..ops import BF16, F32, Geom


def load_layers(sd, L, prefix='encoder.layers.') -> List[dict]:
    """the L pre-LN layers of a CLIP encoder from fp32 device tensors ``sd``: bf16 weights (q|k|v fused), fp32 biases / affines"""

    def w(key):
        return sd[key + '.weight'].to(BF16).contiguous()

    def v(key, what):
        return sd[f'{key}.{what}'].contiguous()

    layers = []
    for i in range(L):
        p = f'{prefix}{i}.'
        a = p + 'self_attn.'
        layers.append(dict(
            ln1=(v(p + 'layer_norm1', 'weight'), v(p + 'layer_norm1', 'bias')),
            wqkv=torch.cat([w(a + 'q_proj'), w(a + 'k_proj'), w(a + 'v_proj')]).contiguous(),
            bqkv=torch.cat([v(a + 'q_proj', 'bias'), v(a + 'k_proj', 'bias'), v(a + 'v_proj', 'bias')]).contiguous(),
            wo=w(a + 'out_proj'), bo=v(a + 'out_proj', 'bias'),
            ln2=(v(p + 'layer_norm2', 'weight'), v(p + 'layer_norm2', 'bias')),
            w1=w(p + 'mlp.fc1'), b1=v(p + 'mlp.fc1', 'bias'), w2=w(p + 'mlp.fc2'), b2=v(p + 'mlp.fc2', 'bias')))
    return layers


def layernorm(x, gb, stats, eps):
    y = torch.empty_like(x)
    ops.layernorm_fwd(x, y, gb[0], gb[1], stats, eps)
    return y


def linear(x, wgt, bias, residual=None, dtype=BF16):
    out = torch.empty(x.shape[0], wgt.shape[0], device=x.device, dtype=dtype)
    ops.gemm_nt(x, wgt, out, Geom.linear(x.shape[0]), bias=bias, residual=residual)
    return out


def run_layers(layers, h, B, T, H, act, eps, stats, causal):
    """``h`` bf16 [B*T, C] through the pre-LN layers: LayerNorm, q|k|v, attention over the T tokens of each of the B
    sequences (causal: the text tower; else every key: the vision tower), output projection + residual, LayerNorm, fc1,
    GELU, fc2 + residual.  ``stats``: fp32 [2*B*T] scratch."""
    M, C = h.shape
    D = C // H
    l2 = torch.empty(B * H * T, device=h.device, dtype=F32)
    for ly in layers:
        x = layernorm(h, ly['ln1'], stats, eps)
        qkv = linear(x, ly['wqkv'], ly['bqkv'])
        o = torch.empty(M, C, device=h.device, dtype=BF16)
        if D == 64 and causal:   # heads are 64-column slices of the fused projection: no transposes (scale D**-0.5 = CLIP's q scaling)
            ops.attn_fwd_causal(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, l2, B, H, T, D ** -0.5)
        elif D == 64:
            ops.attn_fwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, l2, B, H, T, T, D ** -0.5)
        elif causal:
            q, k, v = (qkv[:, j * C:(j + 1) * C].reshape(B, T, H, D).transpose(1, 2) for j in range(3))
            o = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(M, C).contiguous()
        else:
            raise ValueError(f'run_layers: head_dim {D} (the attention kernel takes 64)')
        h = linear(o, ly['wo'], ly['bo'], residual=h)
        x = layernorm(h, ly['ln2'], stats, eps)
        f = linear(x, ly['w1'], ly['b1'])
        if act == 'gelu':
            ops.gelu_fwd(f, f)
        else:
            ops.quick_gelu_fwd(f, f)
        h = linear(f, ly['w2'], ly['b2'], residual=h)
    return h


class TextEncoderHIP:
    """``encoder(input_ids)[0]`` -> last hidden state ``[B, T, C]`` (fp32), like ``CLIPTextModel``."""

    def __init__(self, text_encoder, device='cuda'):
        self.dev = torch.device(device)
        if self.dev.type != 'cuda':
            raise RuntimeError('TextEncoderHIP runs on an MI355X only')
        cfg = text_encoder.config
        self.C, self.H, self.L = cfg.hidden_size, cfg.num_attention_heads, cfg.num_hidden_layers
        self.eps = float(cfg.layer_norm_eps)
        self.act = cfg.hidden_act
        if self.C % self.H or self.act not in ('gelu', 'quick_gelu'):
            raise ValueError(f'TextEncoderHIP: unsupported config (hidden {self.C}, heads {self.H}, act {self.act})')
        # key names with or without the `text_model.` prefix (transformers 4.x checkpoints / 5.x modules)
        sd = {(k[len('text_model.'):] if k.startswith('text_model.') else k): v.detach().to(self.dev, torch.float32)
              for k, v in text_encoder.state_dict().items()}
        e = 'embeddings.'
        self.tok = sd[e + 'token_embedding.weight']
        self.pos = sd[e + 'position_embedding.weight']

        self.layers = load_layers(sd, self.L)
        self.lnf = (sd['final_layer_norm.weight'].contiguous(), sd['final_layer_norm.bias'].contiguous())

    @torch.no_grad()
    def __call__(self, input_ids: torch.Tensor, **_):
        ids = input_ids.to(self.dev)
        if ids.dim() == 1:
            ids = ids[None]
        B, T = ids.shape
        C, H = self.C, self.H
        M = B * T
        if ops.SPLITK_WS is None:
            ops.SPLITK_WS = torch.empty(32 * 1024 * 1024, device=self.dev, dtype=F32)
        h = (self.tok[ids] + self.pos[:T]).reshape(M, C).to(BF16)
        stats = torch.empty(2 * M, device=self.dev, dtype=F32)
        h = run_layers(self.layers, h, B, T, H, self.act, self.eps, stats, causal=True)
        y = layernorm(h, self.lnf, stats, self.eps)
        return (y.view(B, T, C).float(),)
