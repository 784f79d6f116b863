"""Frozen SD-2 VAE on the hand-written gfx950 kernels (forward only): ``VAEEncoderHIP`` and ``VAEDecoderHIP``.

The reference encodes images inside the training step when latents are not precomputed
(/root/reference diffusion/models/stable_diffusion.py:160-174: ``vae.encode(x)['latent_dist'].sample()`` then
``*= 0.18215``) and prices that at x1.4 step time (README.md:52), and decodes sampled latents in ``generate``
(:380 ``vae.decode(latents).sample``).  On PyTorch-ROCm the fp16 encoder alone costs twice the whole U-Net training step per
image (466 vs 1,390 images/s); the VAE's arithmetic is the op set the U-Net kernels already cover -
GroupNorm(32, eps 1e-6)+SiLU, 3x3 / 1x1 convolutions on NHWC bf16, one stride-2 downsampler (gather mode 4 = Downsample2D's
bottom/right zero padding) or one nearest-2x upsampler convolution (gather mode 3, no materialised upsampled tensor) per
level - so this module walks ``models/vae.AutoencoderKL`` through ``da_groupnorm_fwd`` / ``da_gemm_nt``.  The single
512-wide mid-block attention head (1,024 tokens at 256 px) runs on ``da_attn_fwd_wide``; only an ``AutoencoderKL`` built
with another mid width falls to torch SDPA for that one product.

Weights are taken from the torch module (bf16 OHWI copies; the encoder folds ``quant_conv`` into ``conv_out``; the decoder
runs ``post_quant_conv`` as its own 1x1 GEMM because ``conv_in`` zero-pads the BIASED tensor); activations are bf16 with
fp32 accumulation / statistics where the reference runs the VAE in fp16 (``encode_latents_in_fp16``):
tests/test_vae_hip_gpu.py and tests/test_vae_decoder_hip_gpu.py bound the differences against the fp32 torch module.
"""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn.functional as F

from .. import ops
from ..ops import BF16, F32, Geom
from .vae import AutoencoderKL, DiagonalGaussian, _Out


def _ohwi(w: torch.Tensor, cin_pad: int = 0, cout_pad: int = 0) -> torch.Tensor:
    """[O, I, kh, kw] fp32 -> bf16 [O', kh*kw*I'] (I / O zero-padded to multiples the kernels accept)."""
    o, i, kh, kw = w.shape
    ip, op = max(i, cin_pad), max(o, cout_pad)
    t = torch.zeros(op, kh, kw, ip, dtype=torch.float32, device=w.device)
    t[:o, :, :, :i] = w.float().permute(0, 2, 3, 1)
    return t.reshape(op, kh * kw * ip).to(BF16).contiguous()


class _VAEWalkHIP:
    """What the two halves share: weight preparation from the torch module's state dict under ``prefix``, the
    GroupNorm / resnet / mid-block walks and their buffers."""
    name = '_VAEWalkHIP'

    def __init__(self, vae: AutoencoderKL, prefix: str, device='cuda'):
        self.dev = torch.device(device)
        if self.dev.type != 'cuda':
            raise RuntimeError(f'{self.name} runs on an MI355X only')
        self.w: Dict[str, torch.Tensor] = {}
        self.v: Dict[str, torch.Tensor] = {}
        self.prefix = prefix
        self.sd = {k: v.detach().to(self.dev, torch.float32) for k, v in vae.state_dict().items()}
        self._scratch = None

    def _conv(self, key, cin_pad=0, cout_pad=0, prefix=None):
        prefix = self.prefix if prefix is None else prefix
        self.w[key] = _ohwi(self.sd[f'{prefix}{key}.weight'], cin_pad, cout_pad)
        b = self.sd[f'{prefix}{key}.bias']
        self.v[key + '.bias'] = F.pad(b, (0, max(0, cout_pad - b.numel()))).contiguous()

    def _norm(self, key):
        self.v[key + '.weight'] = self.sd[f'{self.prefix}{key}.weight'].contiguous()
        self.v[key + '.bias'] = self.sd[f'{self.prefix}{key}.bias'].contiguous()

    def _lin(self, key):
        self.w[key] = self.sd[f'{self.prefix}{key}.weight'].to(BF16).contiguous()
        self.v[key + '.bias'] = self.sd[f'{self.prefix}{key}.bias'].contiguous()

    def _prep_res(self, key, cin, cout):
        self._norm(key + '.norm1'); self._conv(key + '.conv1'); self._norm(key + '.norm2'); self._conv(key + '.conv2')
        if cin != cout:
            self._conv(key + '.conv_shortcut')

    def _prep_mid(self, c):
        self.cmid = c
        self._prep_res('mid_block.resnets.0', c, c)
        self._prep_res('mid_block.resnets.1', c, c)
        self._norm('mid_block.attentions.0.group_norm')
        for n in ('to_q', 'to_k', 'to_v', 'to_out.0'):
            self._lin(f'mid_block.attentions.0.{n}')
        # fused q|k|v projection
        a = 'mid_block.attentions.0'
        self.w[a + '.qkv'] = torch.cat([self.w[f'{a}.to_q'], self.w[f'{a}.to_k'], self.w[f'{a}.to_v']]).contiguous()
        self.v[a + '.qkv.bias'] = torch.cat([self.v[f'{a}.to_q.bias'], self.v[f'{a}.to_k.bias'], self.v[f'{a}.to_v.bias']])

    # ------------------------------------------------------------------------------------------
    def _bf(self, m, c):
        return torch.empty(m, c, device=self.dev, dtype=BF16)

    def _ensure(self, B, HW, C):
        need = ops.norm_scratch_floats(B, HW, C)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, device=self.dev, dtype=F32)
        if getattr(self, '_ss', None) is None or self._ss.numel() < B * C * 2:
            self._ss = torch.empty(B * C * 2, device=self.dev, dtype=F32)
        if ops.SPLITK_WS is None:
            ops.SPLITK_WS = torch.empty(32 * 1024 * 1024, device=self.dev, dtype=F32)

    def _gn(self, x, key, B, HW, silu):
        C = x.shape[1]
        self._ensure(B, HW, C)
        y = self._bf(B * HW, C)
        st = torch.empty(B * 32 * 2, device=self.dev, dtype=F32)
        ops.groupnorm_fwd(x, y, self.v[key + '.weight'], self.v[key + '.bias'], st, self._ss, self._scratch, B, HW, C,
                          32, 1e-6, silu)
        return y

    def _res(self, key, x, B, H, W):
        cout = self.w[key + '.conv1'].shape[0]
        g3 = Geom.conv(B, H, W)
        a = self._gn(x, key + '.norm1', B, H * W, 1)
        h = self._bf(B * H * W, cout)
        ops.gemm_nt(a, self.w[key + '.conv1'], h, g3, bias=self.v[key + '.conv1.bias'])
        a = self._gn(h, key + '.norm2', B, H * W, 1)
        if (key + '.conv_shortcut') in self.w:
            xs = self._bf(B * H * W, cout)
            ops.gemm_nt(x, self.w[key + '.conv_shortcut'], xs, Geom.conv(B, H, W, 1), bias=self.v[key + '.conv_shortcut.bias'])
            x = xs
        y = self._bf(B * H * W, cout)
        ops.gemm_nt(a, self.w[key + '.conv2'], y, g3, bias=self.v[key + '.conv2.bias'], residual=x)
        return y

    def _mid(self, h, B, H, W):
        """resnet, single-head attention over the H*W tokens, resnet"""
        h = self._res('mid_block.resnets.0', h, B, H, W)
        a = 'mid_block.attentions.0'
        Cm, N = self.cmid, H * W
        g = self._gn(h, a + '.group_norm', B, N, 0)
        qkv = self._bf(B * N, 3 * Cm)
        ops.gemm_nt(g, self.w[a + '.qkv'], qkv, Geom.linear(B * N), bias=self.v[a + '.qkv.bias'])
        if Cm == 512:
            # head_dim = C = 512: the three column slices of the fused buffer go to the kernel as strided views
            o = self._bf(B * N, Cm)
            l2 = torch.empty(B * N, device=self.dev, dtype=F32)
            ops.attn_fwd_wide(qkv[:, :Cm], qkv[:, Cm:2 * Cm], qkv[:, 2 * Cm:], o, l2, B, 1, Cm, N, N, Cm**-0.5)
        else:   # an AutoencoderKL with another mid width: no kernel for that head_dim
            q, k, v = (qkv[:, j * Cm:(j + 1) * Cm].reshape(B, 1, N, Cm) for j in range(3))
            o = F.scaled_dot_product_attention(q, k, v).reshape(B * N, Cm).contiguous()
        y = self._bf(B * N, Cm)
        ops.gemm_nt(o, self.w[a + '.to_out.0'], y, Geom.linear(B * N), bias=self.v[a + '.to_out.0.bias'], residual=h)
        return self._res('mid_block.resnets.1', y, B, H, W)


class VAEEncoderHIP(_VAEWalkHIP):
    """``encode(images)`` -> the same ``{'latent_dist': DiagonalGaussian}`` as ``AutoencoderKL.encode``."""
    name = 'VAEEncoderHIP'

    def __init__(self, vae: AutoencoderKL, device='cuda'):
        super().__init__(vae, 'encoder.', device)
        enc = vae.encoder
        self._conv('conv_in', cin_pad=8)
        self.levels = []
        cin = enc.conv_in.out_channels
        for i, blk in enumerate(enc.down_blocks):
            cout = blk.resnets[0].conv1.out_channels
            self._prep_res(f'down_blocks.{i}.resnets.0', cin, cout)
            self._prep_res(f'down_blocks.{i}.resnets.1', cout, cout)
            down = blk.downsamplers is not None
            if down:
                self._conv(f'down_blocks.{i}.downsamplers.0.conv')
            self.levels.append((cin, cout, down))
            cin = cout
        self._prep_mid(cin)
        self._norm('conv_norm_out')
        # conv_out (3x3, C -> 2z) followed by quant_conv (1x1, 2z -> 2z): one 3x3 conv with composed weights
        wo, bo = self.sd['encoder.conv_out.weight'], self.sd['encoder.conv_out.bias']
        wq, bq = self.sd['quant_conv.weight'][:, :, 0, 0], self.sd['quant_conv.bias']
        self.w['conv_out'] = _ohwi(torch.einsum('pq,qikl->pikl', wq, wo))
        self.v['conv_out.bias'] = (wq @ bo + bq).contiguous()
        self.zc2 = wo.shape[0]
        del self.sd

    @torch.no_grad()
    def moments(self, images: torch.Tensor) -> torch.Tensor:
        """images [B,3,H,W] (any float dtype, NCHW) -> [B, 2*z, H/8, W/8] fp32 (mean | logvar)."""
        B, C, H, W = images.shape
        if C != 3 or H % 8 or W % 8:
            raise ValueError('VAEEncoderHIP: images must be [B,3,H,W] with H, W multiples of 8')
        x = torch.zeros(B * H * W, 8, device=self.dev, dtype=BF16)   # NHWC, 3 channels padded to 8
        x.view(B, H, W, 8)[..., :3] = images.to(self.dev).permute(0, 2, 3, 1)
        return self.moments_nhwc8(x, B, H, W)

    @torch.no_grad()
    def moments_nhwc8(self, x: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
        """``moments`` of images already in the layout conv_in reads: bf16 [B*H*W, 8] NHWC, channels 3..7 zero (what
        ``ops.image_ingest`` kind 0 writes)."""
        if H % 8 or W % 8 or x.dtype != BF16 or not x.is_cuda or not x.is_contiguous() or x.numel() != B * H * W * 8:
            raise ValueError('VAEEncoderHIP: x must be a contiguous bf16 [B*H*W, 8] device tensor, H and W multiples of 8')
        x = x.view(B * H * W, 8)
        h = self._bf(B * H * W, self.w['conv_in'].shape[0])
        ops.gemm_nt(x, self.w['conv_in'], h, Geom.conv(B, H, W), bias=self.v['conv_in.bias'])
        del x
        for i, (cin, cout, down) in enumerate(self.levels):
            h = self._res(f'down_blocks.{i}.resnets.0', h, B, H, W)
            h = self._res(f'down_blocks.{i}.resnets.1', h, B, H, W)
            if down:
                key = f'down_blocks.{i}.downsamplers.0.conv'
                y = self._bf(B * (H // 2) * (W // 2), cout)
                ops.gemm_nt(h, self.w[key], y, Geom.down_vae(B, H, W), bias=self.v[key + '.bias'])
                h, H, W = y, H // 2, W // 2
        h = self._mid(h, B, H, W)
        N = H * W
        g = self._gn(h, 'conv_norm_out', B, N, 1)
        out = torch.empty(B * N, self.zc2, device=self.dev, dtype=F32)
        ops.gemm_nt(g, self.w['conv_out'], out, Geom.conv(B, H, W), bias=self.v['conv_out.bias'])
        return out.view(B, H, W, self.zc2).permute(0, 3, 1, 2)

    def encode(self, images: torch.Tensor):
        return _Out(latent_dist=DiagonalGaussian(self.moments(images)))


class VAEDecoderHIP(_VAEWalkHIP):
    """``decode(z)`` -> the same ``{'sample': images}`` as ``AutoencoderKL.decode`` (fp32, NCHW)."""
    name = 'VAEDecoderHIP'

    def __init__(self, vae: AutoencoderKL, device='cuda'):
        super().__init__(vae, 'decoder.', device)
        dec = vae.decoder
        # post_quant_conv (1x1, z -> z) stays a GEMM of its own: conv_in zero-pads its BIASED output, so composing the two
        # would change the border pixels.  Its 4 output channels are padded to the 8 that conv_in reads (zero rows / bias).
        self._conv('post_quant_conv', cin_pad=8, cout_pad=8, prefix='')
        self._conv('conv_in', cin_pad=8)
        cin = dec.conv_in.out_channels
        self._prep_mid(cin)
        self.levels = []
        for i, blk in enumerate(dec.up_blocks):
            cout = blk.resnets[0].conv1.out_channels
            for j in range(len(blk.resnets)):
                self._prep_res(f'up_blocks.{i}.resnets.{j}', cin if j == 0 else cout, cout)
            up = blk.upsamplers is not None
            if up:
                self._conv(f'up_blocks.{i}.upsamplers.0.conv')
            self.levels.append((len(blk.resnets), cout, up))
            cin = cout
        self._norm('conv_norm_out')
        self._conv('conv_out', cout_pad=8)
        self.zc = dec.conv_in.in_channels
        self.out_channels = dec.conv_out.out_channels
        del self.sd

    @torch.no_grad()
    def decode(self, z: torch.Tensor):
        """z [B,zc,h,w] (any float dtype, NCHW) -> ``sample`` [B,3,8h,8w] fp32"""
        B, C, H, W = z.shape
        if C != self.zc:
            raise ValueError(f'VAEDecoderHIP: latents must be [B,{self.zc},h,w]')
        x = torch.zeros(B * H * W, 8, device=self.dev, dtype=BF16)   # NHWC, latent channels padded to 8
        x.view(B, H, W, 8)[..., :C] = z.to(self.dev).permute(0, 2, 3, 1)
        zq = self._bf(B * H * W, 8)
        ops.gemm_nt(x, self.w['post_quant_conv'], zq, Geom.conv(B, H, W, 1), bias=self.v['post_quant_conv.bias'])
        h = self._bf(B * H * W, self.w['conv_in'].shape[0])
        ops.gemm_nt(zq, self.w['conv_in'], h, Geom.conv(B, H, W), bias=self.v['conv_in.bias'])
        h = self._mid(h, B, H, W)
        for i, (nres, cout, up) in enumerate(self.levels):
            for j in range(nres):
                h = self._res(f'up_blocks.{i}.resnets.{j}', h, B, H, W)
            if up:   # the 3x3 conv reads the nearest-2x upsampled image through the gather: no upsampled tensor
                key = f'up_blocks.{i}.upsamplers.0.conv'
                y = self._bf(B * 4 * H * W, cout)
                ops.gemm_nt(h, self.w[key], y, Geom.up(B, H, W), bias=self.v[key + '.bias'])
                h, H, W = y, 2 * H, 2 * W
        g = self._gn(h, 'conv_norm_out', B, H * W, 1)
        out = torch.empty(B * H * W, 8, device=self.dev, dtype=F32)
        ops.gemm_nt(g, self.w['conv_out'], out, Geom.conv(B, H, W), bias=self.v['conv_out.bias'])
        return _Out(sample=out.view(B, H, W, 8)[..., :self.out_channels].permute(0, 3, 1, 2))
