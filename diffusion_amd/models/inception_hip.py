"""The FID Inception-v3 (torch-fidelity's ``FeatureExtractorInceptionV3`` at ``pool3``, the network torchmetrics'
``FrechetInceptionDistance(feature=2048)`` runs) on the hand-written gfx950 kernels, forward only.

Every unit is convolution (no bias) + BatchNorm (eps 1e-3) + ReLU; the BatchNorm is folded into bf16 weights
``[Cout][kh][kw][Cin]`` and an fp32 bias when the state dict is read, so a unit is one ``da_conv2d_relu_fwd`` launch.  The
network is the table ``plan()`` builds: a list of launches over named NHWC buffers, where the branches of a Mixed block
write their column slice of the block's output buffer (``ldy``: no concatenation pass).  The input transform is
``da_inception_preprocess`` (TF1-style bilinear resize to 299 x 299, (v - 128) / 128), the head ``da_avgpool_global_f32``.

The FID variant differs from torchvision's Inception-v3 in its pooling: the average pools of the A, C and E blocks exclude
the padding from the count, and the branch pool of ``Mixed_7c`` is a MAX pool.  Both were written from torch-fidelity's
documented behaviour; neither that package nor its weights file is available to the tests, which check this walk against a
plain ``torch.nn`` module of the same definition (tests/inception_reference.py).

State-dict keys are torchvision's, which are also those of torch-fidelity's ``pt_inception-2015-12-05`` file:
``<unit>.conv.weight`` and ``<unit>.bn.{weight,bias,running_mean,running_var}``; ``num_batches_tracked`` and ``fc.bias``
are ignored.  ``fc.weight`` ([1008, 2048]) is optional: when it is there the tower keeps it in fp32 for
``logits_unbiased`` (torch-fidelity's bias-free head, ``da_fc_logits_f32``), which the Inception score reads.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import torch

from .. import ops
from ..ops import BF16, F32
from .vae_hip import _ohwi

BN_EPS = 1e-3
FEATURES = 2048
CLASSES = 1008   # the 2015 graph's logits: 1000 ImageNet classes and 8 unused ones
SIDE = ops.INCEPTION_SIDE


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


class _Plan:
    """units: name -> (cin, cout, kh, kw, stride, ph, pw); bufs: name -> (side, channels); ops: the launches in order,
    ('conv', unit, src, dst, dst_col) and ('pool', kind, stride, pad, src, dst, dst_col)."""

    def __init__(self):
        self.units: Dict[str, Tuple[int, ...]] = {}
        self.bufs: Dict[str, Tuple[int, int]] = {}
        self.ops: List[tuple] = []
        self.blocks: List[str] = []   # buffer names of the 11 Mixed outputs, in order

    def buf(self, name, side, C):
        if self.bufs.setdefault(name, (side, C)) != (side, C):
            raise AssertionError(f'buffer {name}: {self.bufs[name]} vs {(side, C)}')
        return name

    def conv(self, unit, src, dst, cin, cout, k=1, s=1, p=0, col=0, width=None):
        (kh, kw), (ph, pw) = _pair(k), _pair(p)
        side = self.bufs[src][0]
        assert self.bufs[src][1] == cin, (unit, self.bufs[src], cin)
        oh, ow = (side + 2 * ph - kh) // s + 1, (side + 2 * pw - kw) // s + 1
        assert oh == ow
        self.buf(dst, oh, width if width is not None else cout)
        self.units[unit] = (cin, cout, kh, kw, s, ph, pw)
        self.ops.append(('conv', unit, src, dst, col))
        return dst

    def pool(self, kind, s, p, src, dst, col=0, width=None):
        side, C = self.bufs[src]
        self.buf(dst, (side + 2 * p - 3) // s + 1, width if width is not None else C)
        self.ops.append(('pool', kind, s, p, src, dst, col))
        return dst


def plan() -> _Plan:
    P = _Plan()
    P.buf('x', SIDE, 8)
    P.conv('Conv2d_1a_3x3', 'x', 's1', 8, 32, 3, 2)
    P.conv('Conv2d_2a_3x3', 's1', 's2', 32, 32, 3)
    P.conv('Conv2d_2b_3x3', 's2', 's3', 32, 64, 3, 1, 1)
    P.pool(0, 2, 0, 's3', 's4')
    P.conv('Conv2d_3b_1x1', 's4', 's5', 64, 80)
    P.conv('Conv2d_4a_3x3', 's5', 's6', 80, 192, 3)
    x = P.pool(0, 2, 0, 's6', 's7')

    for name, cin, pf in (('Mixed_5b', 192, 32), ('Mixed_5c', 256, 64), ('Mixed_5d', 288, 64)):
        w = 224 + pf
        u = lambda b: f'{name}.{b}'
        P.conv(u('branch1x1'), x, name, cin, 64, col=0, width=w)
        P.conv(u('branch5x5_1'), x, 'a48', cin, 48)
        P.conv(u('branch5x5_2'), 'a48', name, 48, 64, 5, 1, 2, col=64, width=w)
        P.conv(u('branch3x3dbl_1'), x, 'a64', cin, 64)
        P.conv(u('branch3x3dbl_2'), 'a64', 'a96', 64, 96, 3, 1, 1)
        P.conv(u('branch3x3dbl_3'), 'a96', name, 96, 96, 3, 1, 1, col=128, width=w)
        P.pool(1, 1, 1, x, f'ap{cin}')
        P.conv(u('branch_pool'), f'ap{cin}', name, cin, pf, col=224, width=w)
        P.blocks.append(name)
        x = name

    name = 'Mixed_6a'
    P.conv(f'{name}.branch3x3', x, name, 288, 384, 3, 2, col=0, width=768)
    P.conv(f'{name}.branch3x3dbl_1', x, 'a64', 288, 64)
    P.conv(f'{name}.branch3x3dbl_2', 'a64', 'a96', 64, 96, 3, 1, 1)
    P.conv(f'{name}.branch3x3dbl_3', 'a96', name, 96, 96, 3, 2, col=384, width=768)
    P.pool(0, 2, 0, x, name, col=480, width=768)
    P.blocks.append(name)
    x = name

    for name, c7 in (('Mixed_6b', 128), ('Mixed_6c', 160), ('Mixed_6d', 160), ('Mixed_6e', 192)):
        u = lambda b: f'{name}.{b}'
        ta, tb = f'c{c7}a', f'c{c7}b'
        P.conv(u('branch1x1'), x, name, 768, 192, col=0, width=768)
        P.conv(u('branch7x7_1'), x, ta, 768, c7)
        P.conv(u('branch7x7_2'), ta, tb, c7, c7, (1, 7), 1, (0, 3))
        P.conv(u('branch7x7_3'), tb, name, c7, 192, (7, 1), 1, (3, 0), col=192, width=768)
        P.conv(u('branch7x7dbl_1'), x, ta, 768, c7)
        P.conv(u('branch7x7dbl_2'), ta, tb, c7, c7, (7, 1), 1, (3, 0))
        P.conv(u('branch7x7dbl_3'), tb, ta, c7, c7, (1, 7), 1, (0, 3))
        P.conv(u('branch7x7dbl_4'), ta, tb, c7, c7, (7, 1), 1, (3, 0))
        P.conv(u('branch7x7dbl_5'), tb, name, c7, 192, (1, 7), 1, (0, 3), col=384, width=768)
        P.pool(1, 1, 1, x, 'cp768')
        P.conv(u('branch_pool'), 'cp768', name, 768, 192, col=576, width=768)
        P.blocks.append(name)
        x = name

    name = 'Mixed_7a'
    P.conv(f'{name}.branch3x3_1', x, 'c192a', 768, 192)
    P.conv(f'{name}.branch3x3_2', 'c192a', name, 192, 320, 3, 2, col=0, width=1280)
    P.conv(f'{name}.branch7x7x3_1', x, 'c192a', 768, 192)
    P.conv(f'{name}.branch7x7x3_2', 'c192a', 'c192b', 192, 192, (1, 7), 1, (0, 3))
    P.conv(f'{name}.branch7x7x3_3', 'c192b', 'c192a', 192, 192, (7, 1), 1, (3, 0))
    P.conv(f'{name}.branch7x7x3_4', 'c192a', name, 192, 192, 3, 2, col=320, width=1280)
    P.pool(0, 2, 0, x, name, col=512, width=1280)
    P.blocks.append(name)
    x = name

    for name, cin, kind in (('Mixed_7b', 1280, 1), ('Mixed_7c', 2048, 0)):   # 7c pools with a MAX: the FID variant
        u = lambda b: f'{name}.{b}'
        P.conv(u('branch1x1'), x, name, cin, 320, col=0, width=2048)
        P.conv(u('branch3x3_1'), x, 'e384', cin, 384)
        P.conv(u('branch3x3_2a'), 'e384', name, 384, 384, (1, 3), 1, (0, 1), col=320, width=2048)
        P.conv(u('branch3x3_2b'), 'e384', name, 384, 384, (3, 1), 1, (1, 0), col=704, width=2048)
        P.conv(u('branch3x3dbl_1'), x, 'e448', cin, 448)
        P.conv(u('branch3x3dbl_2'), 'e448', 'e384', 448, 384, 3, 1, 1)
        P.conv(u('branch3x3dbl_3a'), 'e384', name, 384, 384, (1, 3), 1, (0, 1), col=1088, width=2048)
        P.conv(u('branch3x3dbl_3b'), 'e384', name, 384, 384, (3, 1), 1, (1, 0), col=1472, width=2048)
        P.pool(kind, 1, 1, x, f'ep{cin}')
        P.conv(u('branch_pool'), f'ep{cin}', name, cin, 192, col=1856, width=2048)
        P.blocks.append(name)
        x = name
    return P


def _state_keys(units):
    for name, (cin, cout, kh, kw, *_rest) in units.items():
        yield f'{name}.conv.weight', (cout, 3 if name == 'Conv2d_1a_3x3' else cin, kh, kw)
        for k in ('weight', 'bias', 'running_mean', 'running_var'):
            yield f'{name}.bn.{k}', (cout,)


def random_state_dict(seed: int = 0) -> Dict[str, torch.Tensor]:
    """He-normal convolutions and identity BatchNorm statistics from a fixed generator: every rank and every copy of a
    random-init tower holds the same weights"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in _state_keys(plan().units):
        if key.endswith('conv.weight'):
            fan_in = shape[1] * shape[2] * shape[3]
            sd[key] = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
        elif key.endswith('bn.weight') or key.endswith('running_var'):
            sd[key] = torch.ones(shape)
        else:
            sd[key] = torch.zeros(shape)
    return sd


def random_fc_weight(seed: int = 0) -> torch.Tensor:
    """the [1008, 2048] head of a random-init tower, N(0, 1 / 2048) from a generator of its own: ``random_state_dict`` draws
    nothing for it and returns what it always did"""
    g = torch.Generator().manual_seed(0x1008 + int(seed))
    return torch.randn(CLASSES, FEATURES, generator=g) * FEATURES ** -0.5


def check_state_dict(sd, where='state dict') -> None:
    """strict: every key of every unit, with its shape, and the shape of ``fc.weight`` when that is present; RuntimeError
    otherwise"""
    missing, bad = [], []
    units = plan().units
    for key, shape in _state_keys(units):
        if key not in sd:
            missing.append(key)
        elif tuple(sd[key].shape) != shape:
            bad.append((key, tuple(sd[key].shape), shape))
    if 'fc.weight' in sd and tuple(sd['fc.weight'].shape) != (CLASSES, FEATURES):
        bad.append(('fc.weight', tuple(sd['fc.weight'].shape), (CLASSES, FEATURES)))
    extra = [k for k in sd if k.split('.')[0] != 'fc' and not k.endswith('num_batches_tracked')
             and '.'.join(k.split('.')[:-2]) not in units]
    if missing or bad or extra:
        raise RuntimeError(f'{where}: not an FID Inception-v3 state dict (missing {missing[:4]}, mis-shaped {bad[:4]}, '
                           f'unexpected {extra[:4]})')


def load_state_dict_file(path: str) -> Dict[str, torch.Tensor]:
    sd = torch.load(path, map_location='cpu', weights_only=True)
    if not isinstance(sd, dict):
        raise RuntimeError(f'{path}: not a state dict')
    check_state_dict(sd, path)
    return sd


class InceptionV3HIP:
    """``tower(images)`` -> fp32 [B, 2048] ``pool3`` features of planar [B, 3, H, W] images (uint8 levels, or fp32 in [0, 1]
    which the preprocess kernel turns into levels as ``(x * 255).byte()`` does).  ``state_dict``: checked strictly.  Buffers
    are allocated once per batch size and kept (19.7 MB per image of the batch; batch sizes are at most ``max_batch``);
    inputs larger than ``max_batch`` are walked in chunks."""

    def __init__(self, state_dict, device='cuda', max_batch: int = 32):
        self.dev = torch.device(device)
        if self.dev.type != 'cuda':
            raise RuntimeError('InceptionV3HIP runs on an MI355X only')
        check_state_dict(state_dict)
        self.max_batch = int(max_batch)
        if self.max_batch < 1:
            raise ValueError('max_batch must be >= 1')
        self.plan = plan()
        self.units = {}   # name -> (W bf16 [Cout, kh*kw*Cin], bias fp32 [Cout])
        for name, (cin, cout, kh, kw, *_r) in self.plan.units.items():
            w = state_dict[f'{name}.conv.weight'].detach().to(self.dev, torch.float64)
            bn = {k: state_dict[f'{name}.bn.{k}'].detach().to(self.dev, torch.float64)
                  for k in ('weight', 'bias', 'running_mean', 'running_var')}
            scale = bn['weight'] / torch.sqrt(bn['running_var'] + BN_EPS)
            wf = (w * scale[:, None, None, None]).to(F32)
            bias = (bn['bias'] - bn['running_mean'] * scale).to(F32).contiguous()
            self.units[name] = (_ohwi(wf, cin_pad=cin), bias)
        fc = state_dict.get('fc.weight')
        self.fc_weight = None if fc is None else fc.detach().to(self.dev, F32).contiguous()
        self._bufs = {}   # batch size -> its buffers: a short last batch does not free and reallocate the full one's

    def _buffers(self, B):
        if B not in self._bufs:
            bufs = {name: torch.empty(B * side * side, C, device=self.dev, dtype=BF16)
                    for name, (side, C) in self.plan.bufs.items()}
            bufs['feat'] = torch.empty(B, FEATURES, device=self.dev, dtype=F32)
            self._bufs[B] = bufs
        return self._bufs[B]

    def _walk(self, images, trace: Optional[Callable] = None):
        B = images.shape[0]
        bufs = self._buffers(B)
        ops.inception_preprocess(images, bufs['x'])
        for op in self.plan.ops:
            if op[0] == 'conv':
                _, unit, src, dst, col = op
                cin, cout, kh, kw, s, ph, pw = self.plan.units[unit]
                side = self.plan.bufs[src][0]
                X, Y = bufs[src], bufs[dst][:, col:col + cout]
                W, bias = self.units[unit]
                ops.conv2d_relu_fwd(X, W, bias, Y, B, side, side, kh, kw, s, ph, pw, relu=True)
            else:
                _, kind, s, p, src, dst, col = op
                side, C = self.plan.bufs[src]
                X, Y = bufs[src], bufs[dst][:, col:col + C]
                ops.pool2d_fwd(X, Y, B, side, side, s, p, kind)
            if trace is not None:
                trace(op, X, Y)
        last = self.plan.blocks[-1]
        side = self.plan.bufs[last][0]
        return ops.avgpool_global_f32(bufs[last], bufs['feat'], B, side * side)

    @torch.no_grad()
    def logits_unbiased(self, features: torch.Tensor) -> torch.Tensor:
        """fp32 [B, 1008]: ``features @ fc.weight.T`` without the bias (``da_fc_logits_f32``: float64 sums, one rounding)"""
        if self.fc_weight is None:
            raise RuntimeError("InceptionV3HIP.logits_unbiased: the state dict has no 'fc.weight'")
        out = torch.empty(features.shape[0], CLASSES, device=self.dev, dtype=F32)
        return ops.fc_logits_f32(features, self.fc_weight, out)

    @torch.no_grad()
    def __call__(self, images: torch.Tensor, trace: Optional[Callable] = None) -> torch.Tensor:
        """``trace(op, X, Y)`` is called after every launch with the plan entry and the launch's input and output views
        (the views are live buffers that later launches overwrite)."""
        images = images.to(self.dev).contiguous()
        B = images.shape[0]
        if B <= self.max_batch:
            return self._walk(images, trace).clone()
        out = torch.empty(B, FEATURES, device=self.dev, dtype=F32)
        for i in range(0, B, self.max_batch):
            out[i:i + self.max_batch] = self._walk(images[i:i + self.max_batch], trace)
        return out
