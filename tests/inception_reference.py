"""Shared by the FID tests: the FID Inception-v3 (torch-fidelity's ``FeatureExtractorInceptionV3`` at ``pool3``) in plain
``torch.nn`` with torchvision's module names, its input transform in numpy float64, and seeded weights.  Written from the
network's published definition; torchvision and torch-fidelity are not needed."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


class BasicConv2d(nn.Module):
    def __init__(self, cin, cout, **kw):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, bias=False, **kw)
        self.bn = nn.BatchNorm2d(cout, eps=0.001)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


def _avg(x):
    return F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False)


class InceptionA(nn.Module):
    def __init__(self, cin, pf):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(cin, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(cin, pf, kernel_size=1)

    def forward(self, x):
        return torch.cat([self.branch1x1(x), self.branch5x5_2(self.branch5x5_1(x)),
                          self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))), self.branch_pool(_avg(x))], 1)


class InceptionB(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)

    def forward(self, x):
        return torch.cat([self.branch3x3(x), self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))),
                          F.max_pool2d(x, 3, stride=2)], 1)


class InceptionC(nn.Module):
    def __init__(self, cin, c7):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x):
        b7 = self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)))
        bd = self.branch7x7dbl_1(x)
        for m in (self.branch7x7dbl_2, self.branch7x7dbl_3, self.branch7x7dbl_4, self.branch7x7dbl_5):
            bd = m(bd)
        return torch.cat([self.branch1x1(x), b7, bd, self.branch_pool(_avg(x))], 1)


class InceptionD(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)

    def forward(self, x):
        b7 = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        return torch.cat([self.branch3x3_2(self.branch3x3_1(x)), b7, F.max_pool2d(x, 3, stride=2)], 1)


class InceptionE(nn.Module):
    def __init__(self, cin, pool):
        super().__init__()
        self.pool = pool   # 'avg' (Mixed_7b) or 'max' (Mixed_7c: the FID variant)
        self.branch1x1 = BasicConv2d(cin, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(cin, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x):
        b3 = self.branch3x3_1(x)
        bd = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        p = _avg(x) if self.pool == 'avg' else F.max_pool2d(x, 3, stride=1, padding=1)
        return torch.cat([self.branch1x1(x), self.branch3x3_2a(b3), self.branch3x3_2b(b3), self.branch3x3dbl_3a(bd),
                          self.branch3x3dbl_3b(bd), self.branch_pool(p)], 1)


MIXED = ('Mixed_5b', 'Mixed_5c', 'Mixed_5d', 'Mixed_6a', 'Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e', 'Mixed_7a',
         'Mixed_7b', 'Mixed_7c')


class FIDInceptionV3(nn.Module):
    """forward(x): x is the TRANSFORMED input [B, 3, 299, 299] ((v - 128) / 128); returns (pool3 features [B, 2048], the 11
    Mixed outputs)"""

    def __init__(self):
        super().__init__()
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.Mixed_5b = InceptionA(192, 32)
        self.Mixed_5c = InceptionA(256, 64)
        self.Mixed_5d = InceptionA(288, 64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, 128)
        self.Mixed_6c = InceptionC(768, 160)
        self.Mixed_6d = InceptionC(768, 160)
        self.Mixed_6e = InceptionC(768, 192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280, 'avg')
        self.Mixed_7c = InceptionE(2048, 'max')
        self.fc = nn.Linear(2048, 1008)   # present in the weights file, unused at pool3

    def forward(self, x):
        x = self.Conv2d_2b_3x3(self.Conv2d_2a_3x3(self.Conv2d_1a_3x3(x)))
        x = F.max_pool2d(x, 3, stride=2)
        x = self.Conv2d_4a_3x3(self.Conv2d_3b_1x1(x))
        x = F.max_pool2d(x, 3, stride=2)
        mixed = []
        for name in MIXED:
            x = getattr(self, name)(x)
            mixed.append(x)
        return F.adaptive_avg_pool2d(x, 1).flatten(1), mixed


def seeded_module(seed=3):
    """He-normal convolutions; every BatchNorm with live statistics: gamma in [0.5, 1.5], beta ~ N(0, 0.1), running mean
    ~ N(0, 0.1), running variance in [0.5, 2]"""
    g = torch.Generator().manual_seed(seed)
    net = FIDInceptionV3().eval().requires_grad_(False)
    for m in net.modules():
        if isinstance(m, nn.Conv2d):
            fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
        elif isinstance(m, nn.BatchNorm2d):
            n = m.weight.shape[0]
            m.weight.copy_(torch.rand(n, generator=g) + 0.5)
            m.bias.copy_(torch.randn(n, generator=g) * 0.1)
            m.running_mean.copy_(torch.randn(n, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(n, generator=g) * 1.5 + 0.5)
    return net


def seeded_images(B=2, H=64, W=96, seed=7):
    """B uint8 images [B, 3, H, W] that differ in kind, not only in detail (a random tower averages detail away: two noisy
    images of one kind give features within 4 % of each other): even ones are dark and smooth, odd ones high-contrast blocks
    under noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((B, 3, H, W), np.uint8)
    for b in range(B):
        for c in range(3):
            if b % 2 == 0:
                v = 60 + 40 * np.sin((0.05 + 0.01 * b) * yy + 0.03 * xx + c) + rng.normal(0, 2, (H, W))
            else:
                v = 128 + 120 * np.sign(np.sin((0.9 + 0.05 * b) * yy + c) * np.sin(0.7 * xx)) + rng.normal(0, 30, (H, W))
            out[b, c] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return torch.from_numpy(out)


def levels_of_float(x):
    """torchmetrics normalize=True: (x * 255).byte() of float images in [0, 1]; fp32 product, floor"""
    x = np.asarray(x, np.float32)
    return np.floor(np.clip(np.float32(255.0) * x, 0, 255)).astype(np.float64)


def preprocess_f64(levels, side=299):
    """levels [B, 3, H, W] (0..255, any float / int dtype) -> float64 [B, 3, side, side]: TF1-style bilinear resize
    (scale = in / out, src = dst * scale with no half-pixel offset, lo = floor, hi = min(lo + 1, in - 1), lerp along x then
    along y), then (v - 128) / 128.  The source coordinate is the fp32 product the reference implementation forms, so that
    lo and the fraction are those of the defined transform; everything after it is float64."""
    v = np.asarray(levels, np.float64)
    B, C, H, W = v.shape

    def axis(n_in):
        src = (np.arange(side, dtype=np.float32) * np.float32(n_in / side)).astype(np.float64)
        lo = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
        return lo, np.minimum(lo + 1, n_in - 1), src - lo
    ylo, yhi, dy = axis(H)
    xlo, xhi, dx = axis(W)
    rows = v[:, :, :, xlo] + (v[:, :, :, xhi] - v[:, :, :, xlo]) * dx
    out = rows[:, :, ylo, :] + (rows[:, :, yhi, :] - rows[:, :, ylo, :]) * dy[:, None]
    return (out - 128.0) / 128.0
