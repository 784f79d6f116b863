"""da_pool2d_fwd, da_avgpool_global_f32 and da_inception_preprocess (csrc/inception.hip) against their references.

Pools: integer inputs; the maximum must be bit-equal to torch's fp32 CPU ``max_pool2d`` and the average to torch's fp32 CPU
``avg_pool2d(count_include_pad=False)`` rounded once to bf16 (the kernel DIVIDES the fp32 sum by the count, as the header
says, so the reference is torch's own division).  Forms 3/s2/p0 at 7x9 and 8x8, 3/s1/p1 at 1x1, 2x5 and 8x8; C in {8, 288};
input and output are column views of wider buffers with NaN / sentinel surroundings.
Global average: integer inputs; fp32 division of an exact integer sum by HW is correctly rounded, i.e. equals the float64
quotient rounded to fp32 (a quotient of two fp32 values survives the double rounding: 53 >= 2 * 24 + 2).
Preprocess: the reference is tests/inception_reference.py's float64 restatement.  At 299 x 299 and 598 x 598 every source
coordinate is an integer, (v - 128) / 128 has 8 significant bits and the output must be bit-equal.  At 64x96, 150x150 and
512x512, uint8 and float: the kernel's value on the 0..255 scale carries at most 10 fp32 roundings of 2^-17 each (values
below 256: two lerps along x of a multiply and an add each, the difference of the rows, the lerp along y, the subtraction of
128; the source coordinate and its fraction are exact), i.e. 10 * 2^-24 after the exact division by 128, so the bf16 output
must lie between the float64 reference -/+ that allowance, each rounded once to bf16.  Float inputs are (k + 0.5) / 255, so
floor(255 x) = k whatever the rounding of the product."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_reference as IR

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN = float('nan')
PAD = 8


@pytest.fixture(scope='module')
def ops(dev):
    from diffusion_amd import ops as o
    return o


def in_view(t, dev):
    rows, C = t.shape
    buf = torch.full((rows + 8, PAD + C + PAD), NAN, device=dev, dtype=BF)
    buf[:rows, PAD:PAD + C] = t.to(dev, BF)
    return buf[:rows, PAD:PAD + C]


def out_view(rows, C, dev, seed, dtype=BF):
    g = torch.Generator(device=dev).manual_seed(seed)
    buf = torch.randn(rows + 64, PAD + C + PAD, generator=g, device=dev).to(dtype)
    view = buf[:rows, PAD:PAD + C]
    view.fill_(NAN)
    return buf, view, buf.clone()


def pads_kept(buf, keep, rows, C):
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    mask[:rows, PAD:PAD + C] = False
    it = torch.int16 if buf.dtype == BF else torch.int32
    return torch.equal(buf[mask].view(it), keep[mask].view(it))


POOL_FORMS = [(2, 0, 7, 9), (2, 0, 8, 8), (1, 1, 1, 1), (1, 1, 2, 5), (1, 1, 8, 8)]


@pytest.mark.parametrize('kind', [0, 1], ids=['max', 'avg'])
@pytest.mark.parametrize('C', [8, 288])
@pytest.mark.parametrize('form', POOL_FORMS, ids=[f's{s}p{p}-{h}x{w}' for s, p, h, w in POOL_FORMS])
def test_pool_bit_exact(ops, dev, form, C, kind):
    s, p, H, W = form
    B = 3
    g = torch.Generator().manual_seed(H * 100 + W * 10 + C + kind)
    x = torch.randint(-8, 9, (B, C, H, W), generator=g).float()
    if kind == 0:
        ref = F.max_pool2d(x, 3, stride=s, padding=p)
    else:
        ref = F.avg_pool2d(x, 3, stride=s, padding=p, count_include_pad=False)
    Ho, Wo = ref.shape[2:]
    want = ref.permute(0, 2, 3, 1).reshape(B * Ho * Wo, C).to(BF)
    X = in_view(x.permute(0, 2, 3, 1).reshape(B * H * W, C), dev)
    buf, Y, keep = out_view(B * Ho * Wo, C, dev, 5)
    assert ops.pool2d_fwd(X, Y, B, H, W, s, p, kind) == (Ho, Wo)
    torch.cuda.synchronize()
    assert pads_kept(buf, keep, B * Ho * Wo, C)
    assert torch.equal(Y.cpu(), want), (Y.cpu().float() - want.float()).abs().max()


def test_pool_rejects_before_launch(ops, dev):
    X = torch.zeros(2 * 2 * 5, 8, device=dev, dtype=BF)
    Y = torch.full((2 * 2 * 5, 8), NAN, device=dev, dtype=BF)
    with pytest.raises(ValueError):
        ops.pool2d_fwd(X, Y, 2, 2, 5, 1, 0, 0)   # no window fits 2 x 5 without padding
    from diffusion_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    for Hout, Wout, s, p, kind in ((2, 4, 1, 1, 0), (2, 5, 3, 1, 0), (2, 5, 1, 2, 0), (2, 5, 1, 1, 2)):
        assert _lib.load().da_pool2d_fwd(X.data_ptr(), 8, Y.data_ptr(), 8, 2, 2, 5, Hout, Wout, 8, s, p, kind, st) == 1
    torch.cuda.synchronize()
    assert bool(torch.isnan(Y).all())


@pytest.mark.parametrize('HW', [64, 35, 1])
@pytest.mark.parametrize('C', [8, 2048])
def test_global_average_exact(ops, dev, HW, C):
    B = 3
    g = torch.Generator().manual_seed(HW + C)
    x = torch.randint(-8, 9, (B * HW, C), generator=g).float()
    want = torch.from_numpy((x.double().view(B, HW, C).sum(1).numpy() / HW).astype(np.float32))
    buf, out, keep = out_view(B, C, dev, 9, dtype=F32)
    ops.avgpool_global_f32(in_view(x, dev), out, B, HW)
    torch.cuda.synchronize()
    assert pads_kept(buf, keep, B, C)
    assert torch.equal(out.cpu(), want)


# ------------------------------------------------------------------------------------------------ preprocess
def rne_bf16(x):
    """float64 -> the nearest bf16 value (8 significant bits, ties to even), as float64"""
    m, e = np.frexp(np.asarray(x, np.float64))
    return np.ldexp(np.rint(m * 256.0), e - 8)


def _levels(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, 3, H, W), dtype=np.uint8)


def _run(ops, dev, images):
    B = images.shape[0]
    out = torch.full((B * 299 * 299 + 16, 8), NAN, device=dev, dtype=BF)
    view = out[:B * 299 * 299]
    ops.inception_preprocess(images.to(dev), view)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[B * 299 * 299:]).all())
    got = view.float().cpu().numpy().astype(np.float64).reshape(B, 299, 299, 8)
    assert np.array_equal(got[..., 3:], np.zeros_like(got[..., 3:])) and not np.signbit(got[..., 3:]).any()
    return got[..., :3].transpose(0, 3, 1, 2)


@pytest.mark.parametrize('side', [299, 598])
@pytest.mark.parametrize('as_float', [False, True], ids=['uint8', 'float'])
def test_preprocess_integer_coordinates_bit_equal(ops, dev, side, as_float):
    lv = _levels(2, side, side, side)
    images = torch.from_numpy((lv.astype(np.float32) + np.float32(0.5)) / np.float32(255.0)) if as_float else torch.from_numpy(lv)
    if as_float:
        assert np.array_equal(IR.levels_of_float(images.numpy()), lv.astype(np.float64))
    ref = IR.preprocess_f64(lv)
    assert np.array_equal(ref, (lv[:, :, ::side // 299, ::side // 299].astype(np.float64) - 128) / 128)
    assert np.array_equal(_run(ops, dev, images), ref)


ALLOW = 10 * 2.0 ** -24


@pytest.mark.parametrize('size', [(1, 64, 96), (1, 150, 150), (2, 512, 512), (1, 301, 7)], ids=lambda s: f'b{s[0]}-{s[1]}x{s[2]}')
@pytest.mark.parametrize('as_float', [False, True], ids=['uint8', 'float'])
def test_preprocess_resize_within_one_rounding(ops, dev, size, as_float):
    B, H, W = size
    lv = _levels(B, H, W, H * 7 + W)
    images = torch.from_numpy((lv.astype(np.float32) + np.float32(0.5)) / np.float32(255.0)) if as_float else torch.from_numpy(lv)
    if as_float:
        assert np.array_equal(IR.levels_of_float(images.numpy()), lv.astype(np.float64))
    ref = IR.preprocess_f64(lv)
    got = _run(ops, dev, images)
    lo, hi = rne_bf16(ref - ALLOW), rne_bf16(ref + ALLOW)
    bad = (got < lo) | (got > hi)
    print(f'{size} float={as_float}: max |got - ref| {np.abs(got - ref).max():.3e}, outside one rounding: {int(bad.sum())}')
    assert not bad.any(), (int(bad.sum()), np.abs(got - ref)[bad].max())


def test_preprocess_float_clamps_and_floors(ops, dev):
    """floor(clamp(255 x, 0, 255)): values outside [0, 1] clamp; 299 x 299 keeps the levels, so the output shows them"""
    x = torch.full((1, 3, 299, 299), 0.5)
    x[0, 0, 0, :4] = torch.tensor([-0.3, 1.7, 0.999, 1.0])
    got = _run(ops, dev, x)
    want = (np.array([0.0, 255.0, 254.0, 255.0]) - 128) / 128
    assert np.array_equal(got[0, 0, 0, :4], rne_bf16(want))
    assert np.array_equal(got[0, 1], np.full((299, 299), rne_bf16((127.0 - 128) / 128)))


def test_preprocess_rejects(ops, dev):
    out = torch.empty(299 * 299, 8, device=dev, dtype=BF)
    for bad in (torch.zeros(1, 4, 8, 8, dtype=torch.uint8), torch.zeros(1, 3, 8, 8, dtype=torch.int32),
                torch.zeros(3, 8, 8, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            ops.inception_preprocess(bad.to(dev), out)
    with pytest.raises(ValueError):
        ops.inception_preprocess(torch.zeros(2, 3, 8, 8, dtype=torch.uint8, device=dev), out)
