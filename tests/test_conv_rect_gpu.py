"""da_conv2d_relu_fwd (csrc/conv_rect.hip) at its edges against float64, in the idiom of tests/test_gemm_edges_gpu.py.

Reference (tests/conv_rect_reference.py, which also holds the case tables and the bound; tests/test_fid_host.py checks the
gather against F.conv2d and the tables against what is claimed here): float64 on the bf16-rounded operands through an
explicit gather (row m = (b, oh, ow), column (i, j, c) reads X[b, oh s - ph + i, ow s - pw + j, c] or zero), then one matrix
product, + bias, ReLU.

Exact cases (FORMS x Cin in {8, 48, 80, 160, 448}; Cout in {32, 80, 192, 448}, B in {1, 3}, ReLU and the forced column
tile rotate over the cases): integer inputs, weights and bias with |.| <= 8 and K <= 4032 (5x5 at Cin 448 is the one
combination left out: K = 11200), so every fp32 partial sum is an exact integer below 2^24 and the bf16 output must be
torch.equal to the float64 result rounded once.  Forms: 3x3 stride 2 without padding at odd and even sizes, 3x3, 3x3 p1,
1x1, 5x5 p2, 1x7 p(0,3), 7x1 p(3,0), 1x3 p(0,1), 3x1 p(1,0); every padded form also at a size smaller than its reach; H != W
throughout.  TILE_CASES: each column tile (32 / 64 / 96) forced with Cout below, at and past its width at M = 3 x 128 + 45
rows over 3 images (a row tile spans images, M has a tail).  The largest case is 50624 rows x 448 columns.
Memory, every case: the output is a NaN-prefilled column view with sentinel columns on both sides and 384 sentinel rows
after (bit-identical afterwards); X is a column view with NaN pad columns and NaN trailing rows; W and the bias are slices
between NaN neighbours; a repeated call gives identical bits.
Float cases: N(0,1) inputs, rows scaled from 1e-3 to 1e3, and a near-cancelling set; every element
    |out - ref| <= ulp_bf16(ref) + c2 * 2^-24 * K * (|X| |W|^T + |bias|)[m, n]
with c2 at most 2x the worst value measured on an MI355X (BOUNDS); DA_PARITY_MARGINS=<path> writes
the margins of a run (tests/parity_margins.py).
"""
import os

import pytest
import torch

import parity_margins
from conv_rect_reference import (BOUNDS, EXACT_CASES, F64, LARGE_CASE, TILE_CASES, out_size, reference,  # noqa: F401
                                 ulp_bf16)

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN = float('nan')
PAD_L, PAD_R, PAD_ROWS = 8, 8, 384

_WORST = {}


@pytest.fixture(scope='module')
def ops(dev):
    from diffusion_amd import ops as o
    return o


def gen(seed, dev):
    return torch.Generator(device=dev).manual_seed(seed)


def ints(*shape, seed, dev):
    return torch.randint(-8, 9, shape, generator=gen(seed, dev), device=dev).float()


def in_view(t):
    rows, C = t.shape
    buf = torch.full((rows + 8, PAD_L + C + PAD_R), NAN, device=t.device, dtype=BF)
    buf[:rows, PAD_L:PAD_L + C] = t.to(BF)
    return buf[:rows, PAD_L:PAD_L + C]


def row_slice(t, pad=8):
    buf = torch.full((t.shape[0] + 2 * pad, t.shape[1]), NAN, device=t.device, dtype=t.dtype)
    buf[pad:pad + t.shape[0]] = t
    return buf[pad:pad + t.shape[0]]


def vec_slice(t, pad=16):
    buf = torch.full((t.numel() + 2 * pad,), NAN, device=t.device, dtype=t.dtype)
    buf[pad:pad + t.numel()] = t
    return buf[pad:pad + t.numel()]


def out_view(rows, C, dev, seed):
    buf = torch.randn(rows + PAD_ROWS, PAD_L + C + PAD_R, generator=gen(seed, dev), device=dev).to(BF)
    view = buf[:rows, PAD_L:PAD_L + C]
    view.fill_(NAN)
    return buf, view, buf.clone()


def assert_pads_kept(buf, ref_buf, rows, C, what):
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    keep[:rows, PAD_L:PAD_L + C] = False
    assert torch.equal(buf[keep].view(torch.int16), ref_buf[keep].view(torch.int16)), f'{what}: sentinels changed'


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def first_mismatch(out, ref):
    bad = (out.double() != ref.double()) | torch.isnan(out.double())
    if not bool(bad.any()):
        return ''
    m, n = [int(v) for v in bad.nonzero()[0]]
    return f'{int(bad.sum())} of {bad.numel()} elements differ, first at ({m}, {n}): {out[m, n].item()} vs {ref[m, n].item()}'


def run(ops, X, Wt, bias, geo, Cout, relu, tile_n, dev, seed, what):
    """the launch on sentinel-guarded views, twice; returns the output view"""
    B, H, W, kh, kw, s, ph, pw = geo
    Ho, Wo = out_size(H, W, kh, kw, s, ph, pw)
    M = B * Ho * Wo
    buf, o, keep = out_view(M, Cout, dev, seed)
    xv, wv, bv = in_view(X), row_slice(Wt.to(BF)), (vec_slice(bias) if bias is not None else None)
    ops.conv2d_relu_fwd(xv, wv, bv, o, B, H, W, kh, kw, s, ph, pw, relu=relu, tile_n=tile_n)
    torch.cuda.synchronize()
    assert_pads_kept(buf, keep, M, Cout, what)
    first = o.clone()
    o.fill_(NAN)
    ops.conv2d_relu_fwd(xv, wv, bv, o, B, H, W, kh, kw, s, ph, pw, relu=relu, tile_n=tile_n)
    torch.cuda.synchronize()
    assert bits_equal(first, o), f'{what}: a repeated call changed bits'
    return o


@pytest.mark.parametrize('case', EXACT_CASES + TILE_CASES + LARGE_CASE, ids=[c[0] for c in EXACT_CASES + TILE_CASES + LARGE_CASE])
def test_conv_rect_exact(ops, dev, case):
    cid, geo, Cin, Cout, relu, tile = case
    B, H, W, kh, kw, s, ph, pw = geo
    seed = sum(map(ord, cid)) % 10007
    X = ints(B * H * W, Cin, seed=seed, dev=dev)
    Wt = ints(Cout, kh * kw * Cin, seed=seed + 1, dev=dev)
    bias = ints(Cout, seed=seed + 2, dev=dev)
    ref, _ = reference(X, Wt, bias, geo, relu)
    assert ref.abs().max().item() < 2 ** 24
    o = run(ops, X, Wt, bias, geo, Cout, relu, tile, dev, seed + 10, cid)
    want = ref.to(F32).to(BF)   # the integers are exact in fp32: one rounding
    assert torch.equal(o, want), f'{cid}: {first_mismatch(o, want)}'
    if tile:   # the table's own tile gives the same bits
        o2 = run(ops, X, Wt, bias, geo, Cout, relu, 0, dev, seed + 11, cid)
        assert bits_equal(o, o2)


def test_conv_rect_no_bias_and_tile_table(ops, dev):
    geo = (2, 5, 7, 1, 3, 1, 0, 1)
    X, Wt = ints(2 * 5 * 7, 48, seed=1, dev=dev), ints(80, 3 * 48, seed=2, dev=dev)
    ref, _ = reference(X, Wt, None, geo, False)
    o = run(ops, X, Wt, None, geo, 80, False, 0, dev, 3, 'no-bias')
    assert torch.equal(o, ref.to(F32).to(BF))
    assert [ops.conv2d_tile_for(n) for n in (32, 64, 96, 192, 384)] == [32, 64, 96, 96, 96]
    assert all(ops.conv2d_tile_for(n) in (32, 64, 96) for n in range(8, 456, 8)) and ops.conv2d_tile_for(12) == 0


def test_conv_rect_rejects_before_launch(ops, dev):
    X, Wt = in_view(ints(2 * 5 * 7, 16, seed=1, dev=dev)), ints(16, 9 * 16, seed=2, dev=dev).to(BF)
    Y = torch.full((2 * 3 * 5, 16), NAN, device=dev, dtype=BF)
    from diffusion_amd import _lib
    st = torch.cuda.current_stream().cuda_stream

    def rc(Hout=3, Wout=5, kh=3, kw=3, s=1, ph=0, pw=0, Cin=16, Cout=16, ldy=16, tile=0):
        return _lib.load().da_conv2d_relu_fwd(X.data_ptr(), X.stride(0), Wt.data_ptr(), None, Y.data_ptr(), ldy, 2, 5, 7, Hout,
                                              Wout, Cin, Cout, kh, kw, s, ph, pw, 1, tile, st)
    assert rc() == 0
    for kw_ in (dict(Hout=4), dict(Wout=4), dict(kh=8), dict(kw=0), dict(s=3), dict(ph=4), dict(pw=-1), dict(Cin=12), dict(Cout=12),
                dict(ldy=8), dict(tile=48), dict(kh=7, Hout=1)):
        Y.fill_(NAN)
        assert rc(**kw_) == 1, kw_
        torch.cuda.synchronize()
        assert bool(torch.isnan(Y).all()), kw_


# ------------------------------------------------------------------------------------------------ float cases
def float_operands(kind, rows, C, seed, dev):
    x = torch.randn(rows, C, generator=gen(seed, dev), device=dev)
    if kind == 'rows':
        x = x * torch.pow(10.0, torch.rand(rows, 1, generator=gen(seed + 1, dev), device=dev) * 6 - 3)
    if kind == 'cancel':
        x[:, C // 2:] = x[:, :C // 2]
    return x.to(BF).float()


def cancel_w(Wt, taps, Cin, seed, dev):
    w = Wt.view(Wt.shape[0], taps, Cin).clone()
    h = Cin // 2
    w[:, :, h:] = -w[:, :, :h] + torch.randn(w[:, :, :h].shape, generator=gen(seed, dev), device=dev) * 2 ** -8
    return w.reshape(Wt.shape).to(BF).float()


FLOAT_FORMS = [('3x3s2-c8', (3, 19, 23, 3, 3, 2, 0, 0), 8, 32), ('1x7-c160', (2, 17, 13, 1, 7, 1, 0, 3), 160, 192),
               ('7x1-c80', (2, 13, 17, 7, 1, 1, 3, 0), 80, 80), ('5x5-c48', (2, 12, 15, 5, 5, 1, 2, 2), 48, 64),
               ('3x3p1-c32', (2, 40, 41, 3, 3, 1, 1, 1), 32, 64), ('1x1-c64', (2, 30, 31, 1, 1, 1, 0, 0), 64, 80),
               ('3x3p1-c448', (1, 8, 9, 3, 3, 1, 1, 1), 448, 384), ('1x1-c2048', (1, 8, 9, 1, 1, 1, 0, 0), 2048, 320)]
FLOAT_CASES = [(f'{f[0]}-{kind}', f, kind) for f in FLOAT_FORMS for kind in ('randn', 'rows', 'cancel')]


@pytest.mark.parametrize('case', FLOAT_CASES, ids=[c[0] for c in FLOAT_CASES])
def test_conv_rect_float_bounds(ops, dev, case):
    cid, (_, geo, Cin, Cout), kind = case
    B, H, W, kh, kw, s, ph, pw = geo
    K = kh * kw * Cin
    seed = sum(map(ord, cid)) % 10007
    X = float_operands(kind, B * H * W, Cin, seed, dev)
    Wt = torch.randn(Cout, K, generator=gen(seed + 2, dev), device=dev).mul(K ** -0.5).to(BF).float()
    if kind == 'cancel':
        Wt = cancel_w(Wt, kh * kw, Cin, seed + 3, dev)
    bias = torch.randn(Cout, generator=gen(seed + 4, dev), device=dev) / 8
    relu = kind != 'cancel'
    ref, absprod = reference(X, Wt, bias, geo, relu)
    o = run(ops, X, Wt, bias, geo, Cout, relu, 0, dev, seed + 10, cid)
    err = (o.double() - ref).abs()
    assert bool(torch.isfinite(err).all()), f'{cid}: non-finite output'
    c2 = ((err - ulp_bf16(ref)).clamp(min=0) / (2.0 ** -24 * K * absprod).clamp(min=1e-300)).max().item()
    name = f'{kind}.c2'
    _WORST[name] = max(_WORST.get(name, 0.0), c2)
    print(f'{cid}: c2 {c2:.3e} (bound {BOUNDS[name]:.3e})')
    if os.environ.get('DA_PARITY_MARGINS'):
        parity_margins.record('conv_rect', tolerances=BOUNDS, **_WORST)
    assert c2 <= BOUNDS[name], f'{cid}: c2 {c2:.3e} > bound {BOUNDS[name]:.3e}'
