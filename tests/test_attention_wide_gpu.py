"""da_attn_fwd_wide (attention_wide.hip, head_dim 512: the VAE's mid-block head) at its edges against a float64 reference.

Reference: softmax attention in float64 on the same bf16-rounded inputs, scale = 512**-0.5, logsumexp / ln 2 for L2.
Checks, bounds and buffer discipline are those of tests/test_attention_edges_gpu.py: output rel-L2 < FWD_TOL over the whole
tensor and < 2 FWD_TOL in every (image, head) slice, L2 within 2e-3 absolute, outputs NaN-filled first and finite afterwards,
O a column view inside a wider buffer whose sentinel columns / rows stay bit-unchanged, a second call torch.equal.
A CPU emulation of the flash numerics at d = 512 (bf16 inputs, 32-key blocks, P and O rounded to bf16) gives
2.1e-3 ... 2.7e-3 rel-L2 and <= 6e-4 on L2 for these inputs, so the bounds leave ~2x room.
"""
import math

import pytest
import torch

from test_attention_edges_gpu import FWD_TOL, check_l2, check_sentinels, out_view, randn, rel_l2

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
D = 512
SCALE = D**-0.5


@pytest.fixture(scope='module')
def ops(dev):
    from diffusion_amd import ops as o
    return o


def make_inputs(B, H, Nq, Nk, dev, seed, kind='normal'):
    """q [B*Nq, H*512], k, v [B*Nk, H*512] in bf16.
    'shift':    coordinate 0 = +64 in every q row, -64 in every k row of image 0 and +64 in every k row of image 1: exact in
                bf16, scores ~ -+4096 scale, L2 ~ -+260.
    'dominant': coordinate 1 = 32 in every q row, 0 in every key but 14 in the LAST one (in the partial 32-key block): that
                key's logit is 32 * 14 * 512**-0.5 = 19.8 nats above the rest in every row."""
    q = randn(B, Nq, H, D, seed=seed, dev=dev)
    k = randn(B, Nk, H, D, seed=seed + 1, dev=dev)
    v = randn(B, Nk, H, D, seed=seed + 2, dev=dev)
    if kind == 'shift':
        assert B == 2
        q[..., 0] = 64.0
        k[0, ..., 0], k[1, ..., 0] = -64.0, 64.0
    elif kind == 'dominant':
        q[..., 1] = 32.0
        k[..., 1] = 0.0
        k[:, Nk - 1, :, 1] = 14.0
    f = lambda t, n: t.reshape(B * n, H * D).to(BF).contiguous()
    return f(q, Nq), f(k, Nk), f(v, Nk)


def reference(q, k, v, B, H, Nq, Nk):
    """float64 attention on the bf16 inputs -> O [B, Nq, H, 512], L2 [B, H, Nq]"""
    sp = lambda t, n: t.double().reshape(B, n, H, D).permute(0, 2, 1, 3)
    s = sp(q, Nq) @ sp(k, Nk).transpose(-1, -2) * SCALE
    return (torch.softmax(s, -1) @ sp(v, Nk)).permute(0, 2, 1, 3), torch.logsumexp(s, -1) / math.log(2.0)


def check(got, ref, what, B, H):
    """got [B*N, H*512] (bf16 view), ref [B, N, H, 512]: finite, rel-L2 < FWD_TOL whole, < 2 FWD_TOL per (image, head)"""
    g = got.double().reshape(ref.shape)
    bad = ~torch.isfinite(g)
    assert not bad.any(), (f'{what}: {int(bad.sum())} non-finite values, first in (image, row, head) '
                           f'{tuple(bad.nonzero()[0, :3].tolist())}')
    e = rel_l2(g, ref)
    d = (g - ref).permute(0, 2, 1, 3).reshape(B * H, -1).norm(dim=1)
    n = ref.permute(0, 2, 1, 3).reshape(B * H, -1).norm(dim=1)
    worst = (d / n).max().item()
    print(f'{what}: rel-L2 {e:.3e}, worst (image, head) slice {worst:.3e}')
    assert e < FWD_TOL, f'{what}: rel-L2 {e:.3e} >= {FWD_TOL}'
    assert worst < 2 * FWD_TOL, f'{what}: worst (image, head) slice rel-L2 {worst:.3e} >= {2 * FWD_TOL}'


def run(ops, q, k, v, B, H, Nq, Nk):
    C = H * D
    buf, O, before = out_view(B * Nq, C, q.device, seed=99)
    L2 = torch.full((B * H * Nq,), float('nan'), device=q.device)
    ops.attn_fwd_wide(q, k, v, O, L2, B, H, D, Nq, Nk, SCALE)
    torch.cuda.synchronize()
    check_sentinels(buf, before, B * Nq, C, 'O')
    return O, L2


CASES = [pytest.param(1, 1, 1, 1, 'normal', id='1x1'),                  # smallest possible shape
         pytest.param(2, 1, 64, 64, 'normal', id='8x8-latent'),
         pytest.param(1, 2, 100, 77, 'normal', id='ragged-2-heads'),    # both dimensions ragged; head 1 at column offset 512
         pytest.param(2, 1, 33, 200, 'normal', id='short-query-tile'),
         pytest.param(1, 1, 1024, 1024, 'normal', id='256px'),
         pytest.param(2, 1, 33, 200, 'shift', id='shift'),
         pytest.param(1, 1, 256, 250, 'dominant', id='dominant-last-key')]


@pytest.mark.parametrize('B,H,Nq,Nk,kind', CASES)
def test_attention_wide_forward(ops, dev, B, H, Nq, Nk, kind):
    q, k, v = make_inputs(B, H, Nq, Nk, dev, seed=Nq * 1000 + Nk, kind=kind)
    ref_o, ref_l2 = reference(q, k, v, B, H, Nq, Nk)
    if kind == 'shift':   # the case is as hostile as stated
        assert ref_l2[0].max() < -250 and ref_l2[1].min() > 250
    O, L2 = run(ops, q, k, v, B, H, Nq, Nk)
    check(O, ref_o, f'{kind} O', B, H)
    print(f'{kind} L2: max |err| {(L2.double().reshape(ref_l2.shape) - ref_l2).abs().max().item():.3e}')
    check_l2(L2, ref_l2, f'{kind} L2')
    O2, L22 = run(ops, q, k, v, B, H, Nq, Nk)
    assert torch.equal(O, O2) and torch.equal(L2, L22), 'two identical calls differ'


def test_attention_wide_strided_qkv_slices(ops, dev):
    """the VAE call: q | k | v are column slices of one fused [B*N, 3*512] buffer, passed as strided views"""
    B, N = 2, 70
    q, k, v = make_inputs(B, 1, N, N, dev, seed=5)
    qkv = torch.cat([q, k, v], dim=1).contiguous()
    ref_o, ref_l2 = reference(q, k, v, B, 1, N, N)
    O, L2 = run(ops, qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B, 1, N, N)
    check(O, ref_o, 'strided O', B, 1)
    check_l2(L2, ref_l2, 'strided L2')


def test_attention_wide_rejects_what_it_cannot_run(dev):
    """DA_ERR_SHAPE, nothing launched, outputs bit-unchanged: any D but 512, a row stride that is no multiple of 8, no keys"""
    from diffusion_amd import _lib
    lib = _lib.load()
    B, H, Nq, Nk = 1, 1, 40, 40
    q, k, v = make_inputs(B, H, Nq, Nk, dev, seed=1)
    O = randn(B * Nq, D, seed=2, dev=dev).to(BF)
    L2 = randn(B * H * Nq, seed=3, dev=dev)
    O0, L20 = O.clone(), L2.clone()
    st = torch.cuda.current_stream().cuda_stream

    def call(D_=D, ldq=D, Nk_=Nk):
        rc = lib.da_attn_fwd_wide(q.data_ptr(), ldq, k.data_ptr(), D, v.data_ptr(), D, O.data_ptr(), D, L2.data_ptr(), B, H,
                                  D_, Nq, Nk_, SCALE, st)
        torch.cuda.synchronize()
        return rc

    for kw in ({'D_': 64}, {'D_': 256}, {'ldq': 516}, {'Nk_': 0}):
        assert call(**kw) == 1, kw
        assert torch.equal(O.view(torch.int16), O0.view(torch.int16)) and torch.equal(L2, L20), kw
    assert call() == 0   # and the same buffers are accepted as they are
    assert not torch.equal(O, O0)
