"""Attention at its edges: every backward form (attention.hip) against a float64 reference, at the shapes, tails and
inputs where flash kernels go wrong, and the forms against each other.

Backward forms, forced with da_set_option('attn_fused_bwd', v) (da_attn_bwd's dispatch):

    v | Nk <= 128, Nq >= 64 | Nk 129...256, Nq >= 64 | otherwise
    0 | dQ + dK/dV<32|64>   | pair                   | pair
    1 | fused<4> (default)  | pair                   | pair
    2 | fused<4>            | fused<8>               | pair

Reference: softmax attention in float64 on the same bf16-rounded inputs, autograd for dQ / dK / dV, logsumexp / ln 2
for L2.  Every case asserts, for every form it runs:
  * all outputs finite (O, L2, dQ, dK, dV, Delta) - the outputs are NaN-filled first, so this also proves that every row
    below B*N was written (a ragged last tile that is never stored stays NaN);
  * rel-L2 against the reference under the suite's bounds (6e-3 forward, 1.2e-2 backward) over the whole tensor AND under
    twice that in every (image, head) slice (a wrong head or tile must not hide in a whole-tensor norm, as check_blocks in
    test_bench_shapes_gpu.py); L2 within 2e-3 absolute, Delta = rowsum(dO * O) of the O it was given;
  * the outputs are column views inside wider buffers with 8 sentinel columns (16 bytes) on each side and 8 sentinel rows
    after: the sentinels are bit-unchanged;
  * a second call gives torch.equal outputs (fixed-order reductions, README);
and where two forms run the same shape: dK, dV and Delta torch.equal, dQ within DQ_XFORM_TOL (attention row).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
FWD_TOL, BWD_TOL, L2_TOL = 6e-3, 1.2e-2, 2e-3
# dQ of the one-kernel forms against the pair: the fused kernel sums dS . K over all keys of a 32-query tile with 16x16x32
# MFMAs, the dQ kernel over 64-key steps with 32x32x16 MFMAs - the same products in another fp32 order, so a few elements
# round to the neighbouring bf16 value.  rel-L2 over the whole tensor: 1.2e-5 ... 1.6e-5 at the bench shapes,
# where ~1e6 elements average the flips out; worst 9.0e-5 over the small shapes here (2 x 3 x 65 x 128), where one flipped
# element alone is ~3e-5.
DQ_XFORM_TOL = 1.8e-4
PAD_C, PAD_R = 8, 8


@pytest.fixture(scope='module')
def ops(dev):
    from diffusion_amd import ops as o
    return o


def path(form, Nq, Nk):
    """the kernels da_attn_bwd runs under attn_fused_bwd = form"""
    if form >= 1 and Nk <= 128 and Nq >= 64:
        return 'fused4'
    if form >= 2 and Nk <= 256 and Nq >= 64:
        return 'fused8'
    return 'pair'


def distinct_forms(Nq, Nk):
    """one option value per distinct backward path at this shape: {path: form}"""
    out = {}
    for f in (0, 1, 2):
        out.setdefault(path(f, Nq, Nk), f)
    return out


# ------------------------------------------------------------------------------------------------ inputs, reference
def randn(*shape, seed, dev, scale=1.0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def make_inputs(B, H, Nq, Nk, dev, seed, kind='normal'):
    """q [B*Nq, H*64], k, v [B*Nk, H*64], do [B*Nq, H*64] in bf16 (do = None for 'big_delta': it needs O first).
    'shift':    head 1: coordinate 0 = +32 in every q row, -32 in every k row (scores ~ -1024 + q'.k', L2 ~ -180 at scale
                0.125); head 2: +32 / +32 (L2 ~ +190); head 0 ordinary.  Exact in bf16; the softmax is shift-invariant.
    'dominant': coordinate 1 = 16 in every q row and 10 in the LAST key (the last, partial 32-key block), 0 in the other
                keys: that key's logit is 16 * 10 * 0.125 = 20 nats above the rest in every row.
    'dominant2': the same for the last TWO keys: two keys share each row's softmax, the rest are ~e^-20 of it."""
    C = H * 64
    q = randn(B, Nq, H, 64, seed=seed, dev=dev)
    k = randn(B, Nk, H, 64, seed=seed + 1, dev=dev)
    v = randn(B, Nk, H, 64, seed=seed + 2, dev=dev)
    do = randn(B, Nq, H, 64, seed=seed + 3, dev=dev)
    if kind == 'shift':
        assert H >= 3
        q[:, :, 1, 0], k[:, :, 1, 0] = 32.0, -32.0
        q[:, :, 2, 0], k[:, :, 2, 0] = 32.0, 32.0
    elif kind in ('dominant', 'dominant2'):
        q[:, :, :, 1] = 16.0
        k[:, :, :, 1] = 0.0
        k[:, Nk - (1 if kind == 'dominant' else 2):, :, 1] = 10.0
    f = lambda t, n: t.reshape(B * n, C).to(BF).contiguous()
    return f(q, Nq), f(k, Nk), f(v, Nk), (None if kind == 'big_delta' else f(do, Nq))


def reference(q, k, v, do, B, H, Nq, Nk, scale, causal=False):
    """float64 attention on the bf16 inputs -> O, L2 [B, H, Nq] and (with do) dQ, dK, dV, all [B, N, H, 64]"""
    sp = lambda t, n: t.double().reshape(B, n, H, 64).permute(0, 2, 1, 3).contiguous()
    back = lambda t: t.detach().permute(0, 2, 1, 3)
    qd, kd, vd = sp(q, Nq).requires_grad_(), sp(k, Nk).requires_grad_(), sp(v, Nk).requires_grad_()
    s = qd @ kd.transpose(-1, -2) * scale
    if causal:
        s = s.masked_fill(torch.ones(Nq, Nk, dtype=torch.bool, device=s.device).triu(1), float('-inf'))
    lse = torch.logsumexp(s, -1)
    o = torch.softmax(s, -1) @ vd
    L2 = lse.detach() / math.log(2.0)
    if do is None:
        return back(o), L2
    (o * sp(do, Nq)).sum().backward()
    return back(o), L2, back(qd.grad), back(kd.grad), back(vd.grad)


# ------------------------------------------------------------------------------------------------ checks
def rel_l2(a, r):
    return ((a.double() - r.double()).norm() / r.double().norm()).item()


def check(got, ref, tol, what, B, H):
    """got [B*N, H*64] (bf16 view), ref [B, N, H, 64]: finite, rel-L2 < tol whole, < 2 tol per (image, head) slice"""
    g = got.double().reshape(ref.shape)
    bad = ~torch.isfinite(g)
    assert not bad.any(), (f'{what}: {int(bad.sum())} non-finite values, first in (image, row, head) '
                           f'{tuple(bad.nonzero()[0, :3].tolist())}')
    e = rel_l2(g, ref)
    assert e < tol, f'{what}: rel-L2 {e:.3e} >= {tol}'
    d = (g - ref.double()).permute(0, 2, 1, 3).reshape(B * H, -1).norm(dim=1)
    n = ref.double().permute(0, 2, 1, 3).reshape(B * H, -1).norm(dim=1)
    worst = (d / n).max().item()
    assert worst < 2 * tol, f'{what}: worst (image, head) slice rel-L2 {worst:.3e} >= {2 * tol}'


def check_vanishing(got, what, bound=1e-3):
    """dQ / dK where one key takes a row's whole softmax: 0 with a single key (the softmax is constant), ~1e-8 with one
    key 20 nats above the rest.  A rel-L2 against that is not a test of the kernel: dS = P (dP - delta) is then the
    difference of two equal 64-term fp32 sums (dO . v and dO . O with O = v), and every form leaves their rounding, ~1e-6,
    where the exact value is 1e-8.  Bound: 100x below an ordinary dQ / dK element."""
    g = got.double()
    assert torch.isfinite(g).all(), f'{what}: non-finite values'
    assert g.abs().max().item() < bound, f'{what}: max |x| {g.abs().max().item():.3e} where the exact value is 0'


def check_l2(L2, ref, what):
    g = L2.double().reshape(ref.shape)
    assert torch.isfinite(g).all(), f'{what}: non-finite L2'
    err = (g - ref).abs().max().item()
    assert err < L2_TOL, f'{what}: max |L2 - ref| {err:.3e} >= {L2_TOL}'


def out_view(rows, C, dev, seed):
    """a NaN-filled [rows, C] bf16 column view inside a buffer with PAD_C sentinel columns on each side (16 bytes) and
    PAD_R sentinel rows after; returns (buffer, view, copy of the buffer)"""
    buf = randn(rows + PAD_R, C + 2 * PAD_C, seed=seed, dev=dev).to(BF)
    view = buf[:rows, PAD_C:PAD_C + C]
    view.fill_(float('nan'))
    return buf, view, buf.clone()


def check_sentinels(buf, before, rows, C, what):
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    keep[:rows, PAD_C:PAD_C + C] = False
    assert torch.equal(buf.view(torch.int16)[keep], before.view(torch.int16)[keep]), f'{what}: wrote outside its view'


# ------------------------------------------------------------------------------------------------ kernel calls
def run_fwd(ops, q, k, v, B, H, Nq, Nk, scale, causal=False):
    C = H * 64
    buf, O, before = out_view(B * Nq, C, q.device, seed=99)
    L2 = torch.full((B * H * Nq,), float('nan'), device=q.device)
    if causal:
        ops.attn_fwd_causal(q, k, v, O, L2, B, H, Nq, scale)
    else:
        ops.attn_fwd(q, k, v, O, L2, B, H, Nq, Nk, scale)
    torch.cuda.synchronize()
    check_sentinels(buf, before, B * Nq, C, 'O')
    return O, L2


def run_bwd(ops, form, q, k, v, O, do, L2, B, H, Nq, Nk, scale):
    """da_attn_bwd under attn_fused_bwd = form (restored afterwards): dQ, dK, dV (views with checked sentinels), Delta"""
    C, dev = H * 64, q.device
    bufs = [out_view(B * n, C, dev, seed=100 + i) for i, n in enumerate((Nq, Nk, Nk))]
    Delta = torch.full((B * H * Nq,), float('nan'), device=dev)
    prev = ops._opt('attn_fused_bwd', 1)
    try:
        ops.set_option('attn_fused_bwd', form)
        ops.attn_bwd(q, k, v, O, do, L2, Delta, bufs[0][1], bufs[1][1], bufs[2][1], B, H, Nq, Nk, scale)
        torch.cuda.synchronize()
    finally:
        ops.set_option('attn_fused_bwd', prev)
    for (buf, _, before), n, nm in zip(bufs, (Nq, Nk, Nk), ('dQ', 'dK', 'dV')):
        check_sentinels(buf, before, B * n, C, f'{nm} ({path(form, Nq, Nk)})')
    return bufs[0][1], bufs[1][1], bufs[2][1], Delta


def check_bwd(got, ref, O, do, B, H, Nq, Nk, what, vanishing=False):
    dQ, dK, dV, Delta = got
    _, _, rq, rk, rv = ref
    if Nk == 1 or vanishing:
        check_vanishing(dQ, f'{what} dQ')
        check_vanishing(dK, f'{what} dK')
    else:
        check(dQ, rq, BWD_TOL, f'{what} dQ', B, H)
        check(dK, rk, BWD_TOL, f'{what} dK', B, H)
    check(dV, rv, BWD_TOL, f'{what} dV', B, H)
    prod = (do.double() * O.double()).reshape(B, Nq, H, 64)
    dref = prod.sum(-1).permute(0, 2, 1).reshape(-1)
    dmag = prod.abs().sum(-1).permute(0, 2, 1).reshape(-1)
    assert torch.isfinite(Delta).all(), f'{what}: non-finite Delta'
    derr = ((Delta.double() - dref).abs() / (dmag + 1e-30)).max().item()
    assert derr < 1e-5, f'{what}: Delta != rowsum(dO * O): {derr:.3e}'


def bwd_all_forms(ops, q, k, v, O, do, L2, B, H, Nq, Nk, scale, ref, what, vanishing=False):
    """every distinct backward form at this shape against the reference, twice each (bitwise reproducible), and against
    each other; returns {path: outputs}"""
    res = {}
    for p, form in distinct_forms(Nq, Nk).items():
        got = run_bwd(ops, form, q, k, v, O, do, L2, B, H, Nq, Nk, scale)
        check_bwd(got, ref, O, do, B, H, Nq, Nk, f'{what} [{p}]', vanishing)
        again = run_bwd(ops, form, q, k, v, O, do, L2, B, H, Nq, Nk, scale)
        for a, b, nm in zip(got, again, ('dQ', 'dK', 'dV', 'Delta')):
            assert torch.equal(a, b), f'{what} [{p}]: {nm} differs between two identical calls'
        res[p] = got
    check_forms_agree(res, what)
    return res


def check_forms_agree(res, what):
    if 'pair' not in res:
        return
    pq, pk, pv, pd = res['pair']
    for p, (dq, dk, dv, dd) in res.items():
        if p == 'pair':
            continue
        for a, b, nm in ((dk, pk, 'dK'), (dv, pv, 'dV'), (dd, pd, 'Delta')):
            assert torch.equal(a, b), (f'{what}: {nm} of {p} != pair, max |diff| '
                                       f'{(a.double() - b.double()).abs().max().item():.3e}')
        e = rel_l2(dq, pq)
        assert e < DQ_XFORM_TOL, f'{what}: dQ of {p} vs pair rel-L2 {e:.3e} >= {DQ_XFORM_TOL}'


# ------------------------------------------------------------------------------------------------ shape matrix
def _cases():
    cases = []
    # fused<4> vs pair: every key count a 32-key block boundary can get wrong, ragged and tile-aligned query counts
    for Nk in (1, 16, 31, 32, 33, 64, 77, 96, 127, 128):
        for Nq in (64, 65, 95, 100, 200):
            cases.append((Nq, Nk))
    cases += [(63, 77), (63, 128), (64, 129), (257, 77), (1030, 77)]   # Nq / Nk dispatch boundaries, more tiles
    # fused<8> vs pair
    for Nk in (129, 160, 200, 255, 256):
        for Nq in (64, 100, 256):
            cases.append((Nq, Nk))
    # pair only: dK/dV<32> | <64> switch at Nq = 128
    cases += [(127, 200), (128, 200), (129, 200)]
    out = []
    for i, (Nq, Nk) in enumerate(cases):
        B, H = 1 + i % 3, 2 + (i // 3) % 2
        if B * H * Nq > 8192:
            B = 1
        out.append(pytest.param(B, H, Nq, Nk, 0.125, id=f'b{B}h{H}-{Nq}x{Nk}'))
    # another softmax scale: a constant tied to 0.125 would fail here
    out += [pytest.param(2, 3, 100, 77, 0.2, id='b2h3-100x77-scale0.2'),
            pytest.param(2, 2, 100, 200, 0.2, id='b2h2-100x200-scale0.2')]
    return out


@pytest.mark.parametrize('B,H,Nq,Nk,scale', _cases())
def test_attention_backward_forms(ops, dev, B, H, Nq, Nk, scale):
    q, k, v, do = make_inputs(B, H, Nq, Nk, dev, seed=Nq * 1000 + Nk)
    ref = reference(q, k, v, do, B, H, Nq, Nk, scale)
    O, L2 = run_fwd(ops, q, k, v, B, H, Nq, Nk, scale)
    check(O, ref[0], FWD_TOL, 'O', B, H)
    check_l2(L2, ref[1], 'L2')
    bwd_all_forms(ops, q, k, v, O, do, L2, B, H, Nq, Nk, scale, ref, f'{B}x{H}x{Nq}x{Nk}')


@pytest.mark.parametrize('Nq', [1, 127, 129])
@pytest.mark.parametrize('Nk', [1, 31, 33, 63, 65, 127, 129])
def test_attention_forward_tails(ops, dev, Nq, Nk):
    """da_attn_fwd: ragged 64-key tiles (masked tail step) and ragged 128-query workgroups"""
    B, H, scale = 2, 2, 0.125
    q, k, v, _ = make_inputs(B, H, Nq, Nk, dev, seed=7 * Nq + Nk)
    ref_o, ref_l2 = reference(q, k, v, None, B, H, Nq, Nk, scale)
    O, L2 = run_fwd(ops, q, k, v, B, H, Nq, Nk, scale)
    check(O, ref_o, FWD_TOL, 'O', B, H)
    check_l2(L2, ref_l2, 'L2')
    O2, L22 = run_fwd(ops, q, k, v, B, H, Nq, Nk, scale)
    assert torch.equal(O, O2) and torch.equal(L2, L22)


@pytest.mark.parametrize('N', [1, 33, 65, 127, 129, 257])
def test_attention_forward_causal_tails(ops, dev, N):
    """da_attn_fwd_causal: every tile masked per lane, tiles above a workgroup's last query skipped"""
    B, H, scale = 2, 3, 0.125
    q, k, v, _ = make_inputs(B, H, N, N, dev, seed=N)
    ref_o, ref_l2 = reference(q, k, v, None, B, H, N, N, scale, causal=True)
    O, L2 = run_fwd(ops, q, k, v, B, H, N, N, scale, causal=True)
    check(O, ref_o, FWD_TOL, 'causal O', B, H)
    check_l2(L2, ref_l2, 'causal L2')
    O2, L22 = run_fwd(ops, q, k, v, B, H, N, N, scale, causal=True)
    assert torch.equal(O, O2) and torch.equal(L2, L22)


# ------------------------------------------------------------------------------------------------ hostile inputs
HOSTILE_SHAPES = [pytest.param(2, 3, 100, 77, id='fused4-100x77'), pytest.param(2, 3, 100, 200, id='fused8-100x200'),
                  pytest.param(2, 3, 63, 77, id='pair-63x77'), pytest.param(1, 3, 130, 300, id='pair-130x300')]


@pytest.mark.parametrize('kind', ['shift', 'dominant', 'dominant2', 'big_delta'])
@pytest.mark.parametrize('B,H,Nq,Nk', HOSTILE_SHAPES)
def test_attention_hostile_inputs(ops, dev, kind, B, H, Nq, Nk):
    """Every backward form that applies, on inputs that push the softmax statistics to their ranges:
    * shift: L2 ~ -180 / +190 in two heads (one head ordinary).  Keys past Nk have S = 0 in the one-kernel forms, so their
      p = exp2(-L2) overflows to +inf once L2 < -128: they must not reach dQ (0 * inf = NaN).  L2 keeps the absolute 2e-3
      bound (measured 2.5e-5: the kernels carry it in fp32, ulp 1.5e-5 at 190).  dQ measures ~9e-3 here in every form
      (~2e-3 in the ordinary cases): its shifted column is -32 scale sum_j dS_j, exactly 0, and is left with 32x the bf16
      rounding of the dS row.
    * dominant: one key per row 20 nats above the rest, in the last, partial 32-key block: the running max moves in the
      tail step, and dQ / dK vanish (check_vanishing).  dominant2: two such keys, ordinary dQ / dK.
    * big_delta: dO = 50 O + noise, so delta = rowsum(dO * O) is ~50x its usual size."""
    scale = 0.125
    q, k, v, do = make_inputs(B, H, Nq, Nk, dev, seed=31 + Nq + Nk, kind=kind)
    O, L2 = run_fwd(ops, q, k, v, B, H, Nq, Nk, scale)
    if kind == 'big_delta':
        ref_o, _ = reference(q, k, v, None, B, H, Nq, Nk, scale)
        do = (50.0 * ref_o.reshape(B * Nq, H * 64) + randn(B * Nq, H * 64, seed=5, dev=dev)).to(BF)
    ref = reference(q, k, v, do, B, H, Nq, Nk, scale)
    check(O, ref[0], FWD_TOL, f'{kind} O', B, H)
    check_l2(L2, ref[1], f'{kind} L2')
    if kind == 'shift':
        l2 = ref[1]
        assert l2[:, 1].max() < -150 and l2[:, 2].min() > 150   # the case is as hostile as stated
    res = bwd_all_forms(ops, q, k, v, O, do, L2, B, H, Nq, Nk, scale, ref, f'{kind} {B}x{H}x{Nq}x{Nk}',
                        vanishing=kind == 'dominant')
    assert set(res) == set(distinct_forms(Nq, Nk))


# ------------------------------------------------------------------------------------------------ bench shapes
@pytest.mark.parametrize('B,H,Nq,Nk', [(256, 5, 1024, 77), (256, 20, 64, 64)])
def test_attention_backward_forms_agree_at_bench_shapes(ops, dev, B, H, Nq, Nk):
    """DESIGN.md's claim at the two shapes the one-kernel backward serves in the benchmark step: dK, dV and delta
    bit-identical to the two-kernel path, dQ within DQ_XFORM_TOL (rel-L2, whole tensor)"""
    scale = 0.125
    q, k, v, do = make_inputs(B, H, Nq, Nk, dev, seed=3)
    O, L2 = run_fwd(ops, q, k, v, B, H, Nq, Nk, scale)
    res = {p: run_bwd(ops, form, q, k, v, O, do, L2, B, H, Nq, Nk, scale)
           for p, form in distinct_forms(Nq, Nk).items()}
    assert set(res) == {'pair', 'fused4'}
    for p, got in res.items():
        for t, nm in zip(got, ('dQ', 'dK', 'dV', 'Delta')):
            assert torch.isfinite(t).all(), f'{p}: non-finite {nm}'
    check_forms_agree(res, f'{B}x{H}x{Nq}x{Nk}')
