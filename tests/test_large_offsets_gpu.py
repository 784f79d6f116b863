"""Every kernel family with ONE operand whose byte offsets cross 2 GiB and 4 GiB.

Many kernels here address an operand by a 32-bit byte offset from a uniform base, and a host-side guard picks between that
form and a 64-bit one at exactly 2^31 or 2^32 bytes (the guard table is in DESIGN.md, section 4.3a); the others multiply
`(long)row * ld`.  A small shape sees neither a wrapped offset nor the wrong side of a guard.

Technique: few rows, a giant row stride, one huge operand per case.  The huge operand is a view with ld = 2^20 bf16 elements
(2 MiB per row; 2^19 for fp32) inside one allocation, the "arena": row 1024 starts at byte 2^31 of the view, row 2048 at
2^32, while the arithmetic stays that of a ~2,304-row problem.  Every other operand of the case is compact (the
sentinel-padded views of the edge suites), so a failure names the operand whose addressing is wrong.

Layout, and the reason for it: the view starts 2 GiB + 4 KiB into the arena, and the arena extends past the view's last row.
A byte offset that wraps mod 2^32 (it lands 4 GiB below where it should, i.e. in the view's first 0.5 GiB) or that
sign-extends to a negative value (at most 2 GiB below the view's start) therefore still lands INSIDE the test's own
allocation: it shows up as a wrong value or as a changed sentinel, never as an access outside the allocation.  Where the
memory cap allows it (every view but GroupNorm's 6 GiB) the view starts 4 GiB + 4 KiB in: a sign-extended 32-bit ELEMENT
index reaches 4 GiB below the view (the mutation of gemm_nt.hip's epilogue in DESIGN.md does), and stays inside too.  The arena is
filled with one constant 16-bit pattern: the NaN 0x7FC1 when the huge operand is an input (a stray read poisons the result),
0x3F1B when it is an output (a stray write is visible); after the call the number of 16-bit words outside the view that differ
from the pattern, counted by a reduction on the device, must be 0.  One arena of 9.54 GiB is live at a time and is released
before the contiguous cases, which hold 9.1 GiB of their own.

Reference: every case also runs its compact twin, the same call with the huge operand replaced by a contiguous copy of the
same rows.  GEMM, weight-gradient and convolution cases use the exact-integer inputs of tests/test_gemm_edges_gpu.py and
tests/conv_rect_reference.py: the output is torch.equal to the float64 result rounded once AND bit-equal to the twin (the
pointer / generic / strip forms on one side of a guard and the 32-bit forms on the other are both exact).  Attention, norm,
pointwise and reduction cases are bit-equal to the twin: none of them chooses its kernel by ld, except GroupNorm, where
da_groupnorm_plan_for must report the same plan for both leading dimensions (otherwise the case is held to the float64 bounds
of tests/test_norm_edges_gpu.py through its gn_check_fwd / gn_check_bwd; the AdamW cases go through check_adamw of
tests/test_pointwise_edges_gpu.py).  No tolerance is defined here, and no other family leaves its twin.

Cases (rows straddle both marks unless a guard is probed from below; M = 2047: the last row ends just below 2^32, 2048: the
product is exactly 2^32; kernel templates from one rocprofv3 --kernel-trace run of this file):

    family                      | huge operand         | shapes                                  | form, confirmed by
    da_gemm_nt linear           | A                    | v12/14/15/18 at M 2047 | 2048, 2304     | EARLY | pointer: kernel trace; variant:
                                |                      | v1/4/5/10/11 at 2304                    |   da_gemm_nt_variant_for
                                |                      | stream at 2047 | 2304                   | gemm_nt3_kernel | tiled: kernel trace
                                |                      | ws: 8224 rows of ld 2^18 + 8            | gemm_nt_ws_kernel: kernel trace
    da_gemm_nt linear           | C, R, C == R         | v4/10 (de 1), v12/18 (de 3) at 2047 |   | direct | strip epilogue: kernel trace
                                |                      | 2048, 2304; fp32 C; split-K C           | split-K: the NaN workspace is written
    da_gemm_nt conv             | A modes 0-4, C 0 + 3 | 16x16 source images, v1/4/12/18         | da_gemm_nt_variant_for
    persistent 3x3 walk         | A                    | 63 | 64 images of 16x16 at ld 2^17      | persistent | generic: kernel trace
                                |                      | (exactly 2^32), N 1280                  |
    fused GEGLU fwd / bwd       | F, G, dF; A, dY      | M 2304; 2047; 2048 -> DA_ERR_SHAPE and  | return code
                                |                      | the two-launch path of ops              |
    da_gemm_tn_wgrad (+ group)  | dY, X                | v1 slab / atomic, FAST, ring 4 at lin   | da_gemm_tn_variant_for,
                                |                      | 2304 and conv 9x16x16; v2 generic at    | da_gemm_tn_group_plan,
                                |                      | lin 2344 and conv 9x16x17 (FAST period  | ring: kernel trace
                                |                      | 0); a group of 3 FAST linears           |
    attention fwd / causal /    | Q K V O (dO dQ dK dV)| (36,1,64,64) (30,2,77,77); wide; bwd    | -
    wide / bwd                  |                      | fused (36,1,64,77), pair (3,1,800,800)  |
    GroupNorm fwd / bwd         | X Y / X dY Radd dX   | B 3, C 64, HW 1023 (resident) | 1024    | da_groupnorm_plan_for
    LayerNorm fwd / bwd         | X Y / X dY Radd dX   | M 2304, C 320 | 1280                    | -
    colsum / image_colsum       | X (out)              | 2304 x 64; 9 x 256; 2304 images of 4    | -
    map2d                       | each operand         | geglu_bwd, copy2d, add, silu at 2304x64 | -
    conv2d_relu / pool / avgpool| X, Y                 | 3x3 p1 at 9x16x16, Cin 48; 3/s1/p1      | -
    adamw, adamw_dev, sumsq,    | contiguous           | n = 2^29 + 4099 floats, float64         | -
    cast                        |                      | reference in slices of 2^24             |

The ring guard and the grouped form's guard of the weight gradient (64 * ld < 2^31) have their other side at 64 rows of
66 MiB under gemm_tn_variant 3 ('noring': kernel trace; the group: da_gemm_tn_group_plan with the item's own row strides
reports -1 for the huge item).  v1 takes one split only up to 256 pixels, so its one-split case is those 64 rows too.  Only
the weight-stationary guard (64 * ld * 2 < 2^31) is probed from below only: reserve_cus is capped at 128, so the form needs
8,192 rows, which do not fit the memory cap at rows of 32 MiB.

Out of scope: upsample2x, add_noise, the loss kernels and the sampler kernels have no leading dimension; they reach 2 GiB
only at batch sizes no configuration uses.
"""

import pytest
import torch

from conv_rect_reference import reference
from test_attention_edges_gpu import make_inputs
from test_gemm_edges_gpu import (BF, F32, NAN, first_mismatch, gather, geom, in_view, ints, options, out_view, row_slice,
                                 splitk_floats, vec_slice)
from test_norm_edges_gpu import gn_check_bwd, gn_check_fwd, gn_form, gn_reference
from test_pointwise_edges_gpu import adamw_state, check_adamw, rne_bf16
from test_pointwise_edges_gpu import HYPER as PW_HYPER

pytestmark = pytest.mark.gpu

ROW = 1 << 21                              # bytes per row of the huge view (ld 2^20 bf16, 2^19 fp32)
HEAD, HEAD_DEEP = (1 << 31) + 4096, (1 << 32) + 4096   # bytes of the arena before the huge view: views above 5.5 GiB | the rest
SLACK = 64 * ROW                           # after the view's last row
ARENA = HEAD_DEEP + 2772 * ROW + SLACK     # 9.54 GiB: the attention keys (36 x 77 rows) behind the deep head
IN_PAT, OUT_PAT = 0x7FC1, 0x3F1B           # a NaN for inputs, 0.605 for outputs
M_BELOW, M_AT, M_BOTH = 2047, 2048, 2304   # rows * 2 MiB: just below 2^32, exactly 2^32, straddling 2^31 and 2^32


class Arena:
    """the one big allocation: 16-bit words, allocated on first use"""

    def __init__(self, dev):
        self.dev, self.buf, self.pat = dev, None, None

    def release(self):
        self.buf = None
        torch.cuda.empty_cache()

    def view(self, rows, cols, dtype, pat, ld_bytes=ROW):
        """the arena filled with `pat` and a [rows, cols] view of row stride ld_bytes that starts HEAD_DEEP (HEAD where that does not fit) bytes into it"""
        es = torch.empty(0, dtype=dtype).element_size()
        extent = (rows - 1) * ld_bytes + cols * es
        head = HEAD_DEEP if HEAD_DEEP + extent + SLACK <= ARENA else HEAD
        assert ld_bytes % (8 * es) == 0 and head + extent + SLACK <= ARENA
        if self.buf is None:
            self.buf = torch.empty(ARENA // 2, device=self.dev, dtype=torch.int16)
        self.buf.fill_(pat)
        self.pat, self.region = pat, (rows, cols * es // 2, ld_bytes // 2, head // 2)
        return torch.as_strided(self.buf.view(dtype), (rows, cols), (ld_bytes // es, 1), head // es)

    def strays(self):
        """16-bit words outside the view that differ from the pattern (a reduction on the device, in 512-MiB pieces)"""
        step, total = 1 << 28, 0
        for lo in range(0, self.buf.numel(), step):
            total += int((self.buf[lo:lo + step] != self.pat).sum())
        rows, words, ld, first = self.region
        return total - int((torch.as_strided(self.buf, (rows, words), (ld, 1), first) != self.pat).sum())


@pytest.fixture(scope='module')
def arena(dev):
    a = Arena(dev)
    yield a
    a.release()


@pytest.fixture(scope='module')
def ops(dev):
    from diffusion_amd import ops as o
    return o


def same_bits(a, b):
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def run_huge(arena, make, call, huge, outs, ld_bytes=ROW, what=''):
    """the compact twin, then the same call with operand `huge` inside the arena: every output bit-equal to the twin's, a huge
    input unchanged, no word of the arena outside the view changed.  make() -> a fresh dict of compact operands (an operand
    may appear under two names: the in-place residual); returns the huge run's operands"""
    twin = make()
    call(twin)
    torch.cuda.synchronize()
    t = make()
    src = t[huge]
    hv = arena.view(src.shape[0], src.shape[1], src.dtype, OUT_PAT if huge in outs else IN_PAT, ld_bytes)
    hv.copy_(src)
    for k in t:
        if t[k] is src:
            t[k] = hv
    call(t)
    torch.cuda.synchronize()
    assert arena.strays() == 0, f'{what}: {arena.strays()} words of the allocation outside the huge {huge} changed'
    if huge not in outs:
        assert same_bits(hv, src), f'{what}: the huge input {huge} changed'
    for k in outs:
        if t[k] is not None:
            assert same_bits(t[k], twin[k]), f'{what}: {k} differs from the compact twin: ' + \
                (first_mismatch(t[k], twin[k]) if t[k].dim() == 2 else '')
    return t


def nat_variant(ops, M, N, K, Cin, ws=0):
    return ops._lib.load().da_gemm_nt_variant_for(M, N, K, Cin, ws)


# ------------------------------------------------------------------------------------------------ da_gemm_nt
KN = ((64, 72), (320, 328), (64, 328), (320, 72))


def _nt_cases():
    cases = []   # (id, geometry, N, Cin, opts, variant | None, epilogue, huge operand, ld bytes)

    def add(tag, g, N, Cin, opts, want, epi, huge, ld=ROW):
        oid = '-'.join(f'{k.replace("gemm_nt_", "")}{v}' for k, v in opts.items())
        cases.append((f'{tag}-{"-".join(map(str, g))}-n{N}-c{Cin}-{oid}-{epi or "plain"}-huge{huge}', g, N, Cin, opts, want, epi,
                      huge, ld))

    i = 0
    for v in (12, 14, 15, 18):          # huge A: EARLY below 2^32, the pointer form at and above it
        for M in (M_BELOW, M_AT, M_BOTH):
            K, N = KN[i % 4]
            add('early' if M == M_BELOW else 'pointer', ('lin', M), N, K, {'gemm_nt_variant': v}, v, ('b', 'b+r', '')[i % 3], 'A')
            i += 1
    for v in (1, 4, 5, 10, 11):
        K, N = KN[i % 4]
        add('lin', ('lin', M_BOTH), N, K, {'gemm_nt_variant': v}, v, ('b', 'b+r', '')[i % 3], 'A')
        i += 1
    for M in (M_BELOW, M_BOTH):         # the streaming form (K >= 320) below 2^32, the tiled kernels above
        for huge in ('A', 'out', 'R'):
            add('stream' if M == M_BELOW else 'tiled', ('lin', M), (72, 328)[i % 2], 320, {'gemm_nt_stream': 2, 'gemm_nt_ws': 0},
                None, 'b+r', huge)
            i += 1
    add('ws', ('lin', 8192 + 32), 1280, 320, {'gemm_nt_ws': 3, 'reserve_cus': 128}, None, 'b+r', 'A', ((1 << 18) + 8) * 2)
    for v, de in ((4, 1), (10, 1), (12, 3), (18, 3)):   # huge C / R / C == R: direct epilogue below 2^32, strips at and above
        for M in (M_BELOW, M_AT, M_BOTH):
            for huge, epi in (('out', 'b'), ('R', 'b+r'), ('out', 'ip')):
                K, N = KN[i % 4]
                add('de' if M == M_BELOW else 'strip', ('lin', M), N, K, {'gemm_nt_variant': v, 'gemm_nt_de': de}, v, epi, huge)
                i += 1
    for M in (M_BELOW, M_BOTH):
        add('f32', ('lin', M), 72, 320, {'gemm_nt_variant': 12}, 12, 'f32+b', 'out')
    add('splitk', ('lin', M_BOTH), 72, 2880, {'reserve_cus': 0}, None, 'b+r', 'out')
    # convolutions: every gather mode reads 16 x 16 source images (2,304 source rows); huge C for modes 0 and 3
    for kind, g in (('conv', (9, 16, 16)), ('down', (9, 16, 16)), ('dgrad', (9, 32, 32)), ('up', (9, 16, 16)), ('vae', (9, 16, 16))):
        for v in (1, 4, 12, 18):
            add('conv', (kind,) + g, KN[i % 4][1], 64, {'gemm_nt_variant': v}, v, ('b+rb', 'b+r', 'rb')[i % 3], 'A')
            i += 1
    for kind, g in (('conv', (9, 16, 16)), ('up', (9, 8, 8))):
        for v in (1, 4, 12, 18):
            add('conv', (kind,) + g, KN[i % 4][1], 64, {'gemm_nt_variant': v}, v, ('b+rb', 'b+r', 'ip')[i % 3], 'out')
            i += 1
    # the persistent walk needs more tiles than CUs (> 128 with reserve_cus 128), which 2-MiB rows cannot give below 2^32:
    # rows of 256 KiB (ld 2^17) - 63 images are 252 tiles and end one image below 2^32, 64 images are exactly 2^32
    for B in (63, 64):
        add('pconv' if B == 63 else 'generic', ('conv', B, 16, 16), 1280, 64, {'gemm_nt_variant': 12, 'reserve_cus': 128}, 12,
            'b+rb+r', 'A', 1 << 18)
    return cases


NT_CASES = _nt_cases()


@pytest.mark.parametrize('case', NT_CASES, ids=[c[0] for c in NT_CASES])
def test_gemm_nt(ops, dev, arena, case):
    cid, g, N, Cin, opts, want, epi, huge, ld = case
    G = geom(ops, g)
    M, K, Mi = G.B * G.Hout * G.Wout, G.ksize * G.ksize * Cin, G.B * G.Hin * G.Win
    seed = sum(map(ord, cid)) % 10007
    parts = epi.split('+')
    odt = F32 if 'f32' in parts else BF
    extent = (Mi if huge == 'A' else M) * ld   # what the guards compare with 2^32
    if cid.startswith(('early', 'de-', 'stream', 'pconv')):
        assert (1 << 31) < extent < (1 << 32), cid
    if cid.startswith(('pointer', 'strip', 'tiled', 'generic')):
        assert extent >= (1 << 32), cid
    X, Wt = ints(Mi, Cin, seed=seed, dev=dev), ints(N, K, seed=seed + 1, dev=dev)
    bias = ints(N, seed=seed + 3, dev=dev, lo=-64, hi=64) if 'b' in parts else None
    rb = ints(G.B, N, seed=seed + 4, dev=dev, lo=-64, hi=64) if 'rb' in parts else None
    R = ints(M, N, seed=seed + 5, dev=dev, lo=-256, hi=256) if ('r' in parts or 'ip' in parts) else None
    ref = gather(X, G) @ Wt.double().t()
    for t in (bias, None if rb is None else rb.repeat_interleave(G.Hout * G.Wout, 0), R):
        if t is not None:
            ref += t.double()
    want_out = ref.to(odt)
    ws = torch.full((splitk_floats(M, N),), NAN, device=dev) if cid.startswith('splitk') else None

    def make():
        o = out_view(M, N, odt, dev, seed + 10, fill=None if 'ip' in parts else NAN)[1]
        if 'ip' in parts:
            o.copy_(R)
        return dict(A=in_view(X), W=row_slice(Wt.to(BF)), out=o, bias=vec_slice(bias) if bias is not None else None,
                    rb=in_view(rb) if rb is not None else None,
                    R=o if 'ip' in parts else in_view(R) if R is not None else None)

    def call(t):
        ops.gemm_nt(t['A'], t['W'], t['out'], G, bias=t['bias'], rowbias=t['rb'], residual=t['R'])

    old = ops.SPLITK_WS
    try:
        ops.SPLITK_WS = ws
        with options(ops, opts):
            if want is not None:
                assert nat_variant(ops, M, N, K, Cin) == want, cid
            t = run_huge(arena, make, call, huge, ('out',), ld, cid)
    finally:
        ops.SPLITK_WS = old
    if ws is not None:
        assert bool((~torch.isnan(ws)).any()), f'{cid}: the split-K workspace was not written (no split)'
    assert torch.equal(t['out'], want_out), f'{cid}: ' + first_mismatch(t['out'], want_out)


# ------------------------------------------------------------------------------------------------ fused GEGLU
GEGLU_CASES = [('fwd', M_BOTH, 320, 'F'), ('fwd', M_BOTH, 640, 'G'), ('fwd', M_BOTH, 640, 'F'), ('fwd', M_BOTH, 320, 'G'),
               ('fwd', M_BELOW, 320, 'A'), ('fwd', M_AT, 640, 'A'), ('bwd', M_BOTH, 320, 'dF'), ('bwd', M_BOTH, 640, 'F'),
               ('bwd', M_BOTH, 640, 'dF'), ('bwd', M_BOTH, 320, 'F'), ('bwd', M_BELOW, 640, 'dY'), ('bwd', M_AT, 320, 'dY')]


@pytest.mark.parametrize('case', GEGLU_CASES, ids=['-'.join(map(str, c)) for c in GEGLU_CASES])
def test_geglu(ops, dev, arena, case):
    """the unguarded operands F, G and dF at 2,304 rows; A / dY just below 4 GiB; at exactly 4 GiB the entry rejects the call
    with the outputs untouched and ops takes the two-launch path, whose bits the fused kernel gives"""
    kind, M, inner, huge = case
    K, seed, lib = 64, M + inner + (kind == 'bwd'), ops._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    if kind == 'fwd':
        A, Wt = ints(M, K, seed=seed, dev=dev), ints(2 * inner, K, seed=seed + 1, dev=dev)
        bias = ints(2 * inner, seed=seed + 2, dev=dev, lo=-64, hi=64)
        ref = (A.double() @ Wt.double().t() + bias.double()).to(BF)
        make = lambda: dict(A=in_view(A), W=row_slice(Wt.to(BF)), F=out_view(M, 2 * inner, BF, dev, seed + 3)[1],  # noqa: E731
                            G=out_view(M, inner, BF, dev, seed + 4)[1], bias=vec_slice(bias))
        call = lambda t: ops.gemm_nt_geglu(t['A'], t['W'], t['F'], t['G'], t['bias'])  # noqa: E731
        outs = ('F', 'G')
    else:
        dY, Wt = ints(M, K, seed=seed, dev=dev), ints(inner, K, seed=seed + 1, dev=dev)
        Fs = torch.randn(M, 2 * inner, generator=torch.Generator(device=dev).manual_seed(seed + 2), device=dev).mul(2).to(BF)
        d = (dY.double() @ Wt.double().t()).to(BF)
        ref = torch.empty(M, 2 * inner, device=dev, dtype=BF)
        ops.geglu_bwd(Fs, d, ref)
        make = lambda: dict(dY=in_view(dY), W=row_slice(Wt.to(BF)), F=in_view(Fs),  # noqa: E731
                            dF=out_view(M, 2 * inner, BF, dev, seed + 3)[1])
        call = lambda t: ops.gemm_nt_geglu_bwd(t['dY'], t['W'], t['F'], t['dF'])  # noqa: E731
        outs = ('dF',)
    if M == M_AT:   # the entry itself: rejected, nothing written
        t = make()
        hv = arena.view(M, K, BF, IN_PAT)
        hv.copy_(t[huge])
        keep = {k: t[k].clone() for k in outs}
        if kind == 'fwd':
            rc = lib.da_gemm_nt_geglu(hv.data_ptr(), hv.stride(0), t['W'].data_ptr(), t['F'].data_ptr(), t['F'].stride(0),
                                      t['G'].data_ptr(), t['G'].stride(0), t['bias'].data_ptr(), M, inner, K, st)
        else:
            rc = lib.da_gemm_nt_geglu_bwd(hv.data_ptr(), hv.stride(0), t['W'].data_ptr(), t['F'].data_ptr(), t['F'].stride(0),
                                          t['dF'].data_ptr(), t['dF'].stride(0), M, inner, K, st)
        torch.cuda.synchronize()
        assert rc == 1, f'{case}: the entry returned {rc} for a DMA source of exactly 4 GiB, not DA_ERR_SHAPE'
        assert all(same_bits(t[k], keep[k]) for k in outs), f'{case}: a rejected call wrote its outputs'
    t = run_huge(arena, make, call, huge, outs, what=str(case))
    if kind == 'fwd':
        assert torch.equal(t['F'], ref), 'F: ' + first_mismatch(t['F'], ref)
        g2 = torch.empty(M, inner, device=dev, dtype=BF)
        ops.geglu_fwd(t['F'], g2)
        assert same_bits(t['G'], g2), f'{case}: G differs from the two-kernel path'
    else:
        assert same_bits(t['dF'], ref), f'{case}: dF differs from the two-kernel path: ' + first_mismatch(t['dF'], ref)


# ------------------------------------------------------------------------------------------------ da_gemm_tn_wgrad
def _tn_cases():
    cases = []   # (id, geometry, N, Cin, opts, variant, workspace?, huge)
    for g in (('lin', M_BOTH), ('conv', 9, 16, 16)):
        for form, opts, want, ws in (('v1slab', {'gemm_tn_variant': 1}, 1, True), ('v1atomic', {'gemm_tn_variant': 1}, 1, False),
                                     ('v2', {'gemm_tn_variant': 2}, 2, True), ('fast', {'gemm_tn_variant': 3}, 3, True),
                                     ('ring4', {'gemm_tn_variant': 3, 'gemm_tn_ring': 4}, 3, False)):
            if form == 'ring4' and g[0] != 'lin':
                continue
            gg = g
            if form == 'v2':   # the generic gather runs where the FAST period is 0: a pixel count that is no multiple of 64
                gg = ('lin', M_BOTH + 40) if g[0] == 'lin' else ('conv', 9, 16, 17)
            for huge in ('dY', 'X'):
                cases.append((f'{form}-{"-".join(map(str, gg))}-huge{huge}', gg, 72 if huge == 'dY' else 200, 64, opts, want, ws, huge,
                              ROW))
    # the other side of the ring guard (64 * ld < 2^31): 64 rows of 66 MiB, the last one past 2^32 - the FAST kernel without
    # the ring takes the call
    for huge in ('dY', 'X'):
        cases.append((f'noring-lin-64-huge{huge}', ('lin', 64), 72 if huge == 'dY' else 200, 64,
                      {'gemm_tn_variant': 3, 'gemm_tn_ring': 4}, 3, False, huge, (1 << 26) + ROW))
        # v1 takes one split only up to 256 pixels: the same 64 rows (2,304 rows of 2 MiB always split)
        cases.append((f'v1-lin-64-huge{huge}', ('lin', 64), 72 if huge == 'dY' else 200, 64, {'gemm_tn_variant': 1}, 1, False, huge,
                      (1 << 26) + ROW))
    return cases


TN_CASES = _tn_cases()
TN_WS_FLOATS = 4 << 20


@pytest.mark.parametrize('overwrite', [0, 1])
@pytest.mark.parametrize('case', TN_CASES, ids=[c[0] for c in TN_CASES])
def test_wgrad(ops, dev, arena, case, overwrite):
    cid, g, N, Cin, opts, want, use_ws, huge, ld = case
    G = geom(ops, g)
    M, Kt, Mi = G.B * G.Hout * G.Wout, G.ksize * G.ksize * Cin, G.B * G.Hin * G.Win
    assert (64 * (ld // 2) >= 1 << 31) == cid.startswith(('noring', 'v1-')) and (M - 1) * ld > 1 << 32, cid
    seed = sum(map(ord, cid)) % 10007
    dY, X = ints(M, N, seed=seed, dev=dev), ints(Mi, Cin, seed=seed + 1, dev=dev)
    prior = ints(N * Kt, seed=seed + 2, dev=dev, lo=-1000, hi=1000)
    priorb = ints(N, seed=seed + 3, dev=dev, lo=-1000, hi=1000)
    ref, refb = dY.double().t() @ gather(X, G), dY.double().sum(0)
    if not overwrite:
        ref, refb = ref + prior.double().view(N, Kt), refb + priorb.double()
    make = lambda: dict(dY=in_view(dY), X=in_view(X),  # noqa: E731
                        dW=vec_slice(torch.full_like(prior, NAN) if overwrite else prior.clone(), pad=64),
                        db=vec_slice(torch.full_like(priorb, NAN) if overwrite else priorb.clone(), pad=64))
    call = lambda t: ops.gemm_tn_wgrad(t['dY'], t['X'], t['dW'], G, dbias=t['db'],  # noqa: E731
                                       scratch=torch.full((256 * N * 2,), NAN, device=dev))
    old = ops.SPLITK_WS
    try:
        ops.SPLITK_WS = torch.full((TN_WS_FLOATS,), NAN, device=dev) if use_ws else None
        with options(ops, {**opts, 'grad_overwrite': overwrite}):
            got_v = ops._lib.load().da_gemm_tn_variant_for(M, N, Cin, G.Hin, G.Win, G.Hout, G.Wout, G.ksize, G.mode)
            assert got_v == want, f'{cid}: runs variant {got_v}, the table says {want}'
            t = run_huge(arena, make, call, huge, ('dW', 'db'), ld, cid)
    finally:
        ops.SPLITK_WS = old
    assert torch.equal(t['dW'].view(N, Kt), ref.float()), f'{cid} dW: ' + first_mismatch(t['dW'].view(N, Kt), ref.float())
    assert torch.equal(t['db'], refb.float()), f'{cid} dbias'


def group_plan(ops, shapes, lds, M, ws_floats):
    """da_gemm_tn_group_plan with each item's own row strides (ops.gemm_tn_group_plan passes the compact N / Cin): group_of"""
    import ctypes
    n = len(shapes)
    arr = (ops._lib.DaWgradItem * n)()
    for i, ((N, Cin, db), (lddy, ldx)) in enumerate(zip(shapes, lds)):
        arr[i] = ops._lib.DaWgradItem(None, lddy, None, ldx, None, 1 if db else None, N, Cin)
    splits, group_of = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    assert ops._lib.load().da_gemm_tn_group_plan(arr, n, M, ws_floats, splits, n, group_of) >= 0
    return list(group_of)


# (M, row bytes of the huge operand, options, group_of with the huge item): below the guard of the grouped form (64 * ld < 2^31)
# the huge item stays in the launch; above it (64 rows of 66 MiB, the last one past 2^32) it goes to the per-layer path
GROUP_SIDES = {'below': (M_BOTH, ROW, {}, [0, 0, 0]), 'above': (64, (1 << 26) + ROW, {'gemm_tn_variant': 3}, [0, -1, 0])}


@pytest.mark.parametrize('overwrite', [0, 1])
@pytest.mark.parametrize('huge', ['X', 'dY'])
@pytest.mark.parametrize('side', list(GROUP_SIDES))
def test_wgrad_group(ops, dev, arena, side, huge, overwrite):
    """three FAST linears in one grouped launch, the second item's X (or dY) huge"""
    M, ld, opts, want_plan = GROUP_SIDES[side]
    shapes, wsf = [(320, 320, True), (960, 320, False), (320, 1280, True)], 8 << 20
    assert (64 * (ld // 2) >= 1 << 31) == (side == 'above') and (M - 1) * ld > 1 << 32
    dYs = [ints(M, N, seed=50 + i, dev=dev) for i, (N, _, _) in enumerate(shapes)]
    Xs = [ints(M, C, seed=60 + i, dev=dev) for i, (_, C, _) in enumerate(shapes)]

    def make():
        t = {}
        for i, (N, C, db) in enumerate(shapes):
            t[f'dY{i}'], t[f'X{i}'] = in_view(dYs[i]), in_view(Xs[i])
            t[f'dW{i}'] = vec_slice(torch.full((N * C,), NAN if overwrite else 3.0, device=dev), pad=64)
            t[f'db{i}'] = vec_slice(torch.full((N,), NAN if overwrite else 5.0, device=dev), pad=64) if db else None
        return t

    call = lambda t: ops.gemm_tn_wgrad_group([(t[f'dY{i}'], t[f'X{i}'], t[f'dW{i}'], t[f'db{i}']) for i in range(3)], M)  # noqa: E731
    outs = tuple(f'{k}{i}' for i in range(3) for k in ('dW', 'db'))
    old = ops.SPLITK_WS
    try:
        ops.SPLITK_WS = torch.full((wsf,), NAN, device=dev)
        with options(ops, {**opts, 'grad_overwrite': overwrite}):
            twin = make()
            lds = [[twin[f'dY{i}'].stride(0), twin[f'X{i}'].stride(0)] for i in range(3)]
            assert group_plan(ops, shapes, lds, M, wsf) == [0, 0, 0], 'the compact twin is not one grouped launch'
            lds[1][huge == 'X'] = ld // 2
            got = group_plan(ops, shapes, lds, M, wsf)
            assert got == want_plan, f'group {side} {huge}: plan {got}, expected {want_plan}'
            t = run_huge(arena, make, call, f'{huge}1', outs, ld, f'group {side} {huge}')
    finally:
        ops.SPLITK_WS = old
    for i, (N, C, db) in enumerate(shapes):
        ref = dYs[i].double().t() @ Xs[i].double() + (0 if overwrite else 3.0)
        assert torch.equal(t[f'dW{i}'].view(N, C), ref.float()), f'item {i} dW: ' + first_mismatch(t[f'dW{i}'].view(N, C), ref.float())
        if db:
            assert torch.equal(t[f'db{i}'], (dYs[i].double().sum(0) + (0 if overwrite else 5.0)).float()), f'item {i} dbias'


# ------------------------------------------------------------------------------------------------ attention
ATTN_FWD = [('fwd', 36, 1, 64, 64), ('fwd', 30, 2, 77, 77), ('causal', 30, 2, 77, 77), ('wide', 36, 1, 64, 64)]
ATTN_FWD_CASES = [c + (h,) for c in ATTN_FWD for h in 'QKVO']


def _wide_inputs(B, Nq, Nk, dev):
    g = torch.Generator(device=dev).manual_seed(7)
    return [torch.randn(B * n, 512, generator=g, device=dev).mul(0.25).to(BF) for n in (Nq, Nk, Nk)]


@pytest.mark.parametrize('case', ATTN_FWD_CASES, ids=['-'.join(map(str, c)) for c in ATTN_FWD_CASES])
def test_attention_forward(ops, dev, arena, case):
    kind, B, H, Nq, Nk, huge = case
    D = 512 if kind == 'wide' else 64
    q, k, v = _wide_inputs(B, Nq, Nk, dev) if kind == 'wide' else make_inputs(B, H, Nq, Nk, dev, 11)[:3]
    make = lambda: dict(Q=in_view(q), K=in_view(k), V=in_view(v), O=out_view(B * Nq, H * D, BF, dev, 12)[1],  # noqa: E731
                        L2=torch.full((B * H * Nq,), NAN, device=dev))

    def call(t):
        if kind == 'wide':
            ops.attn_fwd_wide(t['Q'], t['K'], t['V'], t['O'], t['L2'], B, H, D, Nq, Nk, D ** -0.5)
        elif kind == 'causal':
            ops.attn_fwd_causal(t['Q'], t['K'], t['V'], t['O'], t['L2'], B, H, Nq, 0.125)
        else:
            ops.attn_fwd(t['Q'], t['K'], t['V'], t['O'], t['L2'], B, H, Nq, Nk, 0.125)

    t = run_huge(arena, make, call, huge, ('O', 'L2'), what=str(case))
    assert bool(torch.isfinite(t['O'].float()).all()) and bool(torch.isfinite(t['L2']).all())


ATTN_BWD_CASES = [(f, B, H, Nq, Nk, h) for f, B, H, Nq, Nk in ((1, 36, 1, 64, 77), (0, 3, 1, 800, 800))
                  for h in ('Q', 'K', 'V', 'O', 'dO', 'dQ', 'dK', 'dV')]


@pytest.fixture(scope='module')
def attn_bwd_inputs(ops, dev):
    """q, k, v, do and the forward's O, L2 per shape, computed once"""
    out = {}
    for B, H, Nq, Nk in ((36, 1, 64, 77), (3, 1, 800, 800)):
        q, k, v, do = make_inputs(B, H, Nq, Nk, dev, 21)
        O, L2 = torch.empty(B * Nq, H * 64, device=dev, dtype=BF), torch.empty(B * H * Nq, device=dev)
        ops.attn_fwd(q, k, v, O, L2, B, H, Nq, Nk, 0.125)
        out[(B, H, Nq, Nk)] = (q, k, v, do, O, L2)
    return out


@pytest.mark.parametrize('case', ATTN_BWD_CASES, ids=['-'.join(map(str, c)) for c in ATTN_BWD_CASES])
def test_attention_backward(ops, dev, arena, attn_bwd_inputs, case):
    form, B, H, Nq, Nk, huge = case
    q, k, v, do, O, L2 = attn_bwd_inputs[(B, H, Nq, Nk)]
    make = lambda: dict(Q=in_view(q), K=in_view(k), V=in_view(v), O=in_view(O), dO=in_view(do),  # noqa: E731
                        dQ=out_view(B * Nq, H * 64, BF, dev, 22)[1], dK=out_view(B * Nk, H * 64, BF, dev, 23)[1],
                        dV=out_view(B * Nk, H * 64, BF, dev, 24)[1], Delta=torch.full((B * H * Nq,), NAN, device=dev))
    call = lambda t: ops.attn_bwd(t['Q'], t['K'], t['V'], t['O'], t['dO'], L2, t['Delta'], t['dQ'], t['dK'], t['dV'],  # noqa: E731
                                  B, H, Nq, Nk, 0.125)
    prev = ops._opt('attn_fused_bwd', 1)
    try:
        ops.set_option('attn_fused_bwd', form)
        t = run_huge(arena, make, call, huge, ('dQ', 'dK', 'dV', 'Delta'), what=str(case))
    finally:
        ops.set_option('attn_fused_bwd', prev)
    assert all(bool(torch.isfinite(t[n].float()).all()) for n in ('dQ', 'dK', 'dV', 'Delta'))


# ------------------------------------------------------------------------------------------------ GroupNorm, LayerNorm
GN_B, GN_C, GN_G, GN_LD, EPS = 3, 64, 32, 128, 1e-5
GN_CASES = [(HW, d, h, radd) for HW in (1023, 1024) for d, hs in (('fwd', ('X', 'Y')), ('bwd', ('X', 'dY', 'Radd', 'dX')))
            for h in hs for radd in ((1,) if h == 'Radd' or d == 'fwd' else (1, 0))]


def norm_view(t):
    """t [rows, C] as a column view at 8 of a [rows, GN_LD or wider] buffer of NaN"""
    ld = max(GN_LD, (t.shape[1] + 16 + 63) // 64 * 64)
    buf = torch.full((t.shape[0], ld), NAN, device=t.device, dtype=BF)
    buf[:, 8:8 + t.shape[1]] = t
    return buf[:, 8:8 + t.shape[1]]


@pytest.fixture(scope='module')
def gn_data(ops, dev):
    out = {}
    for HW in (1023, 1024):
        g = torch.Generator(device=dev).manual_seed(HW)
        x, dy, r = ((torch.randn(GN_B * HW, GN_C, generator=g, device=dev) * s + m).to(BF) for s, m in ((1.5, 0.5), (1, 0), (1, 0)))
        gamma, beta = 1 + 0.25 * torch.randn(GN_C, generator=g, device=dev), 0.25 * torch.randn(GN_C, generator=g, device=dev)
        mr = torch.empty(GN_B * GN_G * 2, device=dev)
        ops.groupnorm_fwd(x, torch.empty_like(x), gamma, beta, mr, torch.empty(GN_B * GN_C * 2, device=dev),
                          torch.empty(ops.norm_scratch_floats(GN_B, HW, GN_C), device=dev), GN_B, HW, GN_C, GN_G, EPS, 1)
        out[HW] = (x, dy, r, gamma, beta, mr)
    return out


@pytest.mark.parametrize('case', GN_CASES, ids=['-'.join(map(str, c)) for c in GN_CASES])
def test_groupnorm(ops, dev, arena, gn_data, case):
    """HW = 1023: the resident form with in-image offsets up to 2^31 - 2 MiB and image bases past 4 GiB; HW = 1024: exactly
    2^31 per image, which the guard sends to the multi-pass kernels (the twin is run multi-pass too)"""
    HW, direction, huge, radd = case
    B, C, G = GN_B, GN_C, GN_G
    x, dy, r, gamma, beta, mr = gn_data[HW]
    r = r if radd else None
    bwd = direction == 'bwd'
    with gn_form(ops, 'res0'):
        plan_h = ops.groupnorm_plan(B, HW, C, G, GN_LD, 1 << 20, bwd)
        plan_t = ops.groupnorm_plan(B, HW, C, G, GN_LD, GN_LD, bwd)
    assert plan_h['form'] == ('resident' if HW == 1023 else 'multipass') and plan_t['form'] == 'resident', (plan_h, plan_t)
    if HW == 1024:
        with gn_form(ops, 'multipass'):
            plan_t = ops.groupnorm_plan(B, HW, C, G, GN_LD, GN_LD, bwd)
    scratch = lambda: torch.full((ops.norm_scratch_floats(B, HW, C),), NAN, device=dev)  # noqa: E731
    if not bwd:
        make = lambda: dict(X=norm_view(x), Y=norm_view(torch.full_like(x, NAN)), mr=torch.full_like(mr, NAN))  # noqa: E731
        call = lambda t: ops.groupnorm_fwd(t['X'], t['Y'], gamma, beta, t['mr'], torch.empty(B * C * 2, device=dev),  # noqa: E731
                                           scratch(), B, HW, C, G, EPS, 1)
        outs = ('Y', 'mr')
    else:
        make = lambda: dict(X=norm_view(x), dY=norm_view(dy), Radd=norm_view(r) if radd else None,  # noqa: E731
                            dX=norm_view(torch.full_like(x, NAN)), dg=torch.full((C,), NAN, device=dev),
                            db=torch.full((C,), NAN, device=dev))
        call = lambda t: ops.groupnorm_bwd(t['X'], t['dY'], t['Radd'], t['dX'], gamma, beta, mr, t['dg'], t['db'],  # noqa: E731
                                           torch.empty(B * G * 2, device=dev), scratch(), B, HW, C, G, 1)
        outs = ('dX', 'dg', 'db')
    same_plan = plan_h == plan_t

    def call_formed(t):   # the huge run under the resident options (the guard decides), the twin of HW 1024 multi-pass
        is_huge = any(v is not None and v.dim() == 2 and v.stride(0) == 1 << 20 for v in t.values())
        with gn_form(ops, 'res0' if is_huge or HW == 1023 else 'multipass'), options(ops, {'grad_overwrite': 1}):
            call(t)

    if same_plan:
        run_huge(arena, make, call_formed, huge, outs, what=str(case))
        return
    t = make()
    src = t[huge]
    hv = arena.view(src.shape[0], C, BF, OUT_PAT if huge in outs else IN_PAT)
    hv.copy_(src)
    t[huge] = hv
    call_formed(t)
    torch.cuda.synchronize()
    assert arena.strays() == 0, f'{case}: words of the allocation outside the huge {huge} changed'
    ref = gn_reference(x, dy, r, gamma, beta, B, HW, C, G, EPS, 1)
    if bwd:
        gn_check_bwd(t['dX'], t['dg'], t['db'], ref, B, HW, C, G, 'gn', str(case))
    else:
        gn_check_fwd(t['Y'], t['mr'], ref, B, HW, C, G, 'gn', str(case))


LN_CASES = [(C, d, h) for C in (320, 1280) for d, hs in (('fwd', ('X', 'Y')), ('bwd', ('X', 'dY', 'Radd', 'dX'))) for h in hs]


@pytest.mark.parametrize('case', LN_CASES, ids=['-'.join(map(str, c)) for c in LN_CASES])
def test_layernorm(ops, dev, arena, case):
    C, direction, huge = case
    M = M_BOTH
    g = torch.Generator(device=dev).manual_seed(C)
    x, dy, r = ((torch.randn(M, C, generator=g, device=dev) * s + m).to(BF) for s, m in ((1.5, 0.3), (1, 0), (1, 0)))
    gamma, beta = 1 + 0.25 * torch.randn(C, generator=g, device=dev), 0.25 * torch.randn(C, generator=g, device=dev)
    mr = torch.empty(2 * M, device=dev)
    ops.layernorm_fwd(x, torch.empty_like(x), gamma, beta, mr, EPS)
    if direction == 'fwd':
        make = lambda: dict(X=norm_view(x), Y=norm_view(torch.full_like(x, NAN)), mr=torch.full_like(mr, NAN))  # noqa: E731
        call = lambda t: ops.layernorm_fwd(t['X'], t['Y'], gamma, beta, t['mr'], EPS)  # noqa: E731
        outs = ('Y', 'mr')
    else:
        make = lambda: dict(X=norm_view(x), dY=norm_view(dy), Radd=norm_view(r), dX=norm_view(torch.full_like(x, NAN)),  # noqa: E731
                            dg=torch.full((C,), NAN, device=dev), db=torch.full((C,), NAN, device=dev))
        call = lambda t: ops.layernorm_bwd(t['X'], t['dY'], t['Radd'], t['dX'], gamma, mr, t['dg'], t['db'],  # noqa: E731
                                           torch.full((1024 * C * 2,), NAN, device=dev))
        outs = ('dX', 'dg', 'db')
    with options(ops, {'grad_overwrite': 1}):
        t = run_huge(arena, make, call, huge, outs, what=str(case))
    assert all(bool(torch.isfinite(t[k].float()).all()) for k in outs)


# ------------------------------------------------------------------------------------------------ reductions, maps
def test_colsum_accum(ops, dev, arena):
    M, C = M_BOTH, 64
    x = ints(M, C, seed=31, dev=dev, lo=-4, hi=4).to(BF)
    prior = ints(C, seed=32, dev=dev)
    make = lambda: dict(X=norm_view(x), out=prior.clone())  # noqa: E731
    call = lambda t: ops.colsum_accum(t['X'], t['out'], torch.full((256 * C * 2,), NAN, device=dev))  # noqa: E731
    t = run_huge(arena, make, call, 'X', ('out',), what='colsum_accum')
    assert torch.equal(t['out'].double(), x.double().sum(0) + prior.double())


@pytest.mark.parametrize('huge,B,HW', [('X', 9, 256), ('out', M_BOTH, 4)])
def test_image_colsum(ops, dev, arena, huge, B, HW):
    C = 64
    x = ints(B * HW, C, seed=33, dev=dev, lo=-4, hi=4).to(BF)
    make = lambda: dict(X=norm_view(x), out=norm_view(torch.full((B, C), NAN, device=dev, dtype=BF)),  # noqa: E731
                        db=torch.zeros(C, device=dev))
    call = lambda t: ops.image_colsum(t['X'], t['out'], t['db'],  # noqa: E731
                                      torch.full((ops.norm_scratch_floats(B, HW, C),), NAN, device=dev), B, HW)
    t = run_huge(arena, make, call, huge, ('out', 'db'), what=f'image_colsum {huge}')
    sums = x.double().view(B, HW, C).sum(1)
    assert same_bits(t['out'], rne_bf16(sums)) and torch.equal(t['db'].double(), sums.sum(0))


MAP_CASES = [('geglu_bwd', h) for h in ('inp', 'dout', 'din')] + [(n, h) for n in ('copy2d', 'add', 'silu_fwd') for h in ('a', 'out')]


@pytest.mark.parametrize('name,huge', MAP_CASES, ids=['-'.join(c) for c in MAP_CASES])
def test_map2d(ops, dev, arena, name, huge):
    """map2d_kernel: geglu_bwd's five operands (the halves of inp and din, and dout) through its three matrices; one, two
    and one inputs of copy2d, add and silu_fwd, and their output"""
    M, C = M_BOTH, 64
    g = torch.Generator(device=dev).manual_seed(41)
    rnd = lambda c: torch.randn(M, c, generator=g, device=dev).to(BF)  # noqa: E731
    if name == 'geglu_bwd':
        inp, dout = rnd(2 * C), rnd(C)
        make = lambda: dict(inp=norm_view(inp), dout=norm_view(dout), din=norm_view(torch.full_like(inp, NAN)))  # noqa: E731
        call = lambda t: ops.geglu_bwd(t['inp'], t['dout'], t['din'])  # noqa: E731
        outs = ('din',)
    else:
        a, b = rnd(C), rnd(C)
        make = lambda: dict(a=norm_view(a), b=norm_view(b), out=norm_view(torch.full_like(a, NAN)))  # noqa: E731
        call = {'copy2d': lambda t: ops.copy2d(t['a'], t['out']), 'add': lambda t: ops.add(t['a'], t['b'], t['out']),
                'silu_fwd': lambda t: ops.silu_fwd(t['a'], t['out'])}[name]
        outs = ('out',)
    t = run_huge(arena, make, call, huge, outs, what=f'{name} {huge}')
    if name == 'copy2d':
        assert same_bits(t['out'], a)
    if name == 'add':
        assert same_bits(t['out'], rne_bf16(a.double() + b.double()))


# ------------------------------------------------------------------------------------------------ Inception kernels
@pytest.mark.parametrize('huge', ['X', 'Y'])
def test_conv2d_relu(ops, dev, arena, huge):
    geo, Cin, Cout = (9, 16, 16, 3, 3, 1, 1, 1), 48, 80
    X, Wt = ints(9 * 256, Cin, seed=51, dev=dev), ints(Cout, 9 * Cin, seed=52, dev=dev)
    bias = ints(Cout, seed=53, dev=dev, lo=-64, hi=64)
    make = lambda: dict(X=norm_view(X.to(BF)), Y=norm_view(torch.full((9 * 256, Cout), NAN, device=dev, dtype=BF)))  # noqa: E731
    call = lambda t: ops.conv2d_relu_fwd(t['X'], Wt.to(BF), bias, t['Y'], 9, 16, 16, 3, 3, 1, 1, 1, True)  # noqa: E731
    t = run_huge(arena, make, call, huge, ('Y',), what=f'conv2d_relu {huge}')
    ref = reference(X, Wt, bias, geo, True)[0].to(BF)
    assert torch.equal(t['Y'], ref), first_mismatch(t['Y'], ref)


@pytest.mark.parametrize('kind', [0, 1])
@pytest.mark.parametrize('huge', ['X', 'Y'])
def test_pool2d(ops, dev, arena, huge, kind):
    C = 64
    x = torch.randn(9 * 256, C, generator=torch.Generator(device=dev).manual_seed(54), device=dev).to(BF)
    make = lambda: dict(X=norm_view(x), Y=norm_view(torch.full_like(x, NAN)))  # noqa: E731
    call = lambda t: ops.pool2d_fwd(t['X'], t['Y'], 9, 16, 16, 1, 1, kind)  # noqa: E731
    t = run_huge(arena, make, call, huge, ('Y',), what=f'pool2d {kind} {huge}')
    if kind == 0:   # the maximum of bf16 values is one of them
        xp = torch.nn.functional.pad(x.float().view(9, 16, 16, C).permute(0, 3, 1, 2), (1, 1, 1, 1), value=float('-inf'))
        ref = torch.nn.functional.max_pool2d(xp, 3, 1).permute(0, 2, 3, 1).reshape(-1, C)
        assert torch.equal(t['Y'].float(), ref)


@pytest.mark.parametrize('huge,B,HW', [('X', 9, 256), ('out', M_BOTH, 4)])
def test_avgpool_global(ops, dev, arena, huge, B, HW):
    C = 64
    x = ints(B * HW, C, seed=55, dev=dev).to(BF)
    make = lambda: dict(X=norm_view(x), out=torch.full((B, C + 16), NAN, device=dev)[:, 8:8 + C])  # noqa: E731
    call = lambda t: ops.avgpool_global_f32(t['X'], t['out'], B, HW)  # noqa: E731
    t = run_huge(arena, make, call, huge, ('out',), what=f'avgpool {huge}')
    assert torch.equal(t['out'].double(), x.double().view(B, HW, C).sum(1) / HW)   # integer sums over a power of two: exact


# ------------------------------------------------------------------------------------------------ contiguous fp32 state
N_FLAT, SLICE = (1 << 29) + 4099, 1 << 24    # every tensor crosses 2 GiB; the reference walks the whole range in slices


def _slices():
    return [(lo, min(N_FLAT, lo + SLICE)) for lo in range(0, N_FLAT, SLICE)]


@pytest.mark.parametrize('entry', ['adamw', 'adamw_dev'])
def test_adamw_flat(ops, dev, arena, entry):
    """p, g, m, v of 2^29 + 4099 floats and the bf16 shadow (9.1 GiB; no ema), every element against float64 AdamW at the
    bounds of tests/test_pointwise_edges_gpu.py; the inputs of a slice are regenerated from its seed for the check"""
    arena.release()
    p, g, m, v = (torch.empty(N_FLAT, device=dev) for _ in range(4))
    sh = torch.empty(N_FLAT, device=dev, dtype=BF)
    for i, (lo, hi) in enumerate(_slices()):
        (ps, gs, ms, vs, _), _ = adamw_state(hi - lo, dev, 1000 + i)
        p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi] = ps, gs, ms, vs
    H = PW_HYPER
    if entry == 'adamw':
        ops.adamw(p, g, m, v, sh, H['lr'], H['b1'], H['b2'], H['eps'], H['wd'], 3, H['gs'])
    else:
        stats = torch.tensor([0.0, 0.0, H['gs'], 1.0, 0, 0, 0, 0], device=dev)
        ops.adamw_dev(p, g, m, v, sh, H['lr'], H['b1'], H['b2'], H['eps'], H['wd'], 3, stats)
    torch.cuda.synchronize()
    for i, (lo, hi) in enumerate(_slices()):
        state, zero = adamw_state(hi - lo, dev, 1000 + i)
        assert torch.equal(g[lo:hi], state[1]), f'{entry}: the gradient changed in slice {i}'
        check_adamw(state, (p[lo:hi], m[lo:hi], v[lo:hi], sh[lo:hi], None), 3, False, zero, f'{entry} slice {i} [{lo}, {hi})')


def test_cast_flat(ops, dev, arena):
    arena.release()
    src, dst = torch.empty(N_FLAT, device=dev), torch.full((N_FLAT + 64,), NAN, device=dev, dtype=BF)
    for i, (lo, hi) in enumerate(_slices()):
        src[lo:hi] = torch.randn(hi - lo, generator=torch.Generator(device=dev).manual_seed(2000 + i), device=dev)
    ops.cast_f32_bf16(src, dst[:N_FLAT])
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst[N_FLAT:]).all()), 'cast wrote past its end'
    for lo, hi in _slices():
        assert same_bits(dst[lo:hi], rne_bf16(src[lo:hi].double())), f'cast: slice [{lo}, {hi})'


def test_segment_sumsq_flat(ops, dev, arena):
    """integer gradients: every chunk partial is exact, a segment sum is the exact integer rounded once to fp32, and the total
    is the float64 sum of those, rounded once; the middle segment crosses 2 GiB"""
    from diffusion_amd.models.unet import SumsqTables
    arena.release()
    x = torch.full((N_FLAT,), NAN, device=dev)
    segs = [(0, (1 << 28) + 1), ((1 << 28) + 64, (1 << 28) + 936), ((1 << 29) + 1003, 3096)]
    assert segs[1][0] + segs[1][1] == (1 << 29) + 1000 and segs[2][0] + segs[2][1] == N_FLAT
    exact = []
    for s, (off, n) in enumerate(segs):
        tot = 0
        for lo in range(off, off + n, SLICE):
            hi = min(off + n, lo + SLICE)
            x[lo:hi] = ints(hi - lo, seed=3000 + lo // SLICE + s, dev=dev)
            tot += int(x[lo:hi].long().square().sum())
        exact.append(tot)
    tables = SumsqTables(segs).to(dev)
    partials = torch.full((ops.segment_sumsq_scratch_floats(len(tables.chunks)),), NAN, device=dev)
    seg, stats = torch.full((3,), NAN, device=dev), torch.zeros(8, device=dev)
    ops.segment_sumsq(x, tables, partials, seg, stats)
    torch.cuda.synchronize()
    want = torch.tensor(exact, dtype=torch.float64).float()
    assert torch.equal(seg.cpu(), want), (seg.cpu().tolist(), exact)
    assert float(stats[0]) == float(want.double().sum().float()) and float(stats[3]) == 1.0
