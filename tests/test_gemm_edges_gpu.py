"""The implicit GEMM at its edges: every kernel form of gemm_nt*.hip and gemm_tn*.hip against a float64 reference, at the
shapes, gathers, options and memory layouts where GEMM kernels go wrong.

da_gemm_nt forms (NT_CASES; the case's `opts` are set with da_set_option and restored afterwards):

    form          | forced by                                          | tile (BM x BN)        | confirmed by
    v1            | gemm_nt_variant 1; any Cin % 64 != 0               | 128 x 128             | da_gemm_nt_variant_for
    v2 <v>        | gemm_nt_variant v, v in 4 5 10 11 12 14 15 16 18   | 256x128 256x160       | da_gemm_nt_variant_for
                  |                                                    | 256x320 128x320 ...   |
    early         | ksize 1 on the 16-wave forms 12 / 14 / 15 / 18     | persistent tile walk  | kernel trace
    pconv         | 3x3 mode 0, N % 320 == 0, variant 12 (or auto),    | 256 x 320, resident   | kernel trace
                  | tiles > 256 - reserve_cus (reserve_cus 128)        | workgroups            |
    splitk        | auto dispatch, SPLITK_WS given, small M            | + splitk_finalize     | da_gemm_nt_variant_for with
                  |                                                    |                       | the workspace size; the
                  |                                                    |                       | NaN workspace is written
    de / strip    | gemm_nt_de 1 (convs) / 0 / 3 (linears too)         |                       | kernel trace
    ws            | gemm_nt_ws 3, K = 320 / 640, M % 32 == 0,          | gemm_nt_ws_kernel     | kernel trace
                  | M / 32 * N / BN >= 8 * (256 - reserve_cus)         |                       |
    stream        | gemm_nt_stream 2 (gemm_nt_ws 0), K % 64 == 0       | gemm_nt3_kernel       | kernel trace
    korder        | gemm_nt_korder 0 / 1, 3x3 with Cin 320 and 1280    |                       | -

Every form runs linears with M in {1, BM - 1, BM + 1, 3 BM + 17}, N in {8, 72, BN - 8, BN + 8, 2 BN + 8}, K in
{64, 320, 640, 1344} (v1 also K = 8 and 200); 3x3 mode 0 at (B, H, W) in {(3,1,1), (2,2,2), (1,1,7), (5,3,5), (2,4,4)} with
Cin in {8 (v1), 64, 320, 1280}; a 1x1 convolution with per-image row bias; mode 1 (stride 2) at even sizes and at odd
ones with Hout = ceil(H / 2), where the last column tap reaches w == Win - 1; mode 2 (dgrad of stride 2) at (2,2), (2,6),
(4,4), (8,8); mode 3 (nearest-2x) at H, W in {1, 2, 3x5}; mode 4 (bottom / right pad) at (2,2), (4,6).  The options rotate
over the cases: bias, per-image row bias where images straddle tiles, residual, in-place residual, alpha 0.5, fp32 output.
The persistent convolution walk runs with a ragged last row tile (B = 133 at 8x8, N = 1280: 64 rows; B = 300 at 5x7: 4 rows).

da_gemm_tn_wgrad forms (TN_CASES), each with grad_overwrite 0 and 1:

    form          | forced by                                          | confirmed by
    v1            | gemm_tn_variant 1, M <= 256 (one split)            | da_gemm_tn_variant_for
    v1slab        | gemm_tn_variant 1, M > 256, workspace given        | the NaN workspace is written
    v1atomic      | gemm_tn_variant 1, M > 256, no workspace           | -
    v2            | gemm_tn_variant 2 where the FAST period is 0       | da_gemm_tn_variant_for (2)
    fast          | gemm_tn_variant 3 where the period allows          | da_gemm_tn_variant_for (3)
    v2slab / v2at | v2 / FAST with M >= 1024 and few tiles: split      | the NaN workspace is written / -
    ring4 / ring5 | gemm_tn_ring 4 / 5, FAST linears                   | kernel trace

GEGLU_CASES run the fused GEGLU forward (inner 160 / 320 / 640) and backward (320 / 640) at ragged M.

Reference: float64 on the bf16-rounded inputs, through an explicit gather per mode (gather_index; tests/test_abi_and_host.py
checks it against F.conv2d / conv_transpose2d in float64 on the CPU).

Exact cases (all of NT_CASES, TN_CASES, GEGLU_CASES): every input is an integer, |A|, |W| <= 8, integer bias, row bias,
residual and prior dW.  Every fp32 partial sum is then an exact integer below 2^24 in any order (MFMA, split-K slabs,
atomics), so:
  * bf16 outputs are torch.equal to ref.to(bf16) - one round-to-nearest-even; fp32 outputs, dW and dbias equal ref;
  * the fused GEGLU pre-activation F is exact; its gated output and the backward's dF equal, bit for bit, the two-kernel
    path (da_geglu_fwd / da_geglu_bwd) on the same bf16 operands.
Float cases (FLOAT_CASES): N(0,1) inputs, rows scaled from 1e-3 to 1e3, and near-cancelling dot products.  Every element:
    |out - ref| <= ulp_out(ref) + c2 * 2^-24 * K * (|A| |W|^T + |bias| + |row bias| + |residual|)[m, n]
plus rel-L2 over the whole tensor and per (row tile, column tile) block.
Memory, every case: outputs are NaN-prefilled views inside buffers with sentinel pad columns and >= 384 sentinel rows
(bit-identical afterwards); A, the row bias and the residual are column views whose pad columns and 8 trailing rows hold
NaN; W and the bias are slices with NaN rows / elements on either side; the split-K workspace is NaN-prefilled; with
grad_overwrite 1, dW and dbias are written over NaN, with 0 they add onto integer prior contents; a repeated call gives
identical bits.
Bounds: at most 2x the worst margin measured on MI355X; DA_PARITY_MARGINS=<path> writes the margins of a run
(tests/parity_margins.py).
"""
import contextlib
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
NAN = float('nan')
PAD_L, PAD_R = 8, 8     # pad columns left / right of every matrix view
PAD_ROWS = 384          # sentinel rows after every output: a whole row tile of the tallest form (384 x 128)

# ------------------------------------------------------------------------------------------------ bounds
# '<api>.<inputs>.<quantity>': api nt (da_gemm_nt) / tn (da_gemm_tn_wgrad); inputs randn / rows / cancel (FLOAT_CASES);
# c2 of the per-element bound, rel-L2 over the whole tensor, worst rel-L2 of a 128 x 128 block
BOUNDS = {   # bound: worst measured on MI355X
    'nt.randn.c2': 4.9e-03, 'nt.randn.rel': 3.3e-03, 'nt.randn.block': 3.5e-03,
    # 2.46e-03, 1.67e-03, 1.79e-03
    'nt.rows.c2': 1.5e-02, 'nt.rows.rel': 3.3e-03, 'nt.rows.block': 3.9e-03,
    # 7.61e-03, 1.69e-03, 2.00e-03
    'nt.cancel.c2': 4.7e-03, 'nt.cancel.rel': 3.3e-03, 'nt.cancel.block': 3.5e-03,
    # 2.40e-03, 1.68e-03, 1.78e-03
    'tn.randn.c2': 8.3e-03, 'tn.randn.rel': 2.6e-07, 'tn.randn.block': 2.7e-07,
    # 4.20e-03, 1.34e-07, 1.36e-07
    'tn.rows.c2': 2.3e-02, 'tn.rows.rel': 3.1e-07, 'tn.rows.block': 3.2e-07,
    # 1.18e-02, 1.60e-07, 1.62e-07
    'tn.cancel.c2': 8.3e-03, 'tn.cancel.rel': 9.1e-05, 'tn.cancel.block': 9.2e-05,
    # 4.19e-03, 4.58e-05, 4.61e-05
}
_WORST = {}


def _margin(name, value):
    """keep the worst value of each bounded quantity and assert it"""
    _WORST[name] = max(_WORST.get(name, 0.0), value)
    if os.environ.get('DA_PARITY_MARGINS'):
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from parity_margins import record
        record('gemm_edges', tolerances=BOUNDS, **_WORST)
    return value <= BOUNDS[name]


@pytest.fixture(scope='module')
def ops(dev):
    from diffusion_amd import ops as o
    return o


DEFAULTS = {'gemm_nt_variant': 0, 'gemm_nt_de': 1, 'gemm_nt_korder': 1, 'gemm_nt_ws': 1, 'gemm_nt_stream': 0,
            'gemm_nt_stream_lw': 4, 'gemm_nt_persist': -1, 'reserve_cus': 0, 'gemm_tn_variant': 0, 'gemm_tn_ring': 0,
            'grad_overwrite': 0}


@contextlib.contextmanager
def options(ops, opts):
    """set a case's options; every one of them is restored to its default afterwards"""
    try:
        for k, v in opts.items():
            ops.set_option(k, v)
        yield
    finally:
        for k in opts:
            ops.set_option(k, DEFAULTS[k])


# ------------------------------------------------------------------------------------------------ geometry + reference
def geom(ops, g):
    """('lin', M) | (kind, B, H, W) -> ops.Geom; 'down' / 'downo' (odd sizes) take Hout = ceil(H / 2), as a stride-2 conv does"""
    if g[0] == 'lin':
        return ops.Geom.linear(g[1])
    kind, B, H, W = g
    return {'conv': lambda: ops.Geom.conv(B, H, W), 'c1': lambda: ops.Geom.conv(B, H, W, ksize=1),
            'down': lambda: ops.Geom(B, H, W, (H + 1) // 2, (W + 1) // 2, 3, 1),
            'downo': lambda: ops.Geom(B, H, W, (H + 1) // 2, (W + 1) // 2, 3, 1), 'dgrad': lambda: ops.Geom.down_dgrad(B, H, W),
            'up': lambda: ops.Geom.up(B, H, W), 'vae': lambda: ops.Geom.down_vae(B, H, W)}[kind]()


def gather_index(g, device='cpu'):
    """[M, taps] source pixel of output pixel m for tap (r, s) (row-major taps), -1 where the tap reads zero padding"""
    B, Hin, Win, Hout, Wout, k, mode = g.B, g.Hin, g.Win, g.Hout, g.Wout, g.ksize, g.mode
    b = torch.arange(B, device=device).view(B, 1, 1, 1)
    oh = torch.arange(Hout, device=device).view(1, Hout, 1, 1)
    ow = torch.arange(Wout, device=device).view(1, 1, Wout, 1)
    t = torch.arange(k * k, device=device).view(1, 1, 1, k * k)
    r, s = (t // 3, t % 3) if k == 3 else (t * 0, t * 0)
    pad = 1 if k == 3 else 0
    ok = torch.ones(B, Hout, Wout, k * k, dtype=torch.bool, device=device)
    if mode == 0:
        ih, iw = oh + r - pad, ow + s - pad
    elif mode == 1:                       # stride 2, pad 1
        ih, iw = 2 * oh + r - 1, 2 * ow + s - 1
    elif mode == 4:                       # stride 2 over an image zero-padded at the bottom / right only
        ih, iw = 2 * oh + r, 2 * ow + s
    elif mode == 2:                       # dgrad of stride 2: only even positions of the dilated dY are taps
        th, tw = oh + r - 1, ow + s - 1
        ok = ok & (th % 2 == 0) & (tw % 2 == 0)
        ih, iw = torch.div(th, 2, rounding_mode='floor'), torch.div(tw, 2, rounding_mode='floor')
    else:                                 # mode 3: conv (pad 1) over the nearest-2x upsampled image
        th, tw = oh + r - 1, ow + s - 1
        ok = ok & (th >= 0) & (tw >= 0) & (th < Hout) & (tw < Wout)
        ih, iw = torch.div(th, 2, rounding_mode='floor'), torch.div(tw, 2, rounding_mode='floor')
    ok = ok & (ih >= 0) & (iw >= 0) & (ih < Hin) & (iw < Win)
    idx = b * (Hin * Win) + ih * Win + iw
    return torch.where(ok, idx, torch.full_like(idx, -1)).reshape(B * Hout * Wout, k * k)


def gather(X, g):
    """float64 [M, taps * Cin]: the implicit GEMM's A operand, built explicitly"""
    idx = gather_index(g, X.device)
    Xz = torch.cat([X.to(F64), torch.zeros(1, X.shape[1], dtype=F64, device=X.device)])
    idx = torch.where(idx < 0, torch.full_like(idx, X.shape[0]), idx)
    return Xz[idx].reshape(idx.shape[0], -1)


# ------------------------------------------------------------------------------------------------ buffers
def gen(seed, dev):
    return torch.Generator(device=dev).manual_seed(seed)


def ints(*shape, seed, dev, lo=-8, hi=8):
    """integers in [lo, hi], float32"""
    return torch.randint(lo, hi + 1, shape, generator=gen(seed, dev), device=dev).float()


def in_view(t, dtype=BF):
    """t [rows, C] as a column view at PAD_L of a [rows + 8, PAD_L + C + PAD_R] buffer whose other elements hold NaN"""
    rows, C = t.shape
    buf = torch.full((rows + 8, PAD_L + C + PAD_R), NAN, device=t.device, dtype=dtype)
    buf[:rows, PAD_L:PAD_L + C] = t.to(dtype)
    return buf[:rows, PAD_L:PAD_L + C]


def row_slice(t, pad=8):
    """t [N, K] contiguous as rows [pad, pad + N) of a buffer whose other rows hold NaN"""
    buf = torch.full((t.shape[0] + 2 * pad, t.shape[1]), NAN, device=t.device, dtype=t.dtype)
    buf[pad:pad + t.shape[0]] = t
    return buf[pad:pad + t.shape[0]]


def vec_slice(t, pad=16):
    buf = torch.full((t.numel() + 2 * pad,), NAN, device=t.device, dtype=t.dtype)
    buf[pad:pad + t.numel()] = t
    return buf[pad:pad + t.numel()]


def out_view(rows, C, dtype, dev, seed, fill=NAN):
    """a [rows, C] view at PAD_L of a [rows + PAD_ROWS, PAD_L + C + PAD_R] buffer of random sentinels, filled with `fill`:
    (buffer, view, copy of the buffer)"""
    buf = torch.randn(rows + PAD_ROWS, PAD_L + C + PAD_R, generator=gen(seed, dev), device=dev).to(dtype)
    view = buf[:rows, PAD_L:PAD_L + C]
    if fill is not None:
        view.fill_(fill)
    return buf, view, buf.clone()


def assert_pads_kept(buf, ref_buf, rows, C, what):
    """everything of buf outside the [rows, C] view at PAD_L equals ref_buf bit for bit"""
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    keep[:rows, PAD_L:PAD_L + C] = False
    a, b = buf[keep], ref_buf[keep]
    same = (a == b) | (torch.isnan(a) & torch.isnan(b))
    assert bool(same.all()), f'{what}: {int((~same).sum())} sentinel elements outside the output view changed'


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int16 if a.dtype == BF else torch.int32),
                       b.contiguous().view(torch.int16 if b.dtype == BF else torch.int32))


def first_mismatch(out, ref):
    bad = (out.double() != ref.double()) | torch.isnan(out.double())
    if not bool(bad.any()):
        return ''
    m, n = [int(v) for v in bad.nonzero()[0]]
    return (f'{int(bad.sum())} of {bad.numel()} elements differ, first at ({m}, {n}): '
            f'{out[m, n].item()} vs {ref[m, n].item()}')


# ------------------------------------------------------------------------------------------------ da_gemm_nt case table
V2_FORMS = (4, 5, 10, 11, 12, 14, 15, 16, 18)
TILE = {1: (128, 128), 4: (256, 128), 5: (256, 160), 10: (256, 320), 11: (128, 320), 12: (256, 320), 14: (256, 256),
        15: (256, 320), 16: (256, 320), 18: (384, 128)}
# epilogue option sets: b bias, rb per-image row bias, r residual, ip in-place residual, a alpha 0.5, f32 fp32 output
EPIS = ('b', 'rb+r', 'b+rb+r', 'a', 'f32+b', 'ip', 'b+r', 'a+rb+f32', '', 'b+rb')
CONV_SHAPES = ((3, 1, 1), (2, 2, 2), (1, 1, 7), (5, 3, 5), (2, 4, 4))
MODE_SHAPES = {'down': ((2, 2, 2), (3, 2, 6), (2, 4, 4), (1, 8, 8)), 'downo': ((2, 3, 5), (3, 1, 1), (1, 5, 3), (2, 7, 7)),
               'dgrad': ((2, 2, 2), (3, 2, 6), (2, 4, 4), (1, 8, 8)), 'up': ((3, 1, 1), (2, 2, 2), (2, 3, 5)),
               'vae': ((3, 2, 2), (2, 4, 6))}
LIN_K = (64, 320, 640, 1344)


def _nt_cases():
    cases = []   # (id, geometry, N, Cin, opts, variant the query must report (None: not queried), epilogue, form)

    def add(form, g, N, Cin, opts, want, epi):
        gid = '-'.join(str(v) for v in g)
        oid = '-'.join(f'{k.replace("gemm_nt_", "")}{v}' for k, v in opts.items())
        cases.append((f'{form}-{gid}-n{N}-c{Cin}-{oid}-{epi.replace("+", "") or "plain"}', g, N, Cin, opts, want, epi, form))

    for fi, v in enumerate((1,) + V2_FORMS):
        bm, bn = TILE[v]
        Ms, Ns = (1, bm - 1, bm + 1, 3 * bm + 17), (8, 72, bn - 8, bn + 8, 2 * bn + 8)
        form = 'v1' if v == 1 else f'v{v}'
        lin_form = form + ('-early' if v in (12, 14, 15, 18) else '')
        for i in range(5):
            de = (0, 1, 3)[(i + fi) % 3]
            add(lin_form, ('lin', Ms[i % 4]), Ns[i], LIN_K[(i + fi) % 4], {'gemm_nt_variant': v, 'gemm_nt_de': de}, v,
                EPIS[(i + fi) % len(EPIS)])
        for i, (B, H, W) in enumerate(CONV_SHAPES):
            Cin = 8 if v == 1 and i % 2 == 0 else (64, 320, 1280)[(i + fi) % 3]
            opts = {'gemm_nt_variant': v, 'gemm_nt_de': (1, 0)[(i + fi) % 2]}
            if Cin >= 320:
                opts['gemm_nt_korder'] = (i + fi) % 2
            add(form, ('conv', B, H, W), Ns[(i + fi + 1) % 5], Cin, opts, v, EPIS[(i + 2 * fi) % len(EPIS)])
        add(lin_form, ('c1', 5, 3, 5), Ns[(fi + 3) % 5], 64 if v != 1 else 72, {'gemm_nt_variant': v}, v, 'b+rb+r')
        k = 0
        for kind, n in (('down', 2), ('downo', 1), ('dgrad', 2), ('up', 2), ('vae', 1)):
            shapes = MODE_SHAPES[kind]
            for j in range(n):
                B, H, W = shapes[(fi + j) % len(shapes)]
                Cin = 8 if v == 1 and k % 2 else (64, 320)[(fi + k) % 2]
                add(form, (kind, B, H, W), Ns[(fi + k) % 5], Cin, {'gemm_nt_variant': v, 'gemm_nt_de': (1, 0)[k % 2]}, v,
                    EPIS[(fi + 3 * k) % len(EPIS)])
                k += 1
    # K % 64 != 0: v1 whatever variant is forced
    for K, v, epi in ((8, 1, 'b+r'), (200, 1, 'a+rb+f32'), (200, 12, 'ip'), (8, 4, 'f32+b')):
        add('v1', ('lin', 300), 136, K, {'gemm_nt_variant': v}, 1, epi)
    add('v1', ('conv', 2, 3, 5), 328, 72, {'gemm_nt_variant': 14}, 1, 'b+rb+r')
    # the persistent convolution walk with a ragged last row tile (64 rows / 4 rows, images straddling it in the second)
    for g, Cin, opts, epi in ((('conv', 133, 8, 8), 64, {'gemm_nt_variant': 12, 'reserve_cus': 128}, 'b+rb+r'),
                              (('conv', 133, 8, 8), 64, {'gemm_nt_variant': 12, 'reserve_cus': 128, 'gemm_nt_de': 0}, 'b+rb+r'),
                              (('conv', 300, 5, 7), 64, {'gemm_nt_variant': 12, 'reserve_cus': 128}, 'b+rb+r'),
                              (('conv', 300, 5, 7), 64, {'gemm_nt_variant': 12, 'reserve_cus': 128, 'gemm_nt_de': 0}, 'ip'),
                              (('conv', 133, 8, 8), 320, {'gemm_nt_variant': 12, 'reserve_cus': 128, 'gemm_nt_korder': 0}, 'rb'),
                              (('conv', 261, 8, 8), 64, {'gemm_nt_variant': 12}, 'b+r')):
        add('pconv', g, 1280, Cin, opts, 12, epi)
    # split-K over the NaN workspace: auto dispatch at small M
    for g, N, Cin, epi in ((('conv', 2, 4, 4), 320, 320, 'b+rb+r'), (('conv', 5, 3, 5), 648, 320, 'a+rb+f32'),
                           (('conv', 3, 1, 1), 72, 1280, 'b+r'), (('down', 2, 8, 8), 328, 320, 'ip'),
                           (('conv', 1, 1, 7), 200, 640, 'f32+b'), (('lin', 40), 328, 2880, 'rb+r')):
        add('splitk', g, N, Cin, {'reserve_cus': 0}, 4, epi)
    # weight-stationary form: whole 32-row tiles, K = 320 (BN 320) / 640 (BN 128)
    for M, N, K, epi in ((8192 + 32, 1280, 320, 'b+r'), (8192, 1280, 320, 'ip'), (4096 + 32, 1024, 640, 'b'),
                         (4096 + 32, 1024, 640, 'r')):
        add('ws', ('lin', M), N, K, {'gemm_nt_ws': 3, 'reserve_cus': 128}, None, epi)
    # streaming form
    for M, N, K, epi, lw in ((1, 8, 320, 'b', 4), (127, 72, 640, 'b+r', 4), (1169, 648, 1344, 'b+r', 4), (300, 328, 320, 'ip', 4),
                             (129, 968, 384, '', 16), (600, 320, 1344, 'b+r', 16)):
        add('stream', ('lin', M), N, K, {'gemm_nt_stream': 2, 'gemm_nt_ws': 0, 'gemm_nt_stream_lw': lw}, None, epi)
    return cases


NT_CASES = _nt_cases()


def nt_variant(ops, case):
    """what da_gemm_nt_variant_for reports for a case under its options (ws_floats: the workspace the case passes)"""
    from diffusion_amd import _lib
    _, g, N, Cin, opts, _, _, form = case
    G = geom(ops, g)
    M, K = G.B * G.Hout * G.Wout, G.ksize * G.ksize * Cin
    with options(ops, opts):
        return _lib.load().da_gemm_nt_variant_for(M, N, K, Cin, splitk_floats(M, N) if form == 'splitk' else 0)


def splitk_floats(M, N):
    return 8 * M * N + 64


def _epi_inputs(epi, M, N, B, dev, seed):
    bias = ints(N, seed=seed + 3, dev=dev, lo=-64, hi=64) if 'b' in epi.split('+') else None
    rb = ints(B, N, seed=seed + 4, dev=dev, lo=-64, hi=64) if 'rb' in epi.split('+') else None
    R = ints(M, N, seed=seed + 5, dev=dev, lo=-256, hi=256) if ('r' in epi.split('+') or 'ip' in epi.split('+')) else None
    return bias, rb, R


@pytest.mark.parametrize('case', NT_CASES, ids=[c[0] for c in NT_CASES])
def test_gemm_nt_exact(ops, dev, case):
    cid, g, N, Cin, opts, want, epi, form = case
    G = geom(ops, g)
    M, K, Mi = G.B * G.Hout * G.Wout, G.ksize * G.ksize * Cin, G.B * G.Hin * G.Win
    seed = sum(map(ord, cid)) % 10007
    X = ints(Mi, Cin, seed=seed, dev=dev)
    Wt = ints(N, K, seed=seed + 1, dev=dev)
    bias, rb, R = _epi_inputs(epi, M, N, G.B, dev, seed)
    parts = epi.split('+')
    alpha = 0.5 if 'a' in parts else 1.0
    odt = F32 if 'f32' in parts else BF
    ref = gather(X, G) @ Wt.double().t() * alpha
    if bias is not None:
        ref += bias.double()
    if rb is not None:
        ref += rb.double().repeat_interleave(G.Hout * G.Wout, 0)
    if R is not None:
        ref += R.double()
    want_out = ref.to(odt)
    A, Wv = in_view(X), row_slice(Wt.to(BF))
    bv = vec_slice(bias) if bias is not None else None
    rbv = in_view(rb) if rb is not None else None
    ws = torch.full((splitk_floats(M, N),), NAN, device=dev) if form == 'splitk' else None
    old = ops.SPLITK_WS
    outs = []
    try:
        ops.SPLITK_WS = ws
        with options(ops, opts):
            if want is not None:
                got_v = ops._lib.load().da_gemm_nt_variant_for(M, N, K, Cin, ws.numel() if ws is not None else 0)
                assert got_v == want, f'{cid}: runs variant {got_v}, the table says {want}'
            for rep in range(1 if 'ip' in parts else 2):
                buf, o, keep = out_view(M, N, odt, dev, seed + 10 + rep, fill=None if 'ip' in parts else NAN)
                if 'ip' in parts:
                    o.copy_(R)
                    keep = buf.clone()
                    rv = o
                else:
                    rv = in_view(R) if R is not None else None
                ops.gemm_nt(A, Wv, o, G, bias=bv, rowbias=rbv, residual=rv, alpha=alpha)
                torch.cuda.synchronize()
                outs.append((buf, o, keep))
    finally:
        ops.SPLITK_WS = old
    if form == 'splitk':
        assert bool((~torch.isnan(ws)).any()), f'{cid}: the split-K workspace was not written (no split)'
    for buf, o, keep in outs:
        assert torch.equal(o, want_out), f'{cid}: ' + first_mismatch(o, want_out)
        assert_pads_kept(buf, keep, M, N, cid)
    if len(outs) == 2:
        assert bits_equal(outs[0][1], outs[1][1]), f'{cid}: a repeated call differs'


# ------------------------------------------------------------------------------------------------ da_gemm_tn_wgrad cases
def _tn_cases():
    cases = []   # (id, geometry, N, Cin, opts, variant the query must report, workspace?, dbias?, form)

    def add(form, g, N, Cin, opts, want, ws, db=True):
        gid = '-'.join(str(v) for v in g)
        oid = '-'.join(f'{k.replace("gemm_tn_", "")}{v}' for k, v in opts.items())
        cases.append((f'{form}-{gid}-n{N}-c{Cin}-{oid}' + ('-ws' if ws else '') + ('-db' if db else ''), g, N, Cin, opts,
                      want, ws, db, form))

    Ns, Cins = (8, 72, 184, 200, 320), (8, 64, 72, 320)
    small = (('conv', 3, 1, 1), ('conv', 2, 2, 2), ('conv', 1, 1, 7), ('conv', 5, 3, 5), ('c1', 2, 4, 4), ('down', 2, 2, 6),
             ('down', 2, 3, 5), ('up', 3, 1, 1), ('up', 2, 3, 5), ('lin', 1), ('lin', 255))
    for i, g in enumerate(small):   # v1, one split
        add('v1', g, Ns[i % 5], Cins[i % 4], {'gemm_tn_variant': 1}, 1, i % 2 == 0, i % 3 != 2)
    split = (('conv', 3, 9, 11), ('conv', 7, 8, 9), ('lin', 1000), ('down', 5, 18, 14), ('up', 3, 5, 7), ('c1', 9, 7, 5))
    for i, g in enumerate(split):   # v1, split over pixel ranges: slabs with a workspace, atomics without
        add('v1slab', g, Ns[(i + 1) % 5], Cins[(i + 2) % 4], {'gemm_tn_variant': 1}, 1, True, i % 3 != 1)
        add('v1atomic', g, Ns[(i + 3) % 5], Cins[(i + 1) % 4], {'gemm_tn_variant': 1}, 1, False, i % 3 != 0)
    generic = (('conv', 3, 9, 11), ('conv', 5, 3, 5), ('down', 2, 6, 10), ('down', 2, 3, 5), ('up', 3, 1, 1), ('up', 2, 3, 5),
               ('lin', 1000), ('c1', 2, 4, 4), ('conv', 1, 1, 7))
    for i, g in enumerate(generic):   # v2 with the generic gather (period 0)
        add('v2', g, Ns[(i + 2) % 5], Cins[i % 4], {'gemm_tn_variant': 2}, 2, i % 2 == 0, i % 3 != 1)
    fast = (('conv', 4, 4, 4), ('conv', 1, 8, 8), ('c1', 4, 4, 4), ('down', 4, 8, 8), ('down', 1, 16, 16), ('up', 4, 2, 2),
            ('up', 1, 4, 4), ('lin', 64), ('lin', 1024 + 64), ('conv', 2, 16, 24))
    for i, g in enumerate(fast):   # v2 FAST (border period)
        add('fast', g, Ns[(i + 4) % 5], Cins[(i + 1) % 4], {'gemm_tn_variant': 3}, 3, i % 2 == 1, i % 3 != 2)
    for g, N, Cin, v in ((('lin', 2048 + 448), 72, 64, 3), (('lin', 2048 + 40), 200, 72, 2), (('conv', 2, 24, 24), 320, 64, 3),
                         (('conv', 3, 17, 23), 184, 8, 2)):   # v2 split: few tiles, M >= 1024
        add('v2slab', g, N, Cin, {'gemm_tn_variant': v}, v, True)
        add('v2atomic', g, N, Cin, {'gemm_tn_variant': v}, v, False)
    for ring in (4, 5):   # ring form of the FAST linears
        for i, (M, N, Cin) in enumerate(((64, 8, 8), (1024, 200, 72), (2048 + 64, 320, 320), (4096, 72, 64))):
            add(f'ring{ring}', ('lin', M), N, Cin, {'gemm_tn_variant': 3, 'gemm_tn_ring': ring}, 3, i % 2 == 0, i != 1)
    return cases


TN_CASES = _tn_cases()


def tn_variant(ops, case):
    from diffusion_amd import _lib
    _, g, N, Cin, opts, *_ = case
    G = geom(ops, g)
    with options(ops, opts):
        return _lib.load().da_gemm_tn_variant_for(G.B * G.Hout * G.Wout, N, Cin, G.Hin, G.Win, G.Hout, G.Wout, G.ksize, G.mode)


TN_WS_FLOATS = 4 << 20


@pytest.mark.parametrize('overwrite', [0, 1])
@pytest.mark.parametrize('case', TN_CASES, ids=[c[0] for c in TN_CASES])
def test_wgrad_exact(ops, dev, case, overwrite):
    cid, g, N, Cin, opts, want, use_ws, use_db, form = case
    G = geom(ops, g)
    M, Kt, Mi = G.B * G.Hout * G.Wout, G.ksize * G.ksize * Cin, G.B * G.Hin * G.Win
    seed = sum(map(ord, cid)) % 10007
    dY = ints(M, N, seed=seed, dev=dev)
    X = ints(Mi, Cin, seed=seed + 1, dev=dev)
    ref = dY.double().t() @ gather(X, G)
    refb = dY.double().sum(0)
    prior = ints(N * Kt, seed=seed + 2, dev=dev, lo=-1000, hi=1000)
    priorb = ints(N, seed=seed + 3, dev=dev, lo=-1000, hi=1000)
    if not overwrite:
        ref = ref + prior.double().view(N, Kt)
        refb = refb + priorb.double()
    ws = torch.full((TN_WS_FLOATS,), NAN, device=dev) if use_ws else None
    got_v = tn_variant(ops, case)
    assert got_v == want, f'{cid}: runs variant {got_v}, the table says {want}'
    dYv, Xv = in_view(dY), in_view(X)
    old = ops.SPLITK_WS
    outs = []
    try:
        ops.SPLITK_WS = ws
        with options(ops, {**opts, 'grad_overwrite': overwrite}):
            for rep in range(2):
                dW = vec_slice(torch.full_like(prior, NAN) if overwrite else prior.clone(), pad=64)
                db = vec_slice(torch.full_like(priorb, NAN) if overwrite else priorb.clone(), pad=64) if use_db else None
                scratch = torch.full((256 * N * 2,), NAN, device=dev)
                ops.gemm_tn_wgrad(dYv, Xv, dW, G, dbias=db, scratch=scratch)
                torch.cuda.synchronize()
                outs.append((dW, db))
    finally:
        ops.SPLITK_WS = old
    if form in ('v1slab', 'v2slab'):
        assert bool((~torch.isnan(ws)).any()), f'{cid}: the split workspace was not written (no split)'
    for dW, db in outs:
        base = dW.storage_offset()
        whole = torch.as_strided(dW, (dW.numel() + 128,), (1,), base - 64)
        assert bool(torch.isnan(whole[:64]).all() and torch.isnan(whole[-64:]).all()), f'{cid}: dW written outside its slice'
        got = dW.view(N, Kt)
        assert torch.equal(got, ref.float()), f'{cid} dW: ' + first_mismatch(got, ref.float())
        if db is not None:
            assert torch.equal(db, refb.float()), f'{cid} dbias: ' + first_mismatch(db.view(1, -1), refb.float().view(1, -1))
    assert bits_equal(outs[0][0], outs[1][0]), f'{cid}: a repeated call differs'


# ------------------------------------------------------------------------------------------------ fused GEGLU
GEGLU_CASES = [('fwd', 1, 160, 64), ('fwd', 255, 320, 320), ('fwd', 257, 640, 640), ('fwd', 785, 160, 320), ('fwd', 513, 320, 64),
               ('bwd', 1, 320, 64), ('bwd', 255, 640, 320), ('bwd', 257, 320, 640), ('bwd', 785, 640, 64)]


@pytest.mark.parametrize('case', GEGLU_CASES, ids=['-'.join(map(str, c)) for c in GEGLU_CASES])
def test_geglu_exact(ops, dev, case):
    """fused GEGLU forward: F = A W^T + bias exact; G bit-identical to da_geglu_fwd(F).  Backward: dF bit-identical to
    da_geglu_bwd(F, bf16(dY Wt^T)) with the product exact before its one rounding"""
    kind, M, inner, K = case
    seed = M + inner + K + (kind == 'bwd')
    if kind == 'fwd':
        A, Wt = ints(M, K, seed=seed, dev=dev), ints(2 * inner, K, seed=seed + 1, dev=dev)
        bias = ints(2 * inner, seed=seed + 2, dev=dev, lo=-64, hi=64)
        ref = (A.double() @ Wt.double().t() + bias.double()).to(BF)
        outs = []
        for rep in range(2):
            fb, Fv, fk = out_view(M, 2 * inner, BF, dev, seed + 3 + rep)
            gb, Gv, gk = out_view(M, inner, BF, dev, seed + 5 + rep)
            ops.gemm_nt_geglu(in_view(A), row_slice(Wt.to(BF)), Fv, Gv, vec_slice(bias))
            torch.cuda.synchronize()
            assert torch.equal(Fv, ref), 'F: ' + first_mismatch(Fv, ref)
            g2 = torch.empty(M, inner, device=dev, dtype=BF)
            ops.geglu_fwd(Fv, g2)
            assert bits_equal(Gv, g2), 'G differs from the two-kernel path'
            assert_pads_kept(fb, fk, M, 2 * inner, 'F')
            assert_pads_kept(gb, gk, M, inner, 'G')
            outs.append((Fv, Gv))
        assert bits_equal(outs[0][1], outs[1][1])
    else:
        dY, Wt = ints(M, K, seed=seed, dev=dev), ints(inner, K, seed=seed + 1, dev=dev)
        Fs = torch.randn(M, 2 * inner, generator=gen(seed + 2, dev), device=dev).mul(2).to(BF)
        d = (dY.double() @ Wt.double().t()).to(BF)
        ref = torch.empty(M, 2 * inner, device=dev, dtype=BF)
        ops.geglu_bwd(Fs, d, ref)
        outs = []
        for rep in range(2):
            ob, dF, ok = out_view(M, 2 * inner, BF, dev, seed + 3 + rep)
            ops.gemm_nt_geglu_bwd(in_view(dY), row_slice(Wt.to(BF)), in_view(Fs), dF)
            torch.cuda.synchronize()
            assert bits_equal(dF, ref), 'dF differs from the two-kernel path: ' + first_mismatch(dF, ref)
            assert_pads_kept(ob, ok, M, 2 * inner, 'dF')
            outs.append(dF)
        assert bits_equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ float inputs
# (api, geometry, N, Cin, opts, split-K workspace?, epilogue)
FLOAT_FORMS = [
    ('nt', ('lin', 1169), 648, 1344, {'gemm_nt_variant': 1}, False, 'b+r'),
    ('nt', ('conv', 5, 3, 5), 200, 320, {'gemm_nt_variant': 4}, False, 'b+rb+r'),
    ('nt', ('lin', 785), 648, 640, {'gemm_nt_variant': 12}, False, 'b'),
    ('nt', ('conv', 2, 4, 4), 648, 1280, {'gemm_nt_variant': 12, 'gemm_nt_korder': 0}, False, 'rb+r'),
    ('nt', ('up', 2, 3, 5), 328, 320, {'gemm_nt_variant': 15}, False, 'f32+b'),
    ('nt', ('lin', 1169), 264, 1344, {'gemm_nt_variant': 18}, False, 'b+r'),
    ('nt', ('conv', 2, 4, 4), 320, 320, {}, True, 'b+rb+r'),
    ('nt', ('conv', 133, 8, 8), 1280, 64, {'gemm_nt_variant': 12, 'reserve_cus': 128}, False, 'b+rb+r'),
    ('nt', ('lin', 1169), 648, 1344, {'gemm_nt_stream': 2, 'gemm_nt_ws': 0}, False, 'b+r'),
    ('tn', ('conv', 7, 8, 9), 200, 72, {'gemm_tn_variant': 1}, True, ''),
    ('tn', ('lin', 1000), 320, 320, {'gemm_tn_variant': 1}, True, ''),
    ('tn', ('conv', 3, 9, 11), 320, 64, {'gemm_tn_variant': 2}, True, ''),
    ('tn', ('lin', 2048 + 64), 320, 320, {'gemm_tn_variant': 3}, True, ''),
    ('tn', ('lin', 2048 + 64), 200, 72, {'gemm_tn_variant': 3, 'gemm_tn_ring': 4}, True, ''),
]
KINDS = ('randn', 'rows', 'cancel')
FLOAT_CASES = [(f'{f[0]}-{"-".join(map(str, f[1]))}-n{f[2]}-c{f[3]}-' + '-'.join(f'{k}{v}' for k, v in f[4].items()) +
                ('-ws' if f[5] else '') + f'-{kind}', f, kind) for f in FLOAT_FORMS for kind in KINDS]


def ulp(ref, dtype):
    """one unit in the last place of `dtype` at |ref| (float64)"""
    _, e = torch.frexp(ref)
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - (8 if dtype == BF else 24)))


def float_operands(kind, rows, C, seed, dev):
    """[rows, C] N(0,1); 'rows': each row scaled by 10^U(-3, 3); 'cancel': the two channel halves equal (with 'cancel_w'
    the partner's weights are negated, so every product pair nearly cancels)"""
    x = torch.randn(rows, C, generator=gen(seed, dev), device=dev)
    if kind == 'rows':
        x = x * torch.pow(10.0, torch.rand(rows, 1, generator=gen(seed + 1, dev), device=dev) * 6 - 3)
    if kind == 'cancel':
        x[:, C // 2:] = x[:, :C // 2]
    return x.to(BF).float()


def cancel_w(Wt, taps, Cin, seed, dev):
    """weights of tap t, channel c + Cin/2 = -(weights of channel c) + 2^-8 noise"""
    w = Wt.view(Wt.shape[0], taps, Cin)
    h = Cin // 2
    w[:, :, h:] = -w[:, :, :h] + torch.randn(w[:, :, :h].shape, generator=gen(seed, dev), device=dev) * 2 ** -8
    return w.reshape(Wt.shape).to(BF).float()


def check_float(api, kind, out, ref, absprod, K, odt, what):
    """per element: |out - ref| <= ulp + c2 * 2^-24 * K * |A||W|; rel-L2 whole and per 128 x 128 block"""
    err = (out.double() - ref).abs()
    assert bool(torch.isfinite(err).all()), f'{what}: non-finite output'
    c2 = ((err - ulp(ref, odt)).clamp(min=0) / (2.0 ** -24 * K * absprod).clamp(min=1e-300)).max().item()
    rel = (err.norm() / ref.norm().clamp(min=1e-300)).item()
    Mr, Nr = ref.shape
    blk = 0.0
    for m0 in range(0, Mr, 128):
        for n0 in range(0, Nr, 128):
            r = ref[m0:m0 + 128, n0:n0 + 128]
            if r.norm() > 0:
                blk = max(blk, (err[m0:m0 + 128, n0:n0 + 128].norm() / r.norm()).item())
    for q, v in (('c2', c2), ('rel', rel), ('block', blk)):
        assert _margin(f'{api}.{kind}.{q}', v), f'{what}: {q} {v:.3e} > bound {BOUNDS[f"{api}.{kind}.{q}"]:.3e}'


@pytest.mark.parametrize('case', FLOAT_CASES, ids=[c[0] for c in FLOAT_CASES])
def test_gemm_float_bounds(ops, dev, case):
    cid, (api, g, N, Cin, opts, use_ws, epi), kind = case
    G = geom(ops, g)
    M, K, Mi = G.B * G.Hout * G.Wout, G.ksize * G.ksize * Cin, G.B * G.Hin * G.Win
    seed = sum(map(ord, cid)) % 10007
    old = ops.SPLITK_WS
    try:
        if api == 'nt':
            X = float_operands(kind, Mi, Cin, seed, dev)
            Wt = torch.randn(N, K, generator=gen(seed + 2, dev), device=dev).mul(K ** -0.5).to(BF).float()
            if kind == 'cancel':
                Wt = cancel_w(Wt, G.ksize * G.ksize, Cin, seed + 3, dev)
            bias, rb, R = [None if t is None else t.to(BF).float() / 8 for t in _epi_inputs(epi, M, N, G.B, dev, seed)]
            parts = epi.split('+')
            odt = F32 if 'f32' in parts else BF
            Ag = gather(X, G)
            ref = Ag @ Wt.double().t()
            absprod = Ag.abs() @ Wt.double().abs().t()
            for t in (bias, None if rb is None else rb.repeat_interleave(G.Hout * G.Wout, 0), R):
                if t is not None:   # (the bias may start the accumulation: its magnitude counts in every partial sum)
                    ref += t.double()
                    absprod += t.double().abs()
            ops.SPLITK_WS = torch.full((splitk_floats(M, N),), NAN, device=dev) if use_ws else None
            buf, o, keep = out_view(M, N, odt, dev, seed + 10)
            with options(ops, opts):
                ops.gemm_nt(in_view(X), row_slice(Wt.to(BF)), o, G, bias=vec_slice(bias) if bias is not None else None,
                            rowbias=in_view(rb) if rb is not None else None, residual=in_view(R) if R is not None else None)
            torch.cuda.synchronize()
            assert_pads_kept(buf, keep, M, N, cid)
            check_float('nt', kind, o, ref, absprod, K, odt, cid)
        else:
            dY = float_operands('rows' if kind == 'rows' else 'randn', M, N, seed, dev)
            X = torch.randn(Mi, Cin, generator=gen(seed + 2, dev), device=dev).to(BF).float()
            if kind == 'cancel':   # pixel rows in pairs (m, m + M/2) with equal X and opposite dY (+ 2^-8 noise)
                h = M // 2
                X[h:2 * h] = X[:h]
                dY[h:2 * h] = (-dY[:h] + torch.randn(h, N, generator=gen(seed + 3, dev), device=dev) * 2 ** -8).to(BF).float()
            Ag = gather(X, G)
            ref = dY.double().t() @ Ag
            absprod = dY.double().abs().t() @ Ag.abs()
            ops.SPLITK_WS = torch.full((TN_WS_FLOATS,), NAN, device=dev) if use_ws else None
            dW = torch.full((N * K,), NAN, device=dev)
            with options(ops, {**opts, 'grad_overwrite': 1}):
                ops.gemm_tn_wgrad(in_view(dY), in_view(X), dW, G)
            torch.cuda.synchronize()
            check_float('tn', kind, dW.view(N, K), ref, absprod, M, F32, cid)
    finally:
        ops.SPLITK_WS = old
