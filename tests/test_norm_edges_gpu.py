"""GroupNorm and LayerNorm at their edges: every kernel form of norms.hip against a float64 reference, at the shapes,
strides, tails and inputs where norm kernels go wrong.

GroupNorm forms (da_groupnorm_fwd / _bwd), forced with da_set_option:

    form      | gn_resident | gn_resident_form | kernels
    multipass | 0           | -                | chan_reduce -> gn_finalize<BWD> -> gn_apply2, pick_chunks(B, HW) pixel chunks
    res0/1/2  | 1           | 0 / 1 / 2        | gn_res_fwd<NL> / gn_res_bwd<NL, threads> where gn_res_plan takes the shape

(the resident forms also set gn_resident_min_slab = 0).  GN_CASES pins, for every shape, the instantiation each forced form
runs, read back through da_groupnorm_plan_for; tests/test_abi_and_host.py checks the table on the CPU, so a change of the
plan cannot move a case to another instantiation unnoticed.  Together the cases run every forward NL, every backward
(threads, NL) pair, peers8 on and off, one and several parts per image, line-aligned and unaligned slabs.

Reference: float64 autograd on the bf16-rounded inputs.  dy = a + b * xhat + noise with a, b drawn per (image, group) or
per row, so the projection terms c1 = mean(gamma dz) and c2 = mean(gamma dz xhat) are as large as dx itself.  Every case
asserts:
  * all outputs finite: y, dx, mean_rstd are NaN-prefilled (every element written), scratch and coef too (nothing unwritten
    is read);
  * rel-L2 over the whole tensor AND per (image, group) / per row; mean_rstd against float64 as |d mean| / sqrt(var + eps)
    and |d rstd| / rstd; dgamma / dbeta rel-L2;
  * outputs are column views inside wider buffers with sentinel pad columns and rows, unchanged afterwards; inputs are
    column views whose pad columns hold NaN; dgamma / dbeta are slices with 16 sentinel floats on either side;
  * dgamma / dbeta add onto non-zero prior contents; with grad_overwrite = 1 they are written over NaN, and prior + written
    equals added, bit for bit;
  * a repeat call is bit-identical.
Bounds: every bound is at most 2x the worst margin measured on MI355X (DESIGN.md records them); DA_PARITY_MARGINS=<path>
writes the margins of a run (tests/parity_margins.py).
"""
import contextlib
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float('nan')
PAD_L, PAD_R = 8, 8   # left pad columns of every view (16 bytes) and sentinel rows after every output

# name -> bound (rel-L2 unless noted); 'gn256.*': GroupNorm with every group at |mean| / sigma = 256 (one-pass variance)
BOUNDS = {   # bound: worst measured on MI355X
    'gn.y': 3.3e-3, 'gn.y.group': 6.1e-3, 'gn.dx': 8.6e-3, 'gn.dx.group': 1.5e-2,
    # 1.69e-03, 3.05e-03, 4.31e-03, 7.86e-03
    'gn.mean': 1.4e-5, 'gn.rstd': 1.0e-3, 'gn.dgamma': 3.0e-4, 'gn.dbeta': 5.4e-5,
    # 7.20e-06, 5.11e-04, 1.51e-04, 2.73e-05
    'gn256.y': 6.0e-3, 'gn256.y.group': 1.3e-2, 'gn256.dx': 8.7e-3, 'gn256.dx.group': 2.6e-2,
    # 3.05e-03, 6.57e-03, 4.40e-03, 1.34e-02
    'gn256.mean': 3.7e-5, 'gn256.rstd': 1.1e-2, 'gn256.dgamma': 6.7e-3, 'gn256.dbeta': 1.1e-3,
    # 1.87e-05, 5.77e-03, 3.36e-03, 5.94e-04
    'ln.y': 3.8e-3, 'ln.y.row': 7.0e-3, 'ln.dx': 3.6e-3, 'ln.dx.row': 7.0e-3,
    # 1.91e-03, 3.52e-03, 1.82e-03, 3.51e-03
    'ln.mean': 3.4e-5, 'ln.rstd': 6.3e-7, 'ln.dgamma': 1.0e-5, 'ln.dbeta': 1.9e-7,
    # 1.71e-05, 3.19e-07, 5.09e-06, 9.96e-08
}
_WORST = {}


def _margin(name, value):
    """keep the worst value of each bounded quantity and assert it"""
    _WORST[name] = max(_WORST.get(name, 0.0), value)
    if os.environ.get('DA_PARITY_MARGINS'):
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from parity_margins import record
        record('norm_edges', tolerances=BOUNDS, **_WORST)
    return value < BOUNDS[name]


@pytest.fixture(scope='module')
def ops(dev):
    from diffusion_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------ GroupNorm plan table
FORMS = {'multipass': (0, 0), 'res0': (1, 0), 'res1': (1, 1), 'res2': (1, 2)}   # gn_resident, gn_resident_form
# the resident forms only where every CU gets a workgroup: what the default options (192 workgroups, 64-KB slabs) pick at
# batch 64 on some levels, where gn_resident = 1 takes a wider slab
WIDE_FORMS = {'res0w': (256, 0), 'res1w': (256, 1), 'res2w': (256, 2)}


@contextlib.contextmanager
def gn_form(ops, form):
    """force a GroupNorm form; the defaults are restored afterwards"""
    res, rf = {**FORMS, **WIDE_FORMS}[form]
    try:
        ops.set_option('gn_resident', res)
        ops.set_option('gn_resident_form', rf)
        ops.set_option('gn_resident_min_slab', 0)
        yield
    finally:
        ops.set_option('gn_resident', 192)
        ops.set_option('gn_resident_form', 0)
        ops.set_option('gn_resident_min_slab', 64 * 1024)


def row_stride(C, aligned):
    """row stride of every tensor of a case: PAD_L columns left, >= 8 right; a multiple of 64 elements (128-B lines) or not"""
    r = 8
    while ((C + PAD_L + r) % 64 == 0) != bool(aligned):
        r += 8
    return C + PAD_L + r


# (B, HW, C, G, line-aligned rows, eps, silu, Radd): forced-resident targets as 'threads x NL' with '/pN' for N parts per
# image and '+p8' for the 8-apart placement, 'mp' where gn_res_plan declines the shape and the multi-pass kernels run
GN_CASES = [
    # B = 1, HW = 1000: 62 pixel chunks of 17 px in the multi-pass form, the last three empty
    ((1, 1000, 320, 32, 0, 1e-5, 1, 1), '1024x21/p2', ('1024x11/p4', '1024x11/p4', '768x14/p4')),
    ((2, 1, 320, 32, 1, 1e-6, 0, 0), '1024x1', ('1024x1', '1024x1', '1024x1')),
    ((3, 7, 64, 32, 0, 1e-5, 1, 0), 'mp', ('mp', 'mp', 'mp')),             # 64 unaligned channels: multi-pass only
    ((2, 16, 1280, 32, 1, 1e-6, 1, 1), '1024x3', ('768x11', '1024x3', '768x11')),
    ((4, 17, 640, 32, 0, 1e-5, 0, 1), '1024x2', ('768x11', '1024x2', '768x11')),
    ((8, 256, 96, 32, 1, 1e-6, 1, 0), '1024x4', ('768x11', '1024x4', '768x11')),
    ((8, 1024, 320, 32, 0, 1e-5, 1, 1), '1024x21/p2+p8', ('768x14/p4+p8', '1024x11/p4+p8', '768x14/p4+p8')),
    ((2, 2304, 640, 32, 1, 1e-6, 1, 0), 'mp', ('mp', 'mp', 'mp')),        # 2304 px do not fit
    ((1, 4096, 256, 32, 1, 1e-5, 0, 1), 'mp', ('mp', 'mp', 'mp')),
    ((2, 100, 160, 32, 0, 1e-6, 1, 1), '1024x2', ('1024x2', '1024x2', '1024x2')),
    ((3, 200, 480, 32, 0, 1e-5, 1, 0), '1024x16', ('768x11/p2', '1024x6/p2', '768x11/p2')),
    ((2, 64, 960, 32, 1, 1e-6, 0, 1), '1024x8', ('1024x8', '1024x8', '1024x8')),
    ((1, 64, 1920, 32, 0, 1e-5, 1, 1), '1024x16', ('1024x8/p2', '1024x8/p2', '1024x8/p2')),
    ((1, 16, 2560, 32, 1, 1e-6, 1, 0), '1024x3/p2', ('768x11', '1024x3/p2', '768x11')),
    ((2, 49, 64, 64, 1, 1e-5, 0, 0), '1024x1', ('768x11', '1024x1', '768x11')),        # one channel per group
    ((2, 300, 120, 12, 0, 1e-6, 1, 1), '1024x6', ('768x11', '1024x6', '768x11')),      # G = 12: not a multiple of 8
    ((4, 256, 640, 16, 1, 1e-5, 1, 0), '1024x11/p2', ('768x14/p2', '1024x11/p2', '768x14/p2')),
    ((2, 127, 64, 32, 1, 1e-6, 1, 1), '1024x1', ('1024x1', '1024x1', '1024x1')),       # P - 1 (P = 128)
    ((2, 129, 64, 32, 1, 1e-5, 0, 1), '1024x2', ('768x11', '1024x2', '768x11')),       # P + 1
    ((8, 199, 320, 32, 0, 1e-6, 1, 0), '1024x8', ('1024x8', '1024x8', '1024x8')),      # 8 P - 1 (P = 25)
    ((8, 201, 320, 32, 0, 1e-5, 0, 1), '1024x11', ('768x11', '1024x11', '768x11')),    # 8 P + 1
    ((2, 1000, 160, 32, 0, 1e-6, 0, 0), '1024x21', ('1024x11/p2', '1024x11/p2', '768x14/p2')),
    ((8, 512, 160, 32, 1, 1e-5, 1, 1), '1024x11', ('768x14', '1024x11', '768x14')),
    ((2, 600, 320, 32, 1, 1e-6, 1, 0), '1024x16/p2', ('1024x6/p4', '1024x6/p4', '1024x6/p4')),
    ((2, 1024, 64, 32, 1, 1e-5, 1, 1), '1024x8', ('1024x8', '1024x8', '1024x8')),
    ((1, 1500, 96, 32, 1, 1e-6, 0, 1), '1024x21', ('mp', 'mp', 'mp')),   # resident forward, multi-pass backward
    ((2, 255, 96, 32, 0, 1e-5, 1, 0), '1024x3', ('1024x3', '1024x3', '1024x3')),
    ((2, 255, 160, 32, 1, 1e-6, 0, 1), '1024x6', ('1024x6', '1024x6', '1024x6')),
    ((8, 1024, 960, 32, 1, 1e-5, 1, 1), '1024x16/p8+p8', ('mp', 'mp', 'mp')),
    ((16, 16, 2560, 32, 0, 1e-6, 1, 1), '1024x3/p2+p8', ('768x11', '1024x3/p2+p8', '768x11')),
    ((2, 100, 320, 1, 1, 1e-5, 1, 1), '1024x4', ('1024x4', '1024x4', '1024x4')),       # G = 1: one group of 320 channels
    ((3, 40, 640, 4, 0, 1e-6, 0, 1), '1024x4', ('768x11', '1024x4', '768x11')),        # G = 4: 160 channels per group
]


def plan_label(p):
    if p['form'] != 'resident':
        return 'mp'
    return (f"{p['threads']}x{p['nl']}" + (f"/p{p['parts']}" if p['parts'] > 1 else '') +
            ('+p8' if p['peers8'] else ''))


def gn_plan(ops, case, form, bwd):
    """what da_groupnorm_fwd / _bwd runs for a GN_CASES shape under a forced form"""
    B, HW, C, G, aligned = case[:5]
    ld = row_stride(C, aligned)
    with gn_form(ops, form):
        return ops.groupnorm_plan(B, HW, C, G, ld, ld, bwd=bwd)


def gn_target(entry, form, bwd):
    """the table's label for a form: the multi-pass form always runs the multi-pass kernels"""
    _, fwd, bwds = entry
    if form == 'multipass':
        return 'mp'
    return bwds[int(form[-1])] if bwd else fwd


def assert_gn_plans(ops, entry, form):
    for bwd in (False, True):
        got = plan_label(gn_plan(ops, entry[0], form, bwd))
        want = gn_target(entry, form, bwd)
        assert got == want, f'{entry[0]} {form} {"bwd" if bwd else "fwd"}: runs {got}, the table says {want}'


def gn_id(entry):
    B, HW, C, G, al, eps, silu, radd = entry[0]
    return f'b{B}-hw{HW}-c{C}-g{G}' + ('-al' if al else '') + f'-eps{eps:.0e}' + ('-silu' if silu else '') + \
        ('-radd' if radd else '')


# ------------------------------------------------------------------------------------------------ buffers
def randn(*shape, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=dev)


def in_view(t, ld):
    """t [rows, C] as a column view at PAD_L of a [rows, ld] bf16 buffer whose other columns hold NaN"""
    buf = torch.full((t.shape[0], ld), NAN, device=t.device, dtype=BF)
    buf[:, PAD_L:PAD_L + t.shape[1]] = t
    return buf[:, PAD_L:PAD_L + t.shape[1]]


def out_view(rows, C, ld, dev, seed):
    """a NaN-filled [rows, C] bf16 view at PAD_L of a [rows + PAD_R, ld] buffer of random sentinels:
    (buffer, view, copy of the buffer)"""
    buf = randn(rows + PAD_R, ld, seed=seed, dev=dev).to(BF)
    view = buf[:rows, PAD_L:PAD_L + C]
    view.fill_(NAN)
    return buf, view, buf.clone()


def check_sentinels(buf, before, rows, C, what):
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    keep[:rows, PAD_L:PAD_L + C] = False
    assert torch.equal(buf.view(torch.int16)[keep], before.view(torch.int16)[keep]), f'{what}: wrote outside its view'


def f32_view(n, dev, seed, fill):
    """a contiguous fp32[n] slice with 16 random sentinel floats on either side, holding `fill` (a tensor or NaN)"""
    buf = randn(n + 32, seed=seed, dev=dev)
    view = buf[16:16 + n]
    if isinstance(fill, torch.Tensor):
        view.copy_(fill)
    else:
        view.fill_(fill)
    return buf, view, buf.clone()


def check_f32_sentinels(buf, before, n, what):
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    keep[16:16 + n] = False
    assert torch.equal(buf.view(torch.int32)[keep], before.view(torch.int32)[keep]), f'{what}: wrote outside its slice'


# ------------------------------------------------------------------------------------------------ checks
def rel_l2(a, r):
    return ((a.double() - r.double()).norm() / r.double().norm()).item()


def check(got, ref, name, what, parts=None):
    """finite; rel-L2 over the whole tensor < BOUNDS[name]; with parts (a function that reshapes to [nparts, -1]) rel-L2 of
    every part < BOUNDS[name + '.group' | '.row']"""
    g = got.double()
    bad = ~torch.isfinite(g)
    assert not bad.any(), f'{what}: {int(bad.sum())} non-finite values, first at {tuple(bad.nonzero()[0].tolist())}'
    e = rel_l2(g, ref)
    assert _margin(name, e), f'{what}: rel-L2 {e:.3e} >= {BOUNDS[name]}'
    if parts is not None:
        pname, fn = parts
        d, r = fn(g - ref.double()), fn(ref.double())
        per = d.norm(dim=1) / r.norm(dim=1)
        worst, at = per.max().item(), per.argmax().item()
        assert _margin(f'{name}.{pname}', worst), \
            f'{what}: {pname} {at} rel-L2 {worst:.3e} >= {BOUNDS[name + "." + pname]}'


def check_stats(mr, mean, rstd, name, what):
    """mean_rstd [n][2] against float64 mean, rstd [n]: |d mean| * rstd (|d mean| / sqrt(var + eps)), |d rstd| / rstd"""
    m = mr.double().reshape(-1, 2)
    assert torch.isfinite(m).all(), f'{what}: non-finite mean_rstd'
    em = ((m[:, 0] - mean.reshape(-1)).abs() * rstd.reshape(-1)).max().item()
    er = ((m[:, 1] - rstd.reshape(-1)).abs() / rstd.reshape(-1)).max().item()
    assert _margin(f'{name}.mean', em), f'{what}: |d mean| / sigma {em:.3e} >= {BOUNDS[name + ".mean"]}'
    assert _margin(f'{name}.rstd', er), f'{what}: |d rstd| / rstd {er:.3e} >= {BOUNDS[name + ".rstd"]}'


# ------------------------------------------------------------------------------------------------ inputs
def hostile_params(k, eps):
    """(mean, sigma) of the k-th hostile kind: a constant group / row, variance 0.1 eps, eps and 10 eps at mean 0,
    |mean| / sigma = 16 and 64, magnitude ~1e3, an ordinary one"""
    return [(0.0, 0.0), (0.0, math.sqrt(0.1 * eps)), (0.0, math.sqrt(eps)), (0.0, math.sqrt(10 * eps)), (16.0, 1.0),
            (-64.0, 1.0), (300.0, 1000.0), (0.5, 1.5)][k % 8]


def mixed(n, kind, eps, seed, dev):
    """per-part (mean, sigma) [n] for 'ordinary' (mean ~ N(0.5, 1), sigma in [0.5, 2]), 'hostile' (the kinds above in turn)
    or 'shift256' (|mean| / sigma = 256, alternating sign)"""
    if kind == 'ordinary':
        u = torch.rand(n, generator=torch.Generator(device=dev).manual_seed(seed + 1), device=dev)
        return randn(n, seed=seed, dev=dev) + 0.5, 0.5 + 1.5 * u
    if kind == 'hostile':
        p = torch.tensor([hostile_params(k, eps) for k in range(n)], device=dev, dtype=torch.float32)
        return p[:, 0], p[:, 1]
    assert kind == 'shift256'
    sign = 1.0 - 2.0 * (torch.arange(n, device=dev) % 2)
    return 256.0 * sign, torch.ones(n, device=dev)


def correlated_dy(xhat, a, b, seed):
    """dy = a + b * xhat + 0.5 N(0, 1): c1 and c2 carry as much of dx as the noise"""
    return (a + b * xhat + 0.5 * randn(*xhat.shape, seed=seed, dev=xhat.device)).to(BF)


def affine(C, seed, dev):
    return 1 + 0.25 * randn(C, seed=seed, dev=dev), 0.25 * randn(C, seed=seed + 1, dev=dev)


# ------------------------------------------------------------------------------------------------ GroupNorm
def gn_inputs(B, HW, C, G, eps, radd, kind, seed, dev):
    """x, dy, Radd [B*HW, C] bf16 (dense), gamma, beta"""
    cpg = C // G
    mu, sd = mixed(B * G, kind, eps, seed, dev)
    x = (mu.reshape(B, 1, G, 1) + sd.reshape(B, 1, G, 1) * randn(B, HW, G, cpg, seed=seed + 2, dev=dev)).to(BF)
    xd = x.double()
    mean = xd.mean((1, 3), keepdim=True)
    xhat = (xd - mean) * ((xd - mean).square().mean((1, 3), keepdim=True) + eps).rsqrt()
    ab = randn(2, B, 1, G, 1, seed=seed + 3, dev=dev).double()
    dy = correlated_dy(xhat, ab[0], ab[1], seed + 4)
    gamma, beta = affine(C, seed + 5, dev)
    r = randn(B * HW, C, seed=seed + 6, dev=dev).to(BF) if radd else None
    return x.reshape(B * HW, C), dy.reshape(B * HW, C), r, gamma, beta


def gn_reference(x, dy, radd, gamma, beta, B, HW, C, G, eps, silu):
    cpg = C // G
    xd = x.double().reshape(B, HW, G, cpg).requires_grad_()
    gd, bd = gamma.double().requires_grad_(), beta.double().requires_grad_()
    mean = xd.mean((1, 3), keepdim=True)
    rstd = ((xd - mean).square().mean((1, 3), keepdim=True) + eps).rsqrt()
    z = (xd - mean) * rstd * gd.reshape(G, cpg) + bd.reshape(G, cpg)
    y = z * torch.sigmoid(z) if silu else z
    y.backward(dy.double().reshape(B, HW, G, cpg))
    dx = xd.grad.reshape(B * HW, C) + (radd.double() if radd is not None else 0)
    return dict(y=y.detach().reshape(B * HW, C), mean=mean.detach().reshape(B, G), rstd=rstd.detach().reshape(B, G),
                dx=dx, dgamma=gd.grad, dbeta=bd.grad)


def gn_groups(B, HW, C, G):
    return lambda t: t.reshape(B, HW, G, C // G).permute(0, 2, 1, 3).reshape(B * G, -1)


def gn_fwd(ops, x, gamma, beta, B, HW, C, G, eps, silu, ld, seed):
    dev = x.device
    ybuf, y, ybefore = out_view(B * HW, C, ld, dev, seed)
    mbuf, mr, mbefore = f32_view(B * G * 2, dev, seed + 1, NAN)
    ss = torch.full((B * C * 2,), NAN, device=dev)
    scratch = torch.full((ops.norm_scratch_floats(B, HW, C),), NAN, device=dev)
    ops.groupnorm_fwd(x, y, gamma, beta, mr, ss, scratch, B, HW, C, G, eps, silu)
    torch.cuda.synchronize()
    check_sentinels(ybuf, ybefore, B * HW, C, 'y')
    check_f32_sentinels(mbuf, mbefore, B * G * 2, 'mean_rstd')
    assert torch.isnan(ss).all(), 'scale_shift: written (the buffer is unused by every form)'
    return y, mr


def gn_bwd(ops, x, dy, radd, gamma, beta, mr, B, HW, C, G, silu, ld, seed, prior=None):
    """dx, dgamma, dbeta; prior = (dgamma0, dbeta0) adds onto them, None writes over NaN with grad_overwrite = 1"""
    dev = x.device
    dxbuf, dx, dxbefore = out_view(B * HW, C, ld, dev, seed)
    gbuf, dg, gbefore = f32_view(C, dev, seed + 1, prior[0] if prior else NAN)
    bbuf, db, bbefore = f32_view(C, dev, seed + 2, prior[1] if prior else NAN)
    coef = torch.full((B * G * 2,), NAN, device=dev)
    scratch = torch.full((ops.norm_scratch_floats(B, HW, C),), NAN, device=dev)
    try:
        ops.set_option('grad_overwrite', 0 if prior else 1)
        ops.groupnorm_bwd(x, dy, radd, dx, gamma, beta, mr, dg, db, coef, scratch, B, HW, C, G, silu)
        torch.cuda.synchronize()
    finally:
        ops.set_option('grad_overwrite', 0)
    check_sentinels(dxbuf, dxbefore, B * HW, C, 'dx')
    check_f32_sentinels(gbuf, gbefore, C, 'dgamma')
    check_f32_sentinels(bbuf, bbefore, C, 'dbeta')
    return dx, dg, db


def gn_check_fwd(y, mr, ref, B, HW, C, G, name, what):
    check(y, ref['y'], f'{name}.y', f'{what} y', ('group', gn_groups(B, HW, C, G)))
    check_stats(mr, ref['mean'], ref['rstd'], name, f'{what} mean_rstd')


def gn_check_bwd(dx, dg, db, ref, B, HW, C, G, name, what, prior=None):
    check(dx, ref['dx'], f'{name}.dx', f'{what} dx', ('group', gn_groups(B, HW, C, G)))
    check(dg - prior[0] if prior else dg, ref['dgamma'], f'{name}.dgamma', f'{what} dgamma')
    check(db - prior[1] if prior else db, ref['dbeta'], f'{name}.dbeta', f'{what} dbeta')


def gn_run_form(ops, dev, case, form, kind, seed, name='gn', ref=None, inputs=None):
    """one GroupNorm case under one forced form: forward twice, backward adding onto prior gradients and again writing
    them (grad_overwrite), every output against the reference; returns (y, mean_rstd, dx, dgamma, dbeta)"""
    B, HW, C, G, aligned, eps, silu, radd = case
    ld = row_stride(C, aligned)
    x, dy, r, gamma, beta = inputs or gn_inputs(B, HW, C, G, eps, radd, kind, seed, dev)
    ref = ref or gn_reference(x, dy, r, gamma, beta, B, HW, C, G, eps, silu)
    xv, dyv = in_view(x, ld), in_view(dy, ld)
    rv = in_view(r, ld) if r is not None else None
    what = f'{case} {form} {kind}'
    with gn_form(ops, form):
        y, mr = gn_fwd(ops, xv, gamma, beta, B, HW, C, G, eps, silu, ld, seed + 10)
        y2, mr2 = gn_fwd(ops, xv, gamma, beta, B, HW, C, G, eps, silu, ld, seed + 20)
        prior = (randn(C, seed=seed + 30, dev=dev), randn(C, seed=seed + 31, dev=dev))
        dx, dg, db = gn_bwd(ops, xv, dyv, rv, gamma, beta, mr, B, HW, C, G, silu, ld, seed + 40, prior)
        dx2, dg2, db2 = gn_bwd(ops, xv, dyv, rv, gamma, beta, mr, B, HW, C, G, silu, ld, seed + 50)
        dx3, dg3, db3 = gn_bwd(ops, xv, dyv, rv, gamma, beta, mr, B, HW, C, G, silu, ld, seed + 60)
    gn_check_fwd(y, mr, ref, B, HW, C, G, name, what)
    gn_check_bwd(dx, dg, db, ref, B, HW, C, G, name, what, prior)
    gn_check_bwd(dx2, dg2, db2, ref, B, HW, C, G, name, what + ' grad_overwrite')
    assert torch.equal(y, y2) and torch.equal(mr, mr2), f'{what}: forward differs between two identical calls'
    assert torch.equal(dx, dx2) and torch.equal(dx2, dx3), f'{what}: dx differs between identical calls'
    assert torch.equal(dg2, dg3) and torch.equal(db2, db3), f'{what}: dgamma / dbeta differ between two identical calls'
    assert torch.equal(dg, prior[0] + dg2) and torch.equal(db, prior[1] + db2), \
        f'{what}: the added gradients are not prior + the written ones'
    return y, mr, dx, dg2, db2


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('entry', GN_CASES, ids=[gn_id(e) for e in GN_CASES])
def test_groupnorm_forms(ops, dev, entry, form):
    assert_gn_plans(ops, entry, form)
    gn_run_form(ops, dev, entry[0], form, 'ordinary', seed=sum(entry[0][:4]))


# group g of every image takes hostile kind g % 8: with G >= 8 every image holds every kind
HOSTILE_GN = [e for e in GN_CASES if e[0][:4] in {(1, 1000, 320, 32), (8, 1024, 320, 32), (8, 256, 96, 32), (2, 300, 120, 12),
                                                   (4, 256, 640, 16), (2, 64, 960, 32), (2, 1000, 160, 32)}]


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('entry', HOSTILE_GN, ids=[gn_id(e) for e in HOSTILE_GN])
def test_groupnorm_hostile_inputs(ops, dev, entry, form):
    """per-group mixes of a constant group, variance 0.1 eps / eps / 10 eps, |mean| / sigma 16 and 64, magnitude 1e3:
    the ordinary bounds, whole tensor and per group (one bad group must fail the case)"""
    for eps in (1e-5, 1e-6):
        case = entry[0][:5] + (eps,) + entry[0][6:]
        gn_run_form(ops, dev, case, form, 'hostile', seed=7 + sum(case[:4]))


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('entry', [e for e in GN_CASES if e[0][:4] in {(8, 1024, 320, 32), (1, 1000, 320, 32), (2, 64, 960, 32)}],
                         ids=gn_id)
def test_groupnorm_mean_256_sigma(ops, dev, entry, form):
    """every group at |mean| / sigma = 256: the statistics are E[x^2] - mean^2 in fp32 (one pass), which loses
    log2(256^2) = 16 of fp32's 24 bits to the cancellation - bounds of their own ('gn256.*')"""
    gn_run_form(ops, dev, entry[0], form, 'shift256', seed=11, name='gn256')


MIXED_GN = [e for e in GN_CASES if e[0][:4] in {(1, 1500, 96, 32), (8, 1024, 960, 32), (8, 1024, 320, 32), (2, 600, 320, 32)}]


@pytest.mark.parametrize('fwd_form,bwd_form', [('res0', 'multipass'), ('multipass', 'res0'), ('res0', 'res2'), ('multipass', 'res1')])
@pytest.mark.parametrize('entry', MIXED_GN, ids=[gn_id(e) for e in MIXED_GN])
def test_groupnorm_mixed_forms(ops, dev, entry, fwd_form, bwd_form):
    """the backward of one form on the mean_rstd of the other (production mixes them where the backward's plan declines a
    shape the forward's takes: NL <= 11 / 14 against <= 21)"""
    B, HW, C, G, aligned, eps, silu, radd = case = entry[0]
    ld = row_stride(C, aligned)
    x, dy, r, gamma, beta = gn_inputs(B, HW, C, G, eps, radd, 'hostile', 5, dev)
    ref = gn_reference(x, dy, r, gamma, beta, B, HW, C, G, eps, silu)
    xv, dyv, rv = in_view(x, ld), in_view(dy, ld), (in_view(r, ld) if r is not None else None)
    what = f'{case} fwd {fwd_form} -> bwd {bwd_form}'
    with gn_form(ops, fwd_form):
        y, mr = gn_fwd(ops, xv, gamma, beta, B, HW, C, G, eps, silu, ld, 60)
    with gn_form(ops, bwd_form):
        dx, dg, db = gn_bwd(ops, xv, dyv, rv, gamma, beta, mr, B, HW, C, G, silu, ld, 70)
    gn_check_fwd(y, mr, ref, B, HW, C, G, 'gn', what)
    gn_check_bwd(dx, dg, db, ref, B, HW, C, G, 'gn', what)


# the U-Net's GroupNorm levels at 256 px (32 x 32 latents): (C, HW)
UNET_GN = [(320, 1024), (640, 1024), (960, 1024), (640, 256), (960, 256), (1280, 256), (1920, 256), (1280, 64), (1920, 64),
           (2560, 64), (1280, 16), (2560, 16)]
PLAN_KEYS = ('form', 'threads', 'nl', 'cw', 'peers8')


def covered_instantiations():
    fwd, bwd = set(), set()
    for entry in GN_CASES:
        fwd.add(entry[1].split('/')[0].split('+')[0])
        bwd.update(b.split('/')[0].split('+')[0] for b in entry[2])
    return fwd - {'mp'}, bwd - {'mp'}


@pytest.mark.parametrize('B', [1, 2, 8, 64])
def test_groupnorm_default_dispatch_is_a_tested_form(ops, dev, B):
    """With the default options, every U-Net level runs a plan that a forced form also reports (same form, threads, NL, CW,
    peers8; gn_resident 1 or 256 with gn_resident_min_slab = 0 - forcing can change the slab width, so the match is on the
    plan), an instantiation the edge cases above run, and gives torch.equal outputs to that forced run."""
    eps, silu = 1e-5, 1
    fwd_cov, bwd_cov = covered_instantiations()
    for C, HW in UNET_GN:
        G, ld = 32, row_stride(C, True)   # line-aligned rows, as the U-Net's dense tensors (C % 64 == 0)
        x, dy, r, gamma, beta = gn_inputs(B, HW, C, G, eps, True, 'ordinary', C + HW, dev)
        x, dy, r = in_view(x, ld), in_view(dy, ld), in_view(r, ld)
        plans = {}
        for bwd in (False, True):
            default = ops.groupnorm_plan(B, HW, C, G, ld, ld, bwd=bwd)
            match = None
            for form in list(FORMS) + list(WIDE_FORMS):
                with gn_form(ops, form):
                    p = ops.groupnorm_plan(B, HW, C, G, ld, ld, bwd=bwd)
                if all(p[k] == default[k] for k in PLAN_KEYS):
                    match = form
                    break
            assert match, f'B={B} C={C} HW={HW} {"bwd" if bwd else "fwd"}: no forced form runs the default plan {default}'
            label = plan_label(default).split('/')[0].split('+')[0]
            assert label == 'mp' or label in (bwd_cov if bwd else fwd_cov), f'{label} is not among the edge cases'
            plans[bwd] = match
        outs = []
        for fform, bform in ((None, None), (plans[False], plans[True])):
            with gn_form(ops, fform) if fform else contextlib.nullcontext():
                y, mr = gn_fwd(ops, x, gamma, beta, B, HW, C, G, eps, silu, ld, 80)
            with gn_form(ops, bform) if bform else contextlib.nullcontext():
                dx, dg, db = gn_bwd(ops, x, dy, r, gamma, beta, mr, B, HW, C, G, silu, ld, 90)
            outs.append((y, mr, dx, dg, db))
        for a, b, nm in zip(*outs, ('y', 'mean_rstd', 'dx', 'dgamma', 'dbeta')):
            assert torch.isfinite(a.float()).all(), f'B={B} C={C} HW={HW}: non-finite {nm}'
            assert torch.equal(a, b), f'B={B} C={C} HW={HW}: default {nm} != forced ({plans})'


# ------------------------------------------------------------------------------------------------ LayerNorm
LN5_RPW = {320: 8, 640: 4, 1280: 2}   # ln_fwd5 / ln_bwd5: rows per wave


def _ln_cases():
    out = []
    for C, rpw in LN5_RPW.items():
        ms = sorted({1, rpw - 1, rpw, rpw + 1, 4 * rpw + 1} - {0})
        # above the forward's 2048-block grid (loop runs twice) and in ln_bwd5's >= 256-block branch
        ms.append({320: 70001, 640: 40001, 1280: 20001}[C])
        out += [(M, C) for M in ms]
    out.append((65539, 1280))   # ln_bwd5's grid capped at 1024 blocks: more than 32 row groups per wave
    for C in (8, 24, 72, 512, 520, 768, 1024, 1528, 1536):   # the generic kernels: 4 rows per block
        out += [(M, C) for M in (1, 6, 151)]
        out.append((20481, C))   # above both grid caps (4096 / 1024 blocks)
    return out


LN_CASES = _ln_cases()


def ln_inputs(M, C, eps, kind, seed, dev, radd):
    mu, sd = mixed(M, kind, eps, seed, dev)
    x = (mu[:, None] + sd[:, None] * randn(M, C, seed=seed + 2, dev=dev)).to(BF)
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    xhat = (xd - mean) * ((xd - mean).square().mean(1, keepdim=True) + eps).rsqrt()
    ab = randn(2, M, 1, seed=seed + 3, dev=dev).double()
    dy = correlated_dy(xhat, ab[0], ab[1], seed + 4)
    gamma, beta = affine(C, seed + 5, dev)
    r = randn(M, C, seed=seed + 6, dev=dev).to(BF) if radd else None
    return x, dy, r, gamma, beta


def ln_reference(x, dy, radd, gamma, beta, eps):
    xd = x.double().requires_grad_()
    gd, bd = gamma.double().requires_grad_(), beta.double().requires_grad_()
    mean = xd.mean(1, keepdim=True)
    rstd = ((xd - mean).square().mean(1, keepdim=True) + eps).rsqrt()
    y = (xd - mean) * rstd * gd + bd
    y.backward(dy.double())
    return dict(y=y.detach(), mean=mean.detach(), rstd=rstd.detach(),
                dx=xd.grad + (radd.double() if radd is not None else 0), dgamma=gd.grad, dbeta=bd.grad)


def ln_run(ops, dev, M, C, eps, kind, radd, seed):
    ld = row_stride(C, False)
    x, dy, r, gamma, beta = ln_inputs(M, C, eps, kind, seed, dev, radd)
    ref = ln_reference(x, dy, r, gamma, beta, eps)
    xv, dyv, rv = in_view(x, ld), in_view(dy, ld), (in_view(r, ld) if r is not None else None)
    what = f'M={M} C={C} {kind} eps={eps:.0e}' + (' radd' if radd else '')
    rows = ('row', lambda t: t)
    outs = []
    for i, prior in enumerate(((randn(C, seed=seed + 7, dev=dev), randn(C, seed=seed + 8, dev=dev)), None, None)):
        ybuf, y, ybefore = out_view(M, C, ld, dev, seed + 10 + i)
        mbuf, mr, mbefore = f32_view(2 * M, dev, seed + 20 + i, NAN)
        ops.layernorm_fwd(xv, y, gamma, beta, mr, eps)
        dxbuf, dx, dxbefore = out_view(M, C, ld, dev, seed + 30 + i)
        gbuf, dg, gbefore = f32_view(C, dev, seed + 40 + i, prior[0] if prior else NAN)
        bbuf, db, bbefore = f32_view(C, dev, seed + 50 + i, prior[1] if prior else NAN)
        scratch = torch.full((1024 * C * 2,), NAN, device=dev)
        try:
            ops.set_option('grad_overwrite', 0 if prior else 1)
            ops.layernorm_bwd(xv, dyv, rv, dx, gamma, mr, dg, db, scratch)
            torch.cuda.synchronize()
        finally:
            ops.set_option('grad_overwrite', 0)
        check_sentinels(ybuf, ybefore, M, C, 'y')
        check_sentinels(dxbuf, dxbefore, M, C, 'dx')
        for buf, before, n, nm in ((mbuf, mbefore, 2 * M, 'mean_rstd'), (gbuf, gbefore, C, 'dgamma'), (bbuf, bbefore, C, 'dbeta')):
            check_f32_sentinels(buf, before, n, nm)
        tag = what + (' grad_overwrite' if prior is None else '')
        check(y, ref['y'], 'ln.y', f'{tag} y', rows)
        check_stats(mr, ref['mean'], ref['rstd'], 'ln', f'{tag} mean_rstd')
        check(dx, ref['dx'], 'ln.dx', f'{tag} dx', rows)
        check(dg - prior[0] if prior else dg, ref['dgamma'], 'ln.dgamma', f'{tag} dgamma')
        check(db - prior[1] if prior else db, ref['dbeta'], 'ln.dbeta', f'{tag} dbeta')
        outs.append((y, mr, dx, dg, db, prior))
    (y, mr, dx, dg, db, prior), (y2, mr2, dx2, dg2, db2, _) = outs[:2]
    assert torch.equal(y, y2) and torch.equal(mr, mr2) and torch.equal(dx, dx2), f'{what}: differs between two identical calls'
    for a, b, nm in zip(outs[1][:5], outs[2][:5], ('y', 'mean_rstd', 'dx', 'dgamma', 'dbeta')):
        assert torch.equal(a, b), f'{what}: {nm} differs between two identical calls'
    assert torch.equal(dg, prior[0] + dg2) and torch.equal(db, prior[1] + db2), \
        f'{what}: the added gradients are not prior + the written ones'


@pytest.mark.parametrize('M,C', LN_CASES, ids=[f'm{M}-c{C}' for M, C in LN_CASES])
def test_layernorm_forms(ops, dev, M, C):
    """ln_fwd5 / ln_bwd5 at C = 320 / 640 / 1280 (M around the rows of a wave, above the capped grids, both block-count
    branches of the backward) and the generic kernels (lane tails of C / 8 % 64, C = 1536, 4-row block tails, grid-stride
    loops), Radd present every other case"""
    i = LN_CASES.index((M, C))
    ln_run(ops, dev, M, C, (1e-5, 1e-6)[i % 2], 'ordinary', radd=i % 2 == 0, seed=M + C)


@pytest.mark.parametrize('M,C', [(77, 320), (64, 640), (203, 1280), (77, 1024), (64, 72), (40, 1536), (333, 520)])
@pytest.mark.parametrize('kind', ['hostile', 'shift256'])
def test_layernorm_hostile_inputs(ops, dev, M, C, kind):
    """per-row mixes of the GroupNorm hostile kinds, and every row at |mean| / sigma = 256: the statistics are two-pass,
    so the ordinary bounds hold"""
    for eps in (1e-5, 1e-6):
        ln_run(ops, dev, M, C, eps, kind, radd=C % 640 != 0, seed=3 + M)


def test_layernorm_rejects_unsupported_widths(ops, dev):
    """C > 1536 is refused by the entry points (DA_ERR_SHAPE), C % 8 != 0 by the wrapper and by the C ABI"""
    from diffusion_amd import _lib
    M = 16
    for C in (1544, 2048):
        x = torch.zeros(M, C, device=dev, dtype=BF)
        g = torch.ones(C, device=dev)
        with pytest.raises(RuntimeError, match='DA_ERR_SHAPE'):
            ops.layernorm_fwd(x, x.clone(), g, g.clone(), torch.empty(2 * M, device=dev))
        with pytest.raises(RuntimeError, match='DA_ERR_SHAPE'):
            ops.layernorm_bwd(x, x, None, x.clone(), g, torch.zeros(2 * M, device=dev), g.clone(), g.clone(),
                              torch.empty(1024 * C * 2, device=dev))
    buf = torch.zeros(M, 104, device=dev, dtype=BF)
    with pytest.raises(ValueError):
        ops.layernorm_fwd(buf[:, :100], buf.clone()[:, :100], torch.ones(100, device=dev), torch.ones(100, device=dev),
                          torch.empty(2 * M, device=dev))
    lib, s, g, mr = _lib.load(), ops._stream(), torch.ones(104, device=dev), torch.zeros(2 * M, device=dev)
    y = buf.clone()
    assert lib.da_layernorm_fwd(buf.data_ptr(), 104, y.data_ptr(), 104, g.data_ptr(), g.data_ptr(), mr.data_ptr(), M, 100,
                                1e-5, s) == 1
    sc = torch.zeros(1024 * 104 * 2, device=dev)
    assert lib.da_layernorm_bwd(buf.data_ptr(), 104, buf.data_ptr(), 104, 0, 0, y.data_ptr(), 104, g.data_ptr(),
                                mr.data_ptr(), g.data_ptr(), g.data_ptr(), sc.data_ptr(), M, 100, s) == 1
    torch.cuda.synchronize()
    assert torch.equal(y, buf) and torch.equal(mr, torch.zeros_like(mr))   # nothing launched
