"""GPU tests of the kernels behind Min-SNR weighting and guidance rescale, against float64, in the sandwich style of
tests/test_pointwise_edges_gpu.py (whose predicates are imported).  Bounds are counted from the roundings on the path, with
u = 2^-24:

  da_mse_loss_w
    dpred   the sandwich of r = w (p - q) coef at 3 u |r|: the subtraction and two multiplications, u each
    loss    relative (depth + 1) u, depth = mse_geometry()'s count of additions on the longest path (all terms are >= 0, so
            every addition and the extra multiplication by w cost at most u of the total)
    exact on an integer grid with power-of-two weights (dpred bit for bit; the loss up to its two final scalings)
  da_guidance_rescale
    4 x the error that torch's own fp32 route (pu + g (pt - pu), torch.std, the blend, all in fp32 on the CPU) makes on the
    same inputs against float64, worst over the cases of one test, and never less than 4 u |factor|: the result is one fp32
  the four _rs step forms
    the bounds of tests/test_sampler_gpu.py, tests/test_dpm_gpu.py and tests/test_inpaint_gpu.py with the guided term's 8 u
    raised to 9 u for the one multiplication more; the factor is the statistics kernel's own output
"""
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_pointwise_edges_gpu import (BF, F32, NAN, U24, assert_kept, f32, flat_out, gen, mask1d, mse_geometry,  # noqa: E402
                                      needed_c, same_bits, sandwich_ok)

pytestmark = pytest.mark.gpu

U = U24
T = 1000


@pytest.fixture(scope='module')
def ops(dev):
    from diffusion_amd import ops as o
    return o


@pytest.fixture(scope='module')
def snr_tables():
    """the real gamma = 5 tables on the zero-terminal-SNR schedule, as the fp32 values the model uploads"""
    from diffusion_amd.models.schedulers import DDPMScheduler, min_snr_weights
    ac = DDPMScheduler(rescale_betas_zero_snr=True).alphas_cumprod
    return {pt: min_snr_weights(ac, 5.0, pt).float() for pt in ('epsilon', 'v_prediction')}


# ---------------------------------------------------------------------------------------------------------------------
# da_mse_loss_w
# ---------------------------------------------------------------------------------------------------------------------
def guarded_table(w, dev):
    """the table between NaN guards: a read outside it poisons the loss"""
    buf = torch.full((w.numel() + 128,), NAN, device=dev)
    buf[64:64 + w.numel()] = w.to(dev)
    return buf[64:64 + w.numel()]


def run_mse_w(ops, dev, pred, target, total_pix, C, HW, t, wtab, coef, weight, accumulate, prior):
    """(dpred [total_pix, 8], loss) of da_mse_loss_w; twice, the same bits, sentinels kept"""
    bd, vd, kd = flat_out(total_pix * 8, BF, dev, 81)
    bl, vl, kl = flat_out(4, F32, dev, 82, lead=4, fill=prior)
    scratch = torch.full((1024,), NAN, device=dev)
    res = []
    for _ in range(2):
        vd.fill_(NAN), vl[0:1].fill_(prior)
        ops.mse_loss_w(pred, target, vd, vl, scratch, total_pix, C, HW, t, wtab, coef, weight, accumulate)
        res.append((vd.clone(), vl.clone()))
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1][:1], res[1][1][:1]), 'mse_w: a repeated call gave other bits'
    assert_kept(bd, kd, mask1d(bd, total_pix * 8), 'mse_w dpred')
    m = mask1d(bl, 4, lead=4)
    m[5:] = False
    assert_kept(bl, kl, m, 'mse_w loss')
    return res[0][0].view(total_pix, 8), float(res[0][1][0])


def timesteps_for(B, k):
    """0 and T - 1 first, then spread over the table"""
    base = [0, T - 1, 139, 500, 998, 1, 250]
    return torch.tensor([base[(i + k) % len(base)] for i in range(B)], dtype=torch.int64)


MSE_SHAPES = [(1, 1), (3, 5), (4, 63), (2, 257), (5, 300)]
# every shape at every channel count, and one case of more than 1024 * 256 pixels (threads then visit several pixels)
MSE_CASES = [(C, B, HW) for (B, HW), C in itertools.product(MSE_SHAPES, (1, 3, 4, 8))] + [(4, 5, 65537)]


@pytest.mark.parametrize('C,B,HW', MSE_CASES)
def test_mse_loss_w(dev, ops, snr_tables, C, B, HW):
    total_pix = B * HW
    g = gen(183 + C, dev)
    worst_d = worst_l = 0.0
    for grid in (True, False):
        if grid:        # pred - target in {-2 .. 2}, weights in {0, 1/4, 1, 4}: every partial sum is exact
            target = torch.randint(-3, 4, (total_pix, 8), generator=g, device=dev).float()
            pred = target + torch.randint(-2, 3, (total_pix, 8), generator=g, device=dev).float()
            w = torch.tensor([0.0, 0.25, 1.0, 4.0]).repeat(T // 4)
            w[T - 1] = 0.25
            coef = 2.0 ** -10
        else:
            pred, target = torch.randn(2, total_pix, 8, generator=g, device=dev).unbind(0)
            pred, target = pred.contiguous(), target.contiguous()
            w = snr_tables[('epsilon', 'v_prediction')[C % 2]]
            coef = 2.0 / (C * total_pix)
        t = timesteps_for(B, C)
        wtab = guarded_table(w, dev)
        d = (pred.double() - target.double())[:, :C]
        pred[:, C:] = NAN                  # pad lanes must not count
        target[:, C:] = NAN
        wb = w.double()[t].repeat_interleave(HW)[:, None]              # the weight of every pixel's sample
        td = t.to(dev)
        plain = {}
        for weight, accumulate, prior in ((1.0, 0, NAN), (0.25, 0, NAN), (0.25, 1, 3.0)):
            dpred, loss = run_mse_w(ops, dev, pred, target, total_pix, C, HW, td, wtab, coef, weight, accumulate, prior)
            what = f'mse_w C={C} B={B} HW={HW} grid={grid} w={weight} acc={accumulate}'
            assert same_bits(dpred[:, C:], torch.zeros_like(dpred[:, C:])), f'{what}: pad lanes of dpred are not +0'
            rd = d * wb.to(dev) * f32(coef)
            if grid:
                assert same_bits(dpred[:, :C].contiguous(), rd.to(BF)), f'{what}: dpred is not exact on the grid'
            else:
                ok = sandwich_ok(dpred[:, :C], rd, 3 * U * rd.abs())
                worst_d = max(worst_d, needed_c(dpred[:, :C], rd, U * rd.abs()))
                assert bool(ok.all()), f'{what}: {int((~ok).sum())} dpred elements outside 3 u'
            if accumulate:      # one fp32 addition onto the prior value (the weight 0.25 scales exactly)
                assert loss == f32(prior + plain[weight]), f'{what}: {loss} is not {prior} + {plain[weight]}'
                continue
            plain[weight] = loss
            ref = float((wb.to(dev) * d * d).sum()) * f32(1.0 / (C * total_pix)) * weight
            if grid:            # the sum is exact; the two scalings round once each
                assert abs(loss - ref) <= 2 * U * abs(ref), f'{what}: loss {loss} vs {ref}'
            else:
                depth = mse_geometry(total_pix, C)[1] + 1
                rel = abs(loss - ref) / (abs(ref) * depth * U) if ref else float(loss != 0.0)
                worst_l = max(worst_l, rel)
                assert rel <= 1.0, f'{what}: loss {loss} vs {ref}: {rel:.3g} x (depth {depth}) x 2^-24'
        # a sample whose weight is exactly 0 (T - 1 of the v table; the grid's zeros) contributes exactly nothing to dpred
        for b in range(B):
            if float(w[t[b]]) == 0.0:
                rows = dpred[b * HW:(b + 1) * HW, :C]
                assert bool((rows == 0).all()), f'sample {b} of weight 0 left a gradient'
    print(f'mse_loss_w C={C} B={B} HW={HW}: worst dpred needed c {worst_d:.3f} (bound 3), loss {worst_l:.3f} of its bound')


@pytest.mark.parametrize('B,HW', [(3, 5), (2, 257)])
@pytest.mark.parametrize('C', [3, 4])
def test_mse_loss_w_table_of_ones_and_clamped_timesteps(dev, ops, C, B, HW):
    total_pix = B * HW
    pred, target = torch.randn(2, total_pix, 8, generator=gen(7, dev), device=dev).unbind(0)
    pred, target = pred.contiguous(), target.contiguous()
    coef = 2.0 / (C * total_pix)
    scratch = torch.zeros(1024, device=dev)
    t = timesteps_for(B, 0).to(dev)

    def w_call(tt, wtab):
        dp, ls = torch.empty(total_pix, 8, device=dev, dtype=BF), torch.zeros(1, device=dev)
        ops.mse_loss_w(pred, target, dp, ls, scratch, total_pix, C, HW, tt, wtab, coef, 1.0, 0)
        return dp, ls
    dp_c, ls_c = torch.empty(total_pix, 8, device=dev, dtype=BF), torch.zeros(1, device=dev)
    ops.mse_loss_c(pred, target, dp_c, ls_c, scratch, total_pix, C, coef, 1.0, 0)
    dp, ls = w_call(t, guarded_table(torch.ones(T), dev))
    assert same_bits(dp, dp_c) and same_bits(ls, ls_c), 'a table of ones must give the bits of da_mse_loss_c'
    # a timestep outside [0, T) is clamped into the table: the bits of the call with the clamped value, and no read
    # of the NaN guards around the table
    w = guarded_table(torch.rand(T, generator=torch.Generator().manual_seed(3)) + 0.5, dev)
    out = t.clone()
    out[0], out[-1] = -5, T + 7
    clamped = out.clamp(0, T - 1)
    (dp_o, ls_o), (dp_k, ls_k) = w_call(out, w), w_call(clamped, w)
    assert same_bits(dp_o, dp_k) and same_bits(ls_o, ls_k) and bool(torch.isfinite(ls_o).all())
    huge = t.clone()
    huge[0], huge[-1] = -2**62, 2**62
    dp_h, ls_h = w_call(huge, w)
    assert same_bits(dp_h, dp_k) and same_bits(ls_h, ls_k)


def test_mse_loss_w_rejections_launch_nothing(dev, ops):
    from diffusion_amd import _lib
    from diffusion_amd.ops import _stream
    pred = torch.zeros(12 * 8 + 4, device=dev)
    dp = torch.full((12 * 8 + 8,), 7.0, device=dev, dtype=BF)
    loss, scratch = torch.full((1,), 5.0, device=dev), torch.zeros(1024, device=dev)
    t, w = torch.zeros(3, device=dev, dtype=torch.int64), torch.ones(T, device=dev)
    P = pred.data_ptr()

    def rc(p=P, q=P, d=dp.data_ptr(), total=12, C=3, HW=4, t_=t.data_ptr(), w_=w.data_ptr(), T_=T):
        return _lib.load().da_mse_loss_w(p, q, d, loss.data_ptr(), scratch.data_ptr(), total, C, HW, t_, w_, T_, 1.0, 1.0, 0,
                                         _stream())
    for bad in (dict(total=13), dict(total=0), dict(HW=0), dict(HW=-4), dict(HW=5), dict(T_=0), dict(T_=-1), dict(t_=None),
                dict(w_=None), dict(C=0), dict(C=9), dict(p=P + 4), dict(q=P + 8), dict(d=dp.data_ptr() + 2)):
        assert rc(**bad) == 1, bad
    torch.cuda.synchronize()
    assert float(loss) == 5.0 and bool((dp == 7.0).all())
    assert rc() == 0
    # the wrapper
    ok = (pred[:96], pred[:96], dp[:96], loss, scratch, 12, 3, 4, t, w, 1.0, 1.0, 0)
    ops.mse_loss_w(*ok)
    for i, badarg in ((7, 5), (8, t.int()), (8, t[:2]), (9, w.double()), (9, w.cpu()), (6, 9), (0, pred[:96].double())):
        args = list(ok)
        args[i] = badarg
        with pytest.raises(ValueError):
            ops.mse_loss_w(*args)


# ---------------------------------------------------------------------------------------------------------------------
# da_guidance_rescale
# ---------------------------------------------------------------------------------------------------------------------
def std64(z):
    """per sample over everything else, n - 1 in the denominator (it cancels in the ratio)"""
    z = z.double()
    zc = z - z.mean(dim=(1, 2), keepdim=True)
    return (zc * zc).sum(dim=(1, 2)).div(max(z.shape[1] * z.shape[2] - 1, 1)).sqrt()


def run_stats(ops, dev, pred, coef, g_index, phi, B, HW, C):
    buf, view, keep = flat_out(B, F32, dev, 91)
    ops.guidance_rescale(pred, coef, view, phi=phi, HW=HW, C=C, g_index=g_index)
    first = view.clone()
    view.fill_(NAN)
    ops.guidance_rescale(pred, coef, view, phi=phi, HW=HW, C=C, g_index=g_index)
    assert same_bits(first, view), 'guidance_rescale: a repeated call gave other bits'
    assert_kept(buf, keep, mask1d(buf, B), 'guidance_rescale factor')
    return first.cpu()


@pytest.mark.parametrize('HW', [1, 35, 256, 4096])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('C', [3, 4])
def test_guidance_rescale_statistics(dev, ops, C, B, HW):
    npix = B * HW
    gcpu = torch.Generator().manual_seed(29 + C + HW)
    errs, yard = {}, {}
    for kind, (g, phi), g_index in itertools.product(('unit', 'offset'), itertools.product((1.5, 7.5), (0.3, 0.7, 1.0)), (3, 5)):
        if (g_index == 5) != (phi == 0.7):      # the two row layouts take turns
            continue
        pred = torch.randn(2 * npix, 8, generator=gcpu)
        if kind == 'offset':                    # N(8, 0.5^2): |mean| / std = 16
            pred = 8.0 + 0.5 * pred
        pred[:, C:] = NAN
        pu, pt = pred[:npix, :C].view(B, HW, C), pred[npix:, :C].view(B, HW, C)
        want = phi * std64(pt) / std64(pu.double() + g * (pt.double() - pu.double())) + (1 - phi)
        # the yardstick: torch's fp32 route on the CPU
        m32 = pu + g * (pt - pu)
        f32_route = phi * (pt.std(dim=(1, 2)) / m32.std(dim=(1, 2))) + (1 - phi)
        coef = torch.zeros(8)
        coef[g_index] = g
        coef[(g_index + 1) % 8] = NAN            # a neighbour of g must not be what is read
        got = run_stats(ops, dev, pred.to(dev), coef.to(dev), g_index, phi, B, HW, C)
        if C * HW == 1:
            continue
        ok = torch.isfinite(want)
        assert bool(ok.all()) or C * HW < 4
        e = ((got.double() - want).abs() / want.abs())[ok]
        y = ((f32_route.double() - want).abs() / want.abs())[ok]
        errs.setdefault(kind, []).append(e.max().item())
        yard.setdefault(kind, []).append(y.max().item())
    for kind in errs:
        e, y = max(errs[kind]), max(yard[kind])
        bound = 4 * max(y, U)
        print(f'guidance_rescale C={C} B={B} HW={HW} {kind}: kernel error {e:.3e}, torch fp32 route {y:.3e}, '
              f'ratio {e / max(y, 1e-300):.3f}, bound {bound:.3e}')
        assert e <= bound, (kind, e, y)


def test_guidance_rescale_constant_sample_and_phi_zero(dev, ops):
    B, HW, C = 3, 35, 4
    npix = B * HW
    pred = torch.randn(2 * npix, 8, generator=torch.Generator().manual_seed(5))
    pred[:HW], pred[npix:npix + HW] = 2.5, -1.25          # sample 0: both halves constant, so m is constant: std(m) = 0
    pred[:, C:] = NAN
    coef = torch.tensor([0.0, 0.0, 0.0, 7.5]).to(dev)
    got = run_stats(ops, dev, pred.to(dev), coef, 3, 0.7, B, HW, C)
    assert float(got[0]) == 1.0 and bool(torch.isfinite(got).all()) and float(got[1]) != 1.0
    # phi = 0 is no rescale: exactly 1 for every sample
    assert bool((run_stats(ops, dev, pred.to(dev), coef, 3, 0.0, B, HW, C) == 1.0).all())


def test_guidance_rescale_rejections(dev, ops):
    from diffusion_amd import _lib
    from diffusion_amd.ops import _stream
    npix, HW = 70, 35
    pred, coef = torch.zeros(2 * npix * 8 + 4, device=dev), torch.zeros(12, device=dev)
    fac = torch.full((4,), 5.0, device=dev)
    P, K, Fp = pred.data_ptr(), coef.data_ptr(), fac.data_ptr()

    def rc(p=P, k=K, gi=3, phi=0.5, f=Fp, n=npix, hw=HW, C=4):
        return _lib.load().da_guidance_rescale(p, k, gi, phi, f, n, hw, C, _stream())
    for bad in (dict(n=0), dict(hw=0), dict(hw=36), dict(C=0), dict(C=9), dict(gi=-1), dict(gi=8), dict(phi=-0.1), dict(phi=1.5),
                dict(phi=float('nan')), dict(p=None), dict(k=None), dict(f=None), dict(p=P + 4), dict(k=K + 4), dict(f=Fp + 2)):
        assert rc(**bad) == 1, bad
    torch.cuda.synchronize()
    assert bool((fac == 5.0).all())
    assert rc() == 0
    p2 = pred[:2 * npix * 8].view(2 * npix, 8)
    ok = dict(phi=0.5, HW=HW, C=4, g_index=3)
    ops.guidance_rescale(p2, coef[:4], fac[:2], **ok)
    for args, kw in (((p2, coef[:4], fac[:3]), ok), ((p2, coef[:4], fac[:2]), dict(ok, phi=1.5)),
                     ((p2, coef[:4], fac[:2]), dict(ok, g_index=5)), ((p2, coef[:4], fac[:2]), dict(ok, HW=36)),
                     ((p2[:npix], coef[:4], fac[:2]), dict(ok, HW=36)), ((p2, coef[1:5], fac[:2]), ok),
                     ((p2, coef[:4], fac[:2].double()), ok), ((p2.cpu(), coef[:4], fac[:2]), ok)):
        with pytest.raises(ValueError):
            ops.guidance_rescale(*args, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the four step forms with the factor
# ---------------------------------------------------------------------------------------------------------------------
RS_SHAPES = [(1, 1), (70, 35), (257, 257), (512, 256), (300, 100)]      # (npix, HW)


def step_rows():
    """(form, coefficient row without guidance) from real schedules on the zero-terminal-SNR table, trailing spacing"""
    from diffusion_amd.models.schedulers import DDIMScheduler, DPMSolverMultistepScheduler
    rows = []
    for pt in ('v_prediction', 'sample'):
        d = DDIMScheduler(prediction_type=pt, rescale_betas_zero_snr=True, timestep_spacing='trailing')
        d.set_timesteps(4)
        rows += [('ddim', d.step_coefficients(t)) for t in d.timesteps.tolist()]
        m = DPMSolverMultistepScheduler(prediction_type=pt, rescale_betas_zero_snr=True, timestep_spacing='trailing')
        m.set_timesteps(4)
        rows += [('ms', m.step_coefficients_ms(i)) for i in range(4)]
    return rows


def call_form(ops, form, blend, pred, x, hist, coef, known8, eps8, mask, x_out, xt, **kw):
    if form == 'ddim':
        if blend:
            return ops.sampler_step_blend(pred, x, coef, known8, eps8, mask, x_out, xt, None, **kw)
        return ops.sampler_step(pred, x, coef, x_out, xt, None, **kw)
    if blend:
        return ops.sampler_step_ms_blend(pred, x, hist, coef, known8, eps8, mask, x_out, xt, **kw)
    return ops.sampler_step_ms(pred, x, hist, coef, x_out, xt, **kw)


@pytest.mark.parametrize('blend', [False, True], ids=['plain', 'blend'])
@pytest.mark.parametrize('form', ['ddim', 'ms'])
def test_rescaled_step_forms(dev, ops, form, blend):
    rows = [r for f, r in step_rows() if f == form]
    gcpu = torch.Generator().manual_seed(61)
    worst = 0.0
    for count, ((npix, HW), C) in enumerate(itertools.product(RS_SHAPES, (3, 4))):
        B = npix // HW
        row = rows[count % len(rows)]
        g, phi = (1.5, 7.5)[count % 2], (0.3, 0.7, 1.0)[count % 3]
        pred = torch.randn(2 * npix, 8, generator=gcpu)
        x, hist = torch.randn(npix, 8, generator=gcpu), torch.randn(npix, 8, generator=gcpu)
        known, eps = torch.randn(npix, 8, generator=gcpu), torch.randn(npix, 8, generator=gcpu)
        mk = (torch.rand(npix, generator=gcpu) * 1.5 - 0.25).clamp(0, 1)
        for z in (pred, x, hist, known, eps):
            z[:, C:] = 1e30
        bA, bS = 0.8, 0.6
        if form == 'ddim':
            cx, cm, _ = row
            coef = [cx, cm, 0.0, g] + ([bA, bS, 0.0, 0.0] if blend else [])
            g_index = 3
        else:
            ax, am, kx, k0, k1 = row
            coef = [ax, am, kx, k0, k1, g, bA, bS]
            g_index = 5
        coef = torch.tensor(coef, dtype=torch.float64).float().to(dev)
        dpred = pred.to(dev)
        # the kernel's own factor is the input of the step
        fac = torch.empty(B, device=dev)
        ops.guidance_rescale(dpred, coef, fac, phi=phi, HW=HW, C=C, g_index=g_index)
        f = fac.cpu().double().repeat_interleave(HW)[:, None]
        pu, pt, xd = pred[:npix, :C].double(), pred[npix:, :C].double(), x[:, :C].double()
        m = (pu + g * (pt - pu)) * f
        M = (pu.abs() + g * (pt.abs() + pu.abs())) * f.abs()
        if form == 'ddim':
            ref = cx * xd + cm * m
            bv = 8 * U * (cx * xd).abs() + 9 * U * abs(cm) * M
        else:
            x0 = ax * xd + am * m
            ref = kx * xd + k0 * x0
            mag = (kx * xd).abs() + abs(k0) * (ax * xd).abs()
            if k1 != 0.0:
                ref = ref + k1 * hist[:, :C].double()
                mag = mag + (k1 * hist[:, :C].double()).abs()
            bv = 8 * U * mag + 9 * U * abs(k0) * abs(am) * M
        bound = bv
        if blend:       # the bound of tests/test_inpaint_gpu.py around the unblended value
            z0, e0, mm = known[:, :C].double(), eps[:, :C].double(), mk.double()[:, None]
            kn, K = bA * z0 + bS * e0, (bA * z0).abs() + (bS * e0).abs()
            bound = mm * bv + (1 - mm) * 6 * U * K + 4 * U * ((mm * ref).abs() + ((1 - mm) * kn).abs())
            ref = mm * ref + (1 - mm) * kn
        dev_args = dict(known8=known.to(dev), eps8=eps.to(dev), mask=mk.to(dev))
        kw = dict(C=C, cfg=True, copies=2)

        def run(**extra):
            x_out = torch.full((npix, 8), 7.0, device=dev)
            xt = torch.full((2 * npix, 8), 7.0, device=dev, dtype=BF)
            h = hist.clone().to(dev)
            call_form(ops, form, blend, dpred, x.to(dev), h, coef, x_out=x_out, xt=xt, **dev_args, **kw, **extra)
            return x_out, xt, h
        x_out, xt, h = run(factor=fac, HW=HW)
        got = x_out.cpu()
        case = (form, blend, npix, HW, C, g, phi, row)
        ratio = ((got[:, :C].double() - ref).abs() / bound).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (case, ratio)
        assert (got[:, C:] == 0).all() and (xt.cpu()[:, C:] == 0).all(), case          # pad channels exactly 0
        if form == 'ms':
            assert (h.cpu()[:, C:] == 0).all(), case
        want_bf = torch.empty(npix, 8, device=dev, dtype=BF)
        ops.cast_f32_bf16(x_out, want_bf)
        for k in range(2):
            assert same_bits(xt[k * npix:(k + 1) * npix], want_bf), (case, k)
        # a factor of exactly 1 gives the bits of the plain entry
        ones = torch.ones(B, device=dev)
        (x1, xt1, h1), (x0_, xt0, h0) = run(factor=ones, HW=HW), run()
        assert same_bits(x1, x0_) and same_bits(xt1, xt0) and same_bits(h1, h0), case
        assert B == 1 or not same_bits(x_out, x0_), case
    print(f'rescaled {form}{" blend" if blend else ""}: worst |got - ref| / bound = {worst:.3f}')


def test_rescaled_step_forms_reject_bad_arguments(dev, ops):
    from diffusion_amd import _lib
    npix, HW, C = 70, 35, 4
    s = torch.cuda.current_stream().cuda_stream
    pred, x, hist = torch.zeros(2 * npix, 8, device=dev), torch.zeros(npix, 8, device=dev), torch.zeros(npix, 8, device=dev)
    coef, fac = torch.zeros(8, device=dev), torch.ones(4, device=dev)
    k8, e8, mk = torch.zeros(npix, 8, device=dev), torch.zeros(npix, 8, device=dev), torch.zeros(npix, device=dev)
    xo = torch.full((npix, 8), 7.0, device=dev)
    p = lambda t, off=0: t.data_ptr() + off   # noqa: E731
    L = _lib.load()
    forms = {
        'da_sampler_step_rs': lambda f, hw=HW, c=C: L.da_sampler_step_rs(p(pred), p(x), None, p(coef), f, p(xo), None, npix, hw,
                                                                           c, 1, 2, s),
        'da_sampler_step_ms_rs': lambda f, hw=HW, c=C: L.da_sampler_step_ms_rs(p(pred), p(x), p(hist), p(coef), f, p(xo), None,
                                                                                 npix, hw, c, 1, 2, s),
        'da_sampler_step_blend_rs': lambda f, hw=HW, c=C: L.da_sampler_step_blend_rs(
            p(pred), p(x), None, p(coef), p(k8), p(e8), p(mk), f, p(xo), None, npix, hw, c, 1, 2, s),
        'da_sampler_step_ms_blend_rs': lambda f, hw=HW, c=C: L.da_sampler_step_ms_blend_rs(
            p(pred), p(x), p(hist), p(coef), p(k8), p(e8), p(mk), f, p(xo), None, npix, hw, c, 1, 2, s),
    }
    for name, fn in forms.items():
        assert fn(None) == 1 and fn(p(fac, 2)) == 1 and fn(p(fac), hw=36) == 1 and fn(p(fac), hw=0) == 1, name
        assert fn(p(fac), c=9) == 1 and fn(p(fac), c=0) == 1, name
        torch.cuda.synchronize()
        assert bool((xo == 7.0).all()), name
    for name, fn in forms.items():
        assert fn(p(fac)) == 0, name
    # the wrappers: a factor needs the sample's pixel count, and one value per sample
    kw = dict(C=C, cfg=True, copies=2)
    for bad in (dict(factor=fac[:2]), dict(factor=fac[:3], HW=HW), dict(factor=fac[:2], HW=36),
                dict(factor=fac[:2].double(), HW=HW), dict(factor=fac[:2].cpu(), HW=HW)):
        with pytest.raises(ValueError):
            ops.sampler_step(pred, x, coef[:4], xo, None, None, **kw, **bad)
        with pytest.raises(ValueError):
            ops.sampler_step_ms(pred, x, hist, coef, xo, None, **kw, **bad)
        with pytest.raises(ValueError):
            ops.sampler_step_blend(pred, x, coef, k8, e8, mk, xo, None, None, **kw, **bad)
        with pytest.raises(ValueError):
            ops.sampler_step_ms_blend(pred, x, hist, coef, k8, e8, mk, xo, None, **kw, **bad)
