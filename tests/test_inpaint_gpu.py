"""GPU tests of image-to-image and masked inpainting on the HIP sampler: ``da_sampler_step_blend`` /
``da_sampler_step_ms_blend`` and ``da_sampler_init`` against float64, their argument checks, ``LatentSampler`` with ``known`` /
``mask_px`` (eager and graph replay) against the same loop around the oracle U-Net, and ``generate(init_image=, mask=)``.

Bound of the blended steps, elementwise on |got - ref| with u = 2^-24 (tests/test_inpaint_host.py derives it and runs an fp32
emulation against it, peak 0.42):
    m Bv + (1 - m) 6u K + 4u (|m v| + |(1 - m) kn|)        K = |bA z0| + |bS e0|
Bv is the bound of the unblended value v: 8u times the magnitudes of its terms (tests/test_sampler_gpu.py for the first-order
form, tests/test_dpm_gpu.py for the two-step one).  The reference is float64 on the images of the same fp32 inputs with the
schedulers' own ``step()`` and ``add_noise``, not the coefficient form."""
import dataclasses
import itertools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PAD = 1e30
SHAPES = [(1, 1), (255, 1), (257, 1), (2 * 7 * 7, 1), (2 * 7 * 7, 49)]   # (npix, HW) of test_sampler_gpu.py


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-20)).item()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _bf16_of(x_out, dev):
    from diffusion_amd import ops
    want = torch.empty(x_out.shape, device=dev, dtype=torch.bfloat16)
    ops.cast_f32_bf16(x_out, want)
    return want


def _mask(npix, gen, count):
    """exact 0, exact 1 and fractions; a single pixel takes them in turn"""
    mk = (torch.rand(npix, generator=gen) * 1.5 - 0.25).clamp(0, 1)
    mk[0] = (0.0, 1.0, 0.37)[count % 3]
    if npix > 2:
        mk[1], mk[2] = 1.0, 0.0
    return mk


def _renoise(count):
    """(bA, bS) and the timestep they are add_noise at (None: the last step's (1, 0))"""
    from diffusion_amd.models.schedulers import DDIMScheduler
    d = DDIMScheduler()
    tb = (None, 1, 481, 901)[count % 4]
    return d, tb, ((1.0, 0.0) if tb is None else d.add_noise_coefficients(tb))


def _blend_reference(d, tb, known, eps, C, mk, v_ref, bv, bA, bS):
    z0, e0 = known[:, :C].double(), eps[:, :C].double()
    kn = z0 if tb is None else d.add_noise(z0, e0, torch.tensor([tb]))
    K = (bA * z0).abs() + (bS * e0).abs()
    m = mk.double()[:, None]
    ref = m * v_ref + (1 - m) * kn
    bound = m * bv + (1 - m) * 6 * U * K + 4 * U * ((m * v_ref).abs() + ((1 - m) * kn).abs())
    return ref, bound, kn, K


def _check_blend_exactness(case, got, mk, v_dev, kn_dev, known, tb, C):
    one, zero = mk == 1, mk == 0
    assert torch.equal(_bits(got[one]), _bits(v_dev[one])), case          # m == 1: the unmasked step's bits
    assert torch.equal(_bits(got[zero][:, :C]), _bits(kn_dev[zero][:, :C])), case   # m == 0: kn's bits
    if tb is None:                                                         # (1, 0): kn is the known sample's bits
        assert torch.equal(_bits(kn_dev[:, :C]), _bits(known[:, :C])), case
        assert torch.equal(_bits(got[zero][:, :C]), _bits(known[zero][:, :C])), case


def _schedule_steps():
    """(scheduler, timestep) pairs from real schedules, as tests/test_sampler_gpu.py draws them: first, middle and last
    steps, every prediction type; the second list is the SDE (the only steps with a noise term)."""
    from diffusion_amd.models.schedulers import DDIMScheduler
    from diffusion_amd.schedulers.schedulers import ContinuousTimeScheduler
    plain, sde = [], []
    for ptype in ('epsilon', 'v_prediction', 'sample'):
        d = DDIMScheduler(prediction_type=ptype)
        d.set_timesteps(50)
        plain += [(d, d.timesteps[0]), (d, d.timesteps[25]), (d, d.timesteps[-1])]
        o = ContinuousTimeScheduler(t_max=1.56, prediction_type=ptype, use_ode=True)
        o.set_timesteps(20)
        plain += [(o, o.timesteps[0]), (o, o.timesteps[-1])]
        s = ContinuousTimeScheduler(t_max=1.56, prediction_type=ptype, use_ode=False)
        s.set_timesteps(20)
        sde += [(s, s.timesteps[0]), (s, s.timesteps[7]), (s, s.timesteps[-1])]
    return plain, sde


# ---------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_sampler_step_blend_matches_float64(dev, monkeypatch):
    from diffusion_amd import ops
    plain, sde = _schedule_steps()
    gen = torch.Generator().manual_seed(51)
    worst, count = 0.0, 0
    for (npix, HW), C, cfg, copies, with_noise, inplace in itertools.product(SHAPES, (3, 4, 8), (0, 1), (1, 2), (0, 1),
                                                                             (0, 1)):
        sch, t = (sde if with_noise else plain)[count % (len(sde) if with_noise else len(plain))]
        g = (1.5, 7.5)[(count // 3) % 2]
        d, tb, (bA, bS) = _renoise(count)
        count += 1
        B = npix // HW
        pred = torch.randn((2 if cfg else 1) * npix, 8, generator=gen)
        x = torch.randn(npix, 8, generator=gen)
        z = torch.randn(B, C, HW, 1, generator=gen)
        known = 3 * torch.randn(npix, 8, generator=gen)
        eps = torch.randn(npix, 8, generator=gen)
        mk = _mask(npix, gen, count)
        for a in (pred, x, known, eps):
            a[:, C:] = PAD
        cx, cm, cn = sch.step_coefficients(t)
        assert (cn != 0.0) == bool(with_noise)
        pu = pred[:npix, :C].double()
        pt = pred[npix:, :C].double() if cfg else pu
        m = pu + g * (pt - pu) if cfg else pu
        zz = z.double().view(B, C, HW).permute(0, 2, 1).reshape(npix, C)
        monkeypatch.setattr(torch, 'randn_like', lambda like, zz=zz: zz.clone())
        v_ref = sch.step(m, t, x[:, :C].double())['prev_sample']
        monkeypatch.undo()
        bv = 8 * U * ((cx * x[:, :C].double()).abs() + abs(cn) * zz.abs() * (1 if with_noise else 0)
                      + abs(cm) * ((pu.abs() + g * (pt.abs() + pu.abs())) if cfg else pu.abs()))
        ref, bound, kn_ref, K = _blend_reference(d, tb, known, eps, C, mk, v_ref, bv, bA, bS)
        # device
        coef = torch.tensor([cx, cm, cn, g, bA, bS, 0.0, 0.0], dtype=torch.float64).float().to(dev)
        dx, dpred, dz = x.clone().to(dev), pred.to(dev), (z.to(dev) if with_noise else None)
        dk, de, dm = known.to(dev), eps.to(dev), mk.to(dev)
        x_out = dx if inplace else torch.full((npix, 8), 7.0, device=dev)
        xt = torch.full((copies * npix, 8), 7.0, device=dev, dtype=torch.bfloat16)
        ops.sampler_step_blend(dpred, dx, coef, dk, de, dm, x_out, xt, dz, C=C, cfg=cfg, copies=copies)
        got = x_out.cpu()
        ratio = ((got[:, :C].double() - ref).abs() / bound).max().item()
        worst = max(worst, ratio)
        case = (npix, HW, C, cfg, copies, with_noise, inplace, type(sch).__name__, sch.prediction_type, float(t), g, tb)
        assert ratio <= 1.0, (case, ratio)
        assert (got[:, C:] == 0).all() and (xt.cpu()[:, C:] == 0).all(), case
        want_bf = _bf16_of(x_out, dev)
        for k in range(copies):
            assert torch.equal(xt[k * npix:(k + 1) * npix].view(torch.int16), want_bf.view(torch.int16)), (case, k)
        if not inplace:
            assert torch.equal(dx.cpu(), x), case   # the input is only read
        assert torch.equal(dk.cpu(), known) and torch.equal(de.cpu(), eps) and torch.equal(dm.cpu(), mk), case
        # the unmasked step on the same inputs, and kn from a launch that keeps everything of another state
        v_dev = torch.empty(npix, 8, device=dev)
        ops.sampler_step(dpred, x.to(dev), coef[:4], v_dev, None, dz, C=C, cfg=cfg, copies=copies)
        kn_dev = torch.empty(npix, 8, device=dev)
        ops.sampler_step_blend(torch.randn_like(dpred), torch.randn(npix, 8, device=dev), coef, dk, de,
                               torch.zeros(npix, device=dev), kn_dev, None, dz, C=C, cfg=cfg, copies=copies)
        kn_dev = kn_dev.cpu()
        assert ((kn_dev[:, :C].double() - kn_ref).abs() <= 6 * U * K + 4 * U * kn_ref.abs()).all(), case
        _check_blend_exactness(case, got, mk, v_dev.cpu(), kn_dev, known, tb, C)
        # last step: no next U-Net input
        x_last = torch.empty(npix, 8, device=dev)
        ops.sampler_step_blend(dpred, x.to(dev), coef, dk, de, dm, x_last, None, dz, C=C, cfg=cfg, copies=copies)
        assert torch.equal(x_last.cpu(), got), case
    print(f'sampler_step_blend: {count} cases, worst |got - ref| / bound = {worst:.3f}')


def _ms_rows():
    """(scheduler, n, i, first) of real tables: first-order rows (the first step, lower_order_final's last one, the override
    of a schedule entered late) and second-order rows, every prediction type."""
    from diffusion_amd.models.schedulers import DPMSolverMultistepScheduler
    first, second = [], []
    for ptype, n in itertools.product(('epsilon', 'v_prediction', 'sample'), (4, 20, 50)):
        sch = DPMSolverMultistepScheduler(prediction_type=ptype)
        for i in sorted({0, 1, n // 2, n - 2, n - 1}):
            sch.set_timesteps(n)
            (second if sch.step_coefficients_ms(i)[4] != 0.0 else first).append((sch, n, i, False))
            if sch.step_coefficients_ms(i)[4] != 0.0:
                first.append((sch, n, i, True))
    return first, second


def _ms_step_reference(sch, n, i, first, m, x, hist, am_prev):
    """The stateful step() itself.  A second-order step gets its history through the step before it: on a zero sample the
    data prediction is am * (model output), so the model output hist / am leaves exactly-enough hist behind (one float64
    rounding)."""
    sch.set_timesteps(n)
    if first or i == 0 or sch.step_coefficients_ms(i)[4] == 0.0:
        sch.set_begin_index(i)
    else:
        sch.set_begin_index(i - 1)
        sch.step(hist / am_prev, sch.timesteps[i - 1], torch.zeros_like(hist))
    return sch.step(m, sch.timesteps[i], x)['prev_sample']


def test_sampler_step_ms_blend_matches_float64(dev):
    from diffusion_amd import ops
    first_rows, second_rows = _ms_rows()
    gen = torch.Generator().manual_seed(53)
    worst, count = 0.0, 0
    for (npix, HW), C, cfg, copies, inplace, order2 in itertools.product(SHAPES, (3, 4, 8), (0, 1), (1, 2), (0, 1), (0, 1)):
        rows = second_rows if order2 else first_rows
        sch, n, i, first = rows[count % len(rows)]
        g = (1.5, 7.5)[(count // 3) % 2]
        d, tb, (bA, bS) = _renoise(count)
        count += 1
        sch.set_timesteps(n)
        ax, am, kx, k0, k1 = sch.step_coefficients_ms(i, first=first)
        assert (k1 != 0.0) == bool(order2)
        pred = torch.randn((2 if cfg else 1) * npix, 8, generator=gen)
        x = torch.randn(npix, 8, generator=gen)
        hist = torch.randn(npix, 8, generator=gen)
        known = 3 * torch.randn(npix, 8, generator=gen)
        eps = torch.randn(npix, 8, generator=gen)
        mk = _mask(npix, gen, count)
        for a in (pred, x, hist, known, eps):
            a[:, C:] = PAD
        if not order2:
            hist[:] = float('nan')   # a first-order step does not read it
        pu = pred[:npix, :C].double()
        pt = pred[npix:, :C].double() if cfg else pu
        m = pu + g * (pt - pu) if cfg else pu
        M = (pu.abs() + g * (pt.abs() + pu.abs())) if cfg else pu.abs()
        xd = x[:, :C].double()
        am_prev = sch.step_coefficients_ms(i - 1)[1] if order2 else 1.0
        v_ref = _ms_step_reference(sch, n, i, first, m, xd, hist[:, :C].double(), am_prev)
        bv = (kx * xd).abs() + abs(k0) * ((ax * xd).abs() + abs(am) * M)
        if order2:
            bv = bv + (k1 * hist[:, :C].double()).abs()
        bv = 8 * U * bv
        ref, bound, kn_ref, K = _blend_reference(d, tb, known, eps, C, mk, v_ref, bv, bA, bS)
        # device
        coef = torch.tensor([ax, am, kx, k0, k1, g, bA, bS], dtype=torch.float64).float().to(dev)
        dx, dpred, dh = x.clone().to(dev), pred.to(dev), hist.clone().to(dev)
        dk, de, dm = known.to(dev), eps.to(dev), mk.to(dev)
        x_out = dx if inplace else torch.full((npix, 8), 7.0, device=dev)
        xt = torch.full((copies * npix, 8), 7.0, device=dev, dtype=torch.bfloat16)
        ops.sampler_step_ms_blend(dpred, dx, dh, coef, dk, de, dm, x_out, xt, C=C, cfg=cfg, copies=copies)
        got, got_h = x_out.cpu(), dh.cpu()
        case = (npix, HW, C, cfg, copies, inplace, sch.prediction_type, n, i, first, g, tb)
        ratio = ((got[:, :C].double() - ref).abs() / bound).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (case, ratio)          # NaN (a history that leaked into a first-order step) fails here too
        assert (got[:, C:] == 0).all() and (got_h[:, C:] == 0).all() and (xt.cpu()[:, C:] == 0).all(), case
        want_bf = _bf16_of(x_out, dev)
        for k in range(copies):
            assert torch.equal(xt[k * npix:(k + 1) * npix].view(torch.int16), want_bf.view(torch.int16)), (case, k)
        if not inplace:
            assert torch.equal(dx.cpu(), x), case
        # the unmasked two-step launch: its history bit for bit, its sample where m == 1
        v_dev, h_dev = torch.empty(npix, 8, device=dev), hist.clone().to(dev)
        unblended = coef.clone()
        unblended[6:] = 0
        ops.sampler_step_ms(dpred, x.to(dev), h_dev, unblended, v_dev, None, C=C, cfg=cfg, copies=copies)
        assert torch.equal(_bits(got_h), _bits(h_dev.cpu())), case
        kn_dev, h_other = torch.empty(npix, 8, device=dev), hist.clone().to(dev)
        ops.sampler_step_ms_blend(torch.randn_like(dpred), torch.randn(npix, 8, device=dev), h_other, coef, dk, de,
                                  torch.zeros(npix, device=dev), kn_dev, None, C=C, cfg=cfg, copies=copies)
        kn_dev = kn_dev.cpu()
        assert ((kn_dev[:, :C].double() - kn_ref).abs() <= 6 * U * K + 4 * U * kn_ref.abs()).all(), case
        _check_blend_exactness(case, got, mk, v_dev.cpu(), kn_dev, known, tb, C)
    print(f'sampler_step_ms_blend: {count} cases, worst |got - ref| / bound = {worst:.3f}')


INIT_SHAPES = [(1, 4, 1, 1, 8), (2, 4, 7, 9, 8), (3, 3, 8, 8, 1), (1, 8, 5, 3, 2), (1, 4, 1, 257, 1)]   # (B, C, H, W, f)


@pytest.mark.parametrize('B,C,H,W,f', INIT_SHAPES)
def test_sampler_init_matches_float64(dev, B, C, H, W, f):
    from diffusion_amd import ops
    from diffusion_amd.models.schedulers import DDIMScheduler
    gen = torch.Generator().manual_seed(B * 1000 + W)
    npix = B * H * W
    d = DDIMScheduler()
    nhwc = lambda a: a.permute(0, 2, 3, 1).reshape(npix, C)   # noqa: E731
    for copies, t0 in itertools.product((1, 2), (1, 481, 951)):
        a0, s0 = d.add_noise_coefficients(t0)
        known = 3 * torch.randn(B, C, H, W, generator=gen)
        noise = torch.randn(B, C, H, W, generator=gen)
        # blocks that are all 0, all 1, and fractions
        kind = torch.randint(0, 3, (B, H, W), generator=gen)
        if npix >= 3:
            kind.view(-1)[:3] = torch.tensor([0, 1, 2])
        px = torch.rand(B, H * f, W * f, generator=gen)
        up = kind.repeat_interleave(f, 1).repeat_interleave(f, 2)
        px = torch.where(up == 0, torch.zeros(()), torch.where(up == 1, torch.ones(()), px))
        coef = torch.tensor([a0, s0, 0.0, 0.0], dtype=torch.float64).float().to(dev)
        fill = lambda *s, dt=torch.float32: torch.full(s, 7.0, device=dev, dtype=dt)   # noqa: E731
        known8, eps8, mask, x = fill(npix, 8), fill(npix, 8), fill(npix), fill(npix, 8)
        xt = fill(copies * npix, 8, dt=torch.bfloat16)
        ops.sampler_init(known.to(dev), noise.to(dev), coef, x, xt, known8=known8, eps8=eps8, mask_px=px.to(dev), mask=mask,
                         copies=copies)
        case = (B, C, H, W, f, copies, t0)
        for got8, src in ((known8, known), (eps8, noise)):   # bit-exact relayouts, pad channels exactly 0
            assert torch.equal(_bits(got8.cpu()[:, :C]), _bits(nhwc(src))), case
            assert (got8[:, C:] == 0).all(), case
        ref = d.add_noise(nhwc(known).double(), nhwc(noise).double(), torch.tensor([t0]))
        bound = 4 * U * ((a0 * nhwc(known).double()).abs() + (s0 * nhwc(noise).double()).abs())
        got = x.cpu()
        assert ((got[:, :C].double() - ref).abs() <= bound).all(), (case, ((got[:, :C].double() - ref).abs() / bound).max())
        assert (got[:, C:] == 0).all(), case
        want_bf = _bf16_of(x, dev)
        for k in range(copies):
            assert torch.equal(xt[k * npix:(k + 1) * npix].view(torch.int16), want_bf.view(torch.int16)), (case, k)
        mean = px.double().view(B, H, f, W, f).mean(dim=(2, 4)).reshape(npix)
        gm = mask.cpu()
        assert ((gm.double() - mean).abs() <= (f * f + 2) * U).all(), case
        k = kind.reshape(npix)
        assert (gm[k == 0] == 0).all() and (gm[k == 1] == 1).all(), case
        # without a mask, and without the relayouts: the same state, nothing else written
        x2, mask2, k8 = fill(npix, 8), fill(npix), fill(npix, 8)
        ops.sampler_init(known.to(dev), noise.to(dev), coef, x2, None, copies=copies)
        assert torch.equal(x2, x) and (mask2 == 7).all() and (k8 == 7).all(), case


def test_sampler_init_and_blend_reject_bad_arguments(dev):
    from diffusion_amd import _lib, ops
    B, C, H, W, f = 2, 4, 7, 7, 8
    npix = B * H * W
    known, noise = torch.zeros(B, C, H, W + 1, device=dev), torch.zeros(B, C, H, W + 1, device=dev)
    px = torch.zeros(B * H * f * W * f + 4, device=dev)
    coef = torch.zeros(16, device=dev)
    k8, e8, x = (torch.full((npix + 1, 8), 7.0, device=dev) for _ in range(3))
    mask = torch.full((npix + 4,), 7.0, device=dev)
    xt = torch.full((2 * npix + 1, 8), 7.0, device=dev, dtype=torch.bfloat16)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t, off=0: t.data_ptr() + off   # noqa: E731

    def rc(kn=p(known), nz=p(noise), px_=p(px), coef_=p(coef), k8_=p(k8), e8_=p(e8), m_=p(mask), x_=p(x), xt_=p(xt), B_=B,
           H_=H, W_=W, C_=C, f_=f, copies=2):
        return _lib.load().da_sampler_init(kn, nz, px_, coef_, k8_, e8_, m_, x_, xt_, B_, H_, W_, C_, f_, copies, s)

    for bad in (dict(kn=None), dict(nz=None), dict(coef_=None), dict(x_=None), dict(px_=None), dict(m_=None),
                dict(k8_=None), dict(e8_=None), dict(kn=p(known, 4)), dict(nz=p(noise, 8)), dict(px_=p(px, 4)),
                dict(coef_=p(coef, 4)), dict(k8_=p(k8, 4)), dict(e8_=p(e8, 8)), dict(m_=p(mask, 4)), dict(x_=p(x, 4)),
                dict(xt_=p(xt, 2)), dict(B_=0), dict(H_=0), dict(W_=-1), dict(C_=0), dict(C_=9), dict(f_=0), dict(f_=3),
                dict(f_=6), dict(f_=32), dict(f_=-8), dict(copies=0), dict(copies=3), dict(H_=1 << 12, W_=(1 << 11) + 1)):
        assert rc(**bad) == 1, bad
    torch.cuda.synchronize()
    assert all((z == 7).all() for z in (k8, e8, x, mask, xt))   # nothing was launched
    assert rc() == 0 and rc(xt_=None) == 0 and rc(px_=None, m_=None) == 0 and rc(k8_=None, e8_=None) == 0
    torch.cuda.synchronize()
    assert (x[:npix] == 0).all() and (x[npix:] == 7).all() and (mask[:npix] == 0).all() and (mask[npix:] == 7).all()
    # the wrapper
    kc, nc = torch.zeros(B, C, H, W, device=dev), torch.zeros(B, C, H, W, device=dev)
    pc, mc, c4 = torch.zeros(B, H * f, W * f, device=dev), torch.zeros(npix, device=dev), coef[:4]
    k8c, e8c, xc, xtc = k8[:npix], e8[:npix], x[:npix], xt[:2 * npix]
    ok = dict(known8=k8c, eps8=e8c, mask_px=pc, mask=mc, copies=2)
    ops.sampler_init(kc, nc, c4, xc, xtc, **ok)
    for bad_args, bad_kw in (((kc, nc[:1], c4, xc, xtc), ok), ((kc, nc.double(), c4, xc, xtc), ok),
                             ((kc.cpu(), nc, c4, xc, xtc), ok), ((kc, nc, coef[:8], xc, xtc), ok),
                             ((kc, nc, coef[1:5], xc, xtc), ok), ((kc, nc, c4, x[:npix - 1], xtc), ok),
                             ((kc, nc, c4, xc, xt[:npix]), ok), ((kc, nc, c4, xc, xtc), dict(ok, copies=3)),
                             ((kc, nc, c4, xc, xtc), dict(ok, mask=None)), ((kc, nc, c4, xc, xtc), dict(ok, eps8=None)),
                             ((kc, nc, c4, xc, xtc), dict(ok, mask_px=pc[:, :, :W * 4])),
                             ((kc, nc, c4, xc, xtc), dict(ok, mask_px=torch.zeros(B, H * 3, W * 3, device=dev))),
                             ((kc, nc, c4, xc, xtc), dict(ok, mask_px=pc[:1])),
                             ((kc, nc, c4, xc, xtc), dict(ok, mask=mc[:npix - 1])),
                             ((kc, nc, c4, xc, xtc), dict(ok, known8=k8c.double())),
                             ((kc[:, :, :, None], nc, c4, xc, xtc), ok)):
        with pytest.raises(ValueError):
            ops.sampler_init(*bad_args, **bad_kw)

    # the blended steps: the entries, then the wrappers
    pred, hist = torch.zeros(2 * npix, 8, device=dev), torch.zeros(npix + 1, 8, device=dev)
    lib = _lib.load()

    def rb(ms, pred_=p(pred), x_=p(x), third=None, coef_=p(coef), k8_=p(k8), e8_=p(e8), m_=p(mask), xo=p(x), xt_=p(xt),
           npix_=npix, HW=49, C_=C, cfg=1, copies=2):
        fn = lib.da_sampler_step_ms_blend if ms else lib.da_sampler_step_blend
        third = third if third is not None else (p(hist) if ms else p(noise))
        return fn(pred_, x_, third, coef_, k8_, e8_, m_, xo, xt_, npix_, HW, C_, cfg, copies, s)

    x.fill_(7.0)
    xt.fill_(7.0)
    for ms in (0, 1):
        for bad in (dict(k8_=None), dict(e8_=None), dict(m_=None), dict(k8_=p(k8, 4)), dict(e8_=p(e8, 8)), dict(m_=p(mask, 4)),
                    dict(pred_=None), dict(x_=None), dict(coef_=None), dict(xo=None), dict(pred_=p(pred, 4)),
                    dict(x_=p(x, 8)), dict(coef_=p(coef, 4)), dict(xo=p(x, 4)), dict(xt_=p(xt, 2)), dict(C_=0), dict(C_=9),
                    dict(HW=48), dict(HW=0), dict(npix_=0), dict(copies=0), dict(copies=3),
                    dict(third=p(hist, 4) if ms else p(noise, 4))):
            assert rb(ms, **bad) == 1, (ms, bad)
    torch.cuda.synchronize()
    assert (x == 7).all() and (xt == 7).all() and (hist == 0).all()   # nothing was launched
    assert rb(0) == 0 and rb(1) == 0 and rb(0, xt_=None) == 0
    torch.cuda.synchronize()
    c8, hc = coef[:8], hist[:npix]
    kw = dict(C=C, cfg=True, copies=2)
    ops.sampler_step_blend(pred, xc, c8, k8c, e8c, mc, xc, xtc, **kw)
    ops.sampler_step_ms_blend(pred, xc, hc, c8, k8c, e8c, mc, xc, xtc, **kw)
    for fn, lead in ((ops.sampler_step_blend, lambda c=c8: (pred, xc, c)), (ops.sampler_step_ms_blend, lambda c=c8: (pred, xc, hc, c))):
        for tail in ((k8c[:npix - 1], e8c, mc), (k8c, e8c.double(), mc), (k8c, e8c, mc[:npix - 1]), (k8c, e8c, mc[:, None]),
                     (k8c, e8c, mc.cpu()), (k8c.cpu(), e8c, mc), (k8c, e8c, mask[1:npix + 1])):
            with pytest.raises(ValueError):
                fn(*lead(), *tail, xc, None, **kw)
        with pytest.raises(ValueError):
            fn(*lead(coef[:4]), k8c, e8c, mc, xc, None, **kw)                  # a four-float row
        with pytest.raises(ValueError):
            fn(*lead(coef[1:9]), k8c, e8c, mc, xc, None, **kw)                 # misaligned coefficients
        with pytest.raises(ValueError):
            fn(*lead(), k8c, e8c, mc, xc, xt[:npix], **kw)                     # one copy's room for two
        with pytest.raises(ValueError):
            fn(*lead(), k8c, e8c, mc, xc, None, C=9, cfg=True, copies=2)
    with pytest.raises(ValueError):
        ops.sampler_step_ms_blend(pred, xc, k8c, c8, k8c, e8c, mc, xc, None, **kw)   # the history is a buffer of its own


# ---------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------
N_STEPS, START = 6, 3


@pytest.fixture(scope='module')
def tiny(dev):
    from oracle import unet_oracle as O
    from diffusion_amd.models.models import stable_diffusion_2
    ocfg = O.UNetConfig.tiny()
    sd = O.init_state_dict(ocfg, seed=17)
    model = stable_diffusion_2(model_name='tiny', pretrained=False, precomputed_latents=True, fsdp=False)
    model.unet.load_state_dict(sd)
    return O, ocfg, sd, model


def _inputs(ocfg, seed=29, B=2, S=8):
    g = torch.Generator().manual_seed(seed)
    known = torch.randn(B, 4, S, S, generator=g)
    noise = torch.randn(B, 4, S, S, generator=g)
    txt = torch.randn(B, 77, ocfg.cross_attention_dim, generator=g)
    unc = torch.randn(B, 77, ocfg.cross_attention_dim, generator=g)
    m = (torch.rand(B, S, S, generator=g) < 0.5).float()   # one value per latent pixel: 8 x 8 pixel blocks
    m.view(-1)[:2] = torch.tensor([0.0, 1.0])
    return known, noise, txt, unc, m.repeat_interleave(8, 1).repeat_interleave(8, 2), m[:, None]


def _make(kind):
    from diffusion_amd.models.schedulers import DDIMScheduler, DPMSolverMultistepScheduler
    cls, ptype = {'ddim-eps': (DDIMScheduler, 'epsilon'), 'ddim-v': (DDIMScheduler, 'v_prediction'),
                  '2m-eps': (DPMSolverMultistepScheduler, 'epsilon')}[kind]
    return cls(prediction_type=ptype)


def _oracle_loop(O, sd, ocfg, sch, known, noise, txt, unc, mask, guidance):
    """The same partial (and masked) loop around the oracle U-Net, the scheduler's own add_noise / step in torch ops"""
    sch.set_timesteps(N_STEPS)
    ts = sch.timesteps
    if hasattr(sch, 'set_begin_index'):
        sch.set_begin_index(START)
    emb = torch.cat([unc, txt]) if guidance > 1.0 else txt
    x = sch.add_noise(known, noise, ts[START:START + 1])
    with torch.no_grad():
        for i in range(START, N_STEPS):
            t = int(ts[i])
            x_in = torch.cat([x] * 2) if guidance > 1.0 else x
            pred = O.unet_forward(sd, ocfg, x_in, torch.full((x_in.shape[0],), t, dtype=torch.int64), emb)
            if guidance > 1.0:
                pu, pt = pred.chunk(2)
                pred = pu + guidance * (pt - pu)
            x = sch.step(pred, t, x)['prev_sample']
            if mask is not None:
                kn = sch.add_noise(known, noise, ts[i + 1:i + 2]) if i + 1 < N_STEPS else known
                x = mask * x + (1 - mask) * kn
    return x


@pytest.fixture(scope='module')
def oracle_runs(tiny):
    """The float reference, computed once per (scheduler, masked) and shared"""
    O, ocfg, sd, _ = tiny
    known, noise, txt, unc, _, m = _inputs(ocfg)
    out = {}
    for kind in ('ddim-eps', 'ddim-v', '2m-eps'):
        vcfg = dataclasses.replace(ocfg, prediction_type='v_prediction') if kind == 'ddim-v' else ocfg
        for masked in (False, True):
            out[(kind, masked)] = _oracle_loop(O, sd, vcfg, _make(kind), known, noise, txt, unc, m if masked else None, 3.0)
    return out


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('kind', ['ddim-eps', 'ddim-v', '2m-eps'])
def test_partial_and_masked_sampler_match_the_oracle_loop(tiny, oracle_runs, dev, kind, masked):
    from diffusion_amd.sampling import LatentSampler
    O, ocfg, sd, model = tiny
    known, noise, txt, unc, mask_px, _ = _inputs(ocfg)
    got = LatentSampler(model.unet, _make(kind)).sample(
        noise.to(dev), txt.to(dev), unc.to(dev), num_inference_steps=N_STEPS, guidance_scale=3.0, known=known.to(dev),
        start_index=START, mask_px=mask_px.to(dev) if masked else None)
    ref = oracle_runs[(kind, masked)]
    assert got.shape == known.shape and got.dtype == torch.float32 and got.is_contiguous()
    e = _rel(got.cpu(), ref)
    print(f'{kind} masked {masked}: rel-L2 to the oracle loop {e:.3e}')
    assert e < 3e-2, e
    assert not torch.equal(ref, known)


@pytest.mark.parametrize('kind', ['ddim-eps', '2m-eps'])
@pytest.mark.parametrize('guidance', [0.0, 3.0])
def test_exact_properties_of_the_masked_sampler(tiny, dev, kind, guidance):
    from diffusion_amd.sampling import LatentSampler
    O, ocfg, sd, model = tiny
    known, noise, txt, unc, mask_px, m = _inputs(ocfg)
    smp = LatentSampler(model.unet, _make(kind))
    run = lambda **kw: smp.sample(None, txt.to(dev), unc.to(dev), num_inference_steps=N_STEPS,   # noqa: E731
                                  guidance_scale=guidance, known=known.to(dev), noise=noise.to(dev), start_index=START, **kw).cpu()
    plain = run()
    assert torch.equal(run(mask_px=torch.ones_like(mask_px)), plain)          # repaint everything: the unmasked partial run
    assert torch.equal(_bits(run(mask_px=torch.zeros_like(mask_px))), _bits(known))   # keep everything: the known sample
    mixed = run(mask_px=mask_px)
    keep = (m == 0).expand_as(known)
    assert torch.equal(_bits(mixed[keep]), _bits(known[keep]))
    assert not torch.equal(mixed[~keep], known[~keep]) and not torch.equal(mixed, plain)
    # noise defaults to the latents argument; start_index 0 runs the whole schedule from the noised sample
    again = smp.sample(noise.to(dev), txt.to(dev), unc.to(dev), num_inference_steps=N_STEPS, guidance_scale=guidance,
                       known=known.to(dev), start_index=START, mask_px=mask_px.to(dev)).cpu()
    assert torch.equal(again, mixed)
    # without known nothing changed: the plain sampler gives what it gives with the new arguments at their defaults
    full = smp.sample(noise.to(dev), txt.to(dev), unc.to(dev), num_inference_steps=N_STEPS, guidance_scale=guidance)
    assert torch.equal(full, smp.sample(noise.to(dev), txt.to(dev), unc.to(dev), num_inference_steps=N_STEPS,
                                        guidance_scale=guidance, known=None, noise=None, start_index=0, mask_px=None))


@pytest.mark.parametrize('kind', ['ddim-eps', '2m-eps'])
def test_graph_replay_equals_eager_for_partial_and_masked_runs(tiny, dev, kind):
    from diffusion_amd.sampling import LatentSampler
    O, ocfg, sd, model = tiny
    smp = LatentSampler(model.unet, _make(kind))
    smp.graphs.clear()
    kw = dict(num_inference_steps=N_STEPS, guidance_scale=3.0, start_index=START)
    for n, seed in enumerate((29, 83)):   # the second call, other inputs, reuses the captures
        known, noise, txt, unc, mask_px, _ = (z.to(dev) for z in _inputs(ocfg, seed=seed))
        for masked in (False, True):
            extra = dict(known=known, mask_px=mask_px if masked else None)
            eager = smp.sample(noise, txt, unc, **kw, **extra)
            graphed = smp.sample(noise, txt, unc, graph=True, **kw, **extra)
            assert torch.equal(eager, graphed), (n, masked, _rel(graphed, eager))
            assert len(smp.graphs) == (1 + masked if n == 0 else 2), list(smp.graphs)   # masked: a capture of its own
    assert sum('blend' in k for k in smp.graphs) == 1
    # the unmasked capture is the one a plain run uses
    plain = smp.sample(noise, txt, unc, num_inference_steps=N_STEPS, guidance_scale=3.0, graph=True)
    assert len(smp.graphs) == 2
    assert torch.equal(plain, smp.sample(noise, txt, unc, num_inference_steps=N_STEPS, guidance_scale=3.0))
    smp.graphs.clear()


def test_training_step_is_unchanged_by_a_masked_sampler_call_in_between(tiny, dev):
    from diffusion_amd.sampling import LatentSampler
    O, ocfg, sd, model = tiny
    unet = model.unet
    B, S = 4, 8
    gw = torch.Generator().manual_seed(5)
    xt = unet.to_nhwc8(torch.randn(B, 4, S, S, generator=gw).to(dev))
    t = torch.randint(0, 1000, (B,), generator=gw).to(dev)
    ctx = unet.prepare_ctx(torch.randn(B, 77, unet.cfg.cross_attention_dim, generator=gw).to(dev))
    dpred = torch.randn(B * S * S, 8, generator=torch.Generator().manual_seed(6)).to(dev).to(torch.bfloat16)
    dpred[:, 4:] = 0
    known, noise, txt, unc, mask_px, _ = (z.to(dev) for z in _inputs(ocfg))

    def step(interleave):
        unet.zero_grad()
        pred = unet.forward_features(xt, t, ctx, B, S).clone()
        if interleave:   # between the recorded forward and its backward
            for kind in ('ddim-eps', '2m-eps'):
                LatentSampler(unet, _make(kind)).sample(noise, txt, unc, num_inference_steps=4, guidance_scale=3.0,
                                                        known=known, start_index=2, mask_px=mask_px)
        unet.backward_features(dpred)
        return pred, unet.grad.clone()

    p1, g1 = step(False)
    p2, g2 = step(True)
    assert torch.equal(p1, p2) and torch.equal(g1, g2)
    assert float(g1.abs().sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def test_stable_diffusion_generate_from_an_image(dev, monkeypatch):
    from diffusion_amd.models.models import stable_diffusion_2
    monkeypatch.delenv('DA_SAMPLER', raising=False)
    torch.manual_seed(11)
    model = stable_diffusion_2(model_name='tiny', pretrained=False, fsdp=False)
    from oracle import unet_oracle as O
    model.unet.load_state_dict(O.init_state_dict(O.UNetConfig.tiny(), seed=17))   # a U-Net that answers its inputs
    g = torch.Generator().manual_seed(13)
    img = torch.rand(2, 3, 64, 64, generator=g)
    mask = torch.zeros(2, 1, 64, 64)
    mask[0, :, 16:48, 8:40] = 1.0
    mask[1, :, :, 32:] = 1.0
    mask[1, :, 5:9, :20] = 0.5   # soft values blend
    kw = dict(prompt=['a cool doge', 'a hot cat'], num_inference_steps=4, strength=0.5, seed=3, progress_bar=False)
    plain = model.generate(height=64, width=64, **kw)
    for name, sched, extra in (('img2img', 'ddim', dict(init_image=img)),
                               ('inpaint', 'ddim', dict(init_image=img, mask=mask, height=64, width=64)),
                               ('inpaint', 'dpm++2m', dict(init_image=img, mask=mask))):
        ekw = dict(kw, inference_scheduler=sched, **extra)
        hip = model.generate(**ekw)
        assert hip.shape == (2, 3, 64, 64) and torch.isfinite(hip).all() and hip.min() >= 0 and hip.max() <= 1
        assert not torch.equal(hip, plain)
        ref = model.generate(sampler='torch', **ekw)
        e = _rel(hip, ref)
        print(f'StableDiffusion.generate {name} {sched}: hip vs torch image rel-L2 {e:.3e}')
        assert e < 8e-2, e   # the decoder cap of tests/test_sampler_gpu.py for image differences
        assert torch.equal(model.generate(sampler='graph', **ekw), hip)
    # keep everything: whatever the prompt and the guidance, the image is the VAE round trip of the input
    kept = model.generate(**dict(kw, init_image=img, mask=torch.zeros(64, 64)))
    other = model.generate(**dict(kw, prompt=['another', 'prompt entirely'], guidance_scale=7.5, init_image=img,
                                  mask=torch.zeros(1, 1, 64, 64)))
    assert torch.equal(kept, other)
    changed = dict(kw, prompt=['another', 'prompt entirely'], guidance_scale=7.5, init_image=img)   # ... which do matter
    assert not torch.equal(model.generate(**changed), model.generate(**dict(kw, init_image=img)))
    assert not torch.equal(kept, model.generate(**dict(kw, init_image=img, mask=torch.ones(64, 64))))
    # one image and one [H, W] mask for the whole batch
    one = model.generate(**dict(kw, init_image=img[:1], mask=mask[0, 0]))
    both = model.generate(**dict(kw, init_image=img[:1].expand(2, -1, -1, -1), mask=mask[:1].expand(2, -1, -1, -1)))
    assert torch.equal(one, both)
    assert torch.equal(model.generate(height=64, width=64, **kw), plain)   # and the plain call is what it was
    with pytest.raises(ValueError, match='mask'):
        model.generate(**dict(kw, mask=mask))
    with pytest.raises(ValueError, match='strength'):
        model.generate(**dict(kw, init_image=img, strength=0.2))
    assert math.isfinite(float(kept.sum()))
