"""GPU tests of ``da_add_noise_rng``: the noising launch that draws its own timesteps and noise.  Every comparison is bitwise.
The oracles are the existing entries: ``da_add_noise_ex`` for the arithmetic and ``da_randn_philox`` for the draws (itself
checked against tests/philox_reference.py elsewhere); timesteps against the NumPy restatement in train_noise_reference.py.

Not covered here: the rejection of H W > 2^31 - 1, which no tensor of a test's size can express (``HW`` is a C int at the ABI,
and ``ops.add_noise_rng`` refuses the shape before the call)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_noise_reference as TR  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS = [0, 2**64 - 1, 0x9E3779B97F4A7C15]
KINDS = ('epsilon', 'v_prediction', 'sample')
T_MAX = float(np.float32(1.570795))
CS = (1, 3, 4, 8)
HWS = ((1, 1), (5, 7), (8, 8), (32, 32))


@pytest.fixture(scope='module')
def tables(dev):
    from diffusion_amd.models.schedulers import DDPMScheduler
    return DDPMScheduler().device_tables(dev)


def _seeds(dev, B):
    from diffusion_amd import ops
    return ops.philox_seeds(SEEDS[:B] if B > 1 else SEEDS[2:3], B, dev)


def _x0(dev, B, C, H, W):
    g = torch.Generator().manual_seed(1000 * C + 10 * H + W)
    return torch.randn(3, C, H, W, generator=g)[3 - B:].contiguous().to(dev)   # sample B - 1 is the same for every B


def _bufs(dev, npix):
    """outputs pre-filled with NaN: a channel the kernel skipped, or a launch that wrote after a rejection, shows"""
    xt = torch.full((npix, 8), float('nan'), device=dev, dtype=torch.bfloat16)
    tg = torch.full((npix, 8), float('nan'), device=dev, dtype=torch.float32)
    return xt, tg


def _bits(xt, tg):
    return xt.view(torch.int16).cpu(), tg.view(torch.int32).cpu()


def _rng(dev, tables, x0, seeds, kind, cont, t=None, **kw):
    from diffusion_amd import ops
    B, C, H, W = x0.shape
    xt, tg = _bufs(dev, B * H * W)
    draw = t is None
    if draw:
        t = torch.full((B,), -7, device=dev, dtype=torch.float32 if cont else torch.int64)
    if cont:
        kw.setdefault('t_range', (0.0, T_MAX))
        ops.add_noise_rng(x0, seeds, t, xt, tg, kind, draw_t=draw, **kw)
    else:
        ops.add_noise_rng(x0, seeds, t, xt, tg, kind, *tables, draw_t=draw, **kw)
    return xt, tg, t


def _ex(dev, tables, x0, eps, t, kind):
    from diffusion_amd import ops
    B, C, H, W = x0.shape
    xt, tg = _bufs(dev, B * H * W)
    ops.add_noise_ex(x0, eps.contiguous(), t, xt, tg, kind, *(() if t.dtype == torch.float32 else tables))
    return xt, tg


def _words(dev, seeds):
    from diffusion_amd import ops
    w = ops.randn_philox(seeds, 3, 0, (seeds.numel(), 4, 1, 1), kind=1)[:, 0, 0, 0]
    return [int(v) & 0xFFFFFFFF for v in w.view(torch.int32).cpu().tolist()]


def test_drawn_timesteps_equal_the_reference_formulas(dev, tables):
    B = 3
    seeds, x0 = _seeds(dev, B), _x0(dev, B, 4, 8, 8)
    words = _words(dev, seeds)
    assert words == [TR.timestep_word(s) for s in SEEDS]   # the word behind t is draw 3, counter (0, 3, 0, 0), r0
    for lo, hi in ((0, 1000), (20, 980), (0, 1), (999, 1000), (500, 503)):
        t = _rng(dev, tables, x0, seeds, 'epsilon', False, t_range=(lo, hi))[2]
        assert t.cpu().tolist() == [TR.discrete_t(w, lo, hi) for w in words]
        for n_slots, slots in ((3, [0, 1, 2]), (7, [6, 0, 3]), (2048, [2047, 1024, 0])):
            sl = torch.tensor(slots, dtype=torch.int32, device=dev)
            t = _rng(dev, tables, x0, seeds, 'epsilon', False, t_range=(lo, hi), slots=sl, n_slots=n_slots)[2].cpu().tolist()
            assert t == [TR.discrete_t(w, lo, hi, s, n_slots) for w, s in zip(words, slots)]
            for tt, s in zip(t, slots):
                a, b = TR.stratum(lo, hi, s, n_slots)
                assert lo <= a <= tt < b <= hi
    for lo, hi in ((0.0, T_MAX), (float(np.float32(0.3)), float(np.float32(1.2)))):
        t = _rng(dev, tables, x0, seeds, 'epsilon', True, t_range=(lo, hi))[2]
        want = np.array([TR.continuous_t(w, lo, hi) for w in words], dtype=np.float32)
        assert np.array_equal(t.cpu().numpy().view(np.int32), want.view(np.int32))
        for n_slots, slots in ((3, [0, 1, 2]), (7, [6, 0, 3])):
            sl = torch.tensor(slots, dtype=torch.int32, device=dev)
            t = _rng(dev, tables, x0, seeds, 'epsilon', True, t_range=(lo, hi), slots=sl, n_slots=n_slots)[2]
            want = np.array([TR.continuous_t(w, lo, hi, s, n_slots) for w, s in zip(words, slots)], dtype=np.float32)
            assert np.array_equal(t.cpu().numpy().view(np.int32), want.view(np.int32))
            assert all(lo <= v < hi for v in t.cpu().tolist())


@pytest.mark.parametrize('hw', HWS, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('C', CS)
def test_plain_draw_equals_add_noise_ex_of_randn_philox(dev, tables, C, hw):
    """both options 0: the launch is da_add_noise_ex fed da_randn_philox's draw 0, and writes the timesteps it used"""
    from diffusion_amd import ops
    H, W = hw
    for B in (1, 3):
        seeds, x0 = _seeds(dev, B), _x0(dev, B, C, H, W)
        n = ops.randn_philox(seeds, 0, 0, (B, C, H, W))
        for cont in (False, True):
            for kind in KINDS:
                xt, tg, t = _rng(dev, tables, x0, seeds, kind, cont)
                assert t.dtype == (torch.float32 if cont else torch.int64)
                assert bool(((t >= 0) & (t < (T_MAX if cont else 1000))).all())
                xt_ref, tg_ref = _ex(dev, tables, x0, n, t, kind)
                for got, want in zip(_bits(xt, tg), _bits(xt_ref, tg_ref)):
                    assert torch.equal(got, want), (B, cont, kind)
                # pad channels: +0 bit patterns over the NaN the buffers held
                assert not _bits(xt, tg)[0][:, C:].any() and not _bits(xt, tg)[1][:, C:].any()
                if kind == 'epsilon':
                    got = tg.view(B, H, W, 8)[..., :C].permute(0, 3, 1, 2).contiguous()
                    assert torch.equal(got.view(torch.int32), n.view(torch.int32))


@pytest.mark.parametrize('hw', HWS, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('C', CS)
def test_offset_and_perturbation_compose_as_in_numpy(dev, tables, C, hw):
    """n1 = n + fl(0.1 zc), n2 = n1 + fl(0.1 z2) in float32: x_t is add_noise_ex's of n2, the target add_noise_ex's of n1"""
    from diffusion_amd import ops
    H, W = hw
    for B in (1, 3):
        seeds, x0 = _seeds(dev, B), _x0(dev, B, C, H, W)
        n = ops.randn_philox(seeds, 0, 0, (B, C, H, W)).cpu().numpy()
        z2 = ops.randn_philox(seeds, 1, 0, (B, C, H, W)).cpu().numpy()
        zc = ops.randn_philox(seeds, 2, 0, (B, C, 1, 1)).cpu().numpy()
        for off, pert in ((0.1, 0.1), (0.1, 0.0), (0.0, 0.1)):
            n1, n2 = TR.compose(n, zc, z2, off, pert)
            n1, n2 = torch.from_numpy(np.ascontiguousarray(n1)).to(dev), torch.from_numpy(np.ascontiguousarray(n2)).to(dev)
            for cont in (False, True):
                for kind in KINDS:
                    xt, tg, t = _rng(dev, tables, x0, seeds, kind, cont, noise_offset=off, perturbation=pert)
                    xt_ref = _ex(dev, tables, x0, n2, t, kind)[0]
                    tg_ref = _ex(dev, tables, x0, n1, t, kind)[1]
                    assert torch.equal(_bits(xt, tg)[0], xt_ref.view(torch.int16).cpu()), (B, off, pert, cont, kind)
                    assert torch.equal(_bits(xt, tg)[1], tg_ref.view(torch.int32).cpu()), (B, off, pert, cont, kind)


@pytest.mark.parametrize('cont', (False, True))
def test_a_sample_does_not_depend_on_its_batch(dev, tables, cont):
    """seed s alone at B = 1 and at position 2 of B = 3: the same timestep and the same rows"""
    for C, (H, W) in ((3, (5, 7)), (8, (32, 32))):
        for kind in KINDS:
            kw = dict(noise_offset=0.1, perturbation=0.1)
            xt1, tg1, t1 = _rng(dev, tables, _x0(dev, 1, C, H, W), _seeds(dev, 1), kind, cont, **kw)
            xt3, tg3, t3 = _rng(dev, tables, _x0(dev, 3, C, H, W), _seeds(dev, 3), kind, cont, **kw)
            assert torch.equal(t1.cpu(), t3[2:].cpu())
            a, b = _bits(xt1, tg1), _bits(xt3[2 * H * W:], tg3[2 * H * W:])
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_injected_timesteps_are_read_and_left_alone(dev, tables):
    from diffusion_amd import ops
    B, C, H, W = 3, 4, 8, 8
    seeds, x0 = _seeds(dev, B), _x0(dev, B, C, H, W)
    n = ops.randn_philox(seeds, 0, 0, (B, C, H, W))
    for cont, t in ((False, torch.tensor([0, 999, 417], device=dev)),
                    (True, torch.tensor([0.0, 1.5, 0.7], device=dev, dtype=torch.float32))):
        keep = t.clone()
        xt, tg, t_out = _rng(dev, tables, x0, seeds, 'v_prediction', cont, t=t)
        assert t_out is t and torch.equal(t, keep)
        ref = _ex(dev, tables, x0, n, t, 'v_prediction')
        assert torch.equal(_bits(xt, tg)[0], _bits(*ref)[0]) and torch.equal(_bits(xt, tg)[1], _bits(*ref)[1])


def test_table_edges(dev, tables):
    """t_lo = 0 and t_hi = 1000: a range of one timestep at either end of the table gives that timestep, and its table entry"""
    from diffusion_amd import ops
    B, C, H, W = 3, 4, 5, 7
    seeds, x0 = _seeds(dev, B), _x0(dev, B, C, H, W)
    n = ops.randn_philox(seeds, 0, 0, (B, C, H, W))
    for lo, hi in ((0, 1), (999, 1000)):
        for kw in ({}, dict(slots=torch.tensor([2, 0, 1], dtype=torch.int32, device=dev), n_slots=3)):
            xt, tg, t = _rng(dev, tables, x0, seeds, 'v_prediction', False, t_range=(lo, hi), **kw)
            assert t.cpu().tolist() == [lo] * B
            ref = _ex(dev, tables, x0, n, t, 'v_prediction')
            assert torch.equal(_bits(xt, tg)[0], _bits(*ref)[0]) and torch.equal(_bits(xt, tg)[1], _bits(*ref)[1])


def test_rejections_write_nothing(dev, tables):
    """every argument set the header lists returns DA_ERR_SHAPE from the entry itself and leaves xt, target and t as they were;
    the wrapper refuses the same with ValueError before any call"""
    from diffusion_amd import _lib, ops
    B, C, H, W = 2, 4, 4, 4
    HW = H * W
    x0, seeds = _x0(dev, B, C, H, W), _seeds(dev, 2)
    xt, tg = _bufs(dev, B * HW + 1)
    t = torch.full((B + 1,), -7, device=dev, dtype=torch.int64)
    tf = torch.full((B + 1,), -7.0, device=dev, dtype=torch.float32)
    slots = torch.zeros(B, dtype=torch.int32, device=dev)
    sa, sb = tables
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(x0=x0.data_ptr(), seeds=seeds.data_ptr(), slot=None, n_slots=0, t=t.data_ptr(), t_is_f32=0, draw_t=1,
                t_lo=0.0, t_hi=1000.0, sa=sa.data_ptr(), sb=sb.data_ptr(), T=1000, off=0.0, pert=0.0, xt=xt.data_ptr(),
                tg=tg.data_ptr(), B=B, C=C, HW=HW, kind=0, stream=stream)
    nan, inf = float('nan'), float('inf')
    bad = [dict(C=0), dict(C=9), dict(kind=3), dict(kind=-1), dict(B=0), dict(HW=0), dict(HW=-1),
           dict(t_lo=5.0, t_hi=5.0), dict(t_lo=6.0, t_hi=5.0), dict(t_lo=-1.0), dict(t_hi=1001.0), dict(t_lo=0.5),
           dict(n_slots=-1), dict(n_slots=4), dict(slot=slots.data_ptr()),
           dict(slot=slots.data_ptr(), n_slots=2**23),            # n_slots R = 2^23 1000 >= 2^32
           dict(x0=None), dict(seeds=None), dict(t=None), dict(xt=None), dict(tg=None),
           dict(seeds=seeds.data_ptr() + 4), dict(xt=xt.data_ptr() + 2), dict(tg=tg.data_ptr() + 4),
           dict(sa=None), dict(sb=None), dict(T=0),
           dict(off=nan), dict(off=inf), dict(pert=nan), dict(pert=-inf),
           dict(t=tf.data_ptr(), t_is_f32=1, t_lo=1.0, t_hi=1.0),
           dict(t=tf.data_ptr(), t_is_f32=1, t_lo=0.0, t_hi=0.1),   # 0.1 is no fp32 value
           dict(t=tf.data_ptr(), t_is_f32=1, t_lo=0.0, t_hi=inf)]
    fn = _lib.load().da_add_noise_rng
    for delta in bad:
        assert fn(*dict(good, **delta).values()) == 1, delta
    torch.cuda.synchronize()
    assert bool(torch.isnan(xt.float()).all()) and bool(torch.isnan(tg).all())
    assert bool((t == -7).all()) and bool((tf == -7).all())
    assert fn(*good.values()) == 0   # the arguments they were derived from are accepted: each change was the reason
    torch.cuda.synchronize()
    assert bool((t[:B] >= 0).all()) and t[B].item() == -7 and not bool(torch.isnan(tg[:B * HW]).any())
    # the wrapper: ValueError before a launch
    xt3, tg3 = _bufs(dev, B * HW)
    t3 = torch.full((B,), -7, device=dev, dtype=torch.int64)
    t3f = torch.full((B,), -7.0, device=dev, dtype=torch.float32)
    for args, kw in (((x0, seeds, t3, xt3, tg3, 'epsilon'), {}),                               # missing tables
                     ((x0, seeds, t3, xt3, tg3, 'noise', sa, sb), {}),
                     ((x0, seeds, t3, xt3, tg3, 'epsilon', sa, sb), dict(t_range=(5, 5))),
                     ((x0, seeds, t3, xt3, tg3, 'epsilon', sa, sb), dict(t_range=(0, 1001))),
                     ((x0, seeds, t3, xt3, tg3, 'epsilon', sa, sb), dict(t_range=(0.5, 10))),
                     ((x0, seeds, t3, xt3, tg3, 'epsilon', sa, sb), dict(n_slots=2)),
                     ((x0, seeds, t3, xt3, tg3, 'epsilon', sa, sb), dict(slots=slots)),
                     ((x0, seeds, t3, xt3, tg3, 'epsilon', sa, sb), dict(slots=slots, n_slots=-1)),
                     ((x0, seeds, t3, xt3, tg3, 'epsilon', sa, sb), dict(slots=slots, n_slots=2**23)),
                     ((x0, seeds, t3, xt3, tg3, 'epsilon', sa, sb), dict(noise_offset=nan)),
                     ((x0, seeds, t3, xt3, tg3, 'epsilon', sa, sb), dict(perturbation=inf)),
                     ((x0, seeds.view(torch.int64), t3, xt3, tg3, 'epsilon', sa, sb), {}),
                     ((x0, seeds[:1], t3, xt3, tg3, 'epsilon', sa, sb), {}),
                     ((x0, seeds, t3.int(), xt3, tg3, 'epsilon', sa, sb), {}),
                     ((x0, seeds, t3f, xt3, tg3, 'epsilon'), {}),                              # continuous without a range
                     ((x0, seeds, t3f, xt3, tg3, 'epsilon'), dict(t_range=(1.0, 1.0))),
                     ((x0.expand(B, C, H, W)[:, :, :, ::2], seeds, t3, xt3, tg3, 'epsilon', sa, sb), {}),
                     ((torch.zeros(B, 9, H, W, device=dev), seeds, t3, xt3, tg3, 'epsilon', sa, sb), {}),
                     ((x0, seeds, t3, xt3[1:], tg3, 'epsilon', sa, sb), {})):
        with pytest.raises(ValueError):
            ops.add_noise_rng(*args, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(xt3.float()).all()) and bool(torch.isnan(tg3).all()) and bool((t3 == -7).all())
