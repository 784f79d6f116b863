"""Gradient norm, clipping and the non-finite guard on the MI355X: da_segment_sumsq (three fixed-order launches), the clip
record its third launch writes, da_adamw_dev reading that record, and the trainer / optimizer / callbacks on top.

  exact cases   integer inputs |x| <= 8 on segments 1 .. 262,144 laid out with 64-float gaps: every fp32 partial is an exact
                integer <= 2^24, so the per-segment sums equal float64 bit for bit and the total is float64 rounded once
  float cases   relative error per segment and of the total against float64 of the fp32 inputs actually passed
                (bounds: tests/grad_norm_reference.py; measured margins: profiles/grad_norm_margins.json via DA_PARITY_MARGINS)
  buffers       gaps hold NaN, outputs are NaN-prefilled inside sentinel-padded buffers, the sentinels survive
With DA_PARITY_MARGINS set the worst measured values are written next to the bounds (tests/parity_margins.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import grad_norm_reference as R
from grad_norm_reference import CH

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0**-24                 # unit roundoff of fp32
SENT = 12345.0               # sentinel around every output
PADW = 64
NAN = float('nan')

# clip record, the bound an all-fp32 evaluation would need: norm = fl(fl(sqrt(S)) * grad_scale) - a correctly rounded sqrt
# and one product, (1 + u)^2 - 1 < 2.001 u; multiplier = fl(grad_scale * fl(max_norm / fl(norm + 1e-6))) - the norm's 2 u
# carried through, one add, one divide and one product, each correctly rounded: 5 u to first order.  (The kernel evaluates
# the chain in fp64 and rounds once, so it sits well inside; the reference starts from the fp32 total the record reports.)
BOUNDS = {'seg.rel': R.SEG_REL_BOUND, 'total.rel': R.TOTAL_REL_BOUND, 'clip.norm.u': 2.001, 'clip.mult.u': 5.005,
          'monitor.rel': R.SEG_REL_BOUND,
          # the AdamW constants of profiles/pointwise_edges_margins.json (tests/test_pointwise_edges_gpu.py), in units of 2^-24
          'adamw.c_p': 10.0, 'adamw.c_m': 4.0, 'adamw.c_v': 6.0}
_WORST = {}


def _margin(name, value):
    value = float(value)
    _WORST[name] = max(_WORST.get(name, 0.0), value)
    print(f'margin {name} = {value:.4g} (bound {BOUNDS[name]:.4g})')
    if os.environ.get('DA_PARITY_MARGINS'):
        from parity_margins import record
        record('grad_norm', tolerances=BOUNDS, **_WORST)
    return value <= BOUNDS[name]


@pytest.fixture(scope='module')
def ops(dev):
    from diffusion_amd import ops as o
    return o


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).clone()


def padded(n, dev, fill=NAN):
    """(whole buffer, inner view of n floats): sentinels on both sides, `fill` inside"""
    whole = torch.full((n + 2 * PADW,), SENT, device=dev, dtype=torch.float32)
    whole[PADW:PADW + n] = fill
    return whole, whole[PADW:PADW + n]


def sentinels_intact(whole, n):
    return bool((whole[:PADW] == SENT).all()) and bool((whole[PADW + n:] == SENT).all())


class Case:
    """One layout + data on the device, behind a view shifted by 4 floats (16 bytes) from the allocation."""

    def __init__(self, ops, dev, segs, total, x_np):
        self.ops, self.segs, self.x_np = ops, segs, x_np
        self.tables = R.SumsqTables(segs).to(dev)
        self.base = torch.full((total + 4,), NAN, device=dev, dtype=torch.float32)
        self.x = self.base[4:]
        self.x.copy_(torch.from_numpy(x_np))
        assert self.x.data_ptr() % 16 == 0 and self.x.data_ptr() % 64 != 0
        self.nc, self.ns = len(self.tables.chunks), len(segs)

    def run(self, grad_scale=1.0, max_norm=0.0, counter=0, x=None):
        """-> (seg_sumsq, stats words 0..3, counter, chunk partials), all on the host; checks the sentinels"""
        dev = self.base.device
        pw, partials = padded(self.nc, dev)
        sw, seg = padded(self.ns, dev)
        tw, stats = padded(self.ops.GRAD_STATS_WORDS, dev)
        stats[4:8].view(torch.int32).copy_(torch.tensor([counter, 77, 78, 79], dtype=torch.int32))
        self.ops.segment_sumsq(self.x if x is None else x, self.tables, partials, seg, stats, grad_scale, max_norm)
        torch.cuda.synchronize()
        assert sentinels_intact(pw, self.nc) and sentinels_intact(sw, self.ns) and sentinels_intact(tw, 8), 'sentinel overwritten'
        ints = stats[4:8].view(torch.int32).cpu().tolist()
        assert ints[1:] == [77, 78, 79], 'reserved words of the record written'
        return seg.cpu().numpy().copy(), stats[:4].cpu().numpy().copy(), ints[0], partials.cpu().numpy().copy()


def same(a, b):
    return all(np.array_equal(np.asarray(p).view(np.int32), np.asarray(q).view(np.int32)) for p, q in zip(a[:2], b[:2])) \
        and np.array_equal(a[3].view(np.int32), b[3].view(np.int32))


# ------------------------------------------------------------------------------------------------------- the kernel
# starts at odd multiples of 4 floats (4, 12, 20, 36), at non-multiples of 4 (1, 2, 3: the scalar head), and aligned
EXACT_SHIFTS = [0, 4, 12, 1, 0, 20, 3, 0, 36, 2, 4, 0]


def test_exact_integer_cases(dev, ops):
    rng = np.random.default_rng(1)
    sizes = R.EXACT_SIZES
    assert sizes == [1, 3, 4, 5, 63, 64, 65, CH - 1, CH, CH + 1, 2 * CH + 5, 262144]
    segs, total = R.gapped_layout(sizes, EXACT_SHIFTS)
    vals = [rng.integers(-8, 9, n).astype(np.float32) for n in sizes]
    vals[-1][:] = 8.0                                # the largest segment at the largest value: its sum is exactly 2^24
    rest = sum(int(np.sum(v.astype(np.int64)**2)) for v in vals[1:])
    vals[0][:] = 1.0 if rest % 2 == 0 else 2.0       # an odd total above 2^24: float64 -> fp32 has to round
    x = R.fill(segs, total, vals)
    assert np.isnan(x).sum() == total - sum(sizes) > 0            # every gap word is NaN
    ref, ref_total = R.reference(x, segs)
    assert ref[-1] == 2.0**24 and ref.max() <= 2.0**24
    c = Case(ops, dev, segs, total, x)
    got = c.run()
    seg, stats, counter, partials = got
    assert torch.equal(torch.from_numpy(seg).double(), torch.from_numpy(ref)), np.nonzero(seg != ref)
    assert stats[0] == np.float32(ref_total) and float(np.float32(ref_total)) != ref_total   # rounded once, and rounding happened
    assert stats[3] == 1.0 and counter == 0 and stats[2] == 1.0
    assert np.isfinite(partials).all() and (partials == np.round(partials)).all()
    assert same(got, c.run()), 'a repeated call gave other bits'


def float_case(ops, dev, seed=2):
    rng = np.random.default_rng(seed)
    vals, sizes = R.float_case_values(rng, [1, 3, 5, 63, 65, 1000, CH - 1, CH, CH + 1, 2 * CH + 5, 70001])
    segs, total = R.gapped_layout(sizes, shifts=[0, 4, 1, 12, 0, 3, 0, 20, 2, 0, 0, 0, 4])
    x = R.fill(segs, total, vals)
    return Case(ops, dev, segs, total, x), R.reference(x, segs)


def test_float_cases_against_float64(dev, ops):
    c, (ref, ref_total) = float_case(ops, dev)
    got = c.run()
    seg, stats, counter, _ = got
    assert np.isfinite(seg).all() and stats[3] == 1.0 and counter == 0
    floor = np.array([n for _, n in c.segs]) * 2.0**-126      # a square below the normal range may be lost entirely
    err = np.abs(seg.astype(np.float64) - ref)
    rel = np.max(np.maximum(err - floor, 0.0) / ref)
    rel_total = abs(float(stats[0]) - ref_total) / ref_total
    assert seg[-1] <= 300 * 2.0**-126 and seg[-2] >= 2.9e36    # the underflow and the 1e18 segments are what they claim
    ok_seg, ok_total = _margin('seg.rel', rel), _margin('total.rel', rel_total)
    assert ok_seg, f'segment sums off by {rel:.3g} relative'
    assert ok_total, f'total off by {rel_total:.3g} relative'
    assert same(got, c.run()), 'a repeated call gave other bits'


def test_past_the_grid_cap_and_forced_small_grid(dev, ops):
    """One segment of 4 * 4,194,304 + 5 floats = 2,049 chunks, one more than the 2,048-workgroup cap, so workgroup 0 walks
    two chunks; with reserve_cus = 128 the grid halves and every workgroup walks two or three.  Same bits."""
    n = 4 * 4194304 + 5
    assert -(-n // CH) == 256 * 8 + 1
    tables = R.SumsqTables([(0, n)]).to(dev)
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(n, device=dev, generator=g)
    ref = float(x.double().square().sum())

    def run():
        pw, partials = padded(len(tables.chunks), dev)
        sw, seg = padded(1, dev)
        tw, stats = padded(8, dev, 0.0)
        ops.segment_sumsq(x, tables, partials, seg, stats, 1.0, 0.0)
        torch.cuda.synchronize()
        assert sentinels_intact(pw, len(tables.chunks)) and sentinels_intact(sw, 1) and sentinels_intact(tw, 8)
        return bits(partials).cpu(), bits(seg).cpu(), bits(stats).cpu(), float(seg[0]), float(stats[0])

    a = run()
    try:
        ops.set_option('reserve_cus', 128)
        b = run()
    finally:
        ops.set_option('reserve_cus', 0)
    c = run()
    for p, q, r in zip(a[:3], b[:3], c[:3]):
        assert torch.equal(p, q), 'the result depends on the grid'
        assert torch.equal(p, r), 'a repeated call gave other bits'
    ok = _margin('seg.rel', abs(a[3] - ref) / ref)
    assert ok and _margin('total.rel', abs(a[4] - ref) / ref)


def test_nonfinite_gradient_sets_the_guard_and_counts(dev, ops):
    c, _ = float_case(ops, dev, seed=4)
    clean = c.run()
    mid = 5
    off, n = c.segs[mid]
    counter = 0
    for bad in (NAN, float('inf'), 1e20):            # 1e20: finite, its square is not
        x = c.x.clone()
        x[off + n // 2] = bad
        seg, stats, counter_new, _ = c.run(counter=counter, x=x)
        assert not np.isfinite(seg[mid]) and not np.isfinite(stats[0]), bad
        others = np.arange(len(seg)) != mid
        assert np.array_equal(seg[others].view(np.int32), clean[0][others].view(np.int32)), 'another segment changed'
        assert stats[3] == 0.0 and counter_new == counter + 1
        counter = counter_new
    assert counter == 3
    assert c.run(counter=3)[2] == 3                  # a clean pass leaves the counter alone
    # NaN total: min(1, NaN) = 1 keeps the multiplier at grad_scale (the guard word, not the multiplier, stops the step)
    x = c.x.clone()
    x[off] = NAN
    assert c.run(grad_scale=0.5, max_norm=1.0, x=x)[1][2] == 0.5


def test_clip_rule(dev, ops):
    rng = np.random.default_rng(7)
    layouts = [[np.array([3.0, 4.0], dtype=np.float32)],                        # sumsq 25, norm 5 exactly
               [rng.standard_normal(1000).astype(np.float32), (rng.standard_normal(77) * 30).astype(np.float32)]]
    for vals in layouts:
        segs, total = R.gapped_layout([len(v) for v in vals])
        c = Case(ops, dev, segs, total, R.fill(segs, total, vals))
        for gs in (1.0, 0.5):
            s0 = c.run(gs, 0.0)[1]
            norm32 = np.float32(s0[1])
            assert s0[2] == np.float32(gs)                                      # max_norm = 0: clipping off
            cases = {'under': 2.0 * float(norm32), 'equal': float(norm32), 'ulp_above': float(np.nextafter(norm32, np.float32(np.inf))),
                     'ulp_below': float(np.nextafter(norm32, np.float32(0))), 'over': 0.3 * float(norm32), 'far_over': 1e-3}
            for what, mn in cases.items():
                mn = float(np.float32(mn))
                stats = c.run(gs, mn)[1]
                assert stats[0] == s0[0] and stats[3] == 1.0
                rn, rm = R.clip_reference(stats[0], gs, mn)
                ok = _margin('clip.norm.u', abs(float(stats[1]) - rn) / (U * rn))
                assert ok, (what, gs)
                if what in ('under', 'equal', 'ulp_above'):      # no clipping applies: exactly grad_scale, not the formula
                    assert stats[2] == np.float32(gs), f'{what}: multiplier {stats[2]!r} is not exactly grad_scale {gs}'
                else:
                    ok = _margin('clip.mult.u', abs(float(stats[2]) - rm) / (U * rm))
                    assert ok, (what, gs, float(stats[2]), rm)
                    assert stats[2] < np.float32(gs), what


def test_entry_rejections_launch_nothing(dev, ops):
    c, _ = float_case(ops, dev)
    pw, partials = padded(c.nc, dev)
    sw, seg = padded(c.ns, dev)
    tw, stats = padded(8, dev)
    t = c.tables
    args = lambda x=c.x.data_ptr(), nc=c.nc, ns=c.ns: (x, t.chunk_desc.data_ptr(), nc, t.seg_desc.data_ptr(), ns, partials.data_ptr(),
                                                        seg.data_ptr(), stats.data_ptr(), 1.0, 0.0, ops._stream())
    for bad in (args(nc=0), args(nc=-1), args(ns=0), args(x=c.x.data_ptr() + 4), args(x=c.x.data_ptr() + 8)):
        with pytest.raises(RuntimeError, match='DA_ERR_SHAPE'):
            ops._lib.call('da_segment_sumsq', *bad)
    with pytest.raises(ValueError):
        ops.segment_sumsq(c.x[:c.tables.extent - 1], c.tables, partials, seg, stats)     # a table reaching past the buffer
    with pytest.raises(ValueError):
        ops.segment_sumsq(c.x, c.tables, partials[:c.nc - 1], seg, stats)
    torch.cuda.synchronize()
    for w in (pw, sw, tw):
        assert torch.isnan(w[PADW:-PADW]).all() and sentinels_intact(w, w.numel() - 2 * PADW)
    assert ops.segment_sumsq_scratch_floats(c.nc) == c.nc


# ------------------------------------------------------------------------------------------------------ da_adamw_dev
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, ema_s=0.99)


def adamw_state(n, dev, seed):
    g = torch.Generator().manual_seed(seed)
    p, gr, m = (torch.randn(n, generator=g) for _ in range(3))
    v, e = torch.rand(n, generator=g) * 1e-2, torch.randn(n, generator=g)
    return [t.to(dev) for t in (p, gr * 0.1, m * 0.01, v, e)]


def run_adamw(ops, state, n, step, use_ema, stats=None, gs=None):
    """on sentinel-padded copies -> bits of (p, m, v, ema, shadow), gradient untouched"""
    dev = state[0].device
    bufs = [padded(n, dev) for _ in range(4)]
    for (_, inner), src in zip(bufs, (state[0], state[2], state[3], state[4])):
        inner.copy_(src)
    shw = torch.full((n + 2 * PADW,), 7.0, device=dev, dtype=torch.bfloat16)
    sh = shw[PADW:PADW + n]
    (_, p), (_, m), (_, v), (_, e) = bufs
    g = state[1].clone()
    kw = dict(ema=e if use_ema else None, ema_smoothing=HYPER['ema_s'])
    if stats is not None:
        ops.adamw_dev(p, g, m, v, sh, HYPER['lr'], HYPER['b1'], HYPER['b2'], HYPER['eps'], HYPER['wd'], step, stats, **kw)
    else:
        ops.adamw(p, g, m, v, sh, HYPER['lr'], HYPER['b1'], HYPER['b2'], HYPER['eps'], HYPER['wd'], step, gs, **kw)
    torch.cuda.synchronize()
    assert all(sentinels_intact(w, n) for w, _ in bufs) and bool((shw[:PADW] == 7).all()) and bool((shw[PADW + n:] == 7).all())
    assert torch.equal(g, state[1])
    return [bits(t) for t in (p, m, v, e, sh)]


@pytest.mark.parametrize('n', [1, 3, 4, 5, 100003])
def test_adamw_dev_equals_adamw_and_skips_on_the_flag(dev, ops, n):
    state = adamw_state(n, dev, 20 + n)
    c = float(np.float32(0.37))
    for use_ema in (False, True):
        for step in (1, 7):
            stats = torch.tensor([NAN, NAN, c, 1.0, 0, 0, 0, 0], device=dev)
            got = run_adamw(ops, state, n, step, use_ema, stats=stats)
            want = run_adamw(ops, state, n, step, use_ema, gs=c)
            for a, b, what in zip(got, want, ('p', 'm', 'v', 'ema', 'shadow')):
                assert torch.equal(a, b), f'{what} differs from da_adamw (n={n}, step={step}, ema={use_ema})'
            assert not torch.equal(got[0], bits(state[0])) and (use_ema or torch.equal(got[3], bits(state[4])))
    # the guard: stats[3] == 0 -> nothing is written, whatever the buffers hold (NaN included: compared as integers)
    state[0][0] = NAN
    state[3][n - 1] = NAN
    for use_ema in (False, True):
        stats = torch.tensor([NAN, NAN, c, 0.0, 0, 0, 0, 0], device=dev)
        got = run_adamw(ops, state, n, 3, use_ema, stats=stats)
        for a, src, what in zip(got[:4], (state[0], state[2], state[3], state[4]), ('p', 'm', 'v', 'ema')):
            assert torch.equal(a, bits(src)), f'{what} written on a skipped step'
        assert torch.equal(got[4], bits(torch.full((n,), 7.0, device=dev, dtype=torch.bfloat16))), 'shadow written on a skipped step'


def test_adamw_dev_rejections_launch_nothing(dev, ops):
    n = 64
    p, g, m, v, e = [t.clone() for t in adamw_state(n + 8, dev, 30)]
    sh = torch.zeros(n + 8, device=dev, dtype=torch.bfloat16)
    stats = torch.tensor([0, 0, 1.0, 1.0, 0, 0, 0, 0], device=dev)
    before = [bits(t) for t in (p, m, v, e, sh)]

    def call(pp=p.data_ptr(), gg=g.data_ptr(), mm=m.data_ptr(), vv=v.data_ptr(), ss=sh.data_ptr(), ee=e.data_ptr(), nn=n, step=1,
             st=stats.data_ptr()):
        ops._lib.call('da_adamw_dev', pp, gg, mm, vv, ss, ee, 0.99, nn, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, st, ops._stream())

    bad = [dict(step=0), dict(step=-1), dict(nn=0), dict(nn=-5), dict(pp=p.data_ptr() + 4), dict(gg=g.data_ptr() + 8),
           dict(mm=m.data_ptr() + 4), dict(vv=v.data_ptr() + 12), dict(ee=e.data_ptr() + 4), dict(ss=sh.data_ptr() + 2), dict(st=0)]
    for kw in bad:
        with pytest.raises(RuntimeError, match='DA_ERR_SHAPE'):
            call(**kw)
    torch.cuda.synchronize()
    assert all(torch.equal(a, bits(t)) for a, t in zip(before, (p, m, v, e, sh)))
    call()
    torch.cuda.synchronize()
    assert not torch.equal(before[0], bits(p))


# ----------------------------------------------------------------------------------------------------------- trainer
def make_trainer(algorithms=None, callbacks=None, **kw):
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.optim import FusedAdamW
    from diffusion_amd.trainer import Trainer
    model = stable_diffusion_2(model_name='tiny', pretrained=False, precomputed_latents=True, fsdp=False, seed=3)
    opt = FusedAdamW(lr=1e-3, weight_decay=0.01, unet=model.unet)
    return Trainer(model, train_dataloader=None, optimizers=opt, max_duration='3ba', algorithms=algorithms, callbacks=callbacks,
                   log_every=1, **kw)


@pytest.fixture(scope='module')
def batches(dev):
    g = torch.Generator().manual_seed(11)
    B, S = 2, 16
    return [{'image_latents': torch.randn(B, 4, S, S, generator=g).half().to(dev),
             'caption_latents': torch.randn(B, 77, 128, generator=g).half().to(dev),
             '_noise': torch.randn(B, 4, S, S, generator=g).to(dev),
             '_timesteps': torch.randint(0, 1000, (B,), generator=g).to(dev)} for _ in range(3)]


def train(tr, batches, n=3):
    for b in batches[:n]:
        tr.train_batch(b)
        tr.batch_idx += 1
        for c in tr.callbacks:
            c.batch_end(tr)
    torch.cuda.synchronize()
    return tr


@pytest.fixture(scope='module')
def plain(dev, batches):
    """three steps without the feature; also the first step's state for the clipped replay"""
    tr = make_trainer()
    assert not tr.optimizer.device_scaled and 'skipped_steps' not in tr.optimizer.state_dict()
    train(tr, batches)
    u = tr.model.unet
    return {k: getattr(u, k).clone() for k in ('master', 'exp_avg', 'exp_avg_sq', 'shadow')}


def test_trainer_threshold_never_reached_equals_no_clipping(dev, batches, plain):
    from diffusion_amd.algorithms.gradient_clipping import GradientClipping
    tr = train(make_trainer(algorithms=[GradientClipping('norm', 1e30)]), batches)
    u, opt = tr.model.unet, tr.optimizer
    assert opt.device_scaled and opt.clip_max_norm == 1e30 and u.opt_step == 3
    for k in ('master', 'exp_avg', 'exp_avg_sq', 'shadow'):
        assert torch.equal(getattr(u, k), plain[k]), f'{k} differs from the run without the algorithm'
    st = opt.last_grad_stats()
    assert st['finite'] and st['skipped_steps'] == 0 and st['grad_mult'] == 1.0 and st['norm'] > 0
    assert opt.state_dict()['skipped_steps'] == 0


def test_monitor_alone_changes_nothing_and_logs(dev, batches, plain):
    from diffusion_amd.trainer import OptimizerMonitor
    tr = train(make_trainer(callbacks=[OptimizerMonitor(batch_log_interval=2)]), batches)
    assert not tr.optimizer.device_scaled
    for k in ('master', 'exp_avg', 'exp_avg_sq', 'shadow'):
        assert torch.equal(getattr(tr.model.unet, k), plain[k]), k
    assert [d['batch'] for d in tr.logs if 'l2_norm/grad/global' in d] == [2]      # every second batch


def test_trainer_clipped_step_monitor_and_guard(dev, ops, batches, monkeypatch, capsys):
    """(b) a biting threshold against a host replay, (c) the monitor's keys and values, (d) a NaN gradient word skips the
    step bit for bit and the next clean step updates, (e) sliced AdamW is overridden off.  The monitor reports the norm
    backward produced, i.e. BEFORE clipping."""
    from diffusion_amd.algorithms.gradient_clipping import GradientClipping
    from diffusion_amd.trainer import OptimizerMonitor
    probe = train(make_trainer(algorithms=[GradientClipping('norm', 1e30)]), batches, n=1)
    norm1 = probe.optimizer.last_grad_stats()['norm']
    assert np.isfinite(norm1) and norm1 > 0
    thr = norm1 / 2

    monkeypatch.setenv('DA_SLICED_ADAMW', '1')
    mon = OptimizerMonitor()
    tr = make_trainer(algorithms=[GradientClipping('norm', thr)], callbacks=[mon])
    assert tr.sliced_optimizer is False                                             # (e)
    assert 'sliced AdamW off' in capsys.readouterr().out
    u, opt = tr.model.unet, tr.optimizer
    before = {k: getattr(u, k).clone() for k in ('master', 'exp_avg', 'exp_avg_sq', 'shadow')}
    train(tr, batches, n=1)
    st = opt.last_grad_stats()
    names, offs, numels, _ = u.grad_segments()

    # (b) replay: the same gradient buffer, the coefficient in float64 on the host, da_adamw
    gnorm = float(u.grad.double().norm())                                           # gaps of the real buffer are zero
    assert abs(st['norm'] - gnorm) <= R.TOTAL_REL_BOUND * gnorm and st['norm'] == pytest.approx(norm1, rel=1e-6)
    coef = min(1.0, thr / (gnorm + 1e-6))
    assert coef < 0.51 and st['grad_mult'] == pytest.approx(coef, rel=1e-5)
    hp = opt.param_groups[0]
    p, m, v, sh = (before[k].clone() for k in ('master', 'exp_avg', 'exp_avg_sq', 'shadow'))
    ops.adamw(p, u.grad, m, v, sh, hp['lr'], hp['betas'][0], hp['betas'][1], hp['eps'], hp['weight_decay'], 1, coef)
    g64, b1, b2 = u.grad.double() * coef, hp['betas'][0], hp['betas'][1]
    decayed = before['master'].double() * (1 - hp['lr'] * hp['weight_decay'])
    mag_p = decayed.abs() + (p.double() - decayed).abs()
    mag_m = (b1 * before['exp_avg'].double()).abs() + ((1 - b1) * g64).abs()
    live = mag_m > 0
    moved = mag_p > 0                                                               # gap words: p = 0, g = 0, nothing moves
    assert torch.equal(u.master[~moved], p[~moved])
    c_p = ((u.master.double() - p.double()).abs()[moved] / (U * mag_p[moved])).max()
    c_m = ((u.exp_avg.double() - m.double()).abs()[live] / (U * mag_m[live])).max()
    vv = v.double()
    c_v = ((u.exp_avg_sq.double() - vv).abs()[vv > 1e-30] / (U * vv[vv > 1e-30])).max()
    assert torch.equal(u.exp_avg[~live], m[~live])
    ok = [_margin('adamw.c_p', c_p), _margin('adamw.c_m', c_m), _margin('adamw.c_v', c_v)]
    assert all(ok), (float(c_p), float(c_m), float(c_v))
    assert not torch.equal(u.master, before['master'])

    # (c) the monitor: {'global'} + storages, each sqrt(sumsq) / world - the unclipped norms
    log = next(d for d in reversed(tr.logs) if 'l2_norm/grad/global' in d)
    keys = {k[len('l2_norm/grad/'):] for k in log if k.startswith('l2_norm/grad/')}
    assert keys == {'global'} | set(names) and 'global' not in names
    worst = abs(log['l2_norm/grad/global'] - gnorm) / gnorm
    for name, off, n in zip(names, offs, numels):
        ref = float(u.grad[off:off + n].double().norm()) / tr.world
        got = log[f'l2_norm/grad/{name}']
        if ref == 0.0:
            assert got == 0.0, name
        else:
            worst = max(worst, abs(got - ref) / ref)
    assert _margin('monitor.rel', worst)
    assert log['l2_norm/grad/global'] > 1.9 * thr                                   # not the clipped norm

    # (d) a NaN in one gradient word: nothing moves, the device counts one skipped step, the host step still advances
    snap = [bits(t) for t in (u.master, u.exp_avg, u.exp_avg_sq, u.shadow, u.shadow_t)]
    opt.ema = u.master.clone() + 1.0
    opt.ema_smoothing, opt.ema_update_this_step = 0.5, True
    ema_bits = bits(opt.ema)
    word = offs[len(offs) // 2] + 1
    keep = u.grad[word].clone()
    u.grad[word] = NAN
    step_before = u.opt_step
    opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(a, bits(t)) for a, t in zip(snap, (u.master, u.exp_avg, u.exp_avg_sq, u.shadow, u.shadow_t)))
    assert torch.equal(ema_bits, bits(opt.ema)), 'EMA written on a skipped step'
    st = opt.last_grad_stats()
    assert st['skipped_steps'] == 1 and not st['finite'] and u.opt_step == step_before + 1
    assert opt.state_dict()['skipped_steps'] == 1
    u.grad[word] = keep
    opt.step()
    torch.cuda.synchronize()
    st = opt.last_grad_stats()
    assert st['skipped_steps'] == 1 and st['finite']
    assert not torch.equal(snap[0], bits(u.master)) and not torch.equal(ema_bits, bits(opt.ema))
    assert torch.isfinite(u.master).all() and torch.isfinite(opt.ema).all()
    # checkpoints: the counter rides along; one written without the feature still loads
    sd = opt.state_dict()
    sd['skipped_steps'] = 5
    opt.load_state_dict(sd)
    assert opt.last_grad_stats()['skipped_steps'] == 5
    del sd['skipped_steps']
    opt.load_state_dict(sd)
    assert opt.last_grad_stats()['skipped_steps'] == 5


# --------------------------------------------------------------------------------------------------------- two ranks
def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return str(sk.getsockname()[1])


@pytest.mark.parametrize('collective,payload', [(None, None), ('rs_ag', 'bf16')])
def test_two_ranks_agree_on_the_record_and_the_weights(dev, tmp_path, collective, payload):
    """Every rank computes the norm locally from the exchanged gradient (no collective added): the records and the master
    weights after two clipped steps must be equal bit for bit across the ranks."""
    out = str(tmp_path / 'r')
    env = dict(os.environ, PYTHONPATH=ROOT, DA_DIST_BACKEND='gloo')
    env.pop('HSA_ENABLE_IPC_MODE_LEGACY', None)
    if collective:
        env.update(DA_DP_COLLECTIVE=collective, DA_DP_PAYLOAD=payload)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
           '--master-port', _free_port(), os.path.join(ROOT, 'tests', 'grad_norm_dp_worker.py'), out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    a, b = torch.load(out + '.rank0.pt'), torch.load(out + '.rank1.pt')
    assert a['world'] == 2 and a['reducer_enabled'] and a['sliced'] is False
    for sa, sb in zip(a['stats'], b['stats']):
        assert torch.equal(sa.view(torch.int32), sb.view(torch.int32)), 'the ranks disagree on the record'
        mult, finite = float(sa[2]), float(sa[3])
        assert finite == 1.0 and 0 < mult < 0.5, 'the threshold did not bite'
    assert torch.equal(a['master'].view(torch.int32), b['master'].view(torch.int32))
    assert not torch.equal(a['master'], a['before'])
