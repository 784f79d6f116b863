"""CPU-only tests of the gradient-norm feature's host side: the Hydra aliases of GradientClipping and OptimizerMonitor,
their argument checks, the chunk / segment tables of da_segment_sumsq on hand-made layouts, the tiny and the full-width
U-Net, and a numpy emulation of the kernel's three-stage summation order held to the bound the GPU module asserts."""
import os
import re
import struct

import numpy as np
import pytest

import grad_norm_reference as R
from grad_norm_reference import CH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_aliases_resolve_clipping_and_monitor_and_nothing_else():
    from diffusion_amd import hydra_lite as h
    from diffusion_amd.algorithms.gradient_clipping import GradientClipping
    from diffusion_amd.trainer import NoOpCallback, OptimizerMonitor
    assert h.resolve_target('composer.algorithms.GradientClipping') is GradientClipping
    assert h.resolve_target('composer.algorithms.gradient_clipping.GradientClipping') is GradientClipping
    assert h.resolve_target('composer.callbacks.OptimizerMonitor') is OptimizerMonitor
    assert h.resolve_target('composer.callbacks.optimizer_monitor.OptimizerMonitor') is OptimizerMonitor
    assert h.resolve_target('composer.callbacks.lr_monitor.LRMonitor') is NoOpCallback
    assert h.resolve_target('composer.algorithms.SomethingElse') is NoOpCallback
    assert 'OptimizerMonitor' not in NoOpCallback.__doc__
    alg = h.instantiate({'_target_': 'composer.algorithms.GradientClipping', 'clipping_type': 'norm', 'clipping_threshold': 1.0})
    assert isinstance(alg, GradientClipping) and alg.clipping_threshold == 1.0 and hasattr(alg, 'before_optimizer_step')
    mon = h.instantiate({'_target_': 'composer.callbacks.OptimizerMonitor', 'log_optimizer_metrics': True})
    assert isinstance(mon, OptimizerMonitor)


def test_argument_checks():
    from diffusion_amd.algorithms.gradient_clipping import GradientClipping
    from diffusion_amd.trainer import OptimizerMonitor
    for kind in ('value', 'adaptive'):
        with pytest.raises(NotImplementedError, match=kind):
            GradientClipping(kind, 1.0)
    with pytest.raises(ValueError):
        GradientClipping('norm', -1.0)
    with pytest.raises(ValueError):
        GradientClipping('norm', float('nan'))
    with pytest.raises(ValueError):
        GradientClipping('nrom', 1.0)
    with pytest.raises(ValueError):
        OptimizerMonitor(batch_log_interval=0)

    class Opt:
        clip_max_norm, guard_nonfinite = None, False
    o = Opt()
    GradientClipping('norm', 0.5).configure_optimizer(o)
    assert o.clip_max_norm == 0.5 and o.guard_nonfinite is True


def test_chunk_constant_matches_the_header():
    hdr = open(os.path.join(ROOT, 'include', 'diffusion_amd.h')).read()
    assert int(re.search(r'#define DA_SUMSQ_CHUNK (\d+)', hdr).group(1)) == CH
    assert CH % 1024 == 0


def check_tables(segs, total=None):
    """The properties da_segment_sumsq relies on; returns the tables."""
    tb = R.SumsqTables(segs)
    assert len(tb.segs) == len(segs)
    covered = 0
    for s, ((off, n), (first, cnt)) in enumerate(zip(segs, tb.segs)):
        mine = tb.chunks[first:first + cnt]
        assert cnt == -(-n // CH) and first == covered
        pos = off
        for coff, cn, cseg in mine:               # tile the segment, in order, no overlap, never past its end
            assert cseg == s and coff == pos and 1 <= cn <= CH
            pos += cn
        assert pos == off + n
        assert all(cn == CH for _, cn, _ in mine[:-1])
        covered += cnt
    assert covered == len(tb.chunks) and tb.extent == segs[-1][0] + segs[-1][1]
    if total is not None:                         # no chunk touches a word outside the segments (the alignment gaps)
        owner = np.zeros(total, dtype=np.int32)
        for off, n in segs:
            owner[off:off + n] += 1
        hit = np.zeros(total, dtype=np.int32)
        for coff, cn, _ in tb.chunks:
            hit[coff:coff + cn] += 1
        assert np.array_equal(owner, hit) and owner.max() == 1
    cb, sb = tb.pack()
    assert len(cb) == 16 * len(tb.chunks) and len(sb) == 8 * len(tb.segs)
    assert struct.unpack_from('<qii', cb, 16 * (len(tb.chunks) - 1)) == tb.chunks[-1]
    assert struct.unpack_from('<ii', sb, 8 * (len(tb.segs) - 1)) == tb.segs[-1]
    return tb


def test_tables_of_hand_made_layouts():
    sizes = [1, CH - 1, CH, CH + 1, 2 * CH + 5, 3, 64, 65]
    segs, total = R.gapped_layout(sizes)
    tb = check_tables(segs, total)
    assert [c for _, c in tb.segs] == [1, 1, 1, 2, 3, 1, 1, 1]
    segs, total = R.gapped_layout(sizes, shifts=[4, 12, 1, 0, 20, 3, 0, 36])
    check_tables(segs, total)
    for bad in ([], [(0, 0)], [(64, 10), (0, 10)], [(0, 65), (64, 3)]):
        with pytest.raises(ValueError):
            R.SumsqTables(bad)


@pytest.mark.parametrize('width', ['tiny', 'full'])
def test_tables_of_the_unet_layouts(width):
    from diffusion_amd.models.unet import UNetConfig, build_layout, grad_segment_list
    cfg = UNetConfig.tiny() if width == 'tiny' else UNetConfig()
    fp = build_layout(cfg)[0]
    names, offs, numels = grad_segment_list(fp)
    assert names == list(fp.storages)                                   # exactly the storages, in flat order
    assert offs == sorted(offs) and all(o % fp.ALIGN == 0 for o in offs)
    assert [(fp.storages[n].off, fp.storages[n].numel) for n in names] == list(zip(offs, numels))
    tb = check_tables(list(zip(offs, numels)), fp.total if width == 'tiny' else None)
    assert tb.extent <= fp.total
    assert sum(n for _, n, _ in tb.chunks) == sum(numels)
    if width == 'full':
        assert sum(numels) > 865_000_000 and len(names) > 500
        assert len(tb.chunks) < 2**31 and max(o + n for o, n, _ in tb.chunks) == tb.extent


def test_emulated_three_stage_order_meets_the_gpu_bound():
    """The order the kernel sums in, emulated in numpy fp32 / fp64, against float64 on the float cases of the GPU module:
    the bound asserted on the MI355X is one this order can meet (it is no artefact of the hardware's fused multiply-adds)."""
    rng = np.random.default_rng(5)
    vals, sizes = R.float_case_values(rng, [1, 5, 65, 1000, CH - 1, CH + 1, 2 * CH + 5, 70001])
    segs, total = R.gapped_layout(sizes, shifts=[0, 4, 1, 12, 0, 3, 0, 0, 0, 0])
    x = R.fill(segs, total, vals)
    ref, ref_total = R.reference(x, segs)
    seg, tot = R.emulate(x, segs)
    assert np.isfinite(seg).all() and np.isfinite(tot)
    floor = np.array([n for _, n in segs]) * 2.0**-126       # squares that underflow: at most the smallest normal each
    err = np.abs(seg.astype(np.float64) - ref)
    assert (err <= R.SEG_REL_BOUND * ref + floor).all(), (err / ref).max()
    assert abs(float(tot) - ref_total) <= R.TOTAL_REL_BOUND * ref_total
    assert seg[-1] == 0.0 and ref[-1] > 0                     # the underflow segment really underflows


def test_emulation_is_exact_on_small_integers():
    rng = np.random.default_rng(6)
    sizes = [1, 3, 4, 5, 63, 64, 65, CH - 1, CH + 1, 2 * CH + 5]
    segs, total = R.gapped_layout(sizes, shifts=[0, 4, 12, 1, 0, 0, 20, 0, 0, 2])
    x = R.fill(segs, total, [rng.integers(-8, 9, n).astype(np.float32) for n in sizes])
    ref, ref_total = R.reference(x, segs)
    seg, tot = R.emulate(x, segs)
    assert np.array_equal(seg.astype(np.float64), ref) and float(tot) == float(np.float32(ref_total))


def test_clip_rule_reference():
    n, m = R.clip_reference(np.float32(16.0), 0.5, 1.0)
    assert n == 2.0 and abs(m - 0.5 * 1.0 / (2.0 + 1e-6)) < 1e-15
    assert R.clip_reference(np.float32(16.0), 0.5, 0.0) == (2.0, 0.5)
    assert R.clip_reference(np.float32(16.0), 1.0, 8.0) == (4.0, 1.0)
