"""GPU tests of ``da_image_resize`` / ``ops.image_resize``: every geometry x filter x range against the float64 restatement
of tests/resize_reference.py, kind 0 as the bf16 of kind 1, ``(0, 0, 0)`` bit for bit against the two ingest entries, exact
constants under range 1, and the argument checks.

All sources live in ONE packed upload (differently sized images back to back: odd byte offsets) and each launch selects
its images through the offset table; the float64 references are computed once per (source, target, switches)."""
import functools
import itertools

import numpy as np
import pytest
import torch

import parity_margins
import resize_reference as RR

pytestmark = pytest.mark.gpu

SOURCES = {}   # name -> (h, w), packed in this order
LAUNCHES = {}  # (Rh, Rw) -> the sources that go to it, one launch per target
for (_h, _w), _t in RR.CASES:
    SOURCES.setdefault(f'{_h}x{_w}', (_h, _w))
    LAUNCHES.setdefault(_t, []).append(f'{_h}x{_w}')
SWITCHES = list(itertools.product((0, 1), (0, 1), (0, 1)))   # geometry, filter, range


@pytest.fixture(scope='module')
def packed(dev):
    from diffusion_amd.datasets.image_ingest import pack_images
    imgs = {name: RR.seeded_image(h, w, 400 + k) for k, (name, (h, w)) in enumerate(SOURCES.items())}
    raw, off, hw = pack_images([torch.from_numpy(im) for im in imgs.values()])
    assert sum(int(o) % 2 for o in off) >= 2   # at least two images begin at odd byte offsets
    return {'imgs': imgs, 'raw': raw.to(dev), 'off': off, 'hw': hw, 'index': {name: i for i, name in enumerate(imgs)}}


@functools.lru_cache(maxsize=None)
def _ref(name, target, sw, seed):
    h, w = SOURCES[name]
    return RR.resize_f64(RR.seeded_image(h, w, seed), *target, *sw)


def _tables(packed, names, dev):
    sel = torch.tensor([packed['index'][n] for n in names])
    off, hw = packed['off'][sel].contiguous(), packed['hw'][sel].contiguous()
    return off, hw, off.to(dev), hw.to(dev)


def _launch(packed, names, Rh, Rw, kind, dev, sw=None, entry='resize'):
    from diffusion_amd import ops
    off, hw, d_off, d_hw = _tables(packed, names, dev)
    B = len(names)
    if kind == 0:
        out = torch.full((B * Rh * Rw, 8), float('nan'), device=dev, dtype=torch.bfloat16)
    else:
        out = torch.full((B, 3, Rh, Rw), float('nan'), device=dev, dtype=torch.float32)
    if entry == 'square':
        ops.image_ingest(packed['raw'], d_off, d_hw, Rh, out, kind, host=(off, hw))
    elif entry == 'rect':
        ops.image_ingest_rect(packed['raw'], d_off, d_hw, Rh, Rw, out, kind, host=(off, hw))
    else:
        ops.image_resize(packed['raw'], d_off, d_hw, Rh, Rw, out, kind, *sw, host=(off, hw))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('sw', SWITCHES, ids=lambda s: 'g%d-f%d-r%d' % s)
@pytest.mark.parametrize('target', list(LAUNCHES), ids=lambda t: f'{t[0]}x{t[1]}')
def test_kind1_matches_float64_and_kind0_is_its_bf16(packed, dev, target, sw):
    """kind 1 within 1e-5 of the float64 restatement (two fp32 roundings, the row cache at 255 * 2**-24 / 127.5 = 1.2e-7 and
    the output at 2**-24: the project's bound for the ingest); kind 0 the round-to-nearest-even bf16 of kind 1 bit for bit,
    channels 3..7 exactly +0.0 over a NaN pre-fill"""
    Rh, Rw = target
    names = LAUNCHES[target]
    k1 = _launch(packed, names, Rh, Rw, 1, dev, sw).cpu().numpy()
    assert k1.shape == (len(names), 3, Rh, Rw) and np.isfinite(k1).all()
    worst = 0.0
    for b, name in enumerate(names):
        ref = _ref(name, target, sw, 400 + packed['index'][name])
        d = float(np.abs(k1[b].astype(np.float64) - ref).max())
        print(f'{name} -> {Rh}x{Rw} geometry {sw[0]} filter {sw[1]} range {sw[2]}: max|kind1 - f64| = {d:.3e}')
        worst = max(worst, d)
    parity_margins.record('image_resize_g%d_f%d_r%d' % sw, tolerances={'kind1_vs_f64': 1e-5}, **{f'{Rh}x{Rw}': worst})
    assert worst <= 1e-5, (target, sw, worst)
    if sw[2]:
        assert k1.min() >= 0.0 and k1.max() <= 1.0
    k0 = _launch(packed, names, Rh, Rw, 0, dev, sw)
    bits = k0.view(torch.int16).cpu().numpy().view(np.uint16).reshape(len(names), Rh, Rw, 8)
    assert np.array_equal(bits[..., :3], RR.rne_bf16_bits(k1.transpose(0, 2, 3, 1)))
    assert not bits[..., 3:].any()   # +0.0 in every pad channel


@pytest.mark.parametrize('kind', [0, 1])
def test_switches_000_are_the_ingest_entries_bit_for_bit(packed, dev, kind):
    view = torch.int16 if kind == 0 else torch.int32
    for (Rh, Rw), names in LAUNCHES.items():
        a = _launch(packed, names, Rh, Rw, kind, dev, (0, 0, 0))
        b = _launch(packed, names, Rh, Rw, kind, dev, entry='rect')
        assert not torch.isnan(a.float()).any()
        assert torch.equal(a.view(view), b.view(view)), (Rh, Rw)
        if Rh == Rw:
            c = _launch(packed, names, Rh, Rw, kind, dev, entry='square')
            assert torch.equal(a.view(view), c.view(view)), (Rh, Rw)


def test_constant_images_are_exact_under_range_1(dev):
    """a constant image of level c comes out as exactly float32(c) / float32(255), whatever the filter and geometry: the integer
    weights sum to the normaliser"""
    from diffusion_amd import ops
    from diffusion_amd.datasets.image_ingest import pack_images
    sizes = [(7, 5), (40, 23), (400, 7), (5, 61)]
    for c in RR.CONSTANT_LEVELS:
        raw, off, hw = pack_images([torch.full((h, w, 3), c, dtype=torch.uint8) for h, w in sizes])
        d_raw, d_off, d_hw = raw.to(dev), off.to(dev), hw.to(dev)
        want = np.float32(c) / np.float32(255)
        for geometry, filt in itertools.product((0, 1), (0, 1)):
            for Rh, Rw in ((16, 16), (17, 33)):
                out = torch.full((len(sizes), 3, Rh, Rw), float('nan'), device=dev)
                ops.image_resize(d_raw, d_off, d_hw, Rh, Rw, out, 1, geometry, filt, 1, host=(off, hw))
                got = out.cpu().numpy()
                assert (got == want).all(), (c, geometry, filt, Rh, Rw, np.abs(got - want).max())


def test_out_of_range_switches_are_rejected_without_launching(packed, dev):
    from diffusion_amd import _lib, ops
    Rh, Rw, names = 16, 16, ['16x16', '7x5', '40x23']
    off, hw, d_off, d_hw = _tables(packed, names, dev)
    raw = packed['raw']
    out = torch.full((3 * Rh * Rw, 8), float('nan'), device=dev, dtype=torch.bfloat16)
    f32 = torch.full((3, 3, Rh, Rw), float('nan'), device=dev)
    s = torch.cuda.current_stream().cuda_stream
    fn = _lib.load().da_image_resize

    def rc(kind=0, geometry=0, filter=0, range=0, Rh_=Rh, out_=None):
        out_ = out_ if out_ is not None else (out if kind == 0 else f32).data_ptr()
        return fn(raw.data_ptr(), d_off.data_ptr(), d_hw.data_ptr(), 3, Rh_, Rw, out_, kind, geometry, filter, range, s)

    for bad in (dict(geometry=2), dict(geometry=-1), dict(filter=2), dict(filter=-1), dict(range=2), dict(range=-1),
                dict(kind=2, out_=out.data_ptr()), dict(kind=-1, out_=out.data_ptr()), dict(geometry=3, kind=1), dict(Rh_=0),
                dict(Rh_=4097), dict(filter=1 << 30, kind=1)):
        assert rc(**bad) == 1, bad   # DA_ERR_SHAPE
    for kw in (dict(geometry=2), dict(filter=-1), dict(range=2), dict(range=None), dict(kind=2), dict(host=None),
               dict(host=(off - 1, hw)), dict(Rh=0), dict(Rw=4097), dict(out=f32)):
        args = dict(raw=raw, off=d_off, hw=d_hw, Rh=Rh, Rw=Rw, out=out, kind=0, geometry=1, filter=1, range=1, host=(off, hw))
        args.update(kw)
        with pytest.raises(ValueError):
            ops.image_resize(args['raw'], args['off'], args['hw'], args['Rh'], args['Rw'], args['out'], args['kind'],
                             args['geometry'], args['filter'], args['range'], host=args['host'])
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(f32).all()   # the output buffers are untouched
    assert rc(geometry=1, filter=1, range=1) == 0 and rc(kind=1, geometry=1, filter=1, range=1) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and not torch.isnan(f32).any()
