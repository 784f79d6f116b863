"""GPU tests of the augmenting raw-image ingest, ``da_image_ingest_aug`` / ``ops.image_ingest_aug``: the per-image crop
origin and horizontal flip of aspect-ratio bucketed training.

Equalities: the centre origin without a flip is ``da_image_ingest_rect`` bit for bit; the centre origin WITH a flip is
``da_image_ingest_rect`` on the host-mirrored source bit for bit (the horizontal sums are integers exact in fp64, so the
order of the taps cannot matter, and the vertical pass never sees the flip); arbitrary origins are within 1e-5 of the float64
restatement of tests/ingest_aug_reference.py (the bound the other ingest tests hold against float64); kind 0 is the bf16
rounding of kind 1.  All sources (ten, none above 70 px) live in one packed upload next to their mirrored twins; the float64
references are computed once per (image, target, origin)."""
import numpy as np
import pytest
import torch

import ingest_aug_reference as AR

pytestmark = pytest.mark.gpu

N = len(AR.SOURCES)


def _geo(target):
    """per source: (nw, nh, centre top, centre left) at this target"""
    return [AR.geometry(w, h, *target) for h, w in AR.SOURCES]


def _variants(target):
    """name -> int32 [N, 3] aug table.  Flips are mixed inside every batch but the two centre ones."""
    Rh, Rw = target
    geo = _geo(target)
    rng = np.random.default_rng(Rh * 100 + Rw)
    mixed = np.arange(N) % 2
    out = {'centre': [(t, l, 0) for _, _, t, l in geo], 'centre_flip': [(t, l, 1) for _, _, t, l in geo],
           'zero': [(0, 0, int(f)) for f in mixed],
           'far': [(nh - Rh, nw - Rw, int(1 - f)) for (nw, nh, _, _), f in zip(geo, mixed)],
           'random': [(int(rng.integers(0, nh - Rh + 1)), int(rng.integers(0, nw - Rw + 1)), int(rng.integers(0, 2)))
                      for nw, nh, _, _ in geo]}
    return {k: np.array(v, dtype=np.int32) for k, v in out.items()}


def test_the_cases_cover_what_they_claim():
    slack = [(nw - Rw, nh - Rh) for t in AR.TARGETS for (nw, nh, _, _), (Rh, Rw) in zip(_geo(t), [t] * N)]
    assert any(sx == 1 for sx, _ in slack) and any(sy == 1 for _, sy in slack)          # 1 px of slack, either axis
    assert any(nw % 2 == 1 and nw > t[1] for t in AR.TARGETS for nw, _, _, _ in _geo(t))   # odd nw, with room to move
    assert any(w == 1 for _, w in AR.SOURCES) and max(max(s) for s in AR.SOURCES) <= 70
    assert all(R % 16 for t in AR.TARGETS for R in t)
    for t in AR.TARGETS:
        v = _variants(t)
        assert set(v['zero'][:, 2]) == {0, 1} and set(v['far'][:, 2]) == {0, 1} and set(v['random'][:, 2]) == {0, 1}


@pytest.fixture(scope='module')
def packed(dev):
    """the ten sources followed by their host-mirrored twins, one upload"""
    from diffusion_amd.datasets.image_ingest import pack_images
    imgs = [AR.seeded_image(h, w, 300 + k) for k, (h, w) in enumerate(AR.SOURCES)]
    mirrored = [im[:, ::-1].copy() for im in imgs]
    raw, off, hw = pack_images([torch.from_numpy(im) for im in imgs + mirrored])
    assert sum(int(o) % 2 for o in off[:N]) >= 2   # images that begin at odd byte offsets
    return {'imgs': imgs, 'raw': raw.to(dev), 'off': off, 'hw': hw}


@pytest.fixture(scope='module')
def refs(packed):
    return {(t, name): np.stack([AR.aug_f64(packed['imgs'][b], *t, *(int(v) for v in tab[b])) for b in range(N)])
            for t in AR.TARGETS for name, tab in _variants(t).items()}


def _out(B, Rh, Rw, kind, dev):
    if kind == 0:
        return torch.full((B * Rh * Rw, 8), float('nan'), device=dev, dtype=torch.bfloat16)
    return torch.full((B, 3, Rh, Rw), float('nan'), device=dev, dtype=torch.float32)


def _aug(packed, target, tab, kind, dev):
    from diffusion_amd import ops
    off, hw, aug = packed['off'][:N].contiguous(), packed['hw'][:N].contiguous(), torch.from_numpy(tab)
    out = _out(N, *target, kind, dev)
    ops.image_ingest_aug(packed['raw'], off.to(dev), hw.to(dev), aug.to(dev), *target, out, kind, host=(off, hw, aug))
    torch.cuda.synchronize()
    return out


def _rect(packed, target, kind, dev, mirrored=False):
    from diffusion_amd import ops
    sl = slice(N, 2 * N) if mirrored else slice(0, N)
    off, hw = packed['off'][sl].contiguous(), packed['hw'][sl].contiguous()
    out = _out(N, *target, kind, dev)
    ops.image_ingest_rect(packed['raw'], off.to(dev), hw.to(dev), *target, out, kind, host=(off, hw))
    torch.cuda.synchronize()
    return out


def _bits(x):
    return x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize('kind', [0, 1])
@pytest.mark.parametrize('target', AR.TARGETS, ids=lambda t: f'{t[0]}x{t[1]}')
def test_centre_origin_is_the_rect_entry_bit_for_bit(packed, dev, target, kind):
    got = _aug(packed, target, _variants(target)['centre'], kind, dev)
    want = _rect(packed, target, kind, dev)
    assert not torch.isnan(got.float()).any()
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize('kind', [0, 1])
@pytest.mark.parametrize('target', AR.TARGETS, ids=lambda t: f'{t[0]}x{t[1]}')
def test_flip_at_the_centre_is_the_rect_entry_on_the_mirrored_source_bit_for_bit(packed, dev, target, kind):
    got = _aug(packed, target, _variants(target)['centre_flip'], kind, dev)
    want = _rect(packed, target, kind, dev, mirrored=True)
    assert not torch.isnan(got.float()).any()
    assert torch.equal(_bits(got), _bits(want))
    plain = _rect(packed, target, kind, dev)
    assert not torch.equal(_bits(got), _bits(plain))   # the flip does something


@pytest.mark.parametrize('variant', ['centre', 'centre_flip', 'zero', 'far', 'random'])
@pytest.mark.parametrize('target', AR.TARGETS, ids=lambda t: f'{t[0]}x{t[1]}')
def test_any_origin_matches_float64_and_kind0_is_the_bf16_of_kind1(packed, refs, dev, target, variant):
    Rh, Rw = target
    tab = _variants(target)[variant]
    k1 = _aug(packed, target, tab, 1, dev).cpu().numpy()
    assert k1.shape == (N, 3, Rh, Rw) and np.isfinite(k1).all()
    d = np.abs(k1.astype(np.float64) - refs[(target, variant)]).reshape(N, -1).max(1)
    print(f'{variant} -> {Rh}x{Rw}: max|kind1 - f64| per image = {np.array2string(d, precision=2)}')
    assert d.max() <= 1e-5, (target, variant, d)
    k0 = _aug(packed, target, tab, 0, dev)
    bits = k0.view(torch.int16).cpu().numpy().view(np.uint16).reshape(N, Rh, Rw, 8)
    assert np.array_equal(bits[..., :3], AR.rne_bf16_bits(k1.transpose(0, 2, 3, 1)))
    assert not bits[..., 3:].any()   # +0.0 in every pad channel, over the NaN pre-fill


def test_the_kernel_clamps_origins_and_skips_a_bad_flip(packed, dev):
    """Through the C ABI, which cannot see the device table: origins far outside the resized image give the crop at the
    nearest valid origin (every source here is followed by others in the upload, so even an unclamped read would stay inside
    the allocation), and an image whose flip is neither 0 nor 1 is left unwritten."""
    from diffusion_amd import _lib
    target = AR.TARGETS[0]
    Rh, Rw = target
    far = _variants(target)['far'].copy()
    far[:, 2] = 0
    want_far = _aug(packed, target, far, 1, dev)
    zero = np.zeros((N, 3), np.int32)
    want_zero = _aug(packed, target, zero, 1, dev)
    off, hw = packed['off'][:N].contiguous().to(dev), packed['hw'][:N].contiguous().to(dev)
    s = torch.cuda.current_stream().cuda_stream
    fn = _lib.load().da_image_ingest_aug
    for tab, want in ((far + np.array([7, 100000, 0], np.int32), want_far), (zero - np.array([3, 2 ** 30, 0], np.int32), want_zero)):
        out = _out(N, Rh, Rw, 1, dev)
        aug = torch.from_numpy(tab.astype(np.int32)).to(dev)
        assert fn(packed['raw'].data_ptr(), off.data_ptr(), hw.data_ptr(), aug.data_ptr(), N, Rh, Rw, out.data_ptr(), 1, s) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(want))
    bad = zero.copy()
    bad[3, 2], bad[5, 2] = 2, -1
    out = _out(N, Rh, Rw, 1, dev)
    aug = torch.from_numpy(bad).to(dev)
    assert fn(packed['raw'].data_ptr(), off.data_ptr(), hw.data_ptr(), aug.data_ptr(), N, Rh, Rw, out.data_ptr(), 1, s) == 0
    torch.cuda.synchronize()
    for b in range(N):
        if b in (3, 5):
            assert torch.isnan(out[b]).all()
        else:
            assert torch.equal(_bits(out[b]), _bits(want_zero[b]))


def test_aug_entry_rejects_bad_arguments_without_launching(packed, dev):
    from diffusion_amd import _lib, ops
    target = AR.TARGETS[0]
    Rh, Rw = target
    geo = _geo(target)
    off, hw = packed['off'][:N].contiguous(), packed['hw'][:N].contiguous()
    d_off, d_hw = off.to(dev), hw.to(dev)
    tab = torch.from_numpy(_variants(target)['random'])
    d_aug = tab.to(dev)
    raw = packed['raw']
    big = torch.full((N * Rh * Rw * 8 + 8,), float('nan'), device=dev, dtype=torch.bfloat16)
    out = big[:N * Rh * Rw * 8].view(-1, 8)
    f32 = torch.full((N, 3, Rh, Rw), float('nan'), device=dev)
    s = torch.cuda.current_stream().cuda_stream
    fn = _lib.load().da_image_ingest_aug

    def rc(Rh_=Rh, Rw_=Rw, out_=out.data_ptr(), kind=0, B=N, src=raw.data_ptr(), aug_=d_aug.data_ptr(), off_=d_off.data_ptr(),
           hw_=d_hw.data_ptr()):
        return fn(src, off_, hw_, aug_, B, Rh_, Rw_, out_, kind, s)

    for bad in (dict(aug_=None), dict(Rh_=0), dict(Rh_=4097), dict(Rw_=0), dict(Rw_=4097), dict(out_=out.data_ptr() + 2),
                dict(kind=2), dict(kind=-1), dict(kind=1, out_=f32.data_ptr() + 2), dict(B=0), dict(out_=None), dict(src=None),
                dict(off_=None), dict(hw_=None)):
        assert rc(**bad) == 1, bad   # DA_ERR_SHAPE

    def table(b, col, val):
        t = tab.clone()
        t[b, col] = val
        return t

    nw0, nh0 = geo[0][0], geo[0][1]
    cases = [dict(Rh=0), dict(Rw=4097), dict(kind=2), dict(kind=1), dict(out=f32), dict(out=out[:-1]), dict(host=None),
             dict(host=(off, hw)), dict(host=(off - 1, hw, tab)), dict(raw=raw.cpu()), dict(aug=tab), dict(aug=d_aug.long()),
             dict(aug=d_aug[:-1]), dict(aug=d_aug[:, :2].contiguous()), dict(host=(off, hw, tab[:-1])),
             dict(host=(off, hw, d_aug)),
             dict(host=(off, hw, table(0, 0, nh0 - Rh + 1))), dict(host=(off, hw, table(0, 0, -1))),
             dict(host=(off, hw, table(0, 1, nw0 - Rw + 1))), dict(host=(off, hw, table(N - 1, 1, -1))),
             dict(host=(off, hw, table(2, 2, 2))), dict(host=(off, hw, table(2, 2, -1)))]
    for kw in cases:
        args = dict(raw=raw, off=d_off, hw=d_hw, aug=d_aug, Rh=Rh, Rw=Rw, out=out, kind=0, host=(off, hw, tab))
        args.update(kw)
        with pytest.raises(ValueError):
            ops.image_ingest_aug(args['raw'], args['off'], args['hw'], args['aug'], args['Rh'], args['Rw'], args['out'],
                                 args['kind'], host=args['host'])
    torch.cuda.synchronize()
    assert torch.isnan(big).all() and torch.isnan(f32).all()   # nothing was launched
    assert rc() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and torch.isnan(big[-8:]).all()


def test_ingest_batch_takes_the_aug_entry_when_the_batch_carries_image_aug(packed, dev):
    """``datasets.image_ingest.ingest_batch`` (what ``model.ingest_raw`` calls) with ``image_aug`` in the batch is the op by
    hand, for an ``(Rh, Rw)`` pair and for an int target"""
    from diffusion_amd.datasets.image_ingest import ingest_batch
    target = AR.TARGETS[1]
    tab = torch.from_numpy(_variants(target)['random'])
    off = packed['off'][:N].contiguous()
    batch = {'image_raw': packed['raw'].cpu()[:int(packed['off'][N])], 'image_off': off,
             'image_hw': packed['hw'][:N].contiguous(), 'image_aug': tab}
    for kind in (0, 1):
        got = ingest_batch(batch, target, kind, dev)
        assert torch.equal(_bits(got), _bits(_aug(packed, target, tab.numpy(), kind, dev)))
    sq = dict(batch, image_aug=torch.from_numpy(np.array([(t, l, 1) for _, _, t, l in _geo((16, 16))], np.int32)))
    got = ingest_batch(sq, 16, 1, dev)
    assert torch.equal(_bits(got), _bits(_rect(packed, (16, 16), 1, dev, mirrored=True)))
