"""GPU tests of the rectangular raw-image ingest: ``da_image_ingest_rect`` / ``ops.image_ingest_rect`` against the float64
restatement of tests/ingest_rect_reference.py and against PIL, bit for bit against the square entry at Rh == Rw, its argument
checks, and the ``StableDiffusion.ingest_raw`` hook with an ``(Rh, Rw)`` ``image_size``.

As in tests/test_image_ingest_gpu.py all sources live in ONE packed upload and each launch selects its images through the
offset table; the float64 references are computed once."""
import numpy as np
import pytest
import torch

import ingest_reference as IR
import ingest_rect_reference as RR

pytestmark = pytest.mark.gpu

# name -> (h, w); packed in this order.  The rect cases first, then the square kernel cases for the bit-identity test
SOURCES = {}
for (_h, _w), _ in RR.RECT_CASES:
    SOURCES.setdefault(f'{_h}x{_w}', (_h, _w))
for _h, _w in IR.KERNEL_CASES_R16:
    SOURCES.setdefault(f'{_h}x{_w}', (_h, _w))
# one launch per target: (Rh, Rw) -> the sources that go to it
LAUNCHES = {}
for (_h, _w), _t in RR.RECT_CASES:
    LAUNCHES.setdefault(_t, []).append(f'{_h}x{_w}')


@pytest.fixture(scope='module')
def packed(dev):
    from diffusion_amd.datasets.image_ingest import pack_images
    imgs = {name: RR.seeded_image(h, w, 200 + k) for k, (name, (h, w)) in enumerate(SOURCES.items())}
    raw, off, hw = pack_images([torch.from_numpy(im) for im in imgs.values()])
    assert sum(int(o) % 2 for o in off) >= 2   # at least two images begin at odd byte offsets
    return {'imgs': imgs, 'raw': raw.to(dev), 'off': off, 'hw': hw, 'index': {name: i for i, name in enumerate(imgs)}}


@pytest.fixture(scope='module')
def refs(packed):
    return {(name, t): RR.ingest_f64(packed['imgs'][name], *t) for t, names in LAUNCHES.items() for name in names}


def _tables(packed, names, dev):
    sel = torch.tensor([packed['index'][n] for n in names])
    off, hw = packed['off'][sel].contiguous(), packed['hw'][sel].contiguous()
    return off, hw, off.to(dev), hw.to(dev)


def _launch(packed, names, Rh, Rw, kind, dev, square=False):
    from diffusion_amd import ops
    off, hw, d_off, d_hw = _tables(packed, names, dev)
    B = len(names)
    if kind == 0:
        out = torch.full((B * Rh * Rw, 8), float('nan'), device=dev, dtype=torch.bfloat16)
    else:
        out = torch.full((B, 3, Rh, Rw), float('nan'), device=dev, dtype=torch.float32)
    if square:
        ops.image_ingest(packed['raw'], d_off, d_hw, Rh, out, kind, host=(off, hw))
    else:
        ops.image_ingest_rect(packed['raw'], d_off, d_hw, Rh, Rw, out, kind, host=(off, hw))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('target', list(LAUNCHES), ids=lambda t: f'{t[0]}x{t[1]}')
def test_rect_kind1_matches_float64_and_pil_and_kind0_is_its_bf16(packed, refs, dev, target):
    """kind 1 within 1e-5 of the float64 filter and within 1.01 uint8 steps of PIL; kind 0 the round-to-nearest-even bf16 of
    kind 1 bit for bit, channels 3..7 exactly +0.0 over a NaN pre-fill"""
    pytest.importorskip('PIL.Image')
    Rh, Rw = target
    names = LAUNCHES[target]
    k1 = _launch(packed, names, Rh, Rw, 1, dev).cpu().numpy()
    assert k1.shape == (len(names), 3, Rh, Rw) and np.isfinite(k1).all()
    for b, name in enumerate(names):
        d = np.abs(k1[b].astype(np.float64) - refs[(name, target)]).max()
        dp = np.abs(k1[b].astype(np.float64) - RR.ingest_pil(packed['imgs'][name], Rh, Rw)).max()
        print(f'{name} -> {Rh}x{Rw}: max|kind1 - f64| = {d:.3e}, max|kind1 - PIL| = {dp * 127.5:.4f} uint8 steps')
        assert d <= 1e-5, (target, name, d)
        assert dp <= 1.01 * 2 / 255 + 1e-5, (target, name, dp)
    k0 = _launch(packed, names, Rh, Rw, 0, dev)
    bits = k0.view(torch.int16).cpu().numpy().view(np.uint16).reshape(len(names), Rh, Rw, 8)
    assert np.array_equal(bits[..., :3], RR.rne_bf16_bits(k1.transpose(0, 2, 3, 1)))
    assert not bits[..., 3:].any()   # +0.0 in every pad channel


@pytest.mark.parametrize('kind', [0, 1])
def test_rect_entry_at_a_square_target_is_the_square_entry_bit_for_bit(packed, dev, kind):
    names = [f'{h}x{w}' for h, w in IR.KERNEL_CASES_R16]
    a = _launch(packed, names, 16, 16, kind, dev, square=True)
    b = _launch(packed, names, 16, 16, kind, dev)
    view = torch.int16 if kind == 0 else torch.int32
    assert not torch.isnan(a.float()).any()
    assert torch.equal(a.view(view), b.view(view))


def test_rect_entry_rejects_bad_arguments_without_launching(packed, dev):
    from diffusion_amd import _lib, ops
    Rh, Rw, names = 16, 32, ['16x32', '9x23', '37x53']
    off, hw, d_off, d_hw = _tables(packed, names, dev)
    raw = packed['raw']
    big = torch.full((3 * Rh * Rw * 8 + 8,), float('nan'), device=dev, dtype=torch.bfloat16)
    out = big[:3 * Rh * Rw * 8].view(-1, 8)
    f32 = torch.full((3, 3, Rh, Rw), float('nan'), device=dev)
    s = torch.cuda.current_stream().cuda_stream
    fn = _lib.load().da_image_ingest_rect

    def rc(Rh_=Rh, Rw_=Rw, out_=out.data_ptr(), kind=0, B=3, src=raw.data_ptr()):
        return fn(src, d_off.data_ptr(), d_hw.data_ptr(), B, Rh_, Rw_, out_, kind, s)

    for bad in (dict(Rh_=0), dict(Rh_=4097), dict(Rw_=0), dict(Rw_=4097), dict(out_=out.data_ptr() + 2), dict(kind=2),
                dict(kind=-1), dict(kind=1, out_=f32.data_ptr() + 2), dict(B=0), dict(out_=None), dict(src=None)):
        assert rc(**bad) == 1, bad   # DA_ERR_SHAPE
    # the wrapper
    cases = [dict(Rh=0), dict(Rh=4097), dict(Rw=0), dict(Rw=4097), dict(kind=2), dict(kind=1), dict(out=f32), dict(out=out[:-1]),
             dict(out=big[1:1 + 3 * Rh * Rw * 8].view(-1, 8)), dict(host=None), dict(host=(off - 1, hw)), dict(raw=raw.cpu()),
             dict(Rh=Rw, Rw=Rh + 1)]   # a transposed target of another size
    for kw in cases:
        args = dict(raw=raw, off=d_off, hw=d_hw, Rh=Rh, Rw=Rw, out=out, kind=0, host=(off, hw))
        args.update(kw)
        with pytest.raises(ValueError):
            ops.image_ingest_rect(args['raw'], args['off'], args['hw'], args['Rh'], args['Rw'], args['out'], args['kind'],
                                  host=args['host'])
    torch.cuda.synchronize()
    assert torch.isnan(big).all() and torch.isnan(f32).all()   # nothing was launched
    assert rc() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and torch.isnan(big[-8:]).all()


def test_ingest_raw_with_a_rectangular_image_size_feeds_the_encoder(dev):
    """``model.ingest_raw`` on a batch whose ``image_size`` is (32, 64) hands ``vae_hip`` the tensor of ingesting by hand, on
    either image-encoder route, and the encoder turns it into 4 x 8 latents.  The tiny U-Net has 4 levels, so its walk takes
    latents that are multiples of 8: ``forward`` names that rule for the (32, 64) batch and runs on the same images at
    (64, 128)."""
    pytest.importorskip('PIL.Image')
    from diffusion_amd import ops
    from diffusion_amd.datasets.image_ingest import collate_raw_images
    from diffusion_amd.models.models import stable_diffusion_2
    torch.manual_seed(11)
    model = stable_diffusion_2(model_name='tiny', pretrained=False, precomputed_latents=False, fsdp=False)
    assert model.vae_hip is not None
    imgs = [RR.seeded_image(h, w, 7 + i) for i, (h, w) in enumerate([(70, 101), (131, 64)])]
    g = torch.Generator().manual_seed(3)
    samples = [{'image_u8': torch.from_numpy(im), 'captions': torch.randint(0, 49408, (77,), generator=g)} for im in imgs]
    for Rh, Rw in ((32, 64), (64, 128)):
        batch = collate_raw_images(image_size=(Rh, Rw))(samples)
        assert batch['image_size'] == (Rh, Rw)
        hand = torch.empty(2 * Rh * Rw, 8, device=dev, dtype=torch.bfloat16)
        args = (batch['image_raw'].to(dev), batch['image_off'].to(dev), batch['image_hw'].to(dev), Rh, Rw)
        host = (batch['image_off'], batch['image_hw'])
        ops.image_ingest_rect(*args, hand, 0, host=host)
        fed = model.ingest_raw(batch)
        assert 'image_raw' not in fed and 'image_size' not in fed and fed['image_nhwc8'].shape == (2, Rh, Rw, 8)
        assert torch.equal(fed['image_nhwc8'].reshape(-1, 8).view(torch.int16), hand.view(torch.int16))
        ref = np.stack([RR.ingest_f64(im, Rh, Rw) for im in imgs])
        got = hand.float().view(2, Rh, Rw, 8)[..., :3].permute(0, 3, 1, 2).cpu().numpy()
        assert np.abs(got - ref).max() <= 2.0 ** -8 + 1e-5   # bf16: half an ulp below 2, on top of kind 1's 1e-5
        torch.manual_seed(5)
        lat_raw, _ = model._encode(batch)
        torch.manual_seed(5)
        lat_hand, _ = model._encode({'image_nhwc8': hand.view(2, Rh, Rw, 8), 'captions': batch['captions'].to(dev)})
        assert lat_raw.shape == (2, 4, Rh // 8, Rw // 8) and torch.equal(lat_raw, lat_hand)
        image = torch.empty(2, 3, Rh, Rw, device=dev)
        ops.image_ingest_rect(*args, image, 1, host=host)
        hip, model.vae_hip = model.vae_hip, None
        try:   # the fp32 torch VAE path takes kind 1 through the same hook
            assert torch.equal(model.ingest_raw(batch)['image'], image)
        finally:
            model.vae_hip = hip
        if Rh // 8 % 8:
            with pytest.raises(ValueError, match='multiples of 8'):
                model(batch)
            continue
        model.unet.zero_grad()
        out = model(batch)
        assert out[0].shape == (2, 4, Rh // 8, Rw // 8)
        loss = model.loss(out, batch)
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(loss).item() and loss.item() > 0
        assert float(model.unet.grad.abs().sum()) > 0
