"""GPU tests of the raw-image ingest: the kernel (``da_image_ingest`` / ``ops.image_ingest``) against the float64
restatement of tests/ingest_reference.py and against PIL, its argument checks, the ``StableDiffusion._encode`` hook and
tools/precompute_latents.py.

All sources of the kernel tests live in ONE packed upload; each launch selects its images through the offset table, so
every launch has B >= 3 and reads images that begin at odd byte addresses.  The float64 references are computed once."""
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

import ingest_reference as IR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (h, w); packed in this order
SOURCES = {f'{h}x{w}': (h, w) for h, w in IR.KERNEL_CASES_R16}
SOURCES['1000x333'] = IR.CASE_21_TAPS[0]
SOURCES['1x40'] = IR.CASE_ONE_ROW[0]
# launch name -> (R, images)
LAUNCHES = {
    'R16': (16, [f'{h}x{w}' for h, w in IR.KERNEL_CASES_R16]),   # identity, upscale, fractional downscale on either axis, both
    'R24': (24, [f'{h}x{w}' for h, w in IR.KERNEL_CASES_R16]),   # half-even crops, integer x4; R24: a partial tile per axis
    'R32': (32, ['1000x333', '37x53', '64x64']),                 # 21 taps per axis
    'R8': (8, ['1x40', '9x23', '16x16']),                        # a 1-pixel-high source
}


@pytest.fixture(scope='module')
def packed(dev):
    from diffusion_amd.datasets.image_ingest import pack_images
    imgs = {name: IR.seeded_image(h, w, 100 + k) for k, (name, (h, w)) in enumerate(SOURCES.items())}
    raw, off, hw = pack_images([torch.from_numpy(im) for im in imgs.values()])
    assert sum(int(o) % 2 for o in off) >= 2   # at least two images begin at odd byte offsets
    index = {name: i for i, name in enumerate(imgs)}
    return {'imgs': imgs, 'raw': raw.to(dev), 'off': off, 'hw': hw, 'index': index}


@pytest.fixture(scope='module')
def refs():
    cache = {}

    def get(packed, name, R):
        if (name, R) not in cache:
            cache[(name, R)] = IR.ingest_f64(packed['imgs'][name], R)
        return cache[(name, R)]
    return get


def _launch(packed, names, R, kind, dev, fill=float('nan')):
    from diffusion_amd import ops
    sel = torch.tensor([packed['index'][n] for n in names])
    off, hw = packed['off'][sel].contiguous(), packed['hw'][sel].contiguous()
    B = len(names)
    if kind == 0:
        out = torch.full((B * R * R, 8), fill, device=dev, dtype=torch.bfloat16)
    else:
        out = torch.full((B, 3, R, R), fill, device=dev, dtype=torch.float32)
    ops.image_ingest(packed['raw'], off.to(dev), hw.to(dev), R, out, kind, host=(off, hw))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('launch', list(LAUNCHES))
def test_kind1_matches_float64_and_kind0_is_its_bf16(packed, refs, dev, launch):
    """kind 1 within 1e-5 of the float64 filter (fewer than 50 fp32 roundings of 2^-24 on magnitudes <= 2 would give 6e-6);
    kind 0 is the round-to-nearest-even bf16 of kind 1 bit for bit, channels 3..7 exactly 0.0 over a NaN pre-fill."""
    R, names = LAUNCHES[launch]
    k1 = _launch(packed, names, R, 1, dev).cpu().numpy()
    assert np.isfinite(k1).all()
    for b, name in enumerate(names):
        d = np.abs(k1[b].astype(np.float64) - refs(packed, name, R)).max()
        print(f'{launch} {name}: max|kind1 - f64| = {d:.3e}')
        assert d <= 1e-5, (launch, name, d)
    k0 = _launch(packed, names, R, 0, dev)
    bits = k0.view(torch.int16).cpu().numpy().view(np.uint16).reshape(len(names), R, R, 8)
    want = IR.rne_bf16_bits(k1.transpose(0, 2, 3, 1))
    assert np.array_equal(bits[..., :3], want)
    assert not bits[..., 3:].any()   # +0.0 in every pad channel


@pytest.mark.parametrize('launch', list(LAUNCHES))
def test_kind1_within_one_uint8_step_of_pil(packed, dev, launch):
    pytest.importorskip('PIL.Image')
    R, names = LAUNCHES[launch]
    k1 = _launch(packed, names, R, 1, dev).cpu().numpy().astype(np.float64)
    for b, name in enumerate(names):
        d = np.abs(k1[b] - IR.ingest_pil(packed['imgs'][name], R)).max()
        print(f'{launch} {name}: max|kind1 - PIL| = {d * 127.5:.4f} uint8 steps')
        assert d <= 1.01 * 2 / 255 + 1e-5, (launch, name, d)


@pytest.mark.parametrize('k', [0, 255])
@pytest.mark.parametrize('R', [16, 24])
def test_constant_image_between_opposite_extremes(dev, k, R):
    """partition of unity at the borders (the clipped windows renormalise) and no bleed across image boundaries: a constant
    image of value k packed between two images of 255 - k comes out as k / 127.5 - 1 everywhere"""
    from diffusion_amd import ops
    from diffusion_amd.datasets.image_ingest import pack_images
    shapes = [(21, 19), (20, 27), (13, 30)]   # 1197 bytes: the middle image begins at an odd offset; down- and upscale
    vals = [255 - k, k, 255 - k]
    raw, off, hw = pack_images([torch.full((h, w, 3), v, dtype=torch.uint8) for (h, w), v in zip(shapes, vals)])
    assert int(off[1]) % 2 == 1
    for kind in (1, 0):
        out = torch.empty((3, 3, R, R) if kind else (3 * R * R, 8), device=dev, dtype=torch.float32 if kind else torch.bfloat16)
        ops.image_ingest(raw.to(dev), off.to(dev), hw.to(dev), R, out, kind, host=(off, hw))
        got = out.float().cpu() if kind else out.float().cpu().view(3, R, R, 8)[..., :3].permute(0, 3, 1, 2)
        for b, v in enumerate(vals):
            d = (got[b].double() - (v / 127.5 - 1.0)).abs().max().item()
            assert d <= 1e-6, (kind, b, d)   # 0 -> -1 and 255 -> +1 are exact in bf16 too


def test_ops_image_ingest_rejects_bad_arguments_without_launching(packed, dev):
    from diffusion_amd import ops
    R, names = 16, ['16x16', '9x23', '37x53']
    sel = torch.tensor([packed['index'][n] for n in names])
    off, hw = packed['off'][sel].contiguous(), packed['hw'][sel].contiguous()
    d_off, d_hw, raw = off.to(dev), hw.to(dev), packed['raw']
    big = torch.full((3 * R * R * 8 + 8,), float('nan'), device=dev, dtype=torch.bfloat16)
    out = big[:3 * R * R * 8].view(-1, 8)
    f32 = torch.full((3, 3, R, R), float('nan'), device=dev)
    bad_off = off.clone()
    bad_off[2] = raw.numel() - 3 * 37 * 53 + 1   # the last image would end one byte past the buffer
    bad_hw = hw.clone()
    bad_hw[1, 0] = 0
    cases = [
        dict(raw=raw.cpu()),                                        # a host tensor
        dict(off=off), dict(hw=hw),
        dict(out=big[1:1 + 3 * R * R * 8].view(-1, 8)),             # bf16 out 2 bytes off a 16-byte boundary
        dict(out=f32),                                              # wrong dtype for kind 0
        dict(out=out[:-1]),                                         # wrong size
        dict(kind=1),                                               # bf16 out with kind 1
        dict(kind=2), dict(R=0), dict(R=4097),
        dict(off=bad_off.to(dev), host=(bad_off, hw)),              # offset table runs past the buffer
        dict(host=(off - 1, hw)),                                   # ... or before it
        dict(hw=bad_hw.to(dev), host=(off, bad_hw)),                # h = 0
        dict(host=None),                                            # no host copies: the bounds cannot be checked
        dict(off=d_off.int()), dict(raw=raw.view(-1, 3)[:, 0]),     # wrong dtype, not contiguous
    ]
    for kw in cases:
        args = dict(raw=raw, off=d_off, hw=d_hw, R=R, out=out, kind=0, host=(off, hw))
        args.update(kw)
        with pytest.raises(ValueError):
            ops.image_ingest(args['raw'], args['off'], args['hw'], args['R'], args['out'], args['kind'], host=args['host'])
    torch.cuda.synchronize()
    assert torch.isnan(big).all() and torch.isnan(f32).all()   # nothing was launched
    ops.image_ingest(raw, d_off, d_hw, R, out, 0, host=(off, hw))
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and torch.isnan(big[-8:]).all()


def _png(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format='PNG')
    return buf.getvalue()


def test_encode_on_raw_batch_equals_encode_on_ingested_images(dev):
    """``_encode`` on packed raw pixels (kind 0 straight into the VAE encoder's conv_in layout) gives the latents of
    ``_encode`` on the kind-1 ``image`` tensor under the same seed; one training step on the raw batch is finite."""
    pytest.importorskip('PIL.Image')
    from diffusion_amd import ops
    from diffusion_amd.datasets.image_ingest import collate_raw_images, decode_rgb
    from diffusion_amd.models.models import stable_diffusion_2
    torch.manual_seed(11)
    model = stable_diffusion_2(model_name='tiny', pretrained=False, precomputed_latents=False, fsdp=False)
    assert model.vae_hip is not None
    R = 64
    imgs = [decode_rgb(_png(IR.seeded_image(h, w, 7 + i))) for i, (h, w) in enumerate([(70, 101), (131, 64)])]
    g = torch.Generator().manual_seed(3)
    samples = [{'image_u8': torch.from_numpy(im), 'captions': torch.randint(0, 49408, (77,), generator=g)} for im in imgs]
    batch = collate_raw_images(image_size=R)(samples)
    assert batch['image_raw'].numel() == 3 * (70 * 101 + 131 * 64)
    torch.manual_seed(5)
    lat_raw, cond = model._encode(batch)
    image = torch.empty(2, 3, R, R, device=dev)
    ops.image_ingest(batch['image_raw'].to(dev), batch['image_off'].to(dev), batch['image_hw'].to(dev), R, image, 1,
                     host=(batch['image_off'], batch['image_hw']))
    torch.manual_seed(5)
    lat_img, cond2 = model._encode({'image': image, 'captions': batch['captions'].to(dev)})
    assert lat_raw.shape == (2, 4, R // 8, R // 8) and torch.equal(lat_raw, lat_img) and torch.equal(cond, cond2)
    ref = np.stack([IR.ingest_f64(im, R) for im in imgs])
    assert np.abs(image.cpu().numpy() - ref).max() <= 1e-5
    # the fp32 torch VAE path takes kind 1 through the same hook
    hip, model.vae_hip = model.vae_hip, None
    try:
        fed = model.ingest_raw(batch)
        assert 'image_raw' not in fed and torch.equal(fed['image'], image)
    finally:
        model.vae_hip = hip
    model.unet.zero_grad()
    out = model(batch)
    loss = model.loss(out, batch)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item() and loss.item() > 0
    gn = sum(float(p.grad.float().norm()) for p in model.unet.parameters() if p.grad is not None)
    assert np.isfinite(gn) and gn > 0


def test_precompute_latents_tool(dev, tmp_path):
    """tools/precompute_latents.py on a 5-image PNG shard at 32 and 64 px: the written directory trains through
    ``MDSLatentDataset`` at both resolutions, the b'' rule empties exactly the samples whose shorter side is below R,
    ``latents_32`` is ``sample() * 0.18215`` in fp16 under the tool's generator, and the input columns come back unchanged."""
    pytest.importorskip('PIL.Image')
    from diffusion_amd import ops
    from diffusion_amd.datasets.image_ingest import pack_images
    from diffusion_amd.datasets.laion.laion import MDSLatentDataset
    from diffusion_amd.datasets.mds import MDSDirectory, write_mds
    from diffusion_amd.models.vae import DiagonalGaussian
    spec = importlib.util.spec_from_file_location('precompute_latents', os.path.join(ROOT, 'tools', 'precompute_latents.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    shapes = [(70, 90), (40, 33), (64, 100), (31, 80), (32, 32)]   # short sides 70, 33, 64, 31 (< 32), 32
    imgs = [IR.seeded_image(h, w, 60 + i) for i, (h, w) in enumerate(shapes)]
    src = [{'jpg': _png(im), 'caption': f'a picture, number {i}', 'key': str(1000 + i), 'width': np.int32(im.shape[1]),
            'punsafe': np.float64(i / 8)} for i, im in enumerate(imgs)]
    cols = {'jpg': 'bytes', 'caption': 'str', 'key': 'str', 'width': 'int32', 'punsafe': 'float64'}
    in_dir, out_dir = str(tmp_path / 'in'), str(tmp_path / 'out')
    write_mds(in_dir, cols, src)
    enc = tool.build_encoders('tiny', seed=17)
    res = tool.precompute(in_dir, out_dir, resolutions=(32, 64), batch_size=8, seed=17, caption_drop_prob=0.0, encoders=enc)
    assert res['images'] == 5 and res['images_per_s'] > 0
    assert all(k in res for k in ('seconds', 'decode_s', 'ingest_s', 'encode_s', 'write_s'))
    out = MDSDirectory(out_dir)
    assert len(out) == 5
    for i, s in enumerate(src):
        got = out.get(i)
        assert set(got) == set(cols) | {'caption_latents', 'latents_32', 'latents_64'}
        for c in cols:
            assert got[c] == s[c] and type(got[c]) is type(s[c]), c
        assert len(got['caption_latents']) == 77 * 128 * 2
        short = min(shapes[i])
        assert len(got['latents_32']) == (4 * 4 * 4 * 2 if short >= 32 else 0)
        assert len(got['latents_64']) == (4 * 8 * 8 * 2 if short >= 64 else 0)
    d32, d64 = MDSLatentDataset(out_dir, 32), MDSLatentDataset(out_dir, 64)
    got32 = [d32[i] for i in range(5)]
    assert all(s['image_latents'].shape == (4, 4, 4) and s['caption_latents'].shape == (77, 128) for s in got32)
    assert d32.skipped == 1   # sample 3 (31 px) falls to sample 4
    assert torch.equal(got32[3]['image_latents'], got32[4]['image_latents'])
    got64 = [d64[i] for i in range(5)]
    assert all(s['image_latents'].shape == (4, 8, 8) for s in got64)
    assert d64.skipped == 1 + 2 + 1   # index 1 -> 2; indices 3 and 4 -> 0 (3, 4 skipped; 4 skipped)
    # latents_32 of every sample, recomputed: the tool's generator draws the first resolution of the first batch first
    vae_hip = enc[0]
    raw, off, hw = pack_images([torch.from_numpy(im) for im in imgs])
    x = torch.empty(5 * 32 * 32, 8, device=dev, dtype=torch.bfloat16)
    ops.image_ingest(raw.to(dev), off.to(dev), hw.to(dev), 32, x, 0, host=(off, hw))
    gen = torch.Generator(device='cuda').manual_seed(17)
    want = (DiagonalGaussian(vae_hip.moments_nhwc8(x, 5, 32, 32)).sample(generator=gen) * 0.18215).half().cpu()
    for i in (0, 2):
        stored = torch.from_numpy(np.frombuffer(out.get(i)['latents_32'], dtype=np.float16).copy()).view(4, 4, 4)
        assert torch.equal(stored, want[i]), i
