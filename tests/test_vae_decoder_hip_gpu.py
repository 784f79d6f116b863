"""The frozen VAE decoder on the HIP kernels (models/vae_hip.VAEDecoderHIP) against the PyTorch AutoencoderKL with the same
weights (``vae.decode``, reference stable_diffusion.py:380), the encoder / decoder pair with no torch SDPA on the way, and
``generate()`` decoding through it.

Bound of the decoder parity: not a constant chosen in advance but the error of the torch module itself at the same
precision class, measured in the same test - e_hip = rel-L2(HIP, fp32 torch) <= 1.5 x e_bf16 = rel-L2(bf16 torch, fp32 torch).
The walk rounds at the same places or fewer (SiLU and the norms run in fp32); 1.5 x covers the different summation order.
A cap of 8e-2 over the whole tensor and in every image keeps the calibration from hiding a failure: the bf16 torch decoder
measures 3.5e-2 ... 3.6e-2 at these shapes (CPU), a wrong tap, layer order or H / W swap gives >= 0.5.
"""
import copy

import pytest
import torch

from parity_margins import record

pytestmark = pytest.mark.gpu

CAP = 8e-2


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-20)).item()


@pytest.fixture(scope='module')
def vaes(dev):
    from diffusion_amd.models.vae import AutoencoderKL
    from diffusion_amd.models.vae_hip import VAEDecoderHIP, VAEEncoderHIP
    torch.manual_seed(7)
    vae = AutoencoderKL().to(dev).eval()
    with torch.no_grad():   # non-trivial norm affines (torch default is gamma 1, beta 0)
        for n, p in vae.named_parameters():
            if 'norm' in n:
                p.add_(0.1 * torch.randn_like(p))
    return vae, copy.deepcopy(vae).to(torch.bfloat16), VAEEncoderHIP(vae), VAEDecoderHIP(vae)


def _check_calibrated(case, got, low, ref):
    """got (HIP) and low (bf16 torch) against ref (fp32 torch): e_hip <= 1.5 e_bf16, e_hip < CAP whole and per image"""
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert torch.isfinite(got).all()
    e_hip, e_bf16 = _rel(got, ref), _rel(low, ref)
    worst = max(_rel(got[i], ref[i]) for i in range(ref.shape[0]))
    print(f'{case}: e_hip {e_hip:.3e} (worst image {worst:.3e}), e_bf16 {e_bf16:.3e}')
    record(case, tolerances={'e_hip_over_e_bf16': 1.5, 'e_hip': CAP}, e_hip=e_hip, e_bf16=e_bf16, e_hip_worst_image=worst)
    assert e_hip <= 1.5 * e_bf16, (e_hip, e_bf16)
    assert e_hip < CAP and worst < CAP, (e_hip, worst)


@pytest.mark.parametrize('shape', [(2, 4, 8, 8), (1, 4, 16, 16), (1, 4, 8, 24)], ids=lambda s: 'x'.join(map(str, s)))
def test_decoder_matches_torch(vaes, dev, shape):
    vae, vae_bf16, _, dec = vaes
    g = torch.Generator().manual_seed(shape[2] * 100 + shape[3])
    z = torch.randn(*shape, generator=g).to(dev)
    with torch.no_grad():
        ref = vae.decode(z).sample
        low = vae_bf16.decode(z.to(torch.bfloat16)).sample.float()
    got = dec.decode(z).sample
    assert got.shape == (shape[0], 3, 8 * shape[2], 8 * shape[3])
    _check_calibrated('vae_decoder_hip_' + 'x'.join(map(str, shape)), got, low, ref)


def test_no_sdpa_on_the_way(vaes, dev, monkeypatch):
    """image -> latent -> image runs on the library alone: with torch's SDPA made to raise, both halves still run"""
    _, _, enc, dec = vaes

    def boom(*a, **kw):
        raise AssertionError('F.scaled_dot_product_attention was called')

    monkeypatch.setattr(torch.nn.functional, 'scaled_dot_product_attention', boom)
    g = torch.Generator().manual_seed(1)
    mom = enc.moments((torch.rand(1, 3, 64, 64, generator=g) * 2 - 1).to(dev))
    img = dec.decode(torch.randn(1, 4, 8, 8, generator=g).to(dev)).sample
    assert mom.shape == (1, 8, 8, 8) and torch.isfinite(mom).all()
    assert img.shape == (1, 3, 64, 64) and torch.isfinite(img).all()


def test_round_trip_matches_torch(vaes, dev):
    """decode(encode(x).mode()) on the HIP kernels against the same on the fp32 torch module, under the calibrated bound"""
    vae, vae_bf16, enc, dec = vaes
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(1, 3, 64, 64, generator=g) * 2 - 1).to(dev)
    with torch.no_grad():
        ref = vae.decode(vae.encode(x).latent_dist.mode()).sample
        low = vae_bf16.decode(vae_bf16.encode(x.to(torch.bfloat16)).latent_dist.mode()).sample.float()
    got = dec.decode(enc.encode(x).latent_dist.mode()).sample
    _check_calibrated('vae_round_trip_hip_1x3x64x64', got, low, ref)


def test_generate_decodes_through_the_hip_decoder(dev, monkeypatch):
    from diffusion_amd.models.models import stable_diffusion_2
    monkeypatch.delenv('DA_VAE_HIP', raising=False)
    torch.manual_seed(11)
    model = stable_diffusion_2(model_name='tiny', pretrained=False, fsdp=False)
    assert model.vae_dec_hip is not None
    kw = dict(prompt='a cool doge', height=64, width=64, num_inference_steps=1, seed=3, progress_bar=False)
    a = model.generate(**kw)
    assert a.shape == (1, 3, 64, 64) and torch.isfinite(a).all() and a.min() >= 0 and a.max() <= 1
    assert torch.equal(a, model.generate(**kw))
    hip, model.vae_dec_hip = model.vae_dec_hip, None
    ref = model.generate(**kw)   # the torch module, exactly as before
    model.vae_dec_hip = hip
    e = _rel(a, ref)
    print(f'generate: HIP decoder vs torch decoder rel-L2 {e:.3e}')
    # the decoder cap: the / 2 + 0.5 and the clamp only shrink the relative difference
    assert e < CAP, e


def test_fp32_latents_keep_the_torch_decoder(dev, monkeypatch):
    from diffusion_amd.models.models import stable_diffusion_2
    monkeypatch.delenv('DA_VAE_HIP', raising=False)
    model = stable_diffusion_2(model_name='tiny', pretrained=False, fsdp=False, encode_latents_in_fp16=False)
    assert model.vae_dec_hip is None and model.vae_hip is None
