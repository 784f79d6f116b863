"""Sampling with LoRA adapters on the MI355X: ``generate()`` follows the merged weight shadows on every sampler route, a fused
master gives the same bits, and scale 0 / unloading give the base's.  Tiny model, 2 prompts, 3 steps, 64 x 64."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

pytestmark = pytest.mark.gpu

ROUTES = ('hip', 'graph', 'torch')
KW = dict(prompt=['a cool doge', 'a hot cat'], height=64, width=64, num_inference_steps=3, seed=3, progress_bar=False)
RANK, ALPHA = 8, 16.0


def _build(**kw):
    from diffusion_amd.models.models import stable_diffusion_2
    torch.manual_seed(11)    # the random frozen encoders of a model without weights
    return stable_diffusion_2(model_name='tiny', pretrained=False, fsdp=False, **kw)


def _adapter_file(path):
    """An adapter file written from the host layout alone: A as initialised, B ~ U(+-1 / sqrt(r)), default targets plus a conv."""
    from diffusion_amd import lora as L
    from diffusion_amd.models.unet import UNetConfig, build_layout
    ad = L.LoRAAdapters(build_layout(UNetConfig.tiny())[0], RANK, ALPHA, list(L.DEFAULT_TARGETS) + ['up_blocks.3.resnets.2.conv2'])
    ad.params = ad.init_params()
    g = torch.Generator().manual_seed(7)
    for it in ad.items:
        ad.B(it).copy_((torch.rand(it.N, it.r, generator=g) * 2 - 1) / math.sqrt(it.r))
    L.save_file(ad, path)
    return ad


def test_generate_follows_the_adapters_on_every_route(dev, tmp_path, monkeypatch):
    monkeypatch.delenv('DA_SAMPLER', raising=False)
    path = str(tmp_path / 'adapter.safetensors')
    host = _adapter_file(path)
    model = _build()
    unet = model.unet
    shadow0 = unet.shadow.clone()
    base = {s: model.generate(sampler=s, **KW) for s in ROUTES}
    ad = model.load_lora(path)
    assert (ad.rank, ad.alpha) == (RANK, ALPHA) and [i.module for i in ad.items] == [i.module for i in host.items]
    assert torch.equal(ad.params.cpu(), host.params)
    out = {s: model.generate(sampler=s, **KW) for s in ROUTES}
    for s in ROUTES:
        assert out[s].shape == (2, 3, 64, 64) and torch.isfinite(out[s]).all()
        assert not torch.equal(out[s], base[s]) and (out[s] - base[s]).abs().max() > 1e-2, s
    assert torch.equal(out['graph'], out['hip'])
    master = unet.master.clone()
    # strength 0 and unloading: the base's bits
    model.set_lora_scale(0)
    assert torch.equal(unet.shadow.view(torch.int16), shadow0.view(torch.int16))
    for s in ROUTES:
        assert torch.equal(model.generate(sampler=s, **KW), base[s]), s
    model.set_lora_scale(0.5)
    half = model.generate(sampler='hip', **KW)
    assert not torch.equal(half, base['hip']) and not torch.equal(half, out['hip'])
    model.set_lora_scale(1)
    assert torch.equal(model.generate(sampler='hip', **KW), out['hip'])
    model.unload_lora()
    assert unet.lora is None and torch.equal(unet.shadow.view(torch.int16), shadow0.view(torch.int16))
    assert torch.equal(unet.master, master)
    for s in ROUTES:
        assert torch.equal(model.generate(sampler=s, **KW), base[s]), s
    with pytest.raises(RuntimeError):
        model.set_lora_scale(1)
    # a second model whose master was fused with the same adapter: bit for bit the adapted output, on every route
    fused = _build()
    fused.load_lora(path)
    merged = fused.unet.shadow.clone()
    fused.unet.fuse_lora()
    assert fused.unet.lora is None and not torch.equal(fused.unet.master, master)
    assert torch.equal(fused.unet.shadow.view(torch.int16), merged.view(torch.int16))
    for s in ROUTES:
        assert torch.equal(fused.generate(sampler=s, **KW), out[s]), s
    # the factory route
    fac = _build(lora_path=path, lora_scale=0.5)
    assert fac.unet.lora is not None and torch.equal(fac.generate(sampler='hip', **KW), half)
    # save_lora writes what load_lora read
    fac.unet.save_lora(str(tmp_path / 'again.safetensors'))
    from diffusion_amd.lora import read_file
    sd, rank, alpha, _ = read_file(str(tmp_path / 'again.safetensors'))
    assert (rank, alpha) == (RANK, ALPHA) and all(torch.equal(v, host.state_dict()[k]) for k, v in sd.items())
