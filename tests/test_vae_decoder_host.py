"""Host-side contract of models/vae_hip.VAEDecoderHIP (no GPU)."""
import pytest


def test_decoder_refuses_a_cpu_device():
    """as VAEEncoderHIP: the walk has no CPU / PyTorch form, asking for one is an error"""
    from diffusion_amd.models.vae import AutoencoderKL
    from diffusion_amd.models.vae_hip import VAEDecoderHIP, VAEEncoderHIP
    vae = AutoencoderKL(block_out_channels=(32, 32), latent_channels=4)
    with pytest.raises(RuntimeError, match='VAEDecoderHIP'):
        VAEDecoderHIP(vae, device='cpu')
    with pytest.raises(RuntimeError, match='VAEEncoderHIP'):
        VAEEncoderHIP(vae, device='cpu')
