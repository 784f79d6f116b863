"""Constructors for diffusion models - mirrors the reference's diffusion/models/models.py:28-228.

``stable_diffusion_2`` keeps the reference signature (:28-39).  Differences forced by the platform:
  * nothing is fetched: the SD-2-base / SD-2.1 U-Net configs are embedded (``unet.UNetConfig``); ``model_name`` may
    be a LOCAL directory with ``unet/``, ``vae/``, ``text_encoder/``, ``tokenizer/`` sub-folders holding
    safetensors / vocab files, otherwise ``pretrained=True`` raises;
  * the U-Net is ``UNetHIP`` (hand-written gfx950 kernels) instead of ``diffusers.UNet2DConditionModel``;
  * the frozen VAE / text encoder are stock PyTorch-ROCm modules (random-init without local weights) and are only
    built when they can be needed (``precomputed_latents=False``) or when asked for with ``build_encoders=True``;
  * xformers (:109-111) is not a concept here: attention is always the fused flash kernels.

``discrete_pixel_diffusion`` / ``continuous_pixel_diffusion`` keep the reference signatures (:115, :175-179); the same
platform rules apply: the CLIP ViT-L/14 text config is embedded and ``clip_model_name`` may be a local directory with
its weights and tokenizer files (loaded strictly), else the encoder is random-init.  The frozen encoder runs on the HIP
kernels (``TextEncoderHIP``)."""
from __future__ import annotations

import os
import warnings
from typing import List, Optional

import torch

from .composer_shim import MeanSquaredError
from ..schedulers.schedulers import ContinuousTimeScheduler
from .pixel_diffusion import PixelDiffusion
from ..sampling import check_guidance_rescale
from ..train_noise import TrainNoise
from .schedulers import (DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler,  # noqa: F401
                         check_eta, check_inference_scheduler, check_snr_gamma, check_timestep_spacing,
                         make_inference_scheduler)
from .stable_diffusion import StableDiffusion
from .unet import UNetConfig, UNetHIP

_KNOWN = {
    'stabilityai/stable-diffusion-2-base': UNetConfig.sd2_base,
    'stabilityai/stable-diffusion-2-1-base': UNetConfig.sd2_base,
    'stabilityai/stable-diffusion-2': UNetConfig.sd21_768v,
    'stabilityai/stable-diffusion-2-1': UNetConfig.sd21_768v,
    'tiny': UNetConfig.tiny,
}


def _load_local_unet_weights(unet: UNetHIP, directory: str):
    from safetensors.torch import load_file
    for fn in ('diffusion_pytorch_model.safetensors', 'model.safetensors'):
        path = os.path.join(directory, 'unet', fn)
        if os.path.exists(path):
            unet.load_state_dict(load_file(path))
            return
    raise FileNotFoundError(f'no safetensors U-Net weights under {directory}/unet')


# diffusers < 0.17 checkpoints (the published SD-2 VAE files among them) name the mid-block attention projections
# query / key / value / proj_attn; later versions to_q / to_k / to_v / to_out.0.  Accept both.
_VAE_ATTN_RENAMES = (('.query.', '.to_q.'), ('.key.', '.to_k.'), ('.value.', '.to_v.'), ('.proj_attn.', '.to_out.0.'))


def load_local_vae_weights(vae, directory: str):
    """Strictly load ``<directory>/vae/*.safetensors`` into the PyTorch-ROCm AutoencoderKL (reference: models.py:80-85
    always loads pretrained VAE weights)."""
    from safetensors.torch import load_file
    for fn in ('diffusion_pytorch_model.safetensors', 'model.safetensors'):
        path = os.path.join(directory, 'vae', fn)
        if os.path.exists(path):
            sd = {}
            for k, v in load_file(path).items():
                if '.attentions.' in k:
                    for old, new in _VAE_ATTN_RENAMES:
                        k = k.replace(old, new)
                    if v.dim() == 4 and v.shape[-2:] == (1, 1) and ('.to_' in k):
                        v = v[:, :, 0, 0]  # very old checkpoints store the projections as 1x1 convolutions
                sd[k] = v
            vae.load_state_dict(sd, strict=True)
            return path
    raise FileNotFoundError(f'no safetensors VAE weights under {directory}/vae')


def _resolve_unet_config(model_name: str, unet_config: Optional[UNetConfig], probe: bool = False):
    """The U-Net config of ``stable_diffusion_2``: the given one, the embedded one of a known name, SD-2-base's for a local
    directory.  ``probe``: an unknown name gives SD-2-base's instead of raising (the early option checks only read
    ``prediction_type``; the name is refused where it always was, after the device check)."""
    if unet_config is not None:
        return unet_config
    if model_name in _KNOWN:
        return _KNOWN[model_name]()
    if probe or os.path.isdir(model_name):
        return UNetConfig.sd2_base()
    raise ValueError(f'unknown model_name {model_name!r}: known names {sorted(_KNOWN)} or a local directory')


def _check_zero_snr_options(zero_terminal_snr, prediction_type, timestep_spacing, guidance_rescale, snr_gamma):
    """The host-side checks of ``stable_diffusion_2``'s zero-terminal-SNR keywords, before the device is looked for: the
    resolved ``timestep_spacing`` (None: ``'trailing'`` with ``zero_terminal_snr``, else ``'leading'``)."""
    if zero_terminal_snr and prediction_type == 'epsilon':
        raise ValueError("zero_terminal_snr: at the last timestep the input is pure noise, so an epsilon prediction says "
                         "nothing about the sample; use a U-Net config with prediction_type 'v_prediction', got 'epsilon'")
    check_guidance_rescale(guidance_rescale)
    check_snr_gamma(snr_gamma)
    if timestep_spacing is None:
        return 'trailing' if zero_terminal_snr else 'leading'
    return check_timestep_spacing(timestep_spacing)


def _train_noise_options(noise_source, noise_offset, input_perturbation, timestep_range, timestep_sampling) -> TrainNoise:
    """The factories' five noising keywords as ``TrainNoise`` (a YAML list becomes the range's tuple).  Host only."""
    if isinstance(timestep_range, list):
        timestep_range = tuple(timestep_range)
    return TrainNoise(noise_source, noise_offset, input_perturbation, timestep_range, timestep_sampling)


def _check_inference_eta(inference_eta, inference_scheduler) -> float:
    """``inference_eta=`` of the factories: a number in [0, 1], and 0 unless the solver is DDIM.  Host only."""
    inference_eta = check_eta(inference_eta)
    if inference_eta and inference_scheduler != 'ddim':
        raise ValueError(f'inference_eta = {inference_eta} is the DDIM sampler\'s parameter: inference_scheduler '
                         f'{inference_scheduler!r} has none')
    return inference_eta


def stable_diffusion_2(
    model_name: str = 'stabilityai/stable-diffusion-2-base',
    pretrained: bool = True,
    train_metrics: Optional[List] = None,
    val_metrics: Optional[List] = None,
    val_guidance_scales: Optional[List] = None,
    val_seed: int = 1138,
    loss_bins: Optional[List] = None,
    precomputed_latents: bool = False,
    encode_latents_in_fp16: bool = True,
    fsdp: bool = True,
    build_encoders: Optional[bool] = None,
    unet_config: Optional[UNetConfig] = None,
    seed: int = 17,
    inference_scheduler: str = 'ddim',
    zero_terminal_snr: bool = False,
    snr_gamma: Optional[float] = None,
    timestep_spacing: Optional[str] = None,
    guidance_rescale: float = 0.0,
    inference_eta: float = 0.0,
    lora_path: Optional[str] = None,
    lora_scale: float = 1.0,
    noise_source: str = 'torch',
    noise_offset: float = 0.0,
    input_perturbation: float = 0.0,
    timestep_range=None,
    timestep_sampling: str = 'uniform',
):
    """``lora_path``: a safetensors LoRA file (diffusion_amd/lora.py) attached to the U-Net at ``lora_scale`` times its own
    alpha / r; sampling and evaluation then run with the adapted weights (``model.unload_lora()`` restores the base).

    ``inference_scheduler``: the solver ``generate()`` and ``eval_forward`` sample with, ``'ddim'`` (the reference's),
    ``'dpm++2m'`` (``DPMSolverMultistepScheduler``) or ``'dpm++2m-sde'`` (its SDE form: noise in every step).
    ``inference_eta``: the DDIM sampler's eta in [0, 1] (``ValueError`` above 0 with another solver); above 0 the sampler
    is stochastic, 1 is DDPM ancestral sampling.  ``eval_forward``, the image metrics and the image logger follow both, with
    ``val_seed`` as the base of the per-image seeds.

    ``zero_terminal_snr``: both schedulers rescale their betas so that the last timestep is pure noise (Lin et al.,
    arXiv:2305.08891; ``rescale_betas_zero_snr``); needs a v-prediction U-Net config.  ``timestep_spacing``: the inference
    grid, ``'leading'`` or ``'trailing'``; None means ``'trailing'`` with ``zero_terminal_snr``, else ``'leading'``.
    ``guidance_rescale``: the model's default for ``generate()``.  ``snr_gamma``: Min-SNR-gamma loss weighting
    (``StableDiffusion``).  What any of them does to image quality with trained weights has not been measured here.

    ``noise_source``, ``noise_offset``, ``input_perturbation``, ``timestep_range``, ``timestep_sampling``: the noising of the
    training step (``train_noise.TrainNoise``).  ``'philox'`` draws timesteps and noise per sample inside the noising launch,
    independent of the microbatch split and the world size; the other four need it."""
    train_noise = _train_noise_options(noise_source, noise_offset, input_perturbation, timestep_range, timestep_sampling)
    train_noise.discrete_range(1000)
    check_inference_scheduler(inference_scheduler)
    inference_eta = _check_inference_eta(inference_eta, inference_scheduler)
    pt = _resolve_unet_config(model_name, unet_config, probe=True).prediction_type
    timestep_spacing = _check_zero_snr_options(zero_terminal_snr, pt, timestep_spacing, guidance_rescale, snr_gamma)
    if train_metrics is None:
        train_metrics = [MeanSquaredError()]
    if val_metrics is None:
        val_metrics = [MeanSquaredError()]
    if val_guidance_scales is None:
        val_guidance_scales = [1.0, 3.0, 7.0]
    if loss_bins is None:
        loss_bins = [(0, 1)]
    if not torch.cuda.is_available():
        raise RuntimeError('stable_diffusion_2: an MI355X is required (the U-Net has no CPU path)')

    local = model_name if os.path.isdir(model_name) else None
    unet_config = _resolve_unet_config(model_name, unet_config)
    unet = UNetHIP(unet_config, device='cuda', seed=seed, init=True)
    if pretrained:
        if not local:
            raise RuntimeError('pretrained=True needs model_name to be a local checkpoint directory '
                               '(no network / HF hub in this environment)')
        _load_local_unet_weights(unet, local)

    if build_encoders is None:
        build_encoders = not precomputed_latents
    vae = text_encoder = vae_hip = vae_dec_hip = text_hip = None
    from .text import build_text_encoder, build_tokenizer
    tokenizer = build_tokenizer(os.path.join(local, 'tokenizer') if local else None)
    if build_encoders:
        from .vae import AutoencoderKL
        dtype = torch.float16 if encode_latents_in_fp16 else torch.float32
        vae = AutoencoderKL()
        te_dir = os.path.join(local, 'text_encoder') if local else None
        if local and os.path.isdir(os.path.join(local, 'vae')):
            load_local_vae_weights(vae, local)
        elif pretrained:
            raise FileNotFoundError(f'pretrained=True but {local}/vae holds no weights: the frozen VAE would be random '
                                    '(reference models.py:80-85 always loads it)')
        else:
            warnings.warn('AutoencoderKL is RANDOM-INIT (no local checkpoint directory): fine for throughput runs and '
                          'tests, meaningless for real training with precomputed_latents=False or for generate()')
        if pretrained and not (te_dir and os.path.isdir(te_dir)):
            raise FileNotFoundError(f'pretrained=True but {te_dir} is missing: the frozen text encoder would be random')
        # The HIP encoders compute in bf16 (activations and residual stream), i.e. at the precision class the caller asked
        # for with encode_latents_in_fp16=True (the reference default, models.py:37).  With encode_latents_in_fp16=False
        # the reference encodes the training targets in fp32: then the PyTorch-ROCm fp32 modules run unless the HIP
        # encoders are asked for explicitly (DA_VAE_HIP=1 / DA_TEXT_HIP=1).
        hip_default = '1' if encode_latents_in_fp16 else '0'
        if os.environ.get('DA_VAE_HIP', hip_default) != '0':
            # both halves of the frozen VAE on the HIP kernels (models/vae_hip.py), built from the fp32 weights: the encoder
            # for the training step, the decoder for generate()
            from .vae_hip import VAEDecoderHIP, VAEEncoderHIP
            vae_hip = VAEEncoderHIP(vae.to('cuda'))
            vae_dec_hip = VAEDecoderHIP(vae)
        vae = vae.to('cuda', dtype)
        text_encoder = build_text_encoder(te_dir, torch.float32, hidden_size=unet_config.cross_attention_dim).to('cuda')
        text_hip = None
        if os.environ.get('DA_TEXT_HIP', hip_default) != '0' and text_encoder.config.hidden_size % 64 == 0 and \
                text_encoder.config.hidden_size // text_encoder.config.num_attention_heads == 64:
            # the frozen text encoder on the HIP kernels (models/text_hip.py), built from the fp32 weights
            from .text_hip import TextEncoderHIP
            text_hip = TextEncoderHIP(text_encoder)
        text_encoder = text_encoder.to(dtype)
    noise_scheduler = DDPMScheduler(prediction_type=unet_config.prediction_type,
                                    rescale_betas_zero_snr=bool(zero_terminal_snr))
    inference_noise_scheduler = make_inference_scheduler(inference_scheduler, prediction_type=unet_config.prediction_type,
                                                         rescale_betas_zero_snr=bool(zero_terminal_snr),
                                                         timestep_spacing=timestep_spacing)
    if inference_eta:
        inference_noise_scheduler.eta = inference_eta

    model = StableDiffusion(
        unet=unet,
        vae=vae,
        text_encoder=text_encoder,
        tokenizer=tokenizer,
        noise_scheduler=noise_scheduler,
        inference_noise_scheduler=inference_noise_scheduler,
        train_metrics=train_metrics,
        val_metrics=val_metrics,
        val_guidance_scales=val_guidance_scales,
        val_seed=val_seed,
        loss_bins=loss_bins,
        precomputed_latents=precomputed_latents,
        encode_latents_in_fp16=encode_latents_in_fp16,
        fsdp=fsdp,
        snr_gamma=snr_gamma,
        guidance_rescale=guidance_rescale,
        train_noise=train_noise,
    )
    model.vae_hip = vae_hip if build_encoders else None
    model.vae_dec_hip = vae_dec_hip if build_encoders else None
    model.text_hip = text_hip if build_encoders else None
    if lora_path:
        model.load_lora(lora_path, lora_scale)
    return model


def _pixel_text_encoder(clip_model_name: str, hidden_size: int):
    """CLIP ViT-L/14 text encoder + tokenizer (reference models.py:136-137, :197-198), frozen, on the HIP kernels."""
    from .text import build_clip_text_encoder, build_tokenizer
    from .text_hip import TextEncoderHIP
    local = clip_model_name if os.path.isdir(clip_model_name) else None
    if local is None:
        warnings.warn(f'{clip_model_name!r} is not a local directory: the CLIP text encoder is RANDOM-INIT (nothing is '
                      'fetched); fine for throughput runs and tests, meaningless for real training')
        text_encoder = build_clip_text_encoder(None, hidden_size=hidden_size, intermediate_size=4 * hidden_size,
                                               num_attention_heads=max(1, hidden_size // 64))
    else:
        text_encoder = build_clip_text_encoder(local)
    text_encoder = text_encoder.to('cuda').requires_grad_(False)
    return text_encoder, build_tokenizer(local), TextEncoderHIP(text_encoder)


def _pixel_unet(unet_config: Optional[UNetConfig], seed: int) -> UNetHIP:
    # reference: UNet2DConditionModel(in_channels=3, out_channels=3, attention_head_dim=[5, 10, 20, 20],
    # cross_attention_dim=768, flip_sin_to_cos=True, use_linear_projection=True), random-init
    return UNetHIP(unet_config or UNetConfig.pixel(), device='cuda', seed=seed, init=True)


def discrete_pixel_diffusion(clip_model_name: str = 'openai/clip-vit-large-patch14', prediction_type='epsilon',
                             unet_config: Optional[UNetConfig] = None, seed: int = 17, inference_scheduler: str = 'ddim',
                             inference_eta: float = 0.0, noise_source: str = 'torch', noise_offset: float = 0.0,
                             input_perturbation: float = 0.0, timestep_range=None, timestep_sampling: str = 'uniform'):
    """Discrete-time (DDPM, 1000 steps) pixel diffusion; DDIM for inference (reference models.py:115-172), or with
    ``inference_scheduler='dpm++2m'`` the second-order multistep solver (``DPMSolverMultistepScheduler``), with
    ``'dpm++2m-sde'`` its SDE form.  ``inference_eta``: the DDIM sampler's eta in [0, 1] (0: deterministic).  The five
    noising keywords are ``stable_diffusion_2``'s (``train_noise.TrainNoise``)."""
    train_noise = _train_noise_options(noise_source, noise_offset, input_perturbation, timestep_range, timestep_sampling)
    train_noise.discrete_range(1000)
    check_inference_scheduler(inference_scheduler)
    inference_eta = _check_inference_eta(inference_eta, inference_scheduler)
    if not torch.cuda.is_available():
        raise RuntimeError('discrete_pixel_diffusion: an MI355X is required (the U-Net has no CPU path)')
    unet = _pixel_unet(unet_config, seed)
    text_encoder, tokenizer, text_hip = _pixel_text_encoder(clip_model_name, unet.cfg.cross_attention_dim)
    noise_scheduler = DDPMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                                    beta_schedule='scaled_linear', prediction_type=prediction_type, clip_sample=False)
    inference_scheduler = make_inference_scheduler(inference_scheduler, num_train_timesteps=1000, beta_start=0.00085,
                                                   beta_end=0.012, beta_schedule='scaled_linear', clip_sample=False,
                                                   steps_offset=1, prediction_type=prediction_type)
    if inference_eta:
        inference_scheduler.eta = inference_eta
    model = PixelDiffusion(unet, text_encoder, tokenizer, noise_scheduler, inference_scheduler=inference_scheduler,
                           prediction_type=prediction_type, train_metrics=[MeanSquaredError()],
                           val_metrics=[MeanSquaredError()], train_noise=train_noise)
    model.text_hip = text_hip
    return model


def continuous_pixel_diffusion(clip_model_name: str = 'openai/clip-vit-large-patch14', prediction_type='epsilon',
                               use_ode=False, train_t_max=1.570795, inference_t_max=1.56,
                               unet_config: Optional[UNetConfig] = None, seed: int = 17, inference_scheduler=None,
                               noise_source: str = 'torch', noise_offset: float = 0.0, input_perturbation: float = 0.0,
                               timestep_range=None, timestep_sampling: str = 'uniform'):
    """Continuous-time pixel diffusion: the VP process with angle = time (tangent schedule), t in [0, train_t_max) for
    training, the reverse SDE (or with ``use_ode`` the probability-flow ODE) from ``inference_t_max`` for generation
    (reference models.py:175-228).  ``inference_scheduler`` exists to refuse: the named solvers (``'ddim'``,
    ``'dpm++2m'``) and multistep scheduler objects are discrete-time methods and raise ``ValueError``.  The five noising
    keywords are ``stable_diffusion_2``'s; ``timestep_range`` is in fractions of ``train_t_max``."""
    train_noise = _train_noise_options(noise_source, noise_offset, input_perturbation, timestep_range, timestep_sampling)
    train_noise.continuous_range(train_t_max)
    check_inference_scheduler(inference_scheduler, continuous_time=True)
    if inference_scheduler is not None:
        raise ValueError('continuous_pixel_diffusion builds its own ContinuousTimeScheduler (use_ode, inference_t_max)')
    if not torch.cuda.is_available():
        raise RuntimeError('continuous_pixel_diffusion: an MI355X is required (the U-Net has no CPU path)')
    unet = _pixel_unet(unet_config, seed)
    text_encoder, tokenizer, text_hip = _pixel_text_encoder(clip_model_name, unet.cfg.cross_attention_dim)
    noise_scheduler = ContinuousTimeScheduler(t_max=train_t_max, prediction_type=prediction_type)
    inference_scheduler = ContinuousTimeScheduler(t_max=inference_t_max, prediction_type=prediction_type,
                                                  use_ode=use_ode)
    model = PixelDiffusion(unet, text_encoder, tokenizer, noise_scheduler, inference_scheduler=inference_scheduler,
                           prediction_type=prediction_type, continuous_time=True, train_metrics=[MeanSquaredError()],
                           val_metrics=[MeanSquaredError()], train_noise=train_noise)
    model.text_hip = text_hip
    return model
