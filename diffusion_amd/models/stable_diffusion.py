"""``StableDiffusion`` ComposerModel on the HIP U-Net.

Mirrors /root/reference diffusion/models/stable_diffusion.py: constructor kwargs (:69-88), ``forward`` (:154-183),
``loss`` (:185-187), ``eval_forward`` (:189-208), ``get_metrics`` (:210-226), ``update_metric`` (:228-257),
``generate`` (:260-382).  Differences, all on the device side:
  * ``add_noise`` (:180), the NCHW->NHWC relayout, the U-Net (:183), ``F.mse_loss`` (:187) and the whole backward
    run as hand-written gfx950 kernels; RNG draws (:177,179) stay on torch's global generator like the reference.
  * ``loss()`` returns a 0-d tensor whose ``.backward()`` runs the HIP backward into the U-Net's flat fp32
    gradient buffer (so Composer-style trainers work unchanged); ``backward_from_loss()`` is the direct call.
  * ``prediction_type='v_prediction'`` (docstring :40-43, never wired in the reference's forward) follows
    diffusion/models/pixel_diffusion.py:90-91.
"""
from __future__ import annotations

import copy
from typing import List, Optional

import torch
import torch.nn.functional as F

from .. import ops
from ..sampling import (LatentSampler, check_guidance_rescale, check_seed, image_seeds, philox_latents, rescale_noise_cfg,
                        resolve_sampler)
from ..train_noise import TrainNoise, check_injected
from ..train_noise import add_noise as train_noise_add
from .composer_shim import ComposerModel, MeanSquaredError, Metric
from .schedulers import (check_eta, check_inference_scheduler, check_snr_gamma, check_timestep_spacing,
                         check_zero_snr_grid, is_stochastic, min_snr_weights, resolve_inference_scheduler, with_eta,
                         with_timestep_spacing)
from .unet import UNetHIP
from .vae import DiagonalGaussian

try:
    from tqdm.auto import tqdm
except Exception:  # noqa: BLE001
    tqdm = lambda x, **kw: x  # noqa: E731


class _HIPBackward(torch.autograd.Function):
    """Gives the fused-loss scalar an autograd edge: ``loss.backward()`` -> UNetHIP.backward_features."""

    @staticmethod
    def forward(ctx, anchor, loss_value, model):
        ctx.model = model
        return loss_value.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.model._run_backward(g)
        return torch.zeros((), device=g.device), None, None


class StableDiffusion(ComposerModel):

    def __init__(self,
                 unet,
                 vae,
                 text_encoder,
                 tokenizer,
                 noise_scheduler,
                 inference_noise_scheduler,
                 loss_fn=F.mse_loss,
                 train_metrics: Optional[List] = None,
                 val_metrics: Optional[List] = None,
                 val_seed: int = 1138,
                 val_guidance_scales: Optional[List] = None,
                 loss_bins: Optional[List] = None,
                 image_key: str = 'image',
                 text_key: str = 'captions',
                 image_latents_key: str = 'image_latents',
                 text_latents_key: str = 'caption_latents',
                 precomputed_latents: bool = False,
                 encode_latents_in_fp16: bool = False,
                 fsdp: bool = False,
                 prediction_type: Optional[str] = None,
                 snr_gamma: Optional[float] = None,
                 guidance_rescale: float = 0.0,
                 train_noise: Optional[TrainNoise] = None):
        """``snr_gamma``: None, or the gamma of Min-SNR loss weighting (Hang et al., arXiv:2303.09556): every sample's
        squared error and gradient are weighted by its timestep's entry of ``schedulers.min_snr_weights`` in the fused loss
        launch (``ops.mse_loss_w``); ``loss()`` then reports the weighted loss.  ``guidance_rescale``: the default of
        ``generate(guidance_rescale=None)``, hence of ``eval_forward`` and the image metrics and loggers built on it.
        ``train_noise``: the noising options (``train_noise.TrainNoise``); with ``noise_source='philox'`` ``forward`` draws
        timesteps and noise per sample inside the noising launch."""
        super().__init__()
        self.train_noise = train_noise if train_noise is not None else TrainNoise()
        if self.train_noise.timestep_range is not None:   # an out-of-table range is refused here, not at the first step
            self.train_noise.discrete_range(len(noise_scheduler))
        self.snr_gamma = _check_loss_options(snr_gamma, loss_fn)
        self.guidance_rescale = check_guidance_rescale(guidance_rescale)
        self._snr_tables = {}
        self.unet = unet
        self.vae = vae
        self.noise_scheduler = noise_scheduler
        self.loss_fn = loss_fn
        self.val_seed = val_seed
        self.image_key = image_key
        self.image_latents_key = image_latents_key
        self.precomputed_latents = precomputed_latents
        self.prediction_type = prediction_type or getattr(noise_scheduler, 'prediction_type', 'epsilon')
        if self.prediction_type not in ('epsilon', 'v_prediction'):
            raise ValueError(f'prediction type must be epsilon or v_prediction. Got {self.prediction_type}')

        self.train_metrics = [MeanSquaredError()] if train_metrics is None else train_metrics
        if val_metrics is None:
            val_metrics = [MeanSquaredError()]
        if val_guidance_scales is None:
            val_guidance_scales = [0.0]
        if loss_bins is None:
            loss_bins = [(0, 1)]
        self.val_guidance_scales = val_guidance_scales
        self.val_metrics = {}
        metrics_to_sweep = ['FrechetInceptionDistance', 'KernelInceptionDistance', 'InceptionScore', 'CLIPScore']
        for metric in val_metrics:
            name = metric.__class__.__name__
            if name in metrics_to_sweep:
                for scale in val_guidance_scales:
                    new_metric = copy.deepcopy(metric)
                    new_metric.guidance_scale = scale
                    self.val_metrics[f'{name}-scale-{str(scale).replace(".", "p")}'] = new_metric
            elif isinstance(metric, MeanSquaredError):
                for bin in loss_bins:
                    new_metric = copy.deepcopy(metric)
                    new_metric.loss_bin = bin
                    self.val_metrics[f'{name}-bin-{bin[0]}-to-{bin[1]}'.replace('.', 'p')] = new_metric
            else:
                self.val_metrics[name] = metric
        self.val_metrics['MeanSquaredError'] = MeanSquaredError()

        self.text_encoder = text_encoder
        self.tokenizer = tokenizer
        self.inference_scheduler = inference_noise_scheduler
        self.text_key = text_key
        self.text_latents_key = text_latents_key
        self.encode_latents_in_fp16 = encode_latents_in_fp16
        # freeze the encoders (reference :143-147)
        if self.text_encoder is not None:
            self.text_encoder.requires_grad_(False)
        if self.vae is not None:
            self.vae.requires_grad_(False)
        if self.encode_latents_in_fp16:
            if self.text_encoder is not None:
                self.text_encoder.half()
            if self.vae is not None:
                self.vae.half()
        if fsdp:
            if self.text_encoder is not None:
                self.text_encoder._fsdp_wrap = False
            if self.vae is not None:
                self.vae._fsdp_wrap = False
            self.unet._fsdp_wrap = True
        self._pending = None
        self._pending_t = None

    # ------------------------------------------------------------------------------------------
    def _text_states(self, input_ids):
        """``text_encoder(ids)[0]`` (reference :168,172): the HIP-kernel walk of the frozen weights when the factory built
        one (models/text_hip.py), else the PyTorch-ROCm module."""
        enc = getattr(self, 'text_hip', None)
        return (enc if enc is not None else self.text_encoder)(input_ids)[0]

    def ingest_raw(self, batch):
        """A batch of packed raw images (``image_raw`` / ``image_off`` / ``image_hw`` from
        ``datasets.image_ingest.collate_raw_images``) -> the same batch with the three keys replaced by what the image encoder
        reads: ``image_nhwc8`` bf16 [B, Rh, Rw, 8] for the HIP VAE encoder, else the reference's fp32 ``image``
        [B, 3, Rh, Rw].  One non-blocking upload of the bytes and one kernel (``ops.image_ingest``, or
        ``ops.image_ingest_rect`` for a rectangular target): the reference's LargestCenterSquare -> ToTensor -> Normalize
        (laion.py:159-164).  The target is the batch's ``image_size`` (what the dataloader was built with: an int, or an
        ``(Rh, Rw)`` pair; in a bucketed run the batch's bucket), else ``unet.config.sample_size * 8``.  A batch that carries
        ``image_aug`` (crop origin and flip per image, ``datasets/buckets.py``) goes through ``ops.image_ingest_aug``.

        A batch with an ``image_transform`` (the COCO evaluation loader's: the ``ops.image_resize`` switches) always becomes
        the fp32 ``image`` [B, 3, Rh, Rw] in [0, 1], HIP VAE or not: ``eval_forward`` reads its size to generate at and
        ``update_metric`` hands it to the image metrics.  The VAE then sees un-normalised [0, 1] images at evaluation, as in
        the reference (coco_captions.py:105-108 has no Normalize)."""
        from ..datasets.image_ingest import RAW_KEYS, ingest_batch, target_hw
        R = batch.get('image_size') or self.unet.config.sample_size * 8
        R = target_hw(R) if hasattr(R, '__len__') else int(R)
        Rh, Rw = target_hw(R)
        transform = batch.get('image_transform')
        hip = getattr(self, 'vae_hip', None) is not None and transform is None
        out = ingest_batch(batch, R, 0 if hip else 1, self.unet.device_, transform)
        rest = {k: v for k, v in batch.items() if k not in RAW_KEYS and k not in ('image_size', 'image_transform', 'image_aug')}
        rest['image_nhwc8' if hip else self.image_key] = out.view(-1, Rh, Rw, 8) if hip else out
        return rest

    def _encode(self, batch):
        """latents / conditioning selection, reference :155-174."""
        if self.precomputed_latents and self.image_latents_key in batch and self.text_latents_key in batch:
            return batch[self.image_latents_key], batch[self.text_latents_key]
        if self.vae is None or self.text_encoder is None:
            raise RuntimeError('this model was built without VAE / text encoder; pass precomputed latents')
        if 'image_raw' in batch:
            batch = self.ingest_raw(batch)
        vae_hip = getattr(self, 'vae_hip', None)
        nhwc8 = batch.get('image_nhwc8') if vae_hip is not None else None
        inputs, conditioning = (None if nhwc8 is not None else batch[self.image_key]), batch[self.text_key]
        conditioning = conditioning.view(-1, conditioning.shape[-1])
        # image encoder: the HIP-kernel walk of the same frozen weights when the factory built one (models/vae_hip.py),
        # else the PyTorch-ROCm module
        with torch.no_grad():
            if nhwc8 is not None:   # ingested raw images, already in conv_in's layout
                Bn, Hn, Wn, _ = nhwc8.shape
                mom = vae_hip.moments_nhwc8(nhwc8.contiguous().view(-1, 8), Bn, Hn, Wn)
                latents = DiagonalGaussian(mom).sample().data
                with torch.autocast('cuda', enabled=False):
                    conditioning = self._text_states(conditioning)
            elif vae_hip is not None:
                latents = vae_hip.encode(inputs)['latent_dist'].sample().data
                with torch.autocast('cuda', enabled=False):
                    conditioning = self._text_states(conditioning)
            elif self.encode_latents_in_fp16:
                with torch.autocast('cuda', enabled=False):
                    latents = self.vae.encode(inputs.half())['latent_dist'].sample().data
                    conditioning = self._text_states(conditioning)
            else:
                latents = self.vae.encode(inputs)['latent_dist'].sample().data
                conditioning = self._text_states(conditioning)
        latents *= 0.18215
        return latents, conditioning

    def forward(self, batch, timesteps: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None):
        """Returns ``(unet_out, target, timesteps)`` like the reference (:183).  ``timesteps`` / ``noise`` may be
        injected for parity tests (as arguments, or as ``batch['_timesteps']`` / ``batch['_noise']`` so that they pass
        through a trainer's microbatch slicing); by default they are drawn from torch's global RNG exactly as :177-179.

        With ``train_noise.noise_source == 'philox'`` the noising launch draws them per sample (``ops.add_noise_rng``) from
        ``batch['_sample_seeds']`` (uint64 [B]; without it B seeds are drawn from torch's generator on the device) and, for
        stratified timesteps, ``batch['_sample_slots']`` / ``batch['_n_slots']``; ``target`` is then a view of the kernel's
        NHWC-8 target for either prediction type, injected timesteps are read, and injected noise is a ``ValueError``."""
        if timesteps is None:
            timesteps = batch.get('_timesteps')
        if noise is None:
            noise = batch.get('_noise')
        check_injected(self.train_noise, noise)
        latents, conditioning = self._encode(batch)
        unet: UNetHIP = self.unet
        dev = unet.device_
        latents = latents.to(dev)
        B, _, H, W = latents.shape
        unet.check_spatial(H, W)
        if self.train_noise.philox:
            # one launch draws and noises: seeds (and strata) per sample from the batch, no NCHW noise tensor; the kernel
            # leaves the timesteps in device memory for the embedding and the Min-SNR weights
            xt, target8, t = train_noise_add(self.train_noise, batch, latents.float().contiguous(), timesteps,
                                             self.prediction_type, self.noise_scheduler.device_tables(dev))
            ctx = unet.prepare_ctx(conditioning.to(dev))
            pred8 = unet.forward_features(xt, t, ctx, B, (H, W))
            self._pending = (pred8, target8, B * H * W)
            self._pending_t = t if self.snr_gamma is not None else None
            return (pred8.view(B, H, W, 8)[..., :4].permute(0, 3, 1, 2),
                    target8.view(B, H, W, 8)[..., :4].permute(0, 3, 1, 2), t)
        if timesteps is None:
            timesteps = torch.randint(0, len(self.noise_scheduler), (B,), device=dev)
        if noise is None:
            noise = torch.randn_like(latents)
        x0 = latents.float().contiguous()
        eps = noise.to(dev).float().contiguous()
        t = timesteps.to(dev, torch.int64).contiguous()
        sa, sb = self.noise_scheduler.device_tables(dev)
        xt = torch.empty(B * H * W, 8, device=dev, dtype=torch.bfloat16)
        target8 = torch.empty(B * H * W, 8, device=dev, dtype=torch.float32)
        v_pred = self.prediction_type == 'v_prediction'
        ops.add_noise(x0, eps, t, sa, sb, xt, target8, v_pred)
        ctx = unet.prepare_ctx(conditioning.to(dev))
        pred8 = unet.forward_features(xt, t, ctx, B, (H, W))
        pred = pred8.view(B, H, W, 8)[..., :4].permute(0, 3, 1, 2)
        target = target8.view(B, H, W, 8)[..., :4].permute(0, 3, 1, 2) if v_pred else noise
        self._pending = (pred8, target8, B * H * W)
        # the timesteps of the pending forward, kept only for the Min-SNR weighted loss
        self._pending_t = t if self.snr_gamma is not None else None
        return pred, target, timesteps

    def snr_weight_table(self, device):
        """The Min-SNR weight of every training timestep as an fp32 table on ``device``: built once on the host in float64
        (``schedulers.min_snr_weights``) from ``noise_scheduler.alphas_cumprod``, cached per device like ``device_tables``."""
        key = str(device)
        if key not in self._snr_tables:
            w = min_snr_weights(self.noise_scheduler.alphas_cumprod, self.snr_gamma, self.prediction_type)
            self._snr_tables[key] = w.to(torch.float32).to(device).contiguous()
        return self._snr_tables[key]

    def loss(self, outputs, batch, weight: float = 1.0):
        """MSE between U-Net output and target (reference :185-187) - fused loss + gradient kernel.
        ``weight`` pre-scales the gradient (microbatch fraction) when the trainer calls backward directly."""
        if self._pending is None:
            raise RuntimeError('loss() must follow forward()')
        pred8, target8, npix = self._pending
        unet: UNetHIP = self.unet
        if self.loss_fn is F.mse_loss:
            dpred = torch.empty(npix, 8, device=pred8.device, dtype=torch.bfloat16)
            lossbuf = torch.zeros(1, device=pred8.device, dtype=torch.float32)
            if self.snr_gamma is not None:   # the same fused launch with the timestep's Min-SNR weight per sample
                t = self._pending_t
                if t is None:
                    raise RuntimeError('snr_gamma was set after forward(): loss() has no timesteps to weight by')
                ops.mse_loss_w(pred8, target8, dpred, lossbuf, unet._scratch, npix, 4, npix // t.numel(), t,
                               self.snr_weight_table(pred8.device), 2.0 * weight / (4.0 * npix), 1.0, 0)
            else:
                ops.mse_loss(pred8, target8, dpred, lossbuf, unet._scratch, npix, 2.0 * weight / (4.0 * npix), 1.0, 0)
            self._dpred = dpred
            anchor = torch.zeros((), device=pred8.device, requires_grad=True)
            return _HIPBackward.apply(anchor, lossbuf[0], self)
        # user-supplied loss: scalar maths on torch autograd, U-Net backward still on the HIP path
        p = outputs[0].detach().float().requires_grad_(True)
        val = self.loss_fn(p, outputs[1].detach().float())
        (gp,) = torch.autograd.grad(val, p)
        self._dpred = unet.to_nhwc8(gp * weight)
        anchor = torch.zeros((), device=pred8.device, requires_grad=True)
        return _HIPBackward.apply(anchor, val.detach(), self)

    def _run_backward(self, g: Optional[torch.Tensor] = None):
        dpred, self._dpred = self._dpred, None
        if dpred is None:
            raise RuntimeError('backward already consumed')
        if g is not None:
            dpred = (dpred.float() * g).to(torch.bfloat16)  # [M,8] boundary scaling for external trainers
        self.unet.backward_features(dpred)
        self._pending = None

    def backward_from_loss(self):
        """Direct (no autograd) backward for the in-tree trainer; gradient weight was given to ``loss()``."""
        self._run_backward(None)

    # ------------------------------------------------------------------------------------------
    # LoRA adapters (diffusion_amd/lora.py): the U-Net's bf16 weight shadows carry them, so generate(), eval_forward, the
    # metrics and every sampler route follow without knowing
    def load_lora(self, path: str, scale: float = 1.0):
        return self.unet.load_lora(path, scale)

    def unload_lora(self):
        self.unet.remove_lora()

    def set_lora_scale(self, x: float):
        self.unet.set_lora_scale(x)

    # ------------------------------------------------------------------------------------------
    def eval_forward(self, batch, outputs=None):
        if outputs is not None:
            return outputs
        with torch.no_grad():
            unet_out, target, timesteps = self.forward(batch)
        self._pending = None
        self.unet._tape = None
        generated_images = {}
        if self.text_key in batch and self.image_key in batch and self.vae is not None:
            prompts = batch[self.text_key]
            height, width = batch[self.image_key].shape[-2], batch[self.image_key].shape[-1]
            for guidance_scale in self.val_guidance_scales:
                generated_images[guidance_scale] = self.generate(tokenized_prompts=prompts, height=height, width=width,
                                                                 guidance_scale=guidance_scale, seed=self.val_seed,
                                                                 progress_bar=False)
        return unet_out, target, timesteps, generated_images

    def get_metrics(self, is_train: bool = False):
        metrics = self.train_metrics if is_train else self.val_metrics
        if isinstance(metrics, Metric):
            return {metrics.__class__.__name__: metrics}
        if isinstance(metrics, list):
            # the reference keys every list entry by the list's class name (:219); keyed per metric here
            return {m.__class__.__name__: m for m in metrics}
        out = {}
        for name, metric in metrics.items():
            assert isinstance(metric, Metric)
            out[name] = metric
        return out

    def update_metric(self, batch, outputs, metric):
        if isinstance(metric, MeanSquaredError) and hasattr(metric, 'loss_bin'):
            loss_bin = metric.loss_bin
            T_max = self.noise_scheduler.num_train_timesteps
            idx = torch.where((outputs[2] >= loss_bin[0] * T_max) & (outputs[2] < loss_bin[1] * T_max))
            metric.update(outputs[0][idx], outputs[1][idx])
        elif isinstance(metric, MeanSquaredError):
            metric.update(outputs[0], outputs[1])
        elif metric.__class__.__name__ == 'FrechetInceptionDistance':
            metric.update(batch[self.image_key], real=True)
            metric.update(outputs[3][metric.guidance_scale], real=False)
        elif metric.__class__.__name__ == 'KernelInceptionDistance':
            metric.update(batch[self.image_key], real=True)
            metric.update(outputs[3][metric.guidance_scale], real=False)
        elif metric.__class__.__name__ == 'InceptionScore':
            metric.update(outputs[3][metric.guidance_scale])
        elif metric.__class__.__name__ == 'CLIPScore':
            captions = [self.tokenizer.decode(c, skip_special_tokens=True) for c in batch[self.text_key]]
            metric.update((outputs[3][metric.guidance_scale] * 255).to(torch.uint8), captions)
        else:
            metric.update(outputs[0], outputs[1])

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate(self, prompt: Optional[list] = None, negative_prompt: Optional[list] = None,
                 tokenized_prompts: Optional[torch.LongTensor] = None,
                 tokenized_negative_prompts: Optional[torch.LongTensor] = None,
                 prompt_embeds: Optional[torch.FloatTensor] = None,
                 negative_prompt_embeds: Optional[torch.FloatTensor] = None, height: Optional[int] = None,
                 width: Optional[int] = None, num_inference_steps: int = 50, guidance_scale: float = 3.0,
                 num_images_per_prompt: int = 1, seed: Optional[int] = None, progress_bar: bool = True,
                 guidance_rescale: Optional[float] = None, timestep_spacing: Optional[str] = None,
                 eta: Optional[float] = None,
                 sampler: Optional[str] = None, inference_scheduler=None, init_image: Optional[torch.Tensor] = None,
                 strength: float = 0.8, mask: Optional[torch.Tensor] = None):
        """DDIM sampling with classifier-free guidance on the HIP U-Net forward (reference :260-382).

        Stochastic sampling: ``eta`` in [0, 1] is the DDIM sampler's eta for this call (default the scheduler's own, 0 unless
        the factory was given ``inference_eta``; 1 is DDPM ancestral sampling; ``ValueError`` with another solver), and
        ``inference_scheduler='dpm++2m-sde'`` the SDE form of the two-step solver.  Their step noise comes from per-image
        Philox streams (``ops.randn_philox``; drawn inside the step launch on the ``'hip'`` and ``'graph'`` routes, passed as
        ``variance_noise`` on the ``'torch'`` route, the same values on all three).  ``seed`` may then be a sequence of one
        integer in [0, 2^64) per generated image (the ``num_images_per_prompt`` copies included): the initial latents come
        from the image's own stream too and image i depends on nothing else in the batch (up to the U-Net's batch-dependent
        GEMM splits; the VAE posterior draw of ``init_image`` stays on the torch generator, seeded with the first entry).
        With an int ``seed`` the initial latents stay on the torch generator and image b's step noise has seed ``seed + b``;
        with None one base seed is drawn from the torch generator.

        ``sampler``: ``'hip'`` (``sampling.LatentSampler``: forward-only walk, context K/V projected once, one fused
        guidance + scheduler-step launch per step), ``'graph'`` (the same, one hipGraph replay per step) or ``'torch'``
        (the reference's loop in torch ops around ``unet(...)``); default ``DA_SAMPLER``, else ``'hip'``.

        ``inference_scheduler``: the solver of this call only: ``'ddim'``, ``'dpm++2m'`` (``DPMSolverMultistepScheduler``
        on the model's noise tables) or a scheduler object; default the model's own (``self.inference_scheduler``).

        ``init_image`` (image-to-image): floats in [0, 1] (what this method returns), [B, 3, H, W] or [1, 3, H, W] for the
        whole batch; ``height`` / ``width`` default to its size.  It is encoded by the VAE (``z0 = 0.18215 *
        latent_dist.sample()``: the call's generator draws the posterior sample first, the noise second), noised to an
        intermediate timestep and only the last ``int(num_inference_steps * strength)`` steps run; ``strength`` in (0, 1].
        ``mask`` (inpainting, needs ``init_image``): [H, W], [1, 1, H, W] or [B, 1, H, W] in [0, 1], 1 = repaint, 0 = keep,
        fractions blend; after every step the latent outside the mask is replaced by ``z0`` re-noised to the level of the
        next timestep (the 4-channel scheme of diffusers' ``StableDiffusionInpaintPipeline``).  Kept areas come back through
        the VAE round trip: there is no pixel-space composite after decoding.  Every ``sampler=`` route takes them.

        ``guidance_rescale`` (phi in [0, 1]; default the model's ``guidance_rescale``): under guidance the guided prediction
        is scaled per sample to phi std(cond) / std(guided) + 1 - phi times itself (Lin et al., arXiv:2305.08891; diffusers'
        ``rescale_noise_cfg``).  ``timestep_spacing``: ``'leading'`` or ``'trailing'`` for this call; default the
        scheduler's own.  Both apply on every ``sampler=`` route, with either solver, with ``init_image`` and ``mask``.  An
        epsilon-prediction scheduler on a zero-terminal-SNR table raises ``ValueError`` if the grid visits the last
        timestep.  All of it is checked before anything is launched."""
        sampler = resolve_sampler(sampler)
        check_inference_scheduler(inference_scheduler)
        _check_prompt_given(prompt, tokenized_prompts, prompt_embeds)
        _check_prompt_lenths(prompt, negative_prompt)
        _check_prompt_lenths(tokenized_prompts, tokenized_negative_prompts)
        _check_prompt_lenths(prompt_embeds, negative_prompt_embeds)
        height, width, start_index = _check_init_image(
            init_image, strength, mask, height, width, num_inference_steps,
            _prompt_batch(prompt, tokenized_prompts, prompt_embeds) * num_images_per_prompt)
        scheduler, guidance_rescale = _resolve_sampling_options(
            inference_scheduler, self.inference_scheduler, guidance_rescale, self.guidance_rescale, timestep_spacing,
            num_inference_steps, eta)
        seed = check_seed(seed, _prompt_batch(prompt, tokenized_prompts, prompt_embeds) * num_images_per_prompt)
        stochastic = is_stochastic(scheduler)
        device = self.unet.device_
        rng = torch.Generator(device=device)
        if isinstance(seed, list):
            rng = rng.manual_seed(seed[0] % 2**63)
        elif seed:
            rng = rng.manual_seed(seed)
        vae_scale = 8
        height = height or self.unet.config.sample_size * vae_scale
        width = width or self.unet.config.sample_size * vae_scale
        if height % vae_scale or width % vae_scale:
            raise ValueError(f'generate: height and width must be multiples of {vae_scale} (the VAE), got {height} x {width}')
        self.unet.check_spatial(height // vae_scale, width // vae_scale)   # 8 * 2 ** (levels - 1) pixels: 64 for SD-2
        do_cfg = guidance_scale > 1.0
        text_embeddings = self._prepare_text_embeddings(prompt, tokenized_prompts, prompt_embeds, num_images_per_prompt)
        batch_size = len(text_embeddings)
        if do_cfg:
            if not negative_prompt and not tokenized_negative_prompts and not negative_prompt_embeds:
                negative_prompt = [''] * (batch_size // num_images_per_prompt)
            uncond = self._prepare_text_embeddings(negative_prompt, tokenized_negative_prompts, negative_prompt_embeds,
                                                   num_images_per_prompt)
            if sampler == 'torch':
                text_embeddings = torch.cat([uncond, text_embeddings])
        z0 = mask_px = None
        if init_image is not None:   # the posterior sample is drawn before the noise
            z0 = self._encode_init_image(init_image, batch_size, rng)
            if mask is not None:
                mask_px = mask.to(device, torch.float32).reshape(-1, height, width).expand(batch_size, -1, -1).contiguous()
        shape = (batch_size, self.unet.config.in_channels, height // vae_scale, width // vae_scale)
        if isinstance(seed, list):   # per-image seeds: the initial noise from the image's own stream
            latents = philox_latents(seed, shape, device)
        else:
            latents = torch.randn(shape, device=device, generator=rng)
        seeds = image_seeds(seed, batch_size, stochastic, rng)
        scheduler.set_timesteps(num_inference_steps)
        latents = latents * scheduler.init_noise_sigma
        if sampler != 'torch':
            partial = {} if z0 is None else dict(known=z0, start_index=start_index, mask_px=mask_px)
            latents = LatentSampler(self.unet, scheduler).sample(
                latents, text_embeddings, uncond if do_cfg else None, num_inference_steps=num_inference_steps,
                guidance_scale=guidance_scale, graph=sampler == 'graph', progress_bar=progress_bar,
                guidance_rescale=guidance_rescale, **partial, **(dict(seeds=seeds) if stochastic else {}))
        else:   # the reference's loop, the scheduler step in torch ops
            timesteps = scheduler.timesteps
            step_noise = _philox_step_noise(seeds, latents.shape, device) if stochastic else (lambda i: {})
            if z0 is not None:   # the same method in torch ops: start from the noised image, run the tail of the schedule
                noise = latents
                latents = scheduler.add_noise(z0, noise, timesteps[start_index:start_index + 1])
                if start_index and hasattr(scheduler, 'set_begin_index'):
                    scheduler.set_begin_index(start_index)
                if mask_px is not None:
                    m = F.avg_pool2d(mask_px[:, None], vae_scale)
            for i in tqdm(range(start_index, len(timesteps)), disable=not progress_bar):
                t = timesteps[i]
                lin = torch.cat([latents] * 2) if do_cfg else latents
                lin = scheduler.scale_model_input(lin, t)
                pred = self.unet(lin, t, encoder_hidden_states=text_embeddings).sample
                if do_cfg:
                    pu, pt = pred.chunk(2)
                    pred = rescale_noise_cfg(pu + guidance_scale * (pt - pu), pt, guidance_rescale)
                latents = scheduler.step(pred, t, latents, generator=rng, **step_noise(i))['prev_sample']
                if mask_px is not None:   # outside the mask: the known latent at the noise level of the next timestep
                    kn = scheduler.add_noise(z0, noise, timesteps[i + 1:i + 2]) if i + 1 < len(timesteps) else z0
                    latents = m * latents + (1 - m) * kn
        latents = 1 / 0.18215 * latents
        # image decoder: the HIP-kernel walk of the same frozen weights when the factory built one (models/vae_hip.py),
        # else the PyTorch-ROCm module
        vae_dec_hip = getattr(self, 'vae_dec_hip', None)
        if vae_dec_hip is not None:
            image = vae_dec_hip.decode(latents).sample
        else:
            vdtype = next(self.vae.parameters()).dtype
            image = self.vae.decode(latents.to(vdtype)).sample
        image = (image / 2 + 0.5).clamp(0, 1)
        return image.detach().float()

    def _encode_init_image(self, init_image, batch_size, rng):
        """``generate(init_image=...)``: [0, 1] images -> z0 = 0.18215 * latent_dist.sample(generator=rng), [B, C, h, w] fp32,
        through the HIP VAE encoder when the factory built one, else the PyTorch-ROCm module (as ``_encode`` does)."""
        if self.vae is None:
            raise RuntimeError('this model was built without a VAE; init_image needs one')
        device = self.unet.device_
        img = (init_image.to(device, torch.float32) * 2 - 1).expand(batch_size, -1, -1, -1)
        vae_hip = getattr(self, 'vae_hip', None)
        if vae_hip is not None:
            dist = vae_hip.encode(img)['latent_dist']
        else:
            dist = self.vae.encode(img.to(next(self.vae.parameters()).dtype))['latent_dist']
        return (0.18215 * dist.sample(generator=rng)).float()

    def _prepare_text_embeddings(self, prompt, tokenized_prompts, prompt_embeds, num_images_per_prompt):
        device = self.unet.device_
        if prompt_embeds is None:
            if tokenized_prompts is None:
                tokenized_prompts = self.tokenizer(prompt, padding='max_length',
                                                   max_length=self.tokenizer.model_max_length, truncation=True,
                                                   return_tensors='pt').input_ids
            prompt_embeds = self._text_states(tokenized_prompts.to(device))
        prompt_embeds = prompt_embeds.to(device).float()
        bs_embed, seq_len, _ = prompt_embeds.shape
        prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt, 1)
        return prompt_embeds.view(bs_embed * num_images_per_prompt, seq_len, -1)


def _check_loss_options(snr_gamma, loss_fn):
    """``StableDiffusion(snr_gamma=..., loss_fn=...)``: the checked gamma.  The weighting lives in the fused MSE launch, so a
    user ``loss_fn`` together with it is refused rather than silently unweighted."""
    snr_gamma = check_snr_gamma(snr_gamma)
    if snr_gamma is not None and loss_fn is not F.mse_loss:
        raise ValueError('snr_gamma weights the fused MSE loss: it cannot be combined with a custom loss_fn')
    return snr_gamma


def _philox_step_noise(seeds, shape, device):
    """The ``sampler='torch'`` route of a stochastic schedule: step i's noise as the ``variance_noise`` keyword of
    ``scheduler.step``, the values the step kernel draws on the other routes (stream 0, draw number i)."""
    seeds_dev = ops.philox_seeds(seeds, shape[0], device)
    return lambda i: dict(variance_noise=ops.randn_philox(seeds_dev, i, 0, shape))


def _resolve_sampling_options(inference_scheduler, own_scheduler, guidance_rescale, default_rescale, timestep_spacing,
                              num_inference_steps, eta=None):
    """``generate(guidance_rescale=..., timestep_spacing=..., inference_scheduler=..., eta=...)`` on the host: (the scheduler
    of this call with its grid set, phi).  ``ValueError`` for phi or eta outside [0, 1], eta with a solver that has none, an
    unknown spacing, and an epsilon-prediction scheduler whose grid visits a timestep of zero SNR."""
    phi = check_guidance_rescale(default_rescale if guidance_rescale is None else guidance_rescale)
    if eta is not None:
        check_eta(eta)
    if timestep_spacing is not None:
        check_timestep_spacing(timestep_spacing)
    scheduler = with_timestep_spacing(resolve_inference_scheduler(inference_scheduler, own_scheduler), timestep_spacing)
    scheduler = with_eta(scheduler, eta)
    scheduler.set_timesteps(num_inference_steps)
    check_zero_snr_grid(scheduler)
    return scheduler, phi


def _check_prompt_lenths(prompt, negative_prompt):
    if prompt is None and negative_prompt is None:
        return
    batch_size = 1 if isinstance(prompt, str) else len(prompt)
    if negative_prompt:
        negative_prompt_bs = 1 if isinstance(negative_prompt, str) else len(negative_prompt)
        if negative_prompt_bs != batch_size:
            raise ValueError(f'len(prompts) and len(negative_prompts) must be the same. '
                             f'A negative prompt must be provided for each given prompt.')


def _prompt_batch(prompt, tokenized_prompts, prompt_embeds):
    """The number of prompts, in the precedence ``_prepare_text_embeddings`` reads them."""
    for p in (prompt_embeds, tokenized_prompts, prompt):
        if p is not None:
            return 1 if isinstance(p, str) else len(p)


def _check_init_image(init_image, strength, mask, height, width, num_inference_steps, batch_size):
    """The checks of ``generate(init_image=..., strength=..., mask=...)``, all on the host: (height, width, start_index).
    Without an image: (height, width, 0) as given."""
    if init_image is None:
        if mask is not None:
            raise ValueError('generate: mask needs init_image, the image whose unmasked part is kept')
        return height, width, 0
    if not isinstance(init_image, torch.Tensor) or not init_image.is_floating_point() or init_image.dim() != 4 \
            or init_image.shape[1] != 3 or init_image.shape[0] not in (1, batch_size):
        raise ValueError(f'generate: init_image must be floats in [0, 1], [{batch_size}, 3, H, W] or [1, 3, H, W]')
    H, W = init_image.shape[-2:]
    if (height is not None and height != H) or (width is not None and width != W):
        raise ValueError(f'generate: height x width {height} x {width} differ from init_image\'s {H} x {W}')
    if not 0.0 < strength <= 1.0:
        raise ValueError(f'generate: strength must lie in (0, 1], got {strength}')
    n_run = min(int(num_inference_steps * strength), num_inference_steps)
    if n_run == 0:
        raise ValueError(f'generate: strength {strength} runs no step of {num_inference_steps}')
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or not mask.is_floating_point() \
                or tuple(mask.shape) not in ((H, W), (1, 1, H, W), (batch_size, 1, H, W)):
            raise ValueError(f'generate: mask must be floats in [0, 1], [{H}, {W}], [1, 1, {H}, {W}] or '
                             f'[{batch_size}, 1, {H}, {W}], got {tuple(getattr(mask, "shape", ()))}')
        if not bool(((mask >= 0) & (mask <= 1)).all()):
            raise ValueError('generate: mask values must lie in [0, 1] (1 = repaint, 0 = keep)')
    return H, W, num_inference_steps - n_run


def _check_prompt_given(prompt, tokenized_prompts, prompt_embeds):
    if prompt is None and tokenized_prompts is None and prompt_embeds is None:
        raise ValueError('Must provide one of `prompt`, `tokenized_prompts`, or `prompt_embeds`')
