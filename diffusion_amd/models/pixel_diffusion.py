"""``PixelDiffusion`` ComposerModel on the HIP U-Net: diffusion directly in pixel space, discrete (DDPM) or continuous time.

Mirrors the reference's diffusion/models/pixel_diffusion.py: constructor (:38-68), ``forward`` (:70-96), ``loss`` (:98-99),
``eval_forward`` (:101-109), ``get_metrics`` (:111-129), ``update_metric`` (:131-135), ``generate`` (:137-241) and
``_prepare_text_embeddings`` (:243-261).  It reuses the latent model's path end to end - the same U-Net topology on 3
channels padded to 8 - and differs from ``StableDiffusion`` only at the edges:
  * the noising of :81-93 (either schedule, any of the three targets) is one fused kernel (``da_add_noise_ex``); continuous
    time keeps ``t`` in fp32 and the U-Net embeds it unrounded (``da_timestep_embed_f32``);
  * ``F.mse_loss`` (:99) is the fused loss + gradient over the 3 valid channels (``da_mse_loss_c``), and ``loss()`` returns
    a 0-d tensor whose ``.backward()`` runs the HIP backward, as in ``StableDiffusion``;
  * captions are always encoded online, by the frozen CLIP text encoder on the HIP kernels when the factory built one;
  * ``model`` is the U-Net as in the reference, and ``unet`` names the same object for the trainer, EMA and checkpoints.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from .. import ops
from ..sampling import LatentSampler, check_seed, image_seeds, philox_latents, resolve_sampler
from ..train_noise import TrainNoise, check_injected
from ..train_noise import add_noise as train_noise_add
from .composer_shim import ComposerModel, MeanSquaredError, Metric
from .schedulers import check_eta, check_inference_scheduler, is_stochastic, resolve_inference_scheduler, with_eta
from .stable_diffusion import (_HIPBackward, _check_prompt_given, _check_prompt_lenths, _philox_step_noise, _prompt_batch,
                               tqdm)
from .unet import UNetHIP

_PREDICTION_TYPES = ('sample', 'epsilon', 'v_prediction')


class PixelDiffusion(ComposerModel):

    def __init__(self,
                 model,
                 text_encoder,
                 tokenizer,
                 scheduler,
                 inference_scheduler=None,
                 continuous_time: bool = False,
                 input_key: str = 'image',
                 conditioning_key: str = 'captions',
                 prediction_type: str = 'epsilon',
                 train_metrics: Optional[List] = None,
                 val_metrics: Optional[List] = None,
                 val_seed: int = 1138,
                 train_noise: Optional[TrainNoise] = None):
        super().__init__()
        # the noising options (train_noise.TrainNoise): with noise_source='philox' forward draws per sample in the noising
        # launch; a range outside the schedule is refused here
        self.train_noise = train_noise if train_noise is not None else TrainNoise()
        if self.train_noise.timestep_range is not None:
            if continuous_time:
                self.train_noise.continuous_range(scheduler.t_max)
            else:
                self.train_noise.discrete_range(len(scheduler))
        self.model = model
        self.text_encoder = text_encoder
        self.tokenizer = tokenizer
        self.scheduler = scheduler
        self.inference_scheduler = inference_scheduler if inference_scheduler is not None else scheduler
        self.continuous_time = continuous_time
        self.input_key = input_key
        self.conditioning_key = conditioning_key
        if prediction_type not in _PREDICTION_TYPES:
            raise ValueError(f'prediction type must be one of sample, epsilon, or v_prediction. Got {prediction_type}')
        self.prediction_type = prediction_type
        self.train_metrics = train_metrics
        self.val_metrics = val_metrics
        self.val_seed = val_seed
        self.text_hip = None   # the HIP-kernel walk of the frozen text encoder (set by the factories)
        self.text_encoder.requires_grad_(False)
        self._pending = None
        self._dpred = None

    @property
    def unet(self) -> UNetHIP:
        """The U-Net under the name the trainer, EMA and checkpointing use (``StableDiffusion.unet``)."""
        return self.model

    def unet_input_side(self, batch):
        """``(H, W)`` of the U-Net input for the trainer's microbatch sizing: pixels go in as they are (no VAE, no /8)."""
        return int(batch[self.input_key].shape[-2]), int(batch[self.input_key].shape[-1])

    # ------------------------------------------------------------------------------------------
    def _text_states(self, input_ids):
        """``text_encoder(ids)[0]`` (reference :75)."""
        enc = self.text_hip if self.text_hip is not None else self.text_encoder
        with torch.no_grad():
            return enc(input_ids.to(self.model.device_))[0]

    def forward(self, batch, generator=None, timesteps: Optional[torch.Tensor] = None,
                noise: Optional[torch.Tensor] = None):
        """Returns ``(model_out, targets, timesteps)`` like the reference (:96).  ``t`` is ``t_max * rand`` (continuous) or
        ``randint(0, len(scheduler))`` (discrete) from ``generator``; the noise from torch's global generator (:76-82).
        ``timesteps`` / ``noise`` may be injected (as arguments or as ``batch['_timesteps']`` / ``batch['_noise']``).
        With ``train_noise.noise_source == 'philox'`` the noising launch draws both per sample from
        ``batch['_sample_seeds']`` (else from seeds drawn with ``generator``), as in ``StableDiffusion.forward``."""
        if timesteps is None:
            timesteps = batch.get('_timesteps')
        if noise is None:
            noise = batch.get('_noise')
        check_injected(self.train_noise, noise)
        unet: UNetHIP = self.model
        dev = unet.device_
        inputs = batch[self.input_key].to(dev)
        conditioning = self._text_states(batch[self.conditioning_key])
        B, C, H, W = inputs.shape
        unet.check_spatial(H, W)
        if self.train_noise.philox:   # one launch draws and noises, per sample (StableDiffusion.forward has the details)
            sched = dict(t_max=self.scheduler.t_max) if self.continuous_time else dict(tables=self.scheduler.device_tables(dev))
            xt, target8, t = train_noise_add(self.train_noise, batch, inputs.float().contiguous(), timesteps,
                                             self.prediction_type, generator=generator, **sched)
            pred8 = unet.forward_features(xt, t, unet.prepare_ctx(conditioning), B, (H, W))
            self._pending = (pred8, target8, B * H * W, C)
            return (pred8.view(B, H, W, 8)[..., :C].permute(0, 3, 1, 2),
                    target8.view(B, H, W, 8)[..., :C].permute(0, 3, 1, 2), t)
        if timesteps is None:
            if self.continuous_time:
                timesteps = self.scheduler.t_max * torch.rand(B, device=dev, generator=generator)
            else:
                timesteps = torch.randint(0, len(self.scheduler), (B,), device=dev, generator=generator)
        if noise is None:
            noise = torch.randn_like(inputs)
        x0 = inputs.float().contiguous()
        eps = noise.to(dev).float().contiguous()
        t = timesteps.to(dev, torch.float32 if self.continuous_time else torch.int64).contiguous()
        xt = torch.empty(B * H * W, 8, device=dev, dtype=torch.bfloat16)
        target8 = torch.empty(B * H * W, 8, device=dev, dtype=torch.float32)
        if self.continuous_time:
            ops.add_noise_ex(x0, eps, t, xt, target8, self.prediction_type)
        else:
            sa, sb = self.scheduler.device_tables(dev)
            ops.add_noise_ex(x0, eps, t, xt, target8, self.prediction_type, sa, sb)
        ctx = unet.prepare_ctx(conditioning)
        pred8 = unet.forward_features(xt, t, ctx, B, (H, W))
        pred = pred8.view(B, H, W, 8)[..., :C].permute(0, 3, 1, 2)
        target = target8.view(B, H, W, 8)[..., :C].permute(0, 3, 1, 2)
        self._pending = (pred8, target8, B * H * W, C)
        return pred, target, timesteps

    def loss(self, outputs, batch, weight: float = 1.0):
        """MSE between the U-Net output and the target (reference :98-99) - fused loss + gradient kernel.  ``weight``
        pre-scales the gradient (microbatch fraction) when the trainer calls backward directly."""
        if self._pending is None:
            raise RuntimeError('loss() must follow forward()')
        pred8, target8, npix, C = self._pending
        dpred = torch.empty(npix, 8, device=pred8.device, dtype=torch.bfloat16)
        lossbuf = torch.zeros(1, device=pred8.device, dtype=torch.float32)
        ops.mse_loss_c(pred8, target8, dpred, lossbuf, self.model._scratch, npix, C, 2.0 * weight / (C * npix), 1.0, 0)
        self._dpred = dpred
        anchor = torch.zeros((), device=pred8.device, requires_grad=True)
        return _HIPBackward.apply(anchor, lossbuf[0], self)

    def _run_backward(self, g: Optional[torch.Tensor] = None):
        dpred, self._dpred = self._dpred, None
        if dpred is None:
            raise RuntimeError('backward already consumed')
        if g is not None:
            dpred = (dpred.float() * g).to(torch.bfloat16)  # boundary scaling for external trainers
        self.model.backward_features(dpred)
        self._pending = None

    def backward_from_loss(self):
        """Direct (no autograd) backward for the in-tree trainer; the gradient weight was given to ``loss()``."""
        self._run_backward(None)

    # ------------------------------------------------------------------------------------------
    def eval_forward(self, batch, outputs=None):
        """Seeded timesteps (``val_seed``), noise from the global generator (reference :101-109)."""
        if outputs is not None:
            return outputs
        generator = torch.Generator(device=self.model.device_).manual_seed(self.val_seed)
        with torch.no_grad():
            out = self.forward(batch, generator=generator)
        self._pending = None
        self.model._tape = None
        return out

    def get_metrics(self, is_train: bool = False):
        metrics = self.train_metrics if is_train else self.val_metrics
        if isinstance(metrics, Metric):
            return {metrics.__class__.__name__: metrics}
        if isinstance(metrics, list):
            return {m.__class__.__name__: m for m in metrics}
        if isinstance(metrics, dict):
            out = {}
            for name, metric in metrics.items():
                assert isinstance(metric, Metric)
                out[name] = metric
            return out
        raise NotImplementedError(f'Metrics type {metrics.__class__.__name__} not supported.')

    def update_metric(self, batch, outputs, metric):
        if isinstance(metric, MeanSquaredError):
            metric.update(outputs[0], outputs[1])
        else:
            raise NotImplementedError(f'Metric {metric.__class__.__name__} not implemented.')

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate(self, prompt: Optional[list] = None, negative_prompt: Optional[list] = None,
                 tokenized_prompts: Optional[torch.LongTensor] = None,
                 tokenized_negative_prompts: Optional[torch.LongTensor] = None,
                 prompt_embeds: Optional[torch.FloatTensor] = None,
                 negative_prompt_embeds: Optional[torch.FloatTensor] = None, height: int = 64, width: int = 64,
                 num_inference_steps: Optional[int] = 50, guidance_scale: Optional[float] = 3.0,
                 num_images_per_prompt: Optional[int] = 1, seed: Optional[int] = None,
                 progress_bar: Optional[bool] = True, sampler: Optional[str] = None, inference_scheduler=None,
                 eta: Optional[float] = None):
        """Reverse diffusion from noise with classifier-free guidance on the HIP U-Net forward (reference :137-241).
        Returns images in [0, 1], (batch * num_images_per_prompt, 3, h, w).

        ``sampler``: ``'hip'`` (``sampling.LatentSampler``: forward-only walk, context K/V projected once, one fused
        guidance + scheduler-step launch per step), ``'graph'`` (the same, one hipGraph replay per step; the SDE runs
        eagerly) or ``'torch'`` (the reference's loop, the scheduler step in torch ops); default ``DA_SAMPLER``, else
        ``'hip'``.

        ``inference_scheduler``: the solver of this call only: ``'ddim'``, ``'dpm++2m'`` (``DPMSolverMultistepScheduler``
        on the model's noise tables) or a scheduler object; default the model's own.  Discrete-time models only: a
        continuous-time model raises ``ValueError`` for a name or a multistep scheduler.

        Stochastic discrete-time sampling: ``eta`` in [0, 1] is the DDIM sampler's eta for this call (default the
        scheduler's own; ``ValueError`` with any other scheduler, the continuous-time one included) and
        ``inference_scheduler='dpm++2m-sde'`` the SDE form of the two-step solver.  Their step noise comes from per-image
        Philox streams (``ops.randn_philox``), the same values on every ``sampler=`` route.  ``seed`` may be a sequence of
        one integer in [0, 2^64) per generated image: the initial noise then comes from the image's own stream too and
        image i depends on nothing else in the batch.  With an int ``seed`` the initial noise stays on the torch generator
        and image b's step noise has seed ``seed + b``; with None one base seed is drawn from the torch generator.  The
        continuous-time Euler-Maruyama sampler keeps its ``torch.randn`` draws."""
        sampler = resolve_sampler(sampler)
        check_inference_scheduler(inference_scheduler)   # before `self` is read
        if eta is not None:
            check_eta(eta)
        scheduler = resolve_inference_scheduler(inference_scheduler, self.inference_scheduler, self.continuous_time)
        scheduler = with_eta(scheduler, eta)
        _check_prompt_given(prompt, tokenized_prompts, prompt_embeds)
        seed = check_seed(seed, _prompt_batch(prompt, tokenized_prompts, prompt_embeds) * num_images_per_prompt)
        stochastic = not self.continuous_time and is_stochastic(scheduler)
        device = self.model.device_
        rng_generator = torch.Generator(device=device)
        if isinstance(seed, list):
            rng_generator = rng_generator.manual_seed(seed[0] % 2**63)
        elif seed:
            rng_generator = rng_generator.manual_seed(seed)
        self.model.check_spatial(int(height), int(width))   # pixels go in as they are: multiples of 2 ** (levels - 1)
        do_cfg = guidance_scale > 1.0
        text_embeddings = self._prepare_text_embeddings(prompt, tokenized_prompts, prompt_embeds, num_images_per_prompt)
        batch_size = len(text_embeddings)
        if do_cfg:
            _check_prompt_lenths(prompt, negative_prompt)
            if not negative_prompt and tokenized_negative_prompts is None and negative_prompt_embeds is None:
                negative_prompt = [''] * (batch_size // num_images_per_prompt)
            uncond = self._prepare_text_embeddings(negative_prompt, tokenized_negative_prompts, negative_prompt_embeds,
                                                   num_images_per_prompt)
            if sampler == 'torch':
                text_embeddings = torch.cat([uncond, text_embeddings])
        shape = (batch_size, self.model.config.in_channels, height, width)
        if isinstance(seed, list):   # per-image seeds: the initial noise from the image's own stream
            images = philox_latents(seed, shape, device)
        else:
            images = torch.randn(shape, device=device, generator=rng_generator)
        seeds = image_seeds(seed, batch_size, stochastic, rng_generator)
        scheduler.set_timesteps(num_inference_steps)
        images = images * scheduler.init_noise_sigma
        if sampler != 'torch':
            images = LatentSampler(self.model, scheduler).sample(
                images, text_embeddings, uncond if do_cfg else None, num_inference_steps=num_inference_steps,
                guidance_scale=guidance_scale, graph=sampler == 'graph', progress_bar=progress_bar,
                **(dict(seeds=seeds) if stochastic else {}))
        else:   # the reference's loop, the scheduler step in torch ops
            step_noise = _philox_step_noise(seeds, images.shape, device) if stochastic else (lambda i: {})
            for i, t in enumerate(tqdm(scheduler.timesteps, disable=not progress_bar)):
                model_input = torch.cat([images] * 2) if do_cfg else images
                model_input = scheduler.scale_model_input(model_input, t)
                model_output = self.model(model_input, t, encoder_hidden_states=text_embeddings).sample
                if do_cfg:   # only technically correct for epsilon prediction (reference :226)
                    pred_uncond, pred_text = model_output.chunk(2)
                    model_output = pred_uncond + guidance_scale * (pred_text - pred_uncond)
                images = scheduler.step(model_output, t, images, generator=rng_generator, **step_noise(i))['prev_sample']
        images = (images / 2 + 0.5).clamp(0, 1)
        return images.detach().float()

    def _prepare_text_embeddings(self, prompt, tokenized_prompts, prompt_embeds, num_images_per_prompt):
        """Tokenize and embed the prompts if needed, then repeat the embeddings per generated image (reference :243-261)."""
        device = self.model.device_
        if prompt_embeds is None:
            if tokenized_prompts is None:
                tokenized_prompts = self.tokenizer(prompt, padding='max_length',
                                                   max_length=self.tokenizer.model_max_length, truncation=True,
                                                   return_tensors='pt').input_ids
            prompt_embeds = self._text_states(tokenized_prompts)
        prompt_embeds = prompt_embeds.to(device).float()
        bs_embed, seq_len, _ = prompt_embeds.shape
        prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt, 1)
        return prompt_embeds.view(bs_embed * num_images_per_prompt, seq_len, -1)
