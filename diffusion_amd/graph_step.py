"""hipGraph replay of one microbatch of the U-Net training step (whole-step entry).

One microbatch = noising + U-Net forward + fused MSE loss/gradient + U-Net backward into the flat fp32 gradient
buffer: ~1,700 kernel launches issued from Python through the C ABI.  At the reference YAML's microbatch of 16
(``device_train_microbatch_size: 16``, SD-2-base-256.yaml:87) the kernels are short and the step is bound by the host
issuing them (368 images/s against 1,390 at microbatch 256).  Every C-ABI entry point is capture-safe (no allocation,
no host synchronisation, work only on the given stream), so the whole launch sequence of a microbatch is captured ONCE
per (batch, latent height and width, dtype, weight) into a hipGraph and replayed: inputs are copied into static buffers, the
activations of the captured microbatch live in the graph's private memory pool, gradients accumulate into the same
flat buffer as in eager mode.

What stays outside the graph: the RNG draws (timesteps, noise), metric updates, the optimizer step and the bucketed
RCCL exchange (with more than one rank the LAST microbatch of a step runs eagerly so that the all-reduce of finished
gradient buckets still overlaps its backward).  A model in philox mode (train_noise.py) draws inside the captured noising
launch: its graph owns static per-sample seeds (and strata) instead of the noise buffer, and a replay copies those.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import ops


class GraphedMicrobatch:
    """Captured forward + loss + backward for one input signature."""

    def __init__(self, model, latents: torch.Tensor, cond: torch.Tensor, weight: float, n_slots: int = 0,
                 injected_t: bool = False):
        unet = model.unet
        dev = unet.device_
        self.model = model
        self.B, _, H, W = latents.shape
        self.S = (H, W)
        self.weight = float(weight)
        self.lat = torch.empty_like(latents, device=dev)
        self.cond = torch.empty_like(cond, device=dev)
        self.t = torch.zeros(self.B, device=dev, dtype=torch.int64)
        self.philox = getattr(model, 'train_noise', None) is not None and model.train_noise.philox
        self.lat.copy_(latents)
        self.cond.copy_(cond)
        self.graph = torch.cuda.CUDAGraph()
        if self.philox:
            # the draws are part of the captured launch: what varies per replay is the per-sample seeds and, stratified, the
            # samples' places among the n_slots of the global batch (n_slots itself is a launch argument, hence in the key);
            # the kernel writes the timesteps, unless they are injected (self.t then feeds it)
            self.seeds = torch.zeros(self.B, device=dev, dtype=torch.int64).view(torch.uint64)
            self.slots = torch.zeros(self.B, device=dev, dtype=torch.int32)
            self.n_slots, self.injected_t = int(n_slots), bool(injected_t)
            self._capture()
            return
        self.noise = torch.empty(latents.shape, device=dev, dtype=torch.float32)
        # placeholder noise for the warm-up and the capture, from a generator of its own: a capture must not advance the global
        # stream the eager path draws from (a run over aspect-ratio buckets captures whenever a new shape turns up, and every
        # draw after it would differ from the eager run's)
        self.noise.normal_(generator=torch.Generator(device=dev).manual_seed(0))
        self._capture()

    def _capture(self):
        unet = self.model.unet
        # warm-up on a side stream (lazy one-time work - scratch buffers, split-K workspace, hipFuncSetAttribute, the
        # transposed-weight descriptor table - must not happen inside the capture); its gradient contribution is undone
        keep = unet.grad.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._body()
        torch.cuda.current_stream().wait_stream(s)
        unet.grad.copy_(keep)
        del keep
        # buffers the captured launches point at but that live outside the graph's pool: keep them alive with the graph
        # (UNetHIP replaces its scratch when the (batch, height, width) key changes; SPLITK_WS is module state)
        self._keep = (unet._scratch, unet._ss, unet._coef, unet._delta, ops.SPLITK_WS, unet._tdesc if hasattr(unet, '_tdesc') else None)
        cb, unet._grad_ready_cb = unet._grad_ready_cb, None   # host-side hooks do not belong in a captured sequence
        try:
            with torch.cuda.graph(self.graph):
                self.pred, self.target, self.loss = self._body()
        finally:
            unet._grad_ready_cb = cb

    def _body(self):
        model = self.model
        batch = {model.image_latents_key: self.lat, model.text_latents_key: self.cond}
        if self.philox:
            batch['_sample_seeds'] = self.seeds
            if model.train_noise.stratified:
                batch['_sample_slots'], batch['_n_slots'] = self.slots, self.n_slots
            out = model.forward(batch, timesteps=self.t if self.injected_t else None)
        else:
            out = model.forward(batch, timesteps=self.t, noise=self.noise)
        loss = model.loss(out, batch, weight=self.weight)
        model.backward_from_loss()
        self.t_out = out[2]
        return out[0], out[1], loss.detach()

    def replay(self, latents, cond, timesteps, noise):
        self.lat.copy_(latents, non_blocking=True)
        self.cond.copy_(cond, non_blocking=True)
        self.t.copy_(timesteps, non_blocking=True)
        self.noise.copy_(noise, non_blocking=True)
        self.graph.replay()
        return (self.pred, self.target, self.t), self.loss

    def replay_philox(self, latents, cond, seeds, slots=None, timesteps=None):
        self.lat.copy_(latents, non_blocking=True)
        self.cond.copy_(cond, non_blocking=True)
        self.seeds.view(torch.int64).copy_(seeds.view(torch.int64), non_blocking=True)   # the bits, whatever copy_ supports
        if slots is not None:
            self.slots.copy_(slots, non_blocking=True)
        if timesteps is not None:
            self.t.copy_(timesteps, non_blocking=True)
        self.graph.replay()
        return (self.pred, self.target, self.t_out), self.loss


class GraphStepCache:
    """Per-model cache of captured microbatches, keyed by the input signature."""

    def __init__(self, model, max_graphs: int = 4):
        self.model = model
        self.max_graphs = max_graphs
        self.graphs: Dict[Tuple, GraphedMicrobatch] = {}
        self.captures = 0   # graphs captured so far (a run with more shapes than max_graphs keeps re-capturing)

    def usable(self, batch) -> bool:
        """Only latent-space models with precomputed latents are captured: a model without them (PixelDiffusion encodes
        its captions every step and has no latent keys) runs eagerly.  So does a model with ``snr_gamma`` set: its
        timestep-weighted loss launch is not part of the captured microbatch, and declining keeps the weighting.  So does a
        U-Net that carries LoRA adapters: a graph captured before they were attached would replay the skipped weight
        gradients."""
        m = self.model
        return (ops.PROFILE is None and getattr(m, 'precomputed_latents', False) and m.image_latents_key in batch
                and m.text_latents_key in batch and m.loss_fn is torch.nn.functional.mse_loss
                and getattr(m, 'snr_gamma', None) is None and getattr(getattr(m, 'unet', None), 'lora', None) is None)

    def step(self, batch, weight: float):
        """Forward + loss + backward of one microbatch by graph replay.  Returns (outputs, loss) like the eager pair
        ``model(batch)`` / ``model.loss(...)`` followed by ``model.backward_from_loss()``."""
        m = self.model
        lat, cond = batch[m.image_latents_key], batch[m.text_latents_key]
        key = (tuple(lat.shape), lat.dtype, tuple(cond.shape), cond.dtype, round(float(weight), 9), m.prediction_type)
        dev = m.unet.device_
        B = lat.shape[0]
        tn = getattr(m, 'train_noise', None)
        if tn is not None and tn.philox:
            return self._step_philox(batch, weight, key, tn)
        g = self.graphs.get(key)
        # the draws of stable_diffusion.py:177-179, from the same global generator as the eager path
        t = batch.get('_timesteps')
        if t is None:
            t = torch.randint(0, len(m.noise_scheduler), (B,), device=dev)
        noise = batch.get('_noise')
        if noise is None:
            noise = torch.randn(lat.shape, device=dev, dtype=lat.dtype if lat.is_floating_point() else torch.float32)
        return self._graph(key, lat, cond, weight).replay(lat, cond, t, noise)

    def _graph(self, key, lat, cond, weight, **kw) -> GraphedMicrobatch:
        """the captured microbatch of ``key``, captured now if there is none"""
        g = self.graphs.get(key)
        if g is None:
            if len(self.graphs) >= self.max_graphs:
                self.graphs.pop(next(iter(self.graphs)))   # the least recently replayed one
            g = self.graphs[key] = GraphedMicrobatch(self.model, lat, cond, weight, **kw)
            self.captures += 1
        else:   # a bucketed run alternates shapes: keep the ones in use, evict by last use and not by age
            self.graphs[key] = self.graphs.pop(key)
        return g

    def _step_philox(self, batch, weight, key, tn):
        """``step`` of a model in philox mode: the noising options, the number of strata and whether the timesteps are injected
        are arguments of the captured launch, so they are part of the key; seeds absent from the batch come from torch's
        generator, as in the eager ``forward``."""
        from .train_noise import check_injected, generator_seeds
        m = self.model
        lat, cond = batch[m.image_latents_key], batch[m.text_latents_key]
        dev, B = m.unet.device_, lat.shape[0]
        check_injected(tn, batch.get('_noise'))
        t = batch.get('_timesteps')
        seeds = batch.get('_sample_seeds')
        if seeds is None:
            seeds = generator_seeds(B, dev)
        slots, n_slots = None, 0
        if tn.stratified:
            slots, n_slots = batch.get('_sample_slots'), batch.get('_n_slots')
            if slots is None:
                slots, n_slots = torch.arange(B, dtype=torch.int32, device=dev), B
        key = key + (tn.key(), int(n_slots), t is not None)
        g = self._graph(key, lat, cond, weight, n_slots=int(n_slots), injected_t=t is not None)
        return g.replay_philox(lat, cond, seeds, slots, t)
