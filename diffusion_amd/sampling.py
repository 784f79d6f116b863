"""Sampling on the HIP path: what ``generate()`` runs between drawing the initial noise and decoding the result.

``generate()`` used to call the diffusers-style ``UNetHIP.forward`` per step: the training forward with its whole backward
tape alive until the call returned, the 16 cross-attention K/V projections of a context that is the same at every step,
and some twenty torch launches of glue (``cat``, ``to_nhwc8``, ``chunk``, the guidance arithmetic, the eight-op scheduler
``step``, the NHWC -> NCHW view).  ``LatentSampler`` keeps the state in the U-Net's own layout (NHWC-8 fp32) and does per
step
  * the forward-only walk (``UNetHIP.forward_features(kv=..., record=False)``) on the context K/V projected once, and
  * ONE launch (``ops.sampler_step``) for guidance + the scheduler update + the next bf16 U-Net input, with the step's
    coefficients (``scheduler.step_coefficients``, float64 on the host, one table per call) read from device memory.
A two-step scheduler (``scheduler.multistep``: ``DPMSolverMultistepScheduler``) is the same design one operand wider: the
launch is ``ops.sampler_step_ms``, its rows are the eight floats of ``step_coefficients_ms`` and it carries the previous
step's data prediction in a history buffer of the state's shape.
Nothing in the loop reads the device back.  ``graph=True`` replays one captured step (walk + ``sampler_step``) per
denoising step, as ``graph_step.GraphedMicrobatch`` does for a training microbatch; the host then issues two 16-byte-class
copies (the step's timestep and coefficient rows) and a replay.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional

import torch

from . import ops

try:
    from tqdm.auto import tqdm
except Exception:  # noqa: BLE001
    tqdm = lambda x, **kw: x  # noqa: E731

SAMPLERS = ('hip', 'graph', 'torch')


def resolve_sampler(sampler: Optional[str]) -> str:
    """``generate(sampler=...)``: the argument, else ``DA_SAMPLER``, else ``'hip'``.  Raises before anything touches the device."""
    import os
    name = sampler if sampler is not None else (os.environ.get('DA_SAMPLER') or 'hip')
    if name not in SAMPLERS:
        raise ValueError(f'sampler must be one of {SAMPLERS}, got {name!r}')
    return name


class GraphedSamplerStep:
    """One captured denoising step for one signature: forward-only walk + ``sampler_step`` over static buffers."""

    def __init__(self, unet, rows: int, B: int, HW, C: int, cfg: bool, t_dtype, ctx: torch.Tensor, kv: dict,
                 multistep: bool = False):
        dev = unet.device_
        H, W = HW
        self.unet, self.rows, self.HW, self.C, self.cfg, self.multistep = unet, rows, (H, W), C, cfg, multistep
        npix = B * H * W
        self.x = torch.zeros(npix, 8, device=dev, dtype=torch.float32)
        self.xt = torch.zeros(rows * H * W, 8, device=dev, dtype=torch.bfloat16)
        self.t = torch.zeros(rows, device=dev, dtype=t_dtype)
        self.coef = torch.zeros(8 if multistep else 4, device=dev, dtype=torch.float32)
        # the previous step's data prediction; k1 arrives through `coef`, so the one capture serves both orders
        self.hist = torch.zeros(npix, 8, device=dev, dtype=torch.float32) if multistep else None
        self.ctx = ctx.clone()
        self.kv = {k: v.clone() for k, v in kv.items()}
        self.graph = torch.cuda.CUDAGraph()
        # warm-up on a side stream: lazy one-time work (scratch buffers, split-K workspace, hipFuncSetAttribute) must not
        # happen inside the capture; x / xt are rewritten by load() before every use
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._body()
        torch.cuda.current_stream().wait_stream(s)
        # buffers the captured launches point at but that live outside the graph's pool: keep them alive with the graph
        self._keep = (unet._scratch, unet._ss, unet._coef, unet._delta, ops.SPLITK_WS)
        with torch.cuda.graph(self.graph):   # one stream, no branches
            self._body()

    def _body(self):
        pred = self.unet.forward_features(self.xt, self.t, self.ctx, self.rows, self.HW, kv=self.kv, record=False)
        if self.multistep:
            ops.sampler_step_ms(pred, self.x, self.hist, self.coef, self.x, self.xt, C=self.C, cfg=self.cfg,
                                copies=2 if self.cfg else 1)
            return
        ops.sampler_step(pred, self.x, self.coef, self.x, self.xt, None, C=self.C, cfg=self.cfg,
                         copies=2 if self.cfg else 1)

    def load(self, ctx, kv):
        self.ctx.copy_(ctx, non_blocking=True)
        for k, v in kv.items():
            self.kv[k].copy_(v, non_blocking=True)

    def step(self, t_row, coef_row):
        self.t.copy_(t_row, non_blocking=True)
        self.coef.copy_(coef_row, non_blocking=True)
        self.graph.replay()


class LatentSampler:
    """The denoising loop of ``generate()`` on ``unet`` (a ``UNetHIP``) with ``scheduler`` (``DDIMScheduler`` or
    ``ContinuousTimeScheduler``: anything with ``set_timesteps``, ``timesteps`` and ``step_coefficients``; or a two-step
    one, ``DPMSolverMultistepScheduler``: ``multistep`` set and ``step_coefficients_ms`` in place of ``step_coefficients``)."""

    MAX_GRAPHS = 4

    def __init__(self, unet, scheduler):
        self.unet = unet
        self.scheduler = scheduler
        # captured steps live with the U-Net (its weights are what they point at), whoever builds the sampler
        if getattr(unet, '_sampler_graphs', None) is None:
            unet._sampler_graphs = OrderedDict()
        self.graphs = unet._sampler_graphs

    def _graph_for(self, key, *args):
        g = self.graphs.get(key)
        if g is None:
            if len(self.graphs) >= self.MAX_GRAPHS:
                self.graphs.popitem(last=False)
            g = self.graphs[key] = GraphedSamplerStep(self.unet, *args)
        return g

    @torch.no_grad()
    def sample(self, latents: torch.Tensor, cond: torch.Tensor, uncond: Optional[torch.Tensor] = None, *,
               num_inference_steps: int, guidance_scale: float, graph: bool = False,
               progress_bar: bool = False) -> torch.Tensor:
        """latents: the initial noise [B, C, H, W] (already scaled by ``init_noise_sigma``); cond / uncond: [B, L, D] text
        states.  Classifier-free guidance runs iff ``guidance_scale > 1.0`` (``uncond`` is then required).  Returns the
        denoised [B, C, H, W] fp32 (latent models: before the 1 / 0.18215 rescale)."""
        unet, sch = self.unet, self.scheduler
        dev = unet.device_
        B, C, H, W = latents.shape
        unet.check_spatial(H, W)
        if C != unet.cfg.in_channels:
            raise ValueError(f'latents have {C} channels, the U-Net takes {unet.cfg.in_channels}')
        cfg = guidance_scale > 1.0
        if cfg and uncond is None:
            raise ValueError('guidance_scale > 1 needs the unconditional text states')
        rows, npix = (2 * B if cfg else B), B * H * W
        sch.set_timesteps(num_inference_steps)
        ts = sch.timesteps
        ts = ts.tolist() if isinstance(ts, torch.Tensor) else [float(t) for t in ts]
        n = len(ts)
        continuous = any(isinstance(t, float) for t in ts)
        t_dtype = torch.float32 if continuous else torch.int64
        multistep = bool(getattr(sch, 'multistep', False))
        if multistep and continuous:
            raise ValueError('a multistep scheduler is a discrete-time method')
        # per-call device tables, one upload each: the timestep of every step for every row, {cx, cm, cn, guidance}
        # (a two-step scheduler: {ax, am, kx, k0, k1, guidance, 0, 0}, and no noise term)
        t_tab = torch.tensor(ts, dtype=torch.float64 if continuous else torch.int64).to(t_dtype)[:, None] \
            .expand(n, rows).contiguous().to(dev)
        if multistep:
            coef_rows = [list(sch.step_coefficients_ms(i)) + [float(guidance_scale), 0.0, 0.0] for i in range(n)]
            stochastic = False
        else:
            coefs = [sch.step_coefficients(t) for t in ts]
            coef_rows = [[cx, cm, cn, float(guidance_scale)] for cx, cm, cn in coefs]
            stochastic = any(cn != 0.0 for _, _, cn in coefs)
        coef_tab = torch.tensor(coef_rows, dtype=torch.float64).to(torch.float32).to(dev)
        # the context: cast once, projected once
        enc = torch.cat([uncond.to(dev), cond.to(dev)]) if cfg else cond.to(dev)
        ctx = unet.prepare_ctx(enc)
        kv = unet.project_context(ctx)
        copies = 2 if cfg else 1
        g = None
        if graph and not stochastic and ops.PROFILE is None:   # the SDE needs a fresh draw per step: eager
            key = (rows, H, W, C, cfg, t_dtype, ctx.shape[0] // rows, ctx.shape[1]) + (('multistep',) if multistep else ())
            g = self._graph_for(key, rows, B, (H, W), C, cfg, t_dtype, ctx, kv, multistep)
            g.load(ctx, kv)
            x, xt, hist = g.x, g.xt, g.hist
            x.zero_()
        else:
            x = torch.zeros(npix, 8, device=dev, dtype=torch.float32)
            xt = torch.empty(rows * H * W, 8, device=dev, dtype=torch.bfloat16)
            # the first step is first order (k1 = 0) and does not read it: no fill
            hist = torch.empty(npix, 8, device=dev, dtype=torch.float32) if multistep else None
        # NCHW -> NHWC-8 of the initial noise (and its bf16 copies) by the step kernel itself: 0 x + 0 m + 1 z
        lat = latents.to(dev, torch.float32).contiguous()
        one = torch.tensor([0.0, 0.0, 1.0, 0.0], device=dev)
        ops.sampler_step(x, x, one, x, xt, lat, C=C, cfg=False, copies=copies)
        for i in tqdm(range(n), disable=not progress_bar):
            if g is not None:
                g.step(t_tab[i], coef_tab[i])
                continue
            pred = unet.forward_features(xt, t_tab[i], ctx, rows, (H, W), kv=kv, record=False)
            if multistep:
                ops.sampler_step_ms(pred, x, hist, coef_tab[i], x, xt if i + 1 < n else None, C=C, cfg=cfg, copies=copies)
                continue
            # the Euler-Maruyama draw: global generator, after the U-Net call, the shape step() draws (randn_like(sample))
            noise = torch.randn((B, C, H, W), device=dev) if stochastic else None
            ops.sampler_step(pred, x, coef_tab[i], x, xt if i + 1 < n else None, noise, C=C, cfg=cfg, copies=copies)
        return x.view(B, H, W, 8)[..., :C].permute(0, 3, 1, 2).contiguous()
