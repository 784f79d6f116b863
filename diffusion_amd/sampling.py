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
A sample may start from an image (``sample(known=...)``: image-to-image): ``ops.sampler_init`` noises the known sample to
the level of timestep ``start_index`` in one launch and only the tail of the schedule runs.  With a pixel mask
(``mask_px``: inpainting) every step is the blended launch (``ops.sampler_step_blend`` / ``ops.sampler_step_ms_blend``),
which replaces the state outside the mask by the known sample re-noised to the level of the next timestep.
With ``guidance_rescale`` = phi > 0 under guidance (Lin et al., arXiv:2305.08891) one more launch per step
(``ops.guidance_rescale``: per sample phi std(pt) / std(m) + 1 - phi) precedes the step, whose ``_rs`` form multiplies the
guided prediction by it.
A stochastic discrete-time schedule (``DDIMScheduler`` with eta > 0, the SDE form of ``DPMSolverMultistepScheduler``) is
the same loop with ONE other launch, ``ops.sampler_step_rng``: whatever the form (two-step, blended, rescaled), the step's
noise term is drawn inside the kernel from per-image Philox streams (``sample(seeds=...)``), the draw number in the step's
coefficient row, so it replays in the captured graph like any other step and an image's noise does not depend on its batch.
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


def check_guidance_rescale(phi) -> float:
    """``guidance_rescale=`` of the factory, ``generate()`` and ``LatentSampler.sample``: a number in [0, 1], else
    ``ValueError``.  Host only."""
    if isinstance(phi, bool) or not isinstance(phi, (int, float)) or not 0.0 <= float(phi) <= 1.0:
        raise ValueError(f'guidance_rescale must be a number in [0, 1], got {phi!r}')
    return float(phi)


def check_seed(seed, batch_size: int):
    """``generate(seed=...)`` on the host: None and an int pass through; a sequence (or tensor) is one seed per generated
    image, the ``num_images_per_prompt`` copies included, and comes back as a list of ``batch_size`` ints in [0, 2^64).
    ``ValueError`` otherwise, before anything touches the device."""
    if seed is None or (isinstance(seed, int) and not isinstance(seed, bool)):
        return seed
    if isinstance(seed, (str, bytes, bool, float)):
        raise ValueError(f'seed must be None, an int or a sequence of {batch_size} ints, got {seed!r}')
    return [int(v) % 2**64 for v in ops.philox_seeds(seed, batch_size).view(torch.int64).tolist()]


def image_seeds(seed, batch_size: int, stochastic: bool, generator) -> Optional[list]:
    """The per-image Philox seeds of one ``generate()`` call, or None when nothing reads them.  ``seed`` is what
    ``check_seed`` returned: a list is used as it is, whatever the sampler; with a stochastic sampler an
    int gives image b the seed ``seed + b``, and None draws one base seed from ``generator`` (the call's torch generator,
    after the initial latents: a deterministic call draws nothing more than it always did)."""
    if isinstance(seed, list):
        return list(seed)
    if not stochastic:
        return None
    if seed is None:
        seed = int(torch.randint(0, 2**62, (1,), generator=generator, device=generator.device).item())
    return [(int(seed) + b) % 2**64 for b in range(batch_size)]


def philox_latents(seeds, shape, device) -> torch.Tensor:
    """Initial noise from the images' own streams: ``ops.randn_philox`` stream 1, draw 0, so image i of a call depends on
    its seed and on nothing else in the batch."""
    return ops.randn_philox(ops.philox_seeds(seeds, shape[0], device), 0, 1, shape)


def rescale_noise_cfg(guided: torch.Tensor, cond: torch.Tensor, guidance_rescale: float) -> torch.Tensor:
    """diffusers' ``rescale_noise_cfg`` in torch ops, what the ``sampler='torch'`` loop applies: the guided prediction
    [B, C, H, W] scaled per sample back to the conditional prediction's standard deviation, blended by ``guidance_rescale``.
    0 returns ``guided`` itself."""
    if guidance_rescale == 0.0:
        return guided
    dims = list(range(1, guided.dim()))
    rescaled = guided * (cond.std(dim=dims, keepdim=True) / guided.std(dim=dims, keepdim=True))
    return guidance_rescale * rescaled + (1 - guidance_rescale) * guided


class GraphedSamplerStep:
    """One captured denoising step for one signature: forward-only walk + ``sampler_step`` over static buffers."""

    def __init__(self, unet, rows: int, B: int, HW, C: int, cfg: bool, t_dtype, ctx: torch.Tensor, kv: dict,
                 multistep: bool = False, blend: bool = False, phi: float = 0.0, rng: bool = False):
        dev = unet.device_
        H, W = HW
        self.unet, self.rows, self.HW, self.C, self.cfg, self.multistep = unet, rows, (H, W), C, cfg, multistep
        self.blend = blend
        # a stochastic schedule: the captured launch is sampler_step_rng, which reads the per-image seeds from a static
        # buffer (filled by load) and the step's draw number from the coefficient row like everything else
        self.seeds = torch.zeros(B, device=dev, dtype=torch.int64).view(torch.uint64) if rng else None
        # guidance rescale: phi is a launch argument of the captured statistics pass, so it is part of the cache key
        self.phi = phi
        self.factor = torch.ones(B, device=dev, dtype=torch.float32) if phi > 0.0 else None
        npix = B * H * W
        self.x = torch.zeros(npix, 8, device=dev, dtype=torch.float32)
        self.xt = torch.zeros(rows * H * W, 8, device=dev, dtype=torch.bfloat16)
        self.t = torch.zeros(rows, device=dev, dtype=t_dtype)
        self.coef = torch.zeros(coef_row_width(multistep, blend, rng), device=dev, dtype=torch.float32)
        # a masked sample: the known sample, its noise draw and the mask, written by sampler_init before the first replay
        self.known8 = torch.zeros(npix, 8, device=dev, dtype=torch.float32) if blend else None
        self.eps8 = torch.zeros(npix, 8, device=dev, dtype=torch.float32) if blend else None
        self.mask = torch.zeros(npix, device=dev, dtype=torch.float32) if blend else None
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
        rs = _rescale_pass(pred, self.coef, self.factor, self.phi, self.HW[0] * self.HW[1], self.C, self.multistep)
        _step_launch(pred, self.x, self.hist, self.known8, self.eps8, self.mask, self.xt, self.coef, None, self.seeds,
                     self.HW[0] * self.HW[1], C=self.C, cfg=self.cfg, copies=2 if self.cfg else 1, **rs)

    def load(self, ctx, kv, seeds=None):
        self.ctx.copy_(ctx, non_blocking=True)
        for k, v in kv.items():
            self.kv[k].copy_(v, non_blocking=True)
        if self.seeds is not None:   # as int64 bit patterns: the copy needs no uint64 kernel
            self.seeds.view(torch.int64).copy_(seeds.view(torch.int64), non_blocking=True)

    def step(self, t_row, coef_row):
        self.t.copy_(t_row, non_blocking=True)
        self.coef.copy_(coef_row, non_blocking=True)
        self.graph.replay()


def _rescale_pass(pred, coef, factor, phi, HW, C, multistep):
    """The statistics launch of guidance rescale, when there is one (``factor`` is the sampler's buffer, None without
    rescale): the keywords the step launch takes after it."""
    if factor is None:
        return {}
    ops.guidance_rescale(pred, coef, factor, phi=phi, HW=HW, C=C, g_index=5 if multistep else 3)
    return dict(factor=factor, HW=HW)


def coef_row_width(multistep: bool, blend: bool, rng: bool) -> int:
    """Floats in one step's coefficient row: 4, 8 with a history or a blend; a stochastic (``rng``) row is one vector wider
    than the widest deterministic one of its order (8 first order, 12 two-step)."""
    if rng:
        return 12 if multistep else 8
    return 8 if multistep or blend else 4


def stochastic_rows(rows, draw_slot: int, draws) -> torch.Tensor:
    """The fp32 host table of a stochastic schedule's rows: the floats through float64 -> float32 like every table, then the
    draw numbers (uint32 values) into column ``draw_slot`` as BIT PATTERNS through an int32 view, never through a float
    conversion (a float holds no integer above 2^24 exactly and the kernel bit-casts the slot back)."""
    tab = torch.tensor(rows, dtype=torch.float64).to(torch.float32)
    bits = torch.tensor([d - 2**32 if d >= 2**31 else d for d in (int(d) & 0xffffffff for d in draws)], dtype=torch.int32)
    tab.view(torch.int32)[:, draw_slot] = bits
    return tab


def _step_launch(pred, x, hist, known8, eps8, mask, xt, coef, noise, seeds=None, hw=None, **kw):
    """The step launch for this sampler state, in place: the two-step form when there is a history buffer, the blended
    form when there is a mask; ``noise`` is the first-order forms' draw (None without one), ``kw`` the keywords of the step
    wrappers (``C``, ``cfg``, ``copies`` and what ``_rescale_pass`` returned).  With ``seeds`` (a stochastic discrete-time
    schedule) it is the one launch that draws in the kernel, whatever the form; ``hw`` is then the sample's pixel count."""
    if seeds is not None:
        kw.setdefault('HW', hw)
        ops.sampler_step_rng(pred, x, coef, seeds, x, xt, hist=hist, known8=known8, eps8=eps8, mask=mask, **kw)
    elif mask is not None and hist is not None:
        ops.sampler_step_ms_blend(pred, x, hist, coef, known8, eps8, mask, x, xt, **kw)
    elif mask is not None:
        ops.sampler_step_blend(pred, x, coef, known8, eps8, mask, x, xt, noise, **kw)
    elif hist is not None:
        ops.sampler_step_ms(pred, x, hist, coef, x, xt, **kw)
    else:
        ops.sampler_step(pred, x, coef, x, xt, noise, **kw)


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
               progress_bar: bool = False, known: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
               start_index: int = 0, mask_px: Optional[torch.Tensor] = None,
               guidance_rescale: float = 0.0, seeds=None) -> torch.Tensor:
        """latents: the initial noise [B, C, H, W] (already scaled by ``init_noise_sigma``); cond / uncond: [B, L, D] text
        states.  Classifier-free guidance runs iff ``guidance_scale > 1.0`` (``uncond`` is then required).  Returns the
        denoised [B, C, H, W] fp32 (latent models: before the 1 / 0.18215 rescale).

        ``known`` (image-to-image): the clean sample [B, C, H, W] to start from (latent models: already scaled by 0.18215).
        It is noised with ``noise`` (default ``latents``, which may then be None) to the level of timestep number
        ``start_index`` and steps ``start_index .. n - 1`` run; discrete-time schedulers only.  ``mask_px`` (inpainting,
        needs ``known``): fp32 [B, f H, f W] in [0, 1] at f x f pixels per state pixel (f a power of two in 1..16; 8 for the
        latent models), 1 = repaint, 0 = keep; its f x f box mean weighs every step's blend with the re-noised known
        sample.  ``guidance_rescale`` (phi in [0, 1]): under guidance and with phi > 0 every step scales the guided
        prediction per sample by phi std(pt) / std(m) + 1 - phi; otherwise the launches are the ones without it.
        ``seeds``: B integers in [0, 2^64) (a sequence or tensor), required by a stochastic discrete-time schedule (DDIM with
        eta > 0, the SDE solver) and not read otherwise: step ``i`` adds its noise coefficient times image b's Philox draw
        number ``i`` of stream 0 (``ops.randn_philox(seeds, i, 0)``), drawn inside the step launch, on the eager and the
        graph route alike, with ``known`` / ``mask_px`` and with ``guidance_rescale``.  Every check of these raises
        ``ValueError`` before anything is launched."""
        unet, sch = self.unet, self.scheduler
        phi = check_guidance_rescale(guidance_rescale)
        if known is None:
            if mask_px is not None:
                raise ValueError('mask_px needs known: the sample whose unmasked part is kept')
            if noise is not None or start_index != 0:
                raise ValueError('noise and start_index go with known')
        else:
            if noise is None:
                noise = latents
            if noise is None or known.dim() != 4 or tuple(noise.shape) != tuple(known.shape):
                raise ValueError('known and noise (default: latents) must both be [B, C, H, W]')
            if latents is not None and tuple(latents.shape) != tuple(known.shape):
                raise ValueError(f'latents {tuple(latents.shape)} and known {tuple(known.shape)} differ in shape')
            if mask_px is not None:
                ops.mask_factor(tuple(mask_px.shape), known.shape[0], known.shape[2], known.shape[3], 'sample')
            latents = noise
        B, C, H, W = latents.shape
        unet.check_spatial(H, W)
        if C != unet.cfg.in_channels:
            raise ValueError(f'latents have {C} channels, the U-Net takes {unet.cfg.in_channels}')
        cfg = guidance_scale > 1.0
        if cfg and uncond is None:
            raise ValueError('guidance_scale > 1 needs the unconditional text states')
        rows, npix = (2 * B if cfg else B), B * H * W
        phi = phi if cfg else 0.0
        sch.set_timesteps(num_inference_steps)
        ts = sch.timesteps
        ts = ts.tolist() if isinstance(ts, torch.Tensor) else [float(t) for t in ts]
        n = len(ts)
        continuous = any(isinstance(t, float) for t in ts)
        t_dtype = torch.float32 if continuous else torch.int64
        multistep = bool(getattr(sch, 'multistep', False))
        if multistep and continuous:
            raise ValueError('a multistep scheduler is a discrete-time method')
        blend = mask_px is not None
        if known is not None:
            if continuous or not hasattr(sch, 'add_noise_coefficients'):
                raise ValueError('a sample that starts from known needs a discrete-time scheduler (add_noise_coefficients)')
            if not 0 <= int(start_index) < n:
                raise ValueError(f'start_index must lie in [0, {n}), got {start_index}')
        start = int(start_index)
        # a stochastic discrete-time schedule draws in the step kernel from per-image streams; the continuous-time
        # Euler-Maruyama path keeps its torch.randn draw below
        from .models.schedulers import is_stochastic   # here: models imports this module
        rng = not continuous and is_stochastic(sch)
        if rng:
            if seeds is None:
                raise ValueError(f'{type(sch).__name__} adds noise in its steps: sample() needs seeds, one integer per image')
            seeds = ops.philox_seeds(seeds, B)
        dev = unet.device_
        # per-call device tables, one upload each: the timestep of every step for every row, {cx, cm, cn, guidance}
        # (a two-step scheduler: {ax, am, kx, k0, k1, guidance, 0, 0}, and no noise term)
        t_tab = torch.tensor(ts, dtype=torch.float64 if continuous else torch.int64).to(t_dtype)[:, None] \
            .expand(n, rows).contiguous().to(dev)
        # a masked sample: (bA, bS) re-noises the known sample to the level of the next timestep; the last step keeps it clean
        renoise = [(sch.add_noise_coefficients(ts[i + 1]) if i + 1 < n else (1.0, 0.0)) if blend else (0.0, 0.0)
                   for i in range(n)]
        if multistep:
            # the first executed step of a schedule entered late has no history: first order
            first = [known is not None and i == start for i in range(n)]
            stochastic = False
            if rng:   # {ax, am, kx, k0, k1, guidance, bA, bS, kn, draw, 0, 0}: step i uses draw number i
                sde = [sch.step_coefficients_sde(i, first=first[i]) for i in range(n)]
                coef_rows = [list(r[:5]) + [float(guidance_scale), *renoise[i], r[5], 0.0, 0.0, 0.0] for i, r in enumerate(sde)]
            else:
                coef_rows = [list(sch.step_coefficients_ms(i, first=True) if first[i] else sch.step_coefficients_ms(i))
                             + [float(guidance_scale), *renoise[i]] for i in range(n)]
        else:
            coefs = [sch.step_coefficients(t) for t in ts]
            if rng:   # {cx, cm, cn, guidance, bA, bS, draw, 0}
                coef_rows = [[cx, cm, cn, float(guidance_scale), *renoise[i], 0.0, 0.0] for i, (cx, cm, cn) in enumerate(coefs)]
                stochastic = False
            else:
                coef_rows = [[cx, cm, cn, float(guidance_scale)] + ([*renoise[i], 0.0, 0.0] if blend else [])
                             for i, (cx, cm, cn) in enumerate(coefs)]
                stochastic = any(cn != 0.0 for _, _, cn in coefs)
        if rng:
            coef_tab = stochastic_rows(coef_rows, 9 if multistep else 6, range(n)).to(dev)
            seeds = seeds.to(dev)
        else:
            seeds = None   # a deterministic schedule reads none: the launches are the ones it always had
            coef_tab = torch.tensor(coef_rows, dtype=torch.float64).to(torch.float32).to(dev)
        # the context: cast once, projected once
        enc = torch.cat([uncond.to(dev), cond.to(dev)]) if cfg else cond.to(dev)
        ctx = unet.prepare_ctx(enc)
        kv = unet.project_context(ctx)
        copies = 2 if cfg else 1
        g = None
        # the continuous-time SDE needs a fresh torch draw per step: eager.  A discrete-time stochastic schedule draws in
        # the kernel, its draw number in the row: it replays like any other
        if graph and not stochastic and ops.PROFILE is None:
            key = (rows, H, W, C, cfg, t_dtype, ctx.shape[0] // rows, ctx.shape[1]) + (('multistep',) if multistep else ()) \
                + (('blend',) if blend else ()) + (('rescale', phi) if phi > 0.0 else ()) + (('rng',) if rng else ())
            g = self._graph_for(key, rows, B, (H, W), C, cfg, t_dtype, ctx, kv, multistep, blend, phi, rng)
            g.load(ctx, kv, seeds)
            x, xt, hist = g.x, g.xt, g.hist
            known8, eps8, mask = g.known8, g.eps8, g.mask
            x.zero_()
        else:
            x = torch.zeros(npix, 8, device=dev, dtype=torch.float32)
            xt = torch.empty(rows * H * W, 8, device=dev, dtype=torch.bfloat16)
            # the first step is first order (k1 = 0) and does not read it: no fill
            hist = torch.empty(npix, 8, device=dev, dtype=torch.float32) if multistep else None
            known8 = torch.empty(npix, 8, device=dev, dtype=torch.float32) if blend else None
            eps8 = torch.empty(npix, 8, device=dev, dtype=torch.float32) if blend else None
            mask = torch.empty(npix, device=dev, dtype=torch.float32) if blend else None
        factor = torch.empty(B, device=dev, dtype=torch.float32) if phi > 0.0 and g is None else None
        lat = latents.to(dev, torch.float32).contiguous()
        if known is None:
            # NCHW -> NHWC-8 of the initial noise (and its bf16 copies) by the step kernel itself: 0 x + 0 m + 1 z
            one = torch.tensor([0.0, 0.0, 1.0, 0.0], device=dev)
            ops.sampler_step(x, x, one, x, xt, lat, C=C, cfg=False, copies=copies)
        else:
            a0, s0 = sch.add_noise_coefficients(ts[start])
            start_coef = torch.tensor([a0, s0, 0.0, 0.0], dtype=torch.float64).to(torch.float32).to(dev)
            ops.sampler_init(known.to(dev, torch.float32).contiguous(), lat, start_coef, x, xt, known8=known8, eps8=eps8,
                             mask_px=mask_px.to(dev, torch.float32).contiguous() if blend else None, mask=mask,
                             copies=copies)
        for i in tqdm(range(start, n), disable=not progress_bar):
            if g is not None:
                g.step(t_tab[i], coef_tab[i])
                continue
            pred = unet.forward_features(xt, t_tab[i], ctx, rows, (H, W), kv=kv, record=False)
            rs = _rescale_pass(pred, coef_tab[i], factor, phi, H * W, C, multistep)
            # the Euler-Maruyama draw: global generator, after the U-Net call, the shape step() draws (randn_like(sample));
            # a masked sample is discrete time: no draw
            noise = torch.randn((B, C, H, W), device=dev) if stochastic and not blend else None
            _step_launch(pred, x, hist, known8, eps8, mask, xt if i + 1 < n else None, coef_tab[i], noise, seeds, H * W, C=C,
                         cfg=cfg, copies=copies, **rs)
        return x.view(B, H, W, 8)[..., :C].permute(0, 3, 1, 2).contiguous()
