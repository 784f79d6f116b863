"""Fused AdamW over the U-Net's flat buffers (one HIP launch for 866 M parameters).

Stands where diffusion/train.py:33 instantiates ``torch.optim.AdamW`` from yamls/hydra-yamls/SD-2-base-256.yaml:55-58
(lr 1e-4, weight_decay 0.01, torch-default betas/eps).  Same update rule as torch.optim.AdamW; additionally writes
the bf16 compute shadow and refreshes the transposed (dgrad) shadow.

Opt-in, on the device: clipping by the global gradient norm (``clip_max_norm``, torch.nn.utils.clip_grad_norm_'s rule) and a
guard that skips the step when the gradient holds an inf or NaN (``guard_nonfinite``; the reference gets this from the
GradScaler of its ``amp_fp16``).  Both run the segmented sum-of-squares pass over the flat gradient and hand AdamW its
gradient multiplier and the skip flag in device memory - no host sync between backward and the update."""
from __future__ import annotations

import struct
from typing import Optional

import torch

from . import ops


class FusedAdamW(torch.optim.Optimizer):

    def __init__(self, params=None, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, unet=None, clip_max_norm: Optional[float] = None,
                 guard_nonfinite: bool = False):
        if unet is None:
            raise ValueError('FusedAdamW needs the UNetHIP that owns the flat parameter buffers (unet=...)')
        self.unet = unet
        # torch.optim bookkeeping (param_groups / state_dict) over a single flat tensor
        super().__init__([unet.master], dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.grad_scale = 1.0
        self.ema = None            # flat fp32 EMA of the weights (set by algorithms.ema.EMA)
        self.ema_smoothing = 0.0
        self.ema_update_this_step = False
        if clip_max_norm is not None and not clip_max_norm >= 0:
            raise ValueError(f'clip_max_norm must be >= 0 (0 = no clipping), got {clip_max_norm}')
        self.clip_max_norm = clip_max_norm      # None / 0: no clipping
        self.guard_nonfinite = bool(guard_nonfinite)
        self._gn = None                         # buffers of the norm pass (allocated on first use)
        self._gn_fresh = False                  # the record describes the gradient as it stands (trainer: shared pass)
        self._skipped_loaded = 0                # from a checkpoint, until the device record exists
        self.lora = None                        # adapter mode (attach_lora): the LoRAAdapters this optimizer trains
        self._lora_projected = False            # the adapter gradient has been projected from unet.grad this step

    # ---- adapter mode ----------------------------------------------------------------------------------------------------
    def attach_lora(self):
        """Train the adapters ``unet.lora`` instead of the master.  step() then runs the projection (dA, dB from the dense
        dW in ``unet.grad``), AdamW over the adapter buffers with the same hyper-parameters and grad_scale, the merge into
        the shadows and refresh_transposed(); the norm pass, clipping and the non-finite guard work on the adapter gradient.
        The master, its moments and ``unet.opt_step``'s meaning are untouched.  Not with EMA (it averages the frozen master),
        not in step_range() slices."""
        if self.unet.lora is None:
            raise ValueError('attach_lora: the U-Net carries no adapters (UNetHIP.add_lora / load_lora first)')
        if self.ema is not None:
            raise ValueError('LoRA cannot be combined with EMA: the average is over the frozen master')
        if self._gn is not None:   # the norm pass's tables describe the master's storages
            self._skipped_loaded = self.last_grad_stats()['skipped_steps']
            self._gn = None
        self.lora = self.unet.lora
        self._gn_fresh = self._lora_projected = False

    def detach_lora(self):
        if self._gn is not None:
            self._skipped_loaded = self.last_grad_stats()['skipped_steps']
            self._gn = None
        self.lora = None
        self._gn_fresh = self._lora_projected = False

    def _lora_project(self):
        if self.lora is not self.unet.lora:
            raise RuntimeError('the adapters this optimizer trains are no longer attached to the U-Net')
        if not self._lora_projected:
            ops.lora_project(self.unet.grad, self.lora)
            self._lora_projected = True

    def _lora_step(self):
        if self.ema is not None:
            raise ValueError('LoRA cannot be combined with EMA: the average is over the frozen master')
        if getattr(self, '_open', False):
            raise RuntimeError('step_range() slices are not available while adapters are trained')
        if self.device_scaled and not self._gn_fresh:
            self.compute_grad_stats()
        self._lora_project()
        self._gn_fresh = self._lora_projected = False
        g, u, l = self.param_groups[0], self.unet, self.lora
        u.opt_step += 1
        if self.device_scaled:
            ops.adamw_dev(l.params, l.grad, l.exp_avg, l.exp_avg_sq, l.shadow_scratch, g['lr'], g['betas'][0], g['betas'][1],
                          g['eps'], g['weight_decay'], u.opt_step, self._gn['stats'])
        else:
            ops.adamw(l.params, l.grad, l.exp_avg, l.exp_avg_sq, l.shadow_scratch, g['lr'], g['betas'][0], g['betas'][1],
                      g['eps'], g['weight_decay'], u.opt_step, self.grad_scale)
        ops.lora_merge(u.master, l, u.shadow)
        u.refresh_transposed()

    # ---- gradient norm / clipping / non-finite guard -------------------------------------------------------------------
    @property
    def device_scaled(self) -> bool:
        """True when step() takes its gradient multiplier from the device record (clipping or the guard is on).  The norm
        needs every gradient final before any update, so step_range() slices are not available then."""
        return bool(self.clip_max_norm) or self.guard_nonfinite

    def _gn_buffers(self):
        if self._gn is None:
            from . import ops
            u = self.unet
            if self.lora is not None:   # one segment per adapter tensor of the adapter gradient buffer
                names, tables = self.lora.sumsq_tables()
            else:
                names, offs, numels, tables = u.grad_segments()
            dev = u.grad.device
            stats = torch.zeros(ops.GRAD_STATS_WORDS, device=dev, dtype=torch.float32)
            if self._skipped_loaded:
                stats[4:5].view(torch.int32).fill_(self._skipped_loaded)
            self._gn = {'names': names, 'tables': tables, 'stats': stats,
                        'seg': torch.zeros(len(names), device=dev, dtype=torch.float32),
                        'partials': torch.zeros(ops.segment_sumsq_scratch_floats(len(tables.chunks)), device=dev,
                                                dtype=torch.float32)}
        return self._gn

    @torch.no_grad()
    def compute_grad_stats(self):
        """The norm pass over ``unet.grad`` as it stands (three launches on the current stream, no sync): per-storage sums of
        squares, and the device record {sumsq, norm, multiplier, finite} for this step's grad_scale and clip_max_norm.  The
        next step() reuses the record instead of running the pass again (the trainer's monitor and the clipper share it);
        call it only once the gradient is final."""
        gn = self._gn_buffers()
        grad = self.unet.grad
        if self.lora is not None:   # the trainable parameters' gradient: projected once per step, then measured
            self._lora_project()
            grad = self.lora.grad
        ops.segment_sumsq(grad, gn['tables'], gn['partials'], gn['seg'], gn['stats'], self.grad_scale,
                          float(self.clip_max_norm or 0.0))
        self._gn_fresh = True

    def last_grad_stats(self) -> dict:
        """The device record of the last norm pass, read back (this call syncs; nothing else here does):
        sumsq, norm (= sqrt(sumsq) * grad_scale, the norm BEFORE clipping), grad_mult, finite, skipped_steps."""
        if self._gn is None:
            return {'sumsq': 0.0, 'norm': 0.0, 'grad_mult': self.grad_scale, 'finite': True, 'skipped_steps': self._skipped_loaded}
        sumsq, norm, mult, finite, skipped = struct.unpack('<ffffi', self._gn['stats'].cpu().numpy().tobytes()[:20])
        return {'sumsq': sumsq, 'norm': norm, 'grad_mult': mult, 'finite': finite != 0.0, 'skipped_steps': skipped}

    def last_segment_norms(self) -> dict:
        """{storage name: sqrt(sumsq) * grad_scale} and 'global', from the last norm pass: one device-to-host copy."""
        gn = self._gn_buffers()
        host = torch.cat([gn['seg'], gn['stats'][:1]]).cpu().double().sqrt() * self.grad_scale
        out = {n: float(v) for n, v in zip(gn['names'], host[:-1])}
        out['global'] = float(host[-1])
        return out

    # The update can be issued in slices as gradients become final (trainer + parallel.BucketedAllReducer hand over
    # [lo, hi) ranges back-to-front during the last microbatch's backward, on the reducer's side stream), so the
    # HBM-bound optimizer pass hides under the remaining backward GEMMs instead of trailing the step.
    @torch.no_grad()
    def begin_step(self):
        """Open optimizer step number opt_step+1; nothing updated yet."""
        if self.lora is not None:
            raise RuntimeError('step_range() slices are not available while adapters are trained')
        self.unet.opt_step += 1
        self._pending_hi = self.unet.master.numel()
        self._open = True

    @torch.no_grad()
    def step_range(self, lo: int, hi: int):
        """AdamW (+ bf16 shadow, + EMA) on flat offsets [lo, hi) of the step opened by begin_step()."""
        if hi <= lo:
            return
        g = self.param_groups[0]
        u = self.unet
        ema = self.ema[lo:hi] if (self.ema is not None and self.ema_update_this_step) else None
        ops.adamw(u.master[lo:hi], u.grad[lo:hi], u.exp_avg[lo:hi], u.exp_avg_sq[lo:hi], u.shadow[lo:hi], g['lr'],
                  g['betas'][0], g['betas'][1], g['eps'], g['weight_decay'], u.opt_step, self.grad_scale,
                  ema=ema, ema_smoothing=self.ema_smoothing)
        self._pending_hi = min(self._pending_hi, lo)

    @torch.no_grad()
    def step(self, closure=None):
        """Update everything begin_step()/step_range() have not covered yet, then refresh the dgrad weight shadow.

        With clipping or the guard on: the norm pass over the whole gradient (unless compute_grad_stats() already ran on
        it), then one AdamW launch over the whole buffer that reads its multiplier from the device.  On a non-finite
        gradient that launch writes nothing: weights, moments, shadow and EMA keep their bits and the device counter
        ``skipped_steps`` goes up by one.  The host step number (``unet.opt_step``, the bias correction) advances all the
        same - the host does not know, and must not wait to know, whether the device skipped."""
        if self.lora is not None:
            return self._lora_step()
        if self.device_scaled:
            if getattr(self, '_open', False):
                raise RuntimeError('step_range() slices cannot be combined with clip_max_norm / guard_nonfinite')
            if not self._gn_fresh:
                self.compute_grad_stats()
            self._gn_fresh = False
            self.unet.opt_step += 1
            g, u = self.param_groups[0], self.unet
            ema = self.ema if (self.ema is not None and self.ema_update_this_step) else None
            ops.adamw_dev(u.master, u.grad, u.exp_avg, u.exp_avg_sq, u.shadow, g['lr'], g['betas'][0], g['betas'][1],
                          g['eps'], g['weight_decay'], u.opt_step, self._gn['stats'], ema=ema,
                          ema_smoothing=self.ema_smoothing)
            u.refresh_transposed()
            return
        self._gn_fresh = False
        if not getattr(self, '_open', False):
            self.begin_step()
        self.step_range(0, self._pending_hi)
        self._open = False
        self.unet.refresh_transposed()

    def zero_grad(self, set_to_none: bool = False):
        self.unet.grad.zero_()

    def state_dict(self):
        """CPU copies (a checkpoint must not alias live device buffers that the next step overwrites)."""
        u = self.unet
        sd = {'step': u.opt_step, 'exp_avg': u.exp_avg.detach().cpu().clone(), 'exp_avg_sq': u.exp_avg_sq.detach().cpu().clone(),
              'param_groups': [{k: v for k, v in self.param_groups[0].items() if k != 'params'}]}
        if self.ema is not None:
            sd['ema'] = self.ema.detach().cpu().clone()
            sd['ema_smoothing'] = self.ema_smoothing
        if self.device_scaled:
            sd['skipped_steps'] = self.last_grad_stats()['skipped_steps']
        if self.lora is not None:
            l = self.lora
            sd['lora'] = {'rank': l.rank, 'alpha': l.alpha, 'target_modules': list(l.target_modules),
                          'params': l.params.detach().cpu().clone(), 'exp_avg': l.exp_avg.detach().cpu().clone(),
                          'exp_avg_sq': l.exp_avg_sq.detach().cpu().clone()}
        return sd

    def load_state_dict(self, sd):
        u = self.unet
        u.opt_step = int(sd['step'])
        u.exp_avg.copy_(sd['exp_avg'])
        u.exp_avg_sq.copy_(sd['exp_avg_sq'])
        for k, v in sd['param_groups'][0].items():
            self.param_groups[0][k] = v
        if 'ema' in sd:
            self.ema = sd['ema'].to(device=u.master.device, dtype=u.master.dtype).clone()
            self.ema_smoothing = float(sd['ema_smoothing'])
        if 'skipped_steps' in sd:   # absent from checkpoints written without clipping / the guard
            self._skipped_loaded = int(sd['skipped_steps'])
            if self._gn is not None:
                self._gn['stats'][4:5].view(torch.int32).fill_(self._skipped_loaded)
        if 'lora' in sd:
            l, st = self.lora, sd['lora']
            if l is None or (l.rank, list(l.target_modules)) != (st['rank'], list(st['target_modules'])) \
                    or l.total != st['params'].numel():
                raise ValueError('the checkpoint holds adapter state: attach matching adapters (same rank and targets) and '
                                 'call attach_lora() before load_state_dict')
            l.alpha = float(st['alpha'])
            l.upload_table()
            l.params.copy_(st['params'])
            l.exp_avg.copy_(st['exp_avg'])
            l.exp_avg_sq.copy_(st['exp_avg_sq'])
            u.sync_shadows()
        elif self.lora is not None:
            raise ValueError('adapters are attached but the checkpoint holds no adapter state')
