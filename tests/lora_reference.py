"""Shared pieces of the LoRA tests (test_lora_host.py on the CPU, test_lora_*_gpu.py on the GPU): float64 restatements of
da_lora_merge and da_lora_project, raw item tables for the kernel tests, the PEFT / diffusers key naming, and an oracle
training step with adapters - ``sd[key] = W + s B @ A`` with A and B as autograd leaves, through
``oracle.unet_oracle.training_forward``.  Weights, cases, ``emulate_bf16`` and ``metrics`` come from walk_stress.py by import.

BOUNDS: what the GPU test holds every adapter gradient tensor to.  Rule (the one walk_stress.BOUNDS follow): 2 x the worst
figure of the bf16 emulation of the oracle - the reference alone under our number format - against the fp64 oracle, over the
cases and ranks of CASES x RANKS, per adapter tensor, rounded up to two digits.  The figures are recorded below (EMU_WORST);
test_lora_host.py checks the arithmetic, recomputes the emulation and holds it to the record, so the bound cannot drift from
its derivation:

  worst emulation rel-L2 of an adapter gradient tensor   EMU_WORST['tensor_rel']   bound 2 x
  worst emulation cosine                                 EMU_WORST['matrix_cos']   bound 1 - 2 x (1 - cos)
"""
import functools
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import walk_stress as ws  # noqa: E402

CASES = ('tiny-eps-b2-16x16', 'stress-v-b2-8x24')
RANKS = (4, 16)
CONV_TARGET = 'up_blocks.3.resnets.2.conv2'
TARGETS = ('to_q', 'to_k', 'to_v', 'to_out.0', CONV_TARGET)
B_GAIN = 1.0            # B ~ U(+-B_GAIN / sqrt(r)): s B A is then of the order of W itself
ADAPTER_SEED = 23

# worst figures of the bf16 emulation over CASES x RANKS (test_lora_host.py::test_bounds_are_twice_the_emulation recomputes them)
#   case               r    worst tensor rel-L2                          worst cosine
#   tiny-eps-b2-16x16  4    0.0631 (mid_block attn1.to_out.0 lora_A)     0.99806
#   tiny-eps-b2-16x16  16   0.0675 (mid_block attn1.to_k lora_A)         0.99773
#   stress-v-b2-8x24   4    0.0906 (mid_block attn1.to_k lora_A)         0.99645
#   stress-v-b2-8x24   16   0.0810 (mid_block attn1.to_out.0 lora_A)     0.99681
EMU_WORST = {'tensor_rel': 0.0906, 'matrix_cos': 0.99645}
BOUNDS = {'tensor_rel': 0.19, 'matrix_cos': 0.9929}


# ---- the two kernels in float64 ------------------------------------------------------------------------------------------
def merge_ref64(W, A, B, s):
    """v = W + s B A in float64 and the magnitude sum |W| + s sum |B||A| the fp32 error bound scales with."""
    W, A, B = (np.asarray(z, dtype=np.float64) for z in (W, A, B))
    return W + s * (B @ A), np.abs(W) + abs(s) * (np.abs(B) @ np.abs(A))


def project_ref64(dW, A, B, s):
    """(dA, dB, mag_dA, mag_dB): s B^T dW, s dW A^T and s sum |b dW| / s sum |dW a| per element."""
    dW, A, B = (np.asarray(z, dtype=np.float64) for z in (dW, A, B))
    return s * (B.T @ dW), s * (dW @ A.T), abs(s) * (np.abs(B).T @ np.abs(dW)), abs(s) * (np.abs(dW) @ np.abs(A).T)


def merge_bound(ref, mag, r):
    """|out - ref| <= 2^-8 |ref| + (r + 2) 2^-24 mag: the bf16 half-ulp, and the fp32 chain of r products plus the scale
    multiply and the add onto the master."""
    return 2.0 ** -8 * np.abs(ref) + (r + 2) * 2.0 ** -24 * mag


def project_bound(mag, n):
    """|got - ref| <= 2 (n + 2) 2^-24 s sum |b dW|, n the reduction length: an fmaf chain of n terms and the scale."""
    return 2.0 * (n + 2) * 2.0 ** -24 * mag


class RawTable:
    """What ops.lora_merge / ops.lora_project take, for hand-made items (the kernel tests): rows (w_off, a_off, b_off, N, K,
    r, scale), a device table, and adapter / gradient buffers of ``total`` floats."""

    def __init__(self, rows, total, master_extent, device):
        from diffusion_amd.lora import pack_items
        self.rows = rows
        self.items = rows
        self.total, self.master_extent = total, master_extent
        self.table = torch.frombuffer(bytearray(pack_items(rows)), dtype=torch.uint8).to(device)
        self.params = torch.zeros(total, device=device, dtype=torch.float32)
        self.grad = torch.zeros(total, device=device, dtype=torch.float32)

    def tiles(self):
        return (sum(-(-N // 32) * -(-K // 128) for _, _, _, N, K, r, _ in self.rows),
                sum(-(-r // 32) * -(-K // 128) for _, _, _, N, K, r, _ in self.rows),
                sum(-(-N // 32) for _, _, _, N, K, r, _ in self.rows))


# ---- key naming ----------------------------------------------------------------------------------------------------------
def file_shapes(module, weight_shape, r):
    """PEFT / diffusers: lora_A [r, in] and lora_B [out, r]; convolutions [r, cin, kh, kw] and [cout, r, 1, 1]."""
    if len(weight_shape) == 4:
        co, ci, kh, kw = weight_shape
        return (r, ci, kh, kw), (co, r, 1, 1)
    return (r, weight_shape[1]), (weight_shape[0], r)


def keys_of(module):
    return f'unet.{module}.lora_A.weight', f'unet.{module}.lora_B.weight'


def delta_weight(A, B, s):
    """s B A in the weight's own shape (a convolution's A is the k x k conv into r channels, B the 1 x 1 out of them)."""
    d = s * (B.reshape(B.shape[0], -1) @ A.reshape(A.shape[0], -1))
    return d.reshape(B.shape[0], *A.shape[1:])


# ---- the oracle step with adapters -----------------------------------------------------------------------------------------
def hip_config(name):
    width, ptype = ws.CASES[name][:2]
    return ws.stress_config('hip', width, ptype)


@functools.lru_cache(maxsize=None)
def layout(name, r):
    from diffusion_amd.lora import LoRAAdapters
    from diffusion_amd.models.unet import build_layout
    return LoRAAdapters(build_layout(hip_config(name))[0], r, target_modules=TARGETS, seed=ADAPTER_SEED)


@functools.lru_cache(maxsize=None)
def adapter_tensors(name, r):
    """{file key: fp64 tensor in the file's shape}: A as LoRAAdapters initialises it, B ~ U(+-B_GAIN / sqrt(r)) from a seeded
    generator in item order (B = 0 would make every dA zero and the adapter invisible)."""
    from diffusion_amd.lora import to_file_tensors
    ad = layout(name, r)
    p = ad.init_params()
    g = torch.Generator().manual_seed(ADAPTER_SEED + 1)
    out = {}
    for it in ad.items:
        b = ((torch.rand(it.N, it.r, generator=g, dtype=torch.float64) * 2 - 1) * (B_GAIN / math.sqrt(r))).float()
        a = p[it.a_off:it.a_off + it.r * it.K].view(it.r, it.K)
        out.update({k: v.double() for k, v in to_file_tensors(it, a, b).items()})
    return out


def oracle_lora_step(O, sd, cfg, inputs, ad, tensors, dtype=torch.float64):
    """One training step of the oracle with sd[key] = W + s B A.  Returns (loss, pred, adapter grads {file key: tensor},
    dense grads {diffusers weight key: dW} of the adapted matrices)."""
    latents, ctx, noise, t = inputs
    c = lambda z: z.to(dtype)
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in tensors.items()}
    params = {k: v.detach().to(dtype) for k, v in sd.items()}
    merged = {}
    for it in ad.items:
        ka, kb = keys_of(it.module)
        w = (params[it.module + '.weight'] + delta_weight(leaves[ka], leaves[kb], ad.scale))
        merged[it.module + '.weight'] = w
        w.retain_grad()
    params.update(merged)
    pred, target = O.training_forward(params, cfg, c(latents), t, c(ctx), c(noise))
    loss = F.mse_loss(pred, target)
    loss.backward()
    return (loss.detach(), pred.detach(), {k: v.grad.detach() for k, v in leaves.items()},
            {k: v.grad.detach() for k, v in merged.items()})


@functools.lru_cache(maxsize=None)
def case_data(name, r):
    """The fp64 oracle step with adapters, the emulation's figures per adapter tensor against it, and the fp64 prediction
    WITHOUT adapters.  Computed once per process; nothing may modify what it returns."""
    O = ws.oracle()
    width, ptype = ws.CASES[name][:2]
    cfg = ws.stress_config('oracle', width, ptype)
    sd = ws.state_dict64(width)
    inputs = ws.case_inputs(name)
    ad, tensors = layout(name, r), adapter_tensors(name, r)
    loss, pred, grads, dense = oracle_lora_step(O, sd, cfg, inputs, ad, tensors)
    with ws.emulate_bf16(O):
        el, ep, eg, _ = oracle_lora_step(O, sd, cfg, inputs, ad, tensors, dtype=torch.float32)
    emu = ws.metrics(ep, eg, pred, grads, el, loss)
    latents, ctx, noise, t = inputs
    with torch.no_grad():
        base_pred, _ = O.training_forward(sd, cfg, latents.double(), t, ctx.double(), noise.double())
    return types.SimpleNamespace(cfg=cfg, sd=sd, inputs=inputs, ad=ad, tensors=tensors, loss=loss, pred=pred, grads=grads,
                                 dense=dense, emu=emu, base_pred=base_pred)


def emulation_worst(cases=CASES, ranks=RANKS):
    tr = max(max(case_data(n, r).emu['tensor_rel'].values()) for n in cases for r in ranks)
    mc = min(min(case_data(n, r).emu['matrix_cos'].values()) for n in cases for r in ranks)
    return {'tensor_rel': tr, 'matrix_cos': mc}
