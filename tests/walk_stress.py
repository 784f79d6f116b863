"""Shared pieces of the U-Net walk stress tests (test_walk_stress_host.py on the CPU, test_walk_stress_gpu.py on the GPU).

The kernel suites check each launch; what checks ``UNetHIP._walk`` / ``_backward_walk`` - which affine vector, weight shadow,
saved activation, statistics pair, softmax scale, head count and concat column slice goes to which launch - is the parity of
a whole training step against ``oracle/unet_oracle.py``.  At ``init_state_dict`` weights that parity is blind to most wiring
slips: every norm has gamma = 1 and beta = 0, the attention logits have a standard deviation of about 0.3 (softmax is then
nearly a mean over V), and the asserted figures are aggregates.  This module provides

  * ``stress_config`` / ``stress_state_dict``: a width that takes the fused-GEGLU branches (C = 320) and weights under which
    every affine vector and the attention scale carry weight (gamma 1 +- 0.5, beta +- 0.3, to_q / to_k doubled: logit standard
    deviation 1.2 ... 1.9);
  * ``emulate_bf16``: the oracle under our number format (bf16 weights and layer outputs, fp32 maths) - the error the
    reference alone makes, which the bounds must leave room for;
  * ``metrics``: the aggregate figures and the rel-L2 of EVERY gradient tensor on its own;
  * ``MUTATIONS``: wiring slips applied to the fp64 oracle; the host test asserts that each one breaks ``BOUNDS``;
  * ``CASES`` / ``case_data``: the inputs of the GPU cases with their fp64 reference and emulation figures, computed once per
    process and shared by both test modules.
"""
import contextlib
import functools
import math

import torch
import torch.nn.functional as F

# ------------------------------------------------------------------------------------------------------------------------
# bounds.  Rule: each is at most 2 x the worst value measured on an MI355X over the three cases (the project's convention
# for parity bounds; profiles/walk_stress_margins.json holds the measured values next to the emulation's), and
# ``tensor_rel`` stays below the effect of every entry of MUTATIONS (asserted on the CPU by test_walk_stress_host.py).
#
#   entry        worst HIP value (case)            emulation, worst   bound     factor   weakest mutation it still catches
#   pred_rel     1.245e-2 (tiny-eps-b2-16x16)      1.10e-2            2.4e-2    1.93     two heads run as one: 0.114
#   loss_abs     2.58e-4  (stress-eps-b3-16x16)    3.6e-4             5.6e-4    2.17 *   GroupNorm fed its neighbour's affine: 1.2e-3
#   grad_rel     2.54e-2  (stress-v-b2-8x24)       2.11e-2            4e-2      1.57     self-attention scale x 1.1: 0.0465
#   tensor_rel   6.42e-2  (stress-eps-b3-16x16)    6.66e-2            0.12      1.87     self-attention scale x 1.1: 0.201
#   matrix_cos   0.99795  (stress-eps-b3-16x16)    0.99783            0.9959    2.0      cross-attention scale x 1.1: 0.9898
#
#   * the bound test_unet_parity_gpu.py already asserts (TOL_TINY: 2 x the 2.8e-4 measured there at default weights).
#     |loss - oracle| is the difference of two O(1) means at bf16 noise level, it does not depend on the weights' scale; the
#     emulation alone reaches 3.6e-4 on the 384-pixel case.
#   tensor_rel and matrix_cos each catch all seven mutations; the aggregates miss the LayerNorm beta (prediction 0.0009,
#   global gradient 0.0042) and, but for grad_rel by a factor of 1.2, the two 10 % scale slips.  A per-tensor value of the
#   HIP path far above the emulation's for the same tensor points at the layer; a uniform ratio is number-format noise (the
#   measured HIP / emulation ratio of the worst tensor is 0.93 ... 1.26 over the cases).
# ------------------------------------------------------------------------------------------------------------------------
BOUNDS = {'pred_rel': 2.4e-2, 'loss_abs': 5.6e-4, 'grad_rel': 4e-2, 'tensor_rel': 0.12, 'matrix_cos': 0.9959}

SEED = 17
WIDTHS = {
    'stress': dict(block_out_channels=(64, 128, 320, 320), attention_head_dim=(1, 2, 5, 5), cross_attention_dim=128),
    'tiny': dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4), cross_attention_dim=128),
}
STRESS_PARAMS = 49_997_380


def oracle():
    from oracle import unet_oracle as O
    return O


def stress_config(kind='oracle', width='stress', prediction_type='epsilon'):
    """The stressed width as the oracle's ``UNetConfig`` (``kind='oracle'``) or ours (``kind='hip'``).  Heads 1 / 2 / 5 / 5
    keep the levels' head counts apart, and C = 320 puts the fused GEGLU forward and backward (``ops.geglu_fusable``:
    C % 320 == 0) into down_blocks.2, mid_block and up_blocks.1.  ``width='tiny'`` is ``UNetConfig.tiny()``."""
    if kind == 'oracle':
        cls = oracle().UNetConfig
    else:
        from diffusion_amd.models.unet import UNetConfig as cls
    return cls(prediction_type=prediction_type, **WIDTHS[width])


def is_norm_key(k):
    return 'norm' in k.rsplit('.', 2)[-2]


def stress_state_dict(cfg, seed=SEED, dtype=torch.float64):
    """``init_state_dict`` with every norm weight 1 + 0.5 U(-1, 1), every norm bias 0.3 U(-1, 1) (one CPU generator, manifest
    order) and every attention to_q / to_k weight doubled.  Nothing else changes."""
    O = oracle()
    sd = O.init_state_dict(cfg, seed, dtype=torch.float64)
    g = torch.Generator().manual_seed(seed + 1_000_003)
    for k, shape in O.param_manifest(cfg):
        if is_norm_key(k):
            u = torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1
            sd[k] = 1 + 0.5 * u if k.endswith('.weight') else 0.3 * u
        elif k.endswith(('.to_q.weight', '.to_k.weight')):
            sd[k] = sd[k] * 2
    return {k: v.to(dtype) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------------------------------
# the oracle under our number format
# ------------------------------------------------------------------------------------------------------------------------
def _bf16_ste(x):
    """Round to bf16, gradient passed straight through."""
    return x + (x.detach().to(torch.bfloat16).to(x.dtype) - x.detach())


@contextlib.contextmanager
def patched(obj, **attrs):
    old = {k: getattr(obj, k) for k in attrs}
    for k, v in attrs.items():
        setattr(obj, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(obj, k, v)


@contextlib.contextmanager
def emulate_bf16(O):
    """bf16 weight shadows and bf16 layer outputs (GroupNorm, conv, linear), everything else - biases, affines, statistics,
    softmax, accumulation - as the oracle computes it; run it on fp32 inputs.  This is the reference alone under our number
    format: at ``init_state_dict`` weights it is 0.0094 / 0.017 off the fp64 oracle in prediction / global gradient rel-L2
    where the HIP path measured 0.0112 / 0.0208."""
    gn, conv, lin = O._gn, O._conv, O._lin

    def shadow(sd, p):
        return {p + '.weight': _bf16_ste(sd[p + '.weight']), p + '.bias': sd.get(p + '.bias')}

    def _gn(x, sd, p, groups, eps):
        return _bf16_ste(gn(x, sd, p, groups, eps))

    def _conv(x, sd, p, stride=1, padding=1):
        return _bf16_ste(conv(x, shadow(sd, p), p, stride=stride, padding=padding))

    def _lin(x, sd, p, bias=True):
        return _bf16_ste(lin(x, shadow(sd, p), p, bias=bias))

    with patched(O, _gn=_gn, _conv=_conv, _lin=_lin):
        yield


# ------------------------------------------------------------------------------------------------------------------------
# mutations of the oracle: what a wiring slip in the walk would compute
# ------------------------------------------------------------------------------------------------------------------------
def _attention_with(O, scale_mul_of, heads_of):
    """``O.attention`` with the softmax scale of the true head width times ``scale_mul_of(p)``, run over ``heads_of(heads)``
    heads (through ``O._lin``, so it composes with the emulation)."""

    def attention(x, ctx, sd, p, heads):
        b, n, c = x.shape
        scale = (c // heads)**-0.5 * scale_mul_of(p)
        heads = heads_of(heads)
        d = c // heads
        q, k, v = (O._lin(z, sd, f'{p}.{nm}', bias=False).reshape(b, -1, heads, d).permute(0, 2, 1, 3)
                   for z, nm in ((x, 'to_q'), (ctx, 'to_k'), (ctx, 'to_v')))
        w = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1)
        return O._lin((w @ v).permute(0, 2, 1, 3).reshape(b, n, c), sd, p + '.to_out.0')

    return attention


def _mut_scale(which):
    def make(O, params):
        return patched(O, attention=_attention_with(O, lambda p: 1.1 if p.endswith(which) else 1.0, lambda h: h))
    return make


def _mut_heads(O, params):
    return patched(O, attention=_attention_with(O, lambda p: 1.0, lambda h: 1 if h == 2 else h))


def _mut_gn(affine_of):
    """GroupNorm ``p`` takes the (gamma, beta) that ``affine_of(p, sd)`` names instead of its own."""
    def make(O, params):
        gn = O._gn

        def _gn(x, sd, p, groups, eps):
            sub = affine_of(p, sd)
            if sub is None:
                return gn(x, sd, p, groups, eps)
            w, b = sub
            return gn(x, {p + '.weight': w, p + '.bias': b}, p, groups, eps)

        return patched(O, _gn=_gn)
    return make


GN_GAMMA_ONE = 'up_blocks.3.resnets.2.norm2'
GN_SWAP = ('down_blocks.0.resnets.0.norm2', 'down_blocks.0.resnets.1.norm2')
GN_NEIGHBOUR = ('down_blocks.0.attentions.0.norm', 'down_blocks.0.resnets.1.norm1')
LN_BETA_ZERO = 'mid_block.attentions.0.transformer_blocks.0.norm3'   # C = 320 in the stressed width


def _gamma_one(p, sd):
    if p != GN_GAMMA_ONE:
        return None
    w = sd[p + '.weight']
    return w * 0 + 1, sd[p + '.bias']


def _swapped(p, sd):
    if p not in GN_SWAP:
        return None
    q = GN_SWAP[1 - GN_SWAP.index(p)]
    return sd[q + '.weight'], sd[p + '.bias']


def _neighbour(p, sd):
    if p != GN_NEIGHBOUR[0]:
        return None
    return sd[GN_NEIGHBOUR[1] + '.weight'], sd[GN_NEIGHBOUR[1] + '.bias']


def _mut_ln_beta(O, params):
    ln = F.layer_norm
    beta = params[LN_BETA_ZERO + '.bias']

    def layer_norm(x, shape, weight=None, bias=None, eps=1e-5):
        return ln(x, shape, weight, bias * 0 if bias is beta else bias, eps)

    return patched(O.F, layer_norm=layer_norm)


MUTATIONS = {
    'cross_attention_scale_x1.1': _mut_scale('.attn2'),
    'self_attention_scale_x1.1': _mut_scale('.attn1'),
    'groupnorm_gamma_taken_as_1': _mut_gn(_gamma_one),
    'layernorm_beta_taken_as_0': _mut_ln_beta,
    'groupnorm_gammas_swapped': _mut_gn(_swapped),
    'two_heads_run_as_one_of_width_128': _mut_heads,
    'transformer_groupnorm_fed_next_resnet_norm1_affine': _mut_gn(_neighbour),
}


# the gradient tensors a slip takes away from their parameter by construction (the mutated forward does not read the
# parameter, or reads it in another layer's place): left out when a mutation's effect is measured (``metrics(exclude=)``), so
# that what is asserted is the effect on tensors the slip does not name
MUTATION_OWN = {
    'groupnorm_gamma_taken_as_1': (GN_GAMMA_ONE + '.weight',),
    'layernorm_beta_taken_as_0': (LN_BETA_ZERO + '.bias',),
    'groupnorm_gammas_swapped': tuple(p + '.weight' for p in GN_SWAP),
    'transformer_groupnorm_fed_next_resnet_norm1_affine': tuple(p + k for p in GN_NEIGHBOUR for k in ('.weight', '.bias')),
}


def oracle_step(O, sd, cfg, latents, t, ctx, noise, mutation=None):
    """``O.training_loss_and_grads`` with ``MUTATIONS[mutation]`` applied for the forward.  A parameter the mutated forward
    does not read gets a zero gradient."""
    params = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    with (MUTATIONS[mutation](O, params) if mutation else contextlib.nullcontext()):
        pred, target = O.training_forward(params, cfg, latents, t, ctx, noise)
        loss = F.mse_loss(pred, target)
        grads = torch.autograd.grad(loss, list(params.values()), allow_unused=True)
    grads = [torch.zeros_like(p) if g is None else g for g, p in zip(grads, params.values())]
    return loss.detach(), pred.detach(), dict(zip(params.keys(), grads))


# ------------------------------------------------------------------------------------------------------------------------
# figures
# ------------------------------------------------------------------------------------------------------------------------
def metrics(pred, grads, pred_ref, grads_ref, loss=None, loss_ref=None, exclude=()):
    """pred_rel, loss_abs (None without the losses), grad_rel over all gradients, ``tensor_rel`` {name: rel-L2 of that
    gradient tensor on its own} for every tensor, ``matrix_cos`` {name: cosine} for every tensor of 2 or more dimensions.
    ``exclude``: gradient tensors left out of all of it (``MUTATION_OWN``; the GPU tests exclude nothing)."""
    f = lambda z: z.detach().to('cpu', torch.float64)
    pr = f(pred_ref)
    out = {'pred_rel': ((f(pred) - pr).norm() / pr.norm()).item(),
           'loss_abs': None if loss is None else abs(float(loss) - float(loss_ref)),
           'tensor_rel': {}, 'matrix_cos': {}}
    num = den = 0.0
    for k, r in grads_ref.items():
        if k in exclude:
            continue
        r, g = f(r), f(grads[k])
        n, d = ((g - r)**2).sum().item(), (r**2).sum().item()
        num, den = num + n, den + d
        out['tensor_rel'][k] = math.sqrt(n / d) if d > 0 else math.inf
        if r.dim() >= 2:
            out['matrix_cos'][k] = F.cosine_similarity(g.flatten(), r.flatten(), dim=0).item()
    out['grad_rel'] = math.sqrt(num / den)
    return out


def summary(m):
    """The scalar view of ``metrics``: worst tensor, worst matrix and worst vector by name."""
    tr, mc = m['tensor_rel'], m['matrix_cos']
    wt = max(tr, key=tr.get)
    wv = max((k for k in tr if k not in mc), key=tr.get)
    wm = max(mc, key=tr.get)
    wc = min(mc, key=mc.get)
    return {'pred_rel_l2': m['pred_rel'], 'loss_abs_delta': m['loss_abs'], 'grad_rel_l2': m['grad_rel'],
            'worst_tensor_rel_l2': tr[wt], 'worst_tensor': wt, 'worst_matrix_rel_l2': tr[wm], 'worst_matrix': wm,
            'worst_vector_rel_l2': tr[wv], 'worst_vector': wv, 'worst_matrix_cosine': mc[wc], 'worst_cosine_matrix': wc}


def violations(m, bounds=None):
    """[(entry of BOUNDS, value, bound, tensor name or None)] for every bound that ``m`` breaks, worst tensor per entry."""
    b = bounds or BOUNDS
    bad = []
    for key in ('pred_rel', 'loss_abs', 'grad_rel'):
        if m[key] is not None and not m[key] < b[key]:
            bad.append((key, m[key], b[key], None))
    k = max(m['tensor_rel'], key=m['tensor_rel'].get)
    if not m['tensor_rel'][k] < b['tensor_rel']:
        bad.append(('tensor_rel', m['tensor_rel'][k], b['tensor_rel'], k))
    k = min(m['matrix_cos'], key=m['matrix_cos'].get)
    if not m['matrix_cos'][k] >= b['matrix_cos']:
        bad.append(('matrix_cos', m['matrix_cos'][k], b['matrix_cos'], k))
    return bad


# ------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------
CASES = {
    # name: (width, prediction type, B, H, W, timesteps or None for the draw of test_tiny_train_step_parity, input seed)
    'stress-eps-b3-16x16': ('stress', 'epsilon', 3, 16, 16, (0, 999, 500), 29),
    'stress-v-b2-8x24': ('stress', 'v_prediction', 2, 8, 24, (999, 0), 31),
    'tiny-eps-b2-16x16': ('tiny', 'epsilon', 2, 16, 16, None, 17),
}
SQUARE_CASE = 'stress-eps-b3-16x16'


def case_inputs(name):
    width, ptype, B, H, W, ts, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    latents = torch.randn(B, 4, H, W, generator=g)
    ctx = torch.randn(B, 77, WIDTHS[width]['cross_attention_dim'], generator=g)
    noise = torch.randn(B, 4, H, W, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)   # drawn in every case, so that the tiny case has the parity test's inputs
    if ts is not None:
        t = torch.tensor(ts, dtype=torch.int64)
    return latents, ctx, noise, t


@functools.lru_cache(maxsize=None)
def state_dict64(width):
    return stress_state_dict(stress_config('oracle', width))


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Inputs, stressed weights (fp64), the fp64 oracle's (loss, pred, grads) and the emulation's ``metrics`` against it.
    Computed once per process; nothing may modify what it returns."""
    O = oracle()
    width, ptype = CASES[name][:2]
    cfg = stress_config('oracle', width, ptype)
    sd = state_dict64(width)
    latents, ctx, noise, t = case_inputs(name)
    d = lambda z: z.double()
    loss, pred, grads = O.training_loss_and_grads(sd, cfg, d(latents), t, d(ctx), d(noise))
    with emulate_bf16(O):
        el, ep, eg = oracle_step(O, {k: v.float() for k, v in sd.items()}, cfg, latents, t, ctx, noise)
    emu = metrics(ep, eg, pred, grads, el, loss)
    return {'cfg': cfg, 'sd': sd, 'inputs': (latents, ctx, noise, t), 'loss': loss, 'pred': pred, 'grads': grads, 'emu': emu}
