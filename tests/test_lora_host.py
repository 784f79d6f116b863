"""LoRA on the CPU: the host layout (target resolution, refusals, item table), the safetensors format, the identity the design
rests on, and the derivation of the bounds the GPU tests assert (tests/lora_reference.py)."""
import json
import math
import os
import struct
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import lora_reference as lr  # noqa: E402
import walk_stress as ws  # noqa: E402

from diffusion_amd import lora as L  # noqa: E402
from diffusion_amd.models.unet import UNetConfig, build_layout  # noqa: E402

COMBOS = [(n, r) for n in lr.CASES for r in lr.RANKS]


def _fp(cfg=None):
    return build_layout(cfg or UNetConfig.tiny())[0]


def test_default_targets_resolve_to_row_ranges_of_the_fused_storages():
    fp = _fp()
    ad = L.LoRAAdapters(fp, 4)
    assert ad.target_modules == ('to_q', 'to_k', 'to_v', 'to_out.0') and ad.alpha == 4.0 and ad.scale == 1.0
    by = {it.module: it for it in ad.items}
    n_tb = sum(1 for s in fp.storages if s.endswith('attn1.qkv.weight'))
    assert len(ad.items) == 8 * n_tb      # q, k, v, out of attn1 and attn2 in every transformer block
    tb = 'down_blocks.1.attentions.0.transformer_blocks.0'
    qkv, kv = fp.storages[tb + '.attn1.qkv.weight'], fp.storages[tb + '.attn2.kv.weight']
    c, ctx = 128, 128
    for i, nm in enumerate(('to_q', 'to_k', 'to_v')):
        it = by[f'{tb}.attn1.{nm}']
        assert (it.storage, it.row0, it.N, it.K, it.w_off) == (tb + '.attn1.qkv.weight', i * c, c, c, qkv.off + i * c * c)
    for i, nm in enumerate(('to_k', 'to_v')):
        it = by[f'{tb}.attn2.{nm}']
        assert (it.storage, it.row0, it.N, it.K, it.w_off) == (tb + '.attn2.kv.weight', i * c, c, ctx, kv.off + i * c * ctx)
    it = by[tb + '.attn2.to_q']
    assert (it.row0, it.N, it.K, it.w_off) == (0, c, c, fp.storages[tb + '.attn2.to_q.weight'].off)
    # manifest order, 64-float alignment, disjoint tensors, every item inside its storage
    end = 0
    for it in ad.items:
        st = fp.storages[it.storage]
        assert it.a_off % 64 == 0 and it.b_off % 64 == 0 and it.a_off >= end and it.b_off >= it.a_off + it.r * it.K
        end = it.b_off + it.N * it.r
        assert st.off <= it.w_off and it.w_off + it.N * it.K <= st.off + st.numel and it.K == st.ntc[1] * st.ntc[2]
    assert ad.total >= end and ad.total % 64 == 0
    assert [it.w_off for it in ad.items] == sorted(it.w_off for it in ad.items)
    assert ad.storages == sorted({it.storage for it in ad.items}) and len(ad.storages) == 5 * n_tb


def test_conv_and_linear_targets_and_the_item_table():
    fp = _fp()
    ad = L.LoRAAdapters(fp, 3, alpha=6, target_modules=['mid_block.resnets.0.conv1', 'conv_shortcut', 'ff.net.2', 'proj_in'])
    by = {it.module: it for it in ad.items}
    it = by['mid_block.resnets.0.conv1']
    assert (it.T, it.C, it.K, it.N) == (9, 256, 9 * 256, 256)
    sc = [it for it in ad.items if it.module.endswith('conv_shortcut')]
    assert sc and all(it.T == 1 for it in sc)
    assert ad.scale == 2.0
    raw = ad.pack()
    size = struct.calcsize(L.ITEM_FORMAT)
    assert size == 56 and len(raw) == size * len(ad.items)
    fm = fa = fb = 0
    for i, it in enumerate(ad.items):
        w, a, b, N, K, r, s, m0, a0, b0, _ = struct.unpack_from(L.ITEM_FORMAT, raw, i * size)
        assert (w, a, b, N, K, r, s) == (it.w_off, it.a_off, it.b_off, it.N, it.K, 3, 2.0) and (m0, a0, b0) == (fm, fa, fb)
        fm += -(-N // 32) * -(-K // 128)
        fa += -(-r // 32) * -(-K // 128)
        fb += -(-N // 32)
    assert ad.tiles() == (fm, fa, fb)
    ad.scale_mult = 0.5
    assert struct.unpack_from(L.ITEM_FORMAT, ad.pack(), 0)[6] == 1.0
    names, offs, numels = ad.segments()
    assert len(names) == 2 * len(ad.items) and offs == sorted(offs) and names[0].endswith('.lora_A.weight')
    # full width: every offset stays exact past 2^31 bytes
    big = L.LoRAAdapters(build_layout(UNetConfig.sd2_base())[0], 16)
    assert max(it.w_off for it in big.items) * 4 > 2 ** 31 and len(big.items) == 128


@pytest.mark.parametrize('targets', [['conv_in'], ['conv_out'], ['time_emb_proj'], ['down_blocks.0.resnets.0.time_emb_proj'],
                                     ['to_qq'], ['norm1'], ['to_q', 'nothing.like.this']])
def test_refused_targets(targets):
    with pytest.raises(ValueError):
        L.LoRAAdapters(_fp(), 4, target_modules=targets)


@pytest.mark.parametrize('rank', [0, -1, 129, 2.5, True])
def test_refused_ranks(rank):
    with pytest.raises(ValueError):
        L.LoRAAdapters(_fp(), rank)
    from diffusion_amd.algorithms.lora import LoRA
    with pytest.raises(ValueError):
        LoRA(rank=rank)


def test_init_is_pefts():
    ad = L.LoRAAdapters(_fp(), 16, seed=5)
    p, q = ad.init_params(), L.LoRAAdapters(_fp(), 16, seed=5).init_params()
    assert torch.equal(p, q) and not torch.equal(p, L.LoRAAdapters(_fp(), 16, seed=6).init_params())
    for it in ad.items[:12]:
        a = p[it.a_off:it.a_off + it.r * it.K]
        bound = 1 / math.sqrt(it.K)     # kaiming_uniform(a = sqrt 5): gain sqrt(1/3), bound sqrt(3) gain / sqrt(fan_in)
        assert a.abs().max() <= bound and a.abs().max() > 0.9 * bound and abs(a.mean()) < 0.1 * bound
        assert (p[it.b_off:it.b_off + it.N * it.r] == 0).all()


def test_safetensors_round_trip_names_shapes_and_metadata(tmp_path):
    from safetensors import safe_open
    from safetensors.torch import save_file
    fp = _fp()
    targets = ['to_k', 'mid_block.resnets.1.conv2', 'conv_shortcut']
    ad = L.LoRAAdapters(fp, 3, alpha=12, target_modules=targets)
    ad.params = torch.randn(ad.total, generator=torch.Generator().manual_seed(1))
    path = str(tmp_path / 'a.safetensors')
    L.save_file(ad, path)
    with safe_open(path, framework='pt') as f:
        meta, keys = f.metadata(), set(f.keys())
        shapes = {k: tuple(f.get_tensor(k).shape) for k in keys}
    assert meta['rank'] == '3' and float(meta['alpha']) == 12.0 and json.loads(meta['target_modules']) == targets
    views = {k[:-len('.weight')]: (s, fn) for k, s, fn in fp.views if k.endswith('.weight')}
    for it in ad.items:
        s, fn = views[it.module]
        wshape = tuple(fn(torch.empty(fp.storages[s].shape)).shape)
        ka, kb = lr.keys_of(it.module)
        assert (shapes[ka], shapes[kb]) == lr.file_shapes(it.module, wshape, 3)
    assert keys == {k for it in ad.items for k in lr.keys_of(it.module)}
    # s B A in the file's shapes is the kernel layout's B A in the storage's layout (OHWI for a convolution)
    sd = ad.state_dict()
    it = next(i for i in ad.items if i.T == 9)
    ka, kb = lr.keys_of(it.module)
    d_file = lr.delta_weight(sd[ka].double(), sd[kb].double(), 1.0)                       # [cout, cin, 3, 3]
    d_kernel = (ad.B(it).double() @ ad.A(it).double()).view(it.N, 3, 3, it.C).permute(0, 3, 1, 2)
    assert torch.equal(d_file, d_kernel)
    # read back
    sd2, rank, alpha, tg = L.read_file(path)
    assert (rank, alpha, tg) == (3, 12.0, targets)
    ad2 = L.LoRAAdapters(fp, rank, alpha, tg)
    ad2.params = torch.zeros(ad2.total)
    ad2.load_state_dict(sd2)
    for it in ad.items:
        assert torch.equal(ad.A(it), ad2.A(it)) and torch.equal(ad.B(it), ad2.B(it))
    # a file without metadata: alpha = r, the targets are the modules its keys name
    bare = str(tmp_path / 'bare.safetensors')
    save_file(sd, bare)
    sd3, rank, alpha, tg = L.read_file(bare)
    assert (rank, alpha) == (3, 3.0) and sorted(tg) == sorted(it.module for it in ad.items)
    ad3 = L.LoRAAdapters(fp, rank, alpha, tg)
    assert [i.module for i in ad3.items] == [i.module for i in ad.items]
    with pytest.raises(ValueError):
        L.LoRAAdapters(fp, 3, target_modules=['to_q']).load_state_dict(sd)


@pytest.mark.parametrize('name,r', COMBOS)
def test_projection_identity_in_float64(name, r):
    """What the design rests on: with W' = W + s B A, autograd's dA and dB ARE s B^T dW and s dW A^T of autograd's dW."""
    d = lr.case_data(name, r)
    assert len(d.grads) == 2 * len(d.ad.items)
    for it in d.ad.items:
        ka, kb = lr.keys_of(it.module)
        A, B, dW = d.tensors[ka], d.tensors[kb], d.dense[it.module + '.weight']
        dA = d.ad.scale * (B.reshape(it.N, -1).T @ dW.reshape(it.N, -1)).reshape(A.shape)
        dB = d.ad.scale * (dW.reshape(it.N, -1) @ A.reshape(it.r, -1).T).reshape(B.shape)
        for got, ref in ((dA, d.grads[ka]), (dB, d.grads[kb])):
            assert ref.norm() > 0, it.module                           # no adapter tensor has a zero gradient: none is excluded
            assert (got - ref).norm() <= 1e-10 * ref.norm(), it.module


@pytest.mark.parametrize('name,r', COMBOS)
def test_the_adapter_matters(name, r):
    """A path that ignores the adapters cannot pass the GPU parity test: with the test's B the fp64 prediction moves by more
    than 10 x the prediction bound."""
    d = lr.case_data(name, r)
    moved = ((d.pred - d.base_pred).norm() / d.base_pred.norm()).item()
    assert moved > 10 * ws.BOUNDS['pred_rel'], moved


def test_bounds_are_twice_the_emulation():
    """BOUNDS of lora_reference.py is the rule applied to the emulation: 2 x the worst per-tensor figure of the reference alone
    under our number format (EMU_WORST, recorded there), rounded up to two digits; the emulation recomputed here agrees with
    the record and stays inside walk_stress.BOUNDS for the prediction."""
    worst = lr.emulation_worst()
    print('\nemulation, worst over cases and ranks:', worst)
    # the arithmetic of the rule, on the recorded figures: 2 x, rounded up to two digits
    assert 2 * lr.EMU_WORST['tensor_rel'] <= lr.BOUNDS['tensor_rel'] <= 2 * lr.EMU_WORST['tensor_rel'] + 0.01
    assert 2 * (1 - lr.EMU_WORST['matrix_cos']) - 1e-12 <= 1 - lr.BOUNDS['matrix_cos'] <= 2 * (1 - lr.EMU_WORST['matrix_cos']) + 1e-4
    # the record is not stale, and the reference alone passes.  The emulation's worst tensor is a chaotic statistic (which bf16
    # roundings flip depends on the host's fp32 summation order: one case moved from 0.063 to 0.089 between two hosts, the
    # worst over the cases from 0.0906 to 0.0891, the worst cosine from 0.99645 to 0.99613), so it is held inside the bound
    # from above and to half the recorded figure from below: the bound is never more than 4 x a host's own emulation
    assert 0.5 * lr.EMU_WORST['tensor_rel'] <= worst['tensor_rel'] < lr.BOUNDS['tensor_rel']
    assert 0.5 * (1 - lr.EMU_WORST['matrix_cos']) <= 1 - worst['matrix_cos'] <= 1 - lr.BOUNDS['matrix_cos']
    for name, r in COMBOS:
        emu = lr.case_data(name, r).emu
        assert emu['pred_rel'] < ws.BOUNDS['pred_rel']
        assert len(emu['tensor_rel']) == 2 * len(lr.layout(name, r).items)


def test_optimizer_and_algorithm_refuse_what_the_design_excludes():
    from diffusion_amd.algorithms.lora import LoRA
    from diffusion_amd.optim import FusedAdamW

    class _U:
        lora = None
        master = torch.zeros(8)
    opt = FusedAdamW(unet=_U())
    with pytest.raises(ValueError):
        opt.attach_lora()                         # no adapters on the U-Net
    _U.lora = object()
    opt.ema = torch.zeros(8)
    with pytest.raises(ValueError):
        opt.attach_lora()                         # EMA averages the frozen master
    with pytest.raises(ValueError):
        LoRA(rank=4).configure_optimizer(opt)
    opt.ema = None
    opt.attach_lora()
    with pytest.raises(RuntimeError):
        opt.begin_step()                          # no step_range slices in adapter mode
    assert LoRA(rank=8, target_modules=['to_q']).state_dict()['rank'] == 8


def test_reachable_from_yaml_under_the_reference_prefix():
    import diffusion_amd.hydra_lite as hl
    from diffusion_amd.algorithms.lora import LoRA
    assert hl.resolve_target('diffusion.algorithms.lora.LoRA') is LoRA
    a = hl.instantiate({'_target_': 'diffusion.algorithms.lora.LoRA', 'rank': 4, 'alpha': 8, 'target_modules': ['to_q', 'to_v']})
    assert isinstance(a, LoRA) and (a.rank, a.alpha, a.target_modules) == (4, 8, ['to_q', 'to_v'])
    assert hasattr(a, 'configure_optimizer') and hasattr(a, 'before_optimizer_step')
