"""Low-rank adapters (LoRA) on a frozen U-Net, through the bf16 weight shadows.

The kernels never read the fp32 master: they read the bf16 shadow and its transposed twin.  An adapted matrix W [N, K] with
A [r, K], B [N, r] and s = alpha / r therefore needs no second GEMM path: ``da_lora_merge`` writes
shadow = bf16(master + s B A) and every existing launch (training forward, dgrad, the sampling walk, the cached K/V
projections, graph replay) computes with the adapted weight.  The dense weight gradient dW the existing wgrad leaves in
``unet.grad`` gives the adapter gradients exactly, dA = s B^T dW and dB = s dW A^T (``da_lora_project``), once per
optimizer step.  The master stays the frozen base.  One departure from PEFT: there the low-rank path stays separate in the
forward, here it goes through the bf16 rounding of the merged weight.

``LoRAAdapters`` is pure host layout (usable without a GPU, like ``models.unet.build_layout``); ``to(device)`` allocates
the flat buffers and uploads the item table.  File format: safetensors with PEFT / diffusers key names,
``unet.<module>.lora_A.weight`` [r, in] and ``.lora_B.weight`` [out, r] (convolutions [r, cin, kh, kw] / [cout, r, 1, 1]);
rank, alpha and target_modules in the metadata.  Written from the documented layout: interchange with files produced by
those packages has not been verified."""
from __future__ import annotations

import json
import math
import struct
from typing import Dict, List, Optional, Sequence

import torch

DEFAULT_TARGETS = ('to_q', 'to_k', 'to_v', 'to_out.0')
MAX_RANK = 128
ALIGN = 64
ITEM_FORMAT = '<qqqiiifiiii'   # struct DaLoraItem of include/diffusion_amd.h
# views of a fused storage: module suffix -> (storage stem, part, parts); the part is a contiguous row range
_FUSED = {'attn1.to_q': ('attn1.qkv', 0, 3), 'attn1.to_k': ('attn1.qkv', 1, 3), 'attn1.to_v': ('attn1.qkv', 2, 3),
          'attn2.to_k': ('attn2.kv', 0, 2), 'attn2.to_v': ('attn2.kv', 1, 2)}


class LoRAItem:
    """One adapted matrix: rows [row0, row0 + N) of ``storage`` (kernel layout [*, T * C], K = T * C)."""
    __slots__ = ('module', 'storage', 'row0', 'N', 'T', 'C', 'K', 'r', 'w_off', 'a_off', 'b_off')

    def __repr__(self):
        return f'LoRAItem({self.module}: rows {self.row0}+{self.N} of {self.storage}, K={self.K}, r={self.r})'


def matrix_modules(fp) -> Dict[str, tuple]:
    """{diffusers module name: (storage, row0, N)} of every weight matrix of the layout, in manifest order."""
    out = {}
    for key, sname, _ in fp.views:
        if not key.endswith('.weight') or fp.storages[sname].ntc is None:
            continue
        mod = key[:-len('.weight')]
        n_all = fp.storages[sname].ntc[0]
        row0, n = 0, n_all
        for suf, (_, part, parts) in _FUSED.items():
            if mod.endswith('.' + suf):
                n = n_all // parts
                row0 = part * n
        out[mod] = (sname, row0, n)
    return out


def _refusal(mod: str) -> Optional[str]:
    if mod in ('conv_in', 'conv_out'):
        return f'{mod} is stored padded to 8 channels and cannot carry an adapter'
    if mod.endswith('.time_emb_proj'):
        return f'{mod}: the time_emb_proj matrices are fused across resnets into one storage and cannot carry an adapter'
    return None


class LoRAAdapters:

    def __init__(self, fp, rank: int, alpha: Optional[float] = None, target_modules: Optional[Sequence[str]] = None,
                 seed: int = 17):
        if isinstance(rank, bool) or int(rank) != rank or not 1 <= int(rank) <= MAX_RANK:
            raise ValueError(f'LoRA rank must be an integer in 1..{MAX_RANK}, got {rank!r}')
        self.rank = int(rank)
        self.alpha = float(self.rank if alpha is None else alpha)
        if isinstance(target_modules, str):
            target_modules = [target_modules]
        self.target_modules = tuple(target_modules) if target_modules else DEFAULT_TARGETS
        self.seed = int(seed)
        self.scale_mult = 1.0      # set_lora_scale(): sampling at another strength
        mods = matrix_modules(fp)
        chosen: List[str] = []
        for t in self.target_modules:
            hit = [m for m in mods if m == t or m.endswith('.' + t)]
            if not hit:
                raise ValueError(f'LoRA target {t!r} matches no weight matrix of the U-Net')
            for m in hit:
                why = _refusal(m)
                if why:
                    raise ValueError(f'LoRA target {t!r}: {why}')
            chosen += [m for m in hit if m not in chosen]
        order = {m: i for i, m in enumerate(mods)}
        chosen.sort(key=order.__getitem__)
        self.items: List[LoRAItem] = []
        off = 0
        for m in chosen:
            sname, row0, n = mods[m]
            st = fp.storages[sname]
            _, T, C = st.ntc
            it = LoRAItem()
            it.module, it.storage, it.row0, it.N, it.T, it.C, it.K, it.r = m, sname, row0, n, T, C, T * C, self.rank
            it.w_off = st.off + row0 * it.K
            it.a_off = off
            off += -(-(it.r * it.K) // ALIGN) * ALIGN
            it.b_off = off
            off += -(-(it.N * it.r) // ALIGN) * ALIGN
            self.items.append(it)
        self.total = off
        self.master_extent = max(it.w_off + it.N * it.K for it in self.items)
        self.storages = sorted({it.storage for it in self.items})
        self.params = self.grad = self.exp_avg = self.exp_avg_sq = self.shadow_scratch = self.table = None
        self._sumsq = None

    # ---- layout ----------------------------------------------------------------------------------------------------------
    @property
    def scale(self) -> float:
        return self.alpha / self.rank

    def tiles(self):
        """(merge, dA, dB) workgroup counts of the item table."""
        mt = sum(-(-it.N // 32) * -(-it.K // 128) for it in self.items)
        da = sum(-(-it.r // 32) * -(-it.K // 128) for it in self.items)
        db = sum(-(-it.N // 32) for it in self.items)
        return mt, da, db

    def pack(self, scale: Optional[float] = None) -> bytes:
        s = self.scale * self.scale_mult if scale is None else float(scale)
        return pack_items([(it.w_off, it.a_off, it.b_off, it.N, it.K, it.r, s) for it in self.items])

    def segments(self):
        """(names, offsets, numels) of the adapter tensors in buffer order: the segments of the gradient-norm pass."""
        names, offs, numels = [], [], []
        for it in self.items:
            names += [f'unet.{it.module}.lora_A.weight', f'unet.{it.module}.lora_B.weight']
            offs += [it.a_off, it.b_off]
            numels += [it.r * it.K, it.N * it.r]
        return names, offs, numels

    def init_params(self) -> torch.Tensor:
        """PEFT's init on the host: A ~ kaiming_uniform(a = sqrt 5), i.e. U(+-1 / sqrt(fan_in)), from one seeded generator in
        manifest order; B = 0."""
        g = torch.Generator().manual_seed(self.seed)
        p = torch.zeros(self.total, dtype=torch.float32)
        for it in self.items:
            bound = 1.0 / math.sqrt(it.K)
            a = (torch.rand(it.r, it.K, generator=g, dtype=torch.float64) * 2 - 1) * bound
            p[it.a_off:it.a_off + it.r * it.K] = a.float().reshape(-1)
        return p

    # ---- device ----------------------------------------------------------------------------------------------------------
    def to(self, device):
        dev = torch.device(device)
        self.params = self.init_params().to(dev)
        self.grad = torch.zeros(self.total, device=dev, dtype=torch.float32)
        self.exp_avg = torch.zeros_like(self.grad)
        self.exp_avg_sq = torch.zeros_like(self.grad)
        self.shadow_scratch = torch.zeros(self.total, device=dev, dtype=torch.bfloat16)   # da_adamw always writes a shadow
        self.upload_table()
        return self

    def upload_table(self):
        self.table = torch.frombuffer(bytearray(self.pack()), dtype=torch.uint8).to(self.params.device)

    def sumsq_tables(self):
        if self._sumsq is None:
            from .models.unet import SumsqTables
            names, offs, numels = self.segments()
            self._sumsq = (names, SumsqTables(list(zip(offs, numels))).to(self.params.device))
        return self._sumsq

    def A(self, it: LoRAItem, buf=None) -> torch.Tensor:
        return (self.params if buf is None else buf)[it.a_off:it.a_off + it.r * it.K].view(it.r, it.K)

    def B(self, it: LoRAItem, buf=None) -> torch.Tensor:
        return (self.params if buf is None else buf)[it.b_off:it.b_off + it.N * it.r].view(it.N, it.r)

    # ---- files -----------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, torch.Tensor]:
        """PEFT / diffusers names and shapes (CPU fp32 copies)."""
        out = {}
        for it in self.items:
            out.update(to_file_tensors(it, self.A(it).detach().cpu(), self.B(it).detach().cpu()))
        return out

    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        want = {k for it in self.items for k in file_keys(it)}
        if want != set(sd):
            miss, extra = sorted(want - set(sd)), sorted(set(sd) - want)
            raise ValueError(f'LoRA file does not match the adapter layout: missing {miss[:3]}, unexpected {extra[:3]}')
        host = torch.zeros(self.total, dtype=torch.float32)
        for it in self.items:
            a, b = from_file_tensors(it, sd)
            host[it.a_off:it.a_off + it.r * it.K] = a.reshape(-1)
            host[it.b_off:it.b_off + it.N * it.r] = b.reshape(-1)
        self.params.copy_(host)

    def metadata(self) -> Dict[str, str]:
        return {'format': 'pt', 'rank': str(self.rank), 'alpha': repr(self.alpha),
                'target_modules': json.dumps(list(self.target_modules))}


def pack_items(rows) -> bytes:
    """The device table of da_lora_merge / da_lora_project from (w_off, a_off, b_off, N, K, r, scale) rows."""
    out, fm, fa, fb = [], 0, 0, 0
    for w_off, a_off, b_off, N, K, r, s in rows:
        if not (1 <= r <= MAX_RANK and N >= 1 and K >= 1 and min(w_off, a_off, b_off) >= 0):
            raise ValueError(f'LoRA item (N={N}, K={K}, r={r}) out of range (1 <= r <= {MAX_RANK})')
        out.append(struct.pack(ITEM_FORMAT, w_off, a_off, b_off, N, K, r, s, fm, fa, fb, 0))
        fm += -(-N // 32) * -(-K // 128)
        fa += -(-r // 32) * -(-K // 128)
        fb += -(-N // 32)
    return b''.join(out)


def file_keys(it: LoRAItem):
    return f'unet.{it.module}.lora_A.weight', f'unet.{it.module}.lora_B.weight'


def to_file_tensors(it: LoRAItem, A: torch.Tensor, B: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Kernel layout (A [r, T * C] tap-major, B [N, r]) -> the file's shapes."""
    ka, kb = file_keys(it)
    if it.T > 1:                                         # 3x3 convolution: [r, cin, 3, 3] and [cout, r, 1, 1]
        side = math.isqrt(it.T)
        return {ka: A.view(it.r, side, side, it.C).permute(0, 3, 1, 2).contiguous(), kb: B.reshape(it.N, it.r, 1, 1).contiguous()}
    if it.module.endswith('conv_shortcut'):              # 1x1 convolution
        return {ka: A.reshape(it.r, it.C, 1, 1).contiguous(), kb: B.reshape(it.N, it.r, 1, 1).contiguous()}
    return {ka: A.contiguous().clone(), kb: B.contiguous().clone()}


def from_file_tensors(it: LoRAItem, sd):
    ka, kb = file_keys(it)
    a, b = sd[ka].float(), sd[kb].float()
    if a.shape[0] != it.r or a.numel() != it.r * it.K or b.numel() != it.N * it.r:
        raise ValueError(f'{ka}: shapes {tuple(a.shape)} / {tuple(b.shape)} do not fit rank {it.r}, [{it.N}, {it.K}]')
    if a.dim() == 4:
        a = a.permute(0, 2, 3, 1)                        # [r, cin, kh, kw] -> [r, kh, kw, cin]
    return a.reshape(it.r, it.K).contiguous(), b.reshape(it.N, it.r).contiguous()


def save_file(adapters: LoRAAdapters, path: str):
    from safetensors.torch import save_file as _save
    _save(adapters.state_dict(), path, metadata=adapters.metadata())


def read_file(path: str):
    """(tensors, rank, alpha, target_modules or None) of a LoRA file.  Without metadata: the rank is lora_A's first extent,
    alpha = rank, and the targets are the modules the keys name."""
    from safetensors import safe_open
    sd = {}
    with safe_open(path, framework='pt') as f:
        meta = f.metadata() or {}
        for k in f.keys():
            sd[k] = f.get_tensor(k)
    a_keys = [k for k in sd if k.endswith('.lora_A.weight')]
    if not a_keys or any(not k.startswith('unet.') for k in sd):
        raise ValueError(f'{path}: no unet.*.lora_A.weight / lora_B.weight tensors')
    ranks = {int(sd[k].shape[0]) for k in a_keys}
    if len(ranks) != 1:
        raise ValueError(f'{path}: adapters of several ranks {sorted(ranks)} are not supported')
    rank = int(meta.get('rank', ranks.pop()))
    alpha = float(meta['alpha']) if 'alpha' in meta else float(rank)
    targets = json.loads(meta['target_modules']) if 'target_modules' in meta else \
        [k[len('unet.'):-len('.lora_A.weight')] for k in a_keys]
    return sd, rank, alpha, targets
