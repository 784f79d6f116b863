"""Thin host wrappers over the C ABI (include/diffusion_amd.h): shape validation + pointer plumbing.

Tensors are torch CUDA(HIP) tensors used as device memory only; every arithmetic op is a HIP kernel of
libdiffusion_amd.so.  A "matrix" argument is a 2-D tensor with unit column stride; its row stride is
passed as ld, so column slices of wider buffers (fused QKV, concat buffers) are valid arguments.
"""
from __future__ import annotations

import ctypes
import math
import numbers
import os
import struct
from typing import Optional, Tuple

import torch

from . import _lib

BF16 = torch.bfloat16
F32 = torch.float32


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# optional fp32 workspace for split-K (set by the owner of the compute, e.g. UNetHIP): da_gemm_nt splits the K loop
# of small-M calls over several workgroups when this is available
SPLITK_WS = None


# bench.py instrumentation: when PROFILE is a dict, every launch of the named kernel family is bracketed by HIP
# events on the launch stream and its algorithmic FLOPs are recorded: PROFILE[name] -> list of (start, end, flops)
PROFILE = None


class _Timed:
    __slots__ = ('name', 'flops', 'start', 'tag')

    def __init__(self, name, flops, tag=None):
        self.name, self.flops, self.tag = name, flops, tag

    def __enter__(self):
        if PROFILE is not None:
            self.start = torch.cuda.Event(enable_timing=True)
            self.start.record()

    def __exit__(self, *exc):
        if PROFILE is not None:
            end = torch.cuda.Event(enable_timing=True)
            end.record()
            PROFILE.setdefault(self.name, []).append((self.start, end, self.flops))
            if self.tag is not None:
                PROFILE.setdefault('_shapes', []).append((self.start, end, self.flops, (self.name,) + self.tag))


def _mat(x: torch.Tensor, dtype=BF16, name='arg') -> Tuple[int, int]:
    if x.dim() != 2 or x.stride(1) != 1 or x.dtype != dtype or not x.is_cuda:
        raise ValueError(f'{name}: need a 2-D {dtype} device matrix with unit column stride, got '
                         f'{tuple(x.shape)} strides {x.stride()} {x.dtype} {x.device}')
    ld = x.stride(0) if x.shape[0] > 1 else max(x.stride(0), x.shape[1])
    if ld % 8 or x.shape[1] % 8 or (x.data_ptr() % 16):
        raise ValueError(f'{name}: columns, row stride and base must be multiples of 8 elements / 16 bytes')
    return x.data_ptr(), ld


def _vec(x: Optional[torch.Tensor], n: int, name='vec') -> int:
    if x is None:
        return 0
    if x.dtype != F32 or not x.is_contiguous() or x.numel() != n or not x.is_cuda:
        raise ValueError(f'{name}: need contiguous fp32[{n}] on device, got {tuple(x.shape)} {x.dtype}')
    return x.data_ptr()


def _f32buf(x: torch.Tensor, min_numel: int, name='buf') -> int:
    if x.dtype != F32 or not x.is_contiguous() or x.numel() < min_numel or not x.is_cuda:
        raise ValueError(f'{name}: need contiguous fp32 buffer of >= {min_numel} elements')
    return x.data_ptr()


_OPTS = {}   # last value set per key (profiling labels only; the library holds the state)


def set_option(key: str, value: int):
    _lib.call('da_set_option', key.encode(), int(value))
    _OPTS[key] = int(value)


def _opt(key: str, default: int) -> int:
    if key in _OPTS:
        return _OPTS[key]
    for kv in filter(None, os.environ.get('DA_SET_OPTIONS', '').split(',')):
        k, _, v = kv.partition('=')
        if k.strip() == key:
            return int(v)
    return default


class Geom:
    """Geometry of an implicit-GEMM call.  Linear layers: Geom.linear()."""
    __slots__ = ('B', 'Hin', 'Win', 'Hout', 'Wout', 'ksize', 'mode')

    def __init__(self, B, Hin, Win, Hout, Wout, ksize, mode):
        self.B, self.Hin, self.Win, self.Hout, self.Wout, self.ksize, self.mode = B, Hin, Win, Hout, Wout, ksize, mode

    @staticmethod
    def linear(M):
        return Geom(M, 1, 1, 1, 1, 1, 0)

    @staticmethod
    def conv(B, H, W, ksize=3):
        return Geom(B, H, W, H, W, ksize, 0)

    @staticmethod
    def down(B, H, W):  # stride-2 conv, H x W -> H/2 x W/2
        return Geom(B, H, W, H // 2, W // 2, 3, 1)

    @staticmethod
    def down_vae(B, H, W):  # stride-2 conv over an image zero-padded at the bottom / right only (VAE encoder downsampler)
        return Geom(B, H, W, H // 2, W // 2, 3, 4)

    @staticmethod
    def down_dgrad(B, H, W):  # dgrad of the above: "input" dY at H/2, output dX at H
        return Geom(B, H // 2, W // 2, H, W, 3, 2)

    @staticmethod
    def up(B, H, W):  # conv over nearest-2x upsampled input
        return Geom(B, H, W, 2 * H, 2 * W, 3, 3)


def gemm_nt(A, W, out, g: Geom, *, bias=None, rowbias=None, residual=None, alpha=1.0):
    """out[M,N] = alpha * gather(A) @ W^T + bias + rowbias[image] + residual.  W: bf16 [N, k*k*Cin]."""
    a_ptr, lda = _mat(A, BF16, 'A')
    w_ptr, ldw = _mat(W, BF16, 'W')
    N, K = W.shape
    Cin = A.shape[1]
    if ldw != K or K != g.ksize * g.ksize * Cin:
        raise ValueError(f'W must be contiguous [N, {g.ksize * g.ksize * Cin}], got {tuple(W.shape)} ld {ldw}')
    M = g.B * g.Hout * g.Wout
    if A.shape[0] != g.B * g.Hin * g.Win:
        raise ValueError(f'A rows {A.shape[0]} != B*Hin*Win {g.B * g.Hin * g.Win}')
    out_fp32 = out.dtype == F32
    c_ptr, ldc = _mat(out, F32 if out_fp32 else BF16, 'out')
    if tuple(out.shape) != (M, N):
        raise ValueError(f'out shape {tuple(out.shape)} != {(M, N)}')
    rb_ptr, ldrb = (0, 0)
    if rowbias is not None:
        rb_ptr, ldrb = _mat(rowbias, BF16, 'rowbias')
        if tuple(rowbias.shape) != (g.B, N):
            raise ValueError('rowbias must be [B, N]')
    r_ptr, ldr = (0, 0)
    if residual is not None:
        r_ptr, ldr = _mat(residual, BF16, 'residual')
        if tuple(residual.shape) != (M, N):
            raise ValueError('residual must be [M, N]')
    flops = 2.0 * M * N * K * (0.25 if g.mode == 2 else 1.0)  # mode 2: 3 of 4 taps are structurally zero
    name = 'gemm_nt'
    if PROFILE is not None:
        v = _lib.load().da_gemm_nt_variant_for(M, N, K, Cin, SPLITK_WS.numel() if SPLITK_WS is not None else 0)
        name = {1: 'gemm_nt_kernel', 4: 'gemm_nt2_kernel<4,4,4,2>', 5: 'gemm_nt2_kernel<4,5,4,2>',
                10: 'gemm_nt2_kernel<8,5,2,4>', 11: 'gemm_nt2_kernel<4,10,2,2>', 12: 'gemm_nt2_kernel<4,5,4,4>',
                14: 'gemm_nt2_kernel<4,4,4,4>', 15: 'gemm_nt2_kernel<1,5,8,2,mf32>', 16: 'gemm_nt2_kernel<2,5,4,2,mf32>',
                18: 'gemm_nt2_kernel<3,4,8,2>'}[v]
        # the weight-stationary form takes the K = 320 linears first (da_gemm_nt_ws_try, gemm_nt_ws.hip: same conditions)
        ws = _opt('gemm_nt_ws', 1)
        ws_bn = 320 if (K == 320 and (ws & 1) and N <= 1280) else 128 if (K == 640 and (ws & 2) and N <= 1024) else 0
        if (ws_bn and _opt('gemm_nt_variant', 0) == 0 and N % ws_bn == 0 and M % 32 == 0 and (M // 32) * (N // ws_bn) >= 8 * 256
                and g.ksize == 1 and g.mode == 0 and not out_fp32 and alpha == 1.0 and rowbias is None):
            name = 'gemm_nt_ws_kernel'
    with _Timed(name, flops, (M, N, K, g.ksize, g.mode)):
        _lib.call('da_gemm_nt', a_ptr, lda, w_ptr, c_ptr, ldc, _vec(bias, N, 'bias'), rb_ptr, ldrb, r_ptr, ldr, M, N,
                  K, Cin, g.Hin, g.Win, g.Hout, g.Wout, g.ksize, g.mode, int(out_fp32), float(alpha),
                  SPLITK_WS.data_ptr() if SPLITK_WS is not None else 0,
                  SPLITK_WS.numel() if SPLITK_WS is not None else 0, _stream())
    return out


def geglu_fusable(inner: int, K: int) -> bool:
    """shapes da_gemm_nt_geglu accepts (160 hidden units per column tile, 64-deep K steps)"""
    return inner % 160 == 0 and K % 64 == 0


def gemm_nt_geglu(A, W, F, G, bias):
    """F[M, 2*inner] = A @ W^T + bias ; G[M, inner] = F[:, :inner] * gelu(F[:, inner:]) - one launch."""
    a_ptr, lda = _mat(A, BF16, 'A')
    w_ptr, ldw = _mat(W, BF16, 'W')
    f_ptr, ldf = _mat(F, BF16, 'F')
    g_ptr, ldg = _mat(G, BF16, 'G')
    M, K = A.shape
    inner = G.shape[1]
    if tuple(W.shape) != (2 * inner, K) or ldw != K or tuple(F.shape) != (M, 2 * inner) or G.shape[0] != M:
        raise ValueError('gemm_nt_geglu: shape mismatch')
    if not geglu_fusable(inner, K):
        raise ValueError(f'gemm_nt_geglu needs inner % 160 == 0 and K % 64 == 0, got {inner}, {K}')
    if M * lda * 2 >= 1 << 32:   # the fused kernel addresses A by 32-bit byte offsets (DA_ERR_SHAPE): two launches, same bits
        gemm_nt(A, W, F, Geom.linear(M), bias=bias)
        geglu_fwd(F, G)
        return
    with _Timed('gemm_nt2_kernel<4,5,4,4>', 2.0 * M * 2 * inner * K, (M, 2 * inner, K, 1, 'geglu')):
        _lib.call('da_gemm_nt_geglu', a_ptr, lda, w_ptr, f_ptr, ldf, g_ptr, ldg, _vec(bias, 2 * inner, 'bias'), M, inner,
                  K, _stream())


def geglu_bwd_fusable(inner: int, K: int) -> bool:
    return inner % 320 == 0 and K % 64 == 0


def gemm_nt_geglu_bwd(dY, Wt, F, dF):
    """dF[M, 2*inner] = geglu_bwd(F, dY @ Wt^T) with the [M, inner] product never written to HBM.  Wt: [inner, K]."""
    dy_ptr, lddy = _mat(dY, BF16, 'dY')
    w_ptr, ldw = _mat(Wt, BF16, 'Wt')
    f_ptr, ldf = _mat(F, BF16, 'F')
    df_ptr, lddf = _mat(dF, BF16, 'dF')
    M, K = dY.shape
    inner = Wt.shape[0]
    if ldw != K or Wt.shape[1] != K or tuple(F.shape) != (M, 2 * inner) or tuple(dF.shape) != (M, 2 * inner):
        raise ValueError('gemm_nt_geglu_bwd: shape mismatch')
    if not geglu_bwd_fusable(inner, K):
        raise ValueError(f'gemm_nt_geglu_bwd needs inner % 320 == 0 and K % 64 == 0, got {inner}, {K}')
    if M * lddy * 2 >= 1 << 32:   # as in gemm_nt_geglu: the product goes through HBM once, then da_geglu_bwd
        dG = torch.empty(M, inner, device=dY.device, dtype=BF16)
        gemm_nt(dY, Wt, dG, Geom.linear(M))
        geglu_bwd(F, dG, dF)
        return
    with _Timed('gemm_nt2_kernel<4,5,4,4>', 2.0 * M * inner * K, (M, inner, K, 1, 'geglu_bwd')):
        _lib.call('da_gemm_nt_geglu_bwd', dy_ptr, lddy, w_ptr, f_ptr, ldf, df_ptr, lddf, M, inner, K, _stream())


def gemm_tn_wgrad(dY, X, dW, g: Geom, dbias=None, scratch=None):
    """dW[N, k*k*Cin] (fp32) += dY^T @ gather(X);  optionally dbias[N] += column sums of dY (fused)."""
    dy_ptr, lddy = _mat(dY, BF16, 'dY')
    x_ptr, ldx = _mat(X, BF16, 'X')
    M, N = dY.shape
    Cin = X.shape[1]
    if M != g.B * g.Hout * g.Wout or X.shape[0] != g.B * g.Hin * g.Win:
        raise ValueError('wgrad: row counts do not match the geometry')
    if dW.dtype != F32 or not dW.is_contiguous() or dW.numel() != N * g.ksize * g.ksize * Cin:
        raise ValueError(f'dW must be contiguous fp32 with {N * g.ksize * g.ksize * Cin} elements')
    mode = g.mode
    if mode == 2:
        raise ValueError('wgrad has no mode 2')
    with _Timed('gemm_tn', 2.0 * M * N * g.ksize * g.ksize * Cin, (M, N, g.ksize * g.ksize * Cin, g.ksize, g.mode)):
        db = _vec(dbias, N, 'dbias') if dbias is not None else 0
        sc = _f32buf(scratch, 256 * N * 2, 'scratch') if dbias is not None else 0
        _lib.call('da_gemm_tn_wgrad', dy_ptr, lddy, x_ptr, ldx, dW.data_ptr(), db, sc, M, N, Cin, g.Hin, g.Win,
                  g.Hout, g.Wout, g.ksize, mode, SPLITK_WS.data_ptr() if SPLITK_WS is not None else 0,
                  SPLITK_WS.numel() if SPLITK_WS is not None else 0, _stream())


def _wgrad_items(items, M):
    """(dY, X, dW, dbias | None) per linear layer -> the DaWgradItem array of da_gemm_tn_wgrad_group, validated as
    gemm_tn_wgrad validates one layer"""
    arr = (_lib.DaWgradItem * max(len(items), 1))()
    flops = 0.0
    for i, (dY, X, dW, dbias) in enumerate(items):
        dy_ptr, lddy = _mat(dY, BF16, f'items[{i}].dY')
        x_ptr, ldx = _mat(X, BF16, f'items[{i}].X')
        N, Cin = dY.shape[1], X.shape[1]
        if dY.shape[0] != M or X.shape[0] != M:
            raise ValueError(f'wgrad group: items[{i}] has {dY.shape[0]} / {X.shape[0]} rows, the group has {M}')
        if dW.dtype != F32 or not dW.is_contiguous() or dW.numel() != N * Cin or not dW.is_cuda:
            raise ValueError(f'items[{i}].dW must be contiguous fp32 with {N * Cin} elements on the device')
        db = _vec(dbias, N, f'items[{i}].dbias') if dbias is not None else 0
        arr[i] = _lib.DaWgradItem(dy_ptr, lddy, x_ptr, ldx, dW.data_ptr(), db or None, N, Cin)
        flops += 2.0 * M * N * Cin
    return arr, flops


def gemm_tn_wgrad_group(items, M):
    """The weight (and bias) gradients of several linear layers over the same M rows - items: (dY, X, dW, dbias | None) - as
    grouped launches (da_gemm_tn_wgrad_group; the per-layer path for what is not eligible).  Recorded as ONE 'gemm_tn' entry
    with the summed FLOPs, its time including the reduction."""
    if not items:
        return
    arr, flops = _wgrad_items(items, M)
    with _Timed('gemm_tn', flops, (M, len(items), 0, 1, 'group')):
        _lib.call('da_gemm_tn_wgrad_group', arr, len(items), M, SPLITK_WS.data_ptr() if SPLITK_WS is not None else 0,
                  SPLITK_WS.numel() if SPLITK_WS is not None else 0, _stream())


def gemm_tn_group_plan(shapes, M, ws_floats):
    """da_gemm_tn_group_plan (host only): shapes (N, Cin, has_dbias) -> {'splits': pixel splits of each grouped launch,
    'group_of': launch of item i or -1 for the per-layer path}"""
    n = len(shapes)
    arr = (_lib.DaWgradItem * max(n, 1))()
    for i, (N, Cin, has_db) in enumerate(shapes):
        arr[i] = _lib.DaWgradItem(None, N, None, Cin, None, 1 if has_db else None, N, Cin)
    splits = (ctypes.c_int * max(n, 1))()
    group_of = (ctypes.c_int * max(n, 1))()
    ng = _lib.load().da_gemm_tn_group_plan(arr, n, M, int(ws_floats), splits, n, group_of)
    if ng < 0:
        raise ValueError('da_gemm_tn_group_plan rejected the arguments')
    return {'splits': list(splits[:ng]), 'group_of': list(group_of[:n])}


def attn_fwd(Q, K, V, O, L2, B, H, Nq, Nk, scale):
    q, ldq = _mat(Q, BF16, 'Q')
    k, ldk = _mat(K, BF16, 'K')
    v, ldv = _mat(V, BF16, 'V')
    o, ldo = _mat(O, BF16, 'O')
    for t, n in ((Q, Nq), (O, Nq), (K, Nk), (V, Nk)):
        if tuple(t.shape) != (B * n, H * 64):
            raise ValueError(f'attention operand shape {tuple(t.shape)} != {(B * n, H * 64)}')
    with _Timed('attn_fwd', 4.0 * B * H * Nq * Nk * 64, (B, H, Nq, Nk, 0)):
        _lib.call('da_attn_fwd', q, ldq, k, ldk, v, ldv, o, ldo, _f32buf(L2, B * H * Nq, 'L2'), B, H, Nq, Nk,
                  float(scale), _stream())


def attn_fwd_wide(Q, K, V, O, L2, B, H, D, Nq, Nk, scale):
    """da_attn_fwd for head_dim D = 512 (the VAE's single mid-block head), forward only; same operand layout"""
    q, ldq = _mat(Q, BF16, 'Q')
    k, ldk = _mat(K, BF16, 'K')
    v, ldv = _mat(V, BF16, 'V')
    o, ldo = _mat(O, BF16, 'O')
    for t, n in ((Q, Nq), (O, Nq), (K, Nk), (V, Nk)):
        if tuple(t.shape) != (B * n, H * D):
            raise ValueError(f'attention operand shape {tuple(t.shape)} != {(B * n, H * D)}')
    with _Timed('attn_fwd_wide', 4.0 * B * H * Nq * Nk * D, (B, H, Nq, Nk, D)):
        _lib.call('da_attn_fwd_wide', q, ldq, k, ldk, v, ldv, o, ldo, _f32buf(L2, B * H * Nq, 'L2'), B, H, D, Nq, Nk,
                  float(scale), _stream())


def attn_fwd_causal(Q, K, V, O, L2, B, H, N, scale):
    """causal self-attention (key j <= query q), forward only: the frozen text encoder"""
    q, ldq = _mat(Q, BF16, 'Q')
    k, ldk = _mat(K, BF16, 'K')
    v, ldv = _mat(V, BF16, 'V')
    o, ldo = _mat(O, BF16, 'O')
    for t in (Q, K, V, O):
        if tuple(t.shape) != (B * N, H * 64):
            raise ValueError(f'attention operand shape {tuple(t.shape)} != {(B * N, H * 64)}')
    _lib.call('da_attn_fwd_causal', q, ldq, k, ldk, v, ldv, o, ldo, _f32buf(L2, B * H * N, 'L2'), B, H, N, float(scale),
              _stream())


def attn_bwd(Q, K, V, O, dO, L2, Delta, dQ, dK, dV, B, H, Nq, Nk, scale):
    ptrs = []
    for t, n, nm in ((Q, Nq, 'Q'), (K, Nk, 'K'), (V, Nk, 'V'), (O, Nq, 'O'), (dO, Nq, 'dO')):
        if tuple(t.shape) != (B * n, H * 64):
            raise ValueError(f'{nm} shape {tuple(t.shape)} != {(B * n, H * 64)}')
        ptrs += list(_mat(t, BF16, nm))
    outs = []
    for t, n, nm in ((dQ, Nq, 'dQ'), (dK, Nk, 'dK'), (dV, Nk, 'dV')):
        if tuple(t.shape) != (B * n, H * 64):
            raise ValueError(f'{nm} shape {tuple(t.shape)} != {(B * n, H * 64)}')
        outs += list(_mat(t, BF16, nm))
    with _Timed('attn_bwd', 8.0 * B * H * Nq * Nk * 64, (B, H, Nq, Nk, 0)):
        _lib.call('da_attn_bwd', *ptrs, _f32buf(L2, B * H * Nq, 'L2'), _f32buf(Delta, B * H * Nq, 'Delta'), *outs, B,
                  H, Nq, Nk, float(scale), _stream())


def norm_scratch_floats(B, HW, C) -> int:
    return int(_lib.load().da_norm_scratch_floats(B, HW, C))


def groupnorm_fwd(X, Y, gamma, beta, mean_rstd, scale_shift, scratch, B, HW, C, G, eps, silu):
    x, ldx = _mat(X, BF16, 'X')
    y, ldy = _mat(Y, BF16, 'Y')
    if tuple(X.shape) != (B * HW, C) or tuple(Y.shape) != (B * HW, C):
        raise ValueError('groupnorm: bad shapes')
    _lib.call('da_groupnorm_fwd', x, ldx, y, ldy, _vec(gamma, C), _vec(beta, C), _f32buf(mean_rstd, B * G * 2),
              _f32buf(scale_shift, B * C * 2), _f32buf(scratch, norm_scratch_floats(B, HW, C)), B, HW, C, G,
              float(eps), int(silu), _stream())


def groupnorm_bwd(X, dY, Radd, dX, gamma, beta, mean_rstd, dgamma, dbeta, coef, scratch, B, HW, C, G, silu):
    x, ldx = _mat(X, BF16, 'X')
    dy, lddy = _mat(dY, BF16, 'dY')
    dx, lddx = _mat(dX, BF16, 'dX')
    r, ldr = _mat(Radd, BF16, 'Radd') if Radd is not None else (0, 0)
    for t in (X, dY, dX) + ((Radd,) if Radd is not None else ()):
        if tuple(t.shape) != (B * HW, C):
            raise ValueError('groupnorm_bwd: bad shapes')
    _lib.call('da_groupnorm_bwd', x, ldx, dy, lddy, r, ldr, dx, lddx, _vec(gamma, C), _vec(beta, C),
              _f32buf(mean_rstd, B * G * 2), _vec(dgamma, C), _vec(dbeta, C), _f32buf(coef, B * G * 2),
              _f32buf(scratch, norm_scratch_floats(B, HW, C)), B, HW, C, G, int(silu), _stream())


GN_PLAN_FIELDS = ('threads', 'nl', 'cw', 'parts', 'peers8', 'P', 'nchunks')


def groupnorm_plan(B, HW, C, G, ld_min=None, ld_max=None, bwd=False) -> dict:
    """the GroupNorm form da_groupnorm_fwd / _bwd runs for this call under the current options (da_groupnorm_plan_for):
    {'form': 'resident' | 'multipass', 'threads', 'nl', 'cw', 'parts', 'peers8', 'P', 'nchunks'}; ld_min / ld_max are
    the smallest / largest row stride of the call's tensors (default C)"""
    out = (ctypes.c_int * 7)()
    ld_min = C if ld_min is None else ld_min
    ld_max = ld_min if ld_max is None else ld_max
    form = _lib.load().da_groupnorm_plan_for(B, HW, C, G, ld_min, ld_max, int(bool(bwd)), out)
    if form < 0:
        raise ValueError(f'groupnorm_plan: arguments rejected ({B}, {HW}, {C}, {G}, {ld_min}, {ld_max})')
    return dict(form='resident' if form == 1 else 'multipass', **dict(zip(GN_PLAN_FIELDS, out)))


def layernorm_fwd(X, Y, gamma, beta, mean_rstd, eps=1e-5):
    x, ldx = _mat(X, BF16, 'X')
    y, ldy = _mat(Y, BF16, 'Y')
    M, C = X.shape
    _lib.call('da_layernorm_fwd', x, ldx, y, ldy, _vec(gamma, C), _vec(beta, C), _f32buf(mean_rstd, 2 * M), M, C,
              float(eps), _stream())


def layernorm_bwd(X, dY, Radd, dX, gamma, mean_rstd, dgamma, dbeta, scratch):
    x, ldx = _mat(X, BF16, 'X')
    dy, lddy = _mat(dY, BF16, 'dY')
    dx, lddx = _mat(dX, BF16, 'dX')
    r, ldr = _mat(Radd, BF16, 'Radd') if Radd is not None else (0, 0)
    M, C = X.shape
    _lib.call('da_layernorm_bwd', x, ldx, dy, lddy, r, ldr, dx, lddx, _vec(gamma, C), _f32buf(mean_rstd, 2 * M),
              _vec(dgamma, C), _vec(dbeta, C), _f32buf(scratch, 1024 * C * 2), M, C, _stream())


def colsum_accum(X, out, scratch):
    x, ldx = _mat(X, BF16, 'X')
    M, C = X.shape
    _lib.call('da_colsum_accum', x, ldx, _vec(out, C), _f32buf(scratch, 256 * C * 2), M, C, _stream())


def image_colsum(X, out, db, scratch, B, HW):
    x, ldx = _mat(X, BF16, 'X')
    o, ldo = _mat(out, BF16, 'out')
    C = X.shape[1]
    if tuple(out.shape) != (B, C) or X.shape[0] != B * HW:
        raise ValueError('image_colsum: bad shapes')
    _lib.call('da_image_colsum', x, ldx, o, ldo, _vec(db, C) if db is not None else 0,
              _f32buf(scratch, norm_scratch_floats(B, HW, C)), B, HW, C, _stream())


def _map2d(entry, *mats, wide=()):
    """The strided-map entry points: (pointer, row stride) per operand, then M and C.  Every operand is a `_mat` of
    one shape [M, C]; those at the indices in ``wide`` are GEGLU projections [a | g] of 2 * C columns.  The kernel trusts
    M and C for every operand, so a smaller one would be read or written past its end.  Returns the last operand."""
    args = [v for m in mats for v in _mat(m, BF16, entry)]
    M, C = mats[0].shape[0], mats[0].shape[1] // (2 if 0 in wide else 1)
    for k, m in enumerate(mats):
        if tuple(m.shape) != (M, 2 * C if k in wide else C):
            raise ValueError(f'{entry[3:]}: shape mismatch: operand {k} is {tuple(m.shape)}, operand 0 '
                             f'{tuple(mats[0].shape)}' + (f' (operands {wide} have twice the columns)' if wide else ''))
    _lib.call(entry, *args, M, C, _stream())
    return mats[-1]


def geglu_fwd(inp, out):
    _map2d('da_geglu_fwd', inp, out, wide=(0,))


def geglu_bwd(inp, dout, din):
    _map2d('da_geglu_bwd', inp, dout, din, wide=(0, 2))


def silu_fwd(x, y):
    _map2d('da_silu_fwd', x, y)


def gelu_fwd(x, y):
    _map2d('da_gelu_fwd', x, y)


def quick_gelu_fwd(x, y):
    _map2d('da_quick_gelu_fwd', x, y)


def silu_bwd(x, dy, dx):
    _map2d('da_silu_bwd', x, dy, dx)


def add(a, b, out):
    return _map2d('da_add', a, b, out)


def copy2d(a, out):
    return _map2d('da_copy2d', a, out)


def upsample2x_bwd(dy, dx, B, H, W, C):
    if not (dy.is_contiguous() and dx.is_contiguous()) or dy.numel() != 4 * B * H * W * C or dx.numel() != B * H * W * C:
        raise ValueError('upsample2x_bwd: bad shapes')
    _lib.call('da_upsample2x_bwd', dy.data_ptr(), dx.data_ptr(), B, H, W, C, _stream())


def upsample2x_fwd(x, y, B, H, W, C):
    if not (x.is_contiguous() and y.is_contiguous()) or y.numel() != 4 * B * H * W * C or x.numel() != B * H * W * C:
        raise ValueError('upsample2x_fwd: bad shapes')
    _lib.call('da_upsample2x_fwd', x.data_ptr(), y.data_ptr(), B, H, W, C, _stream())


def timestep_embed(t, out):
    if t.dtype != torch.int64 or not t.is_contiguous() or out.dtype != BF16 or not out.is_contiguous():
        raise ValueError('timestep_embed: t int64 contiguous, out bf16 contiguous')
    _lib.call('da_timestep_embed', t.data_ptr(), out.data_ptr(), t.numel(), out.shape[1], _stream())


def timestep_embed_f32(t, out):
    if t.dtype != F32 or not t.is_cuda or not t.is_contiguous() or out.dtype != BF16 or not out.is_cuda \
            or not out.is_contiguous() or out.shape[0] != t.numel():
        raise ValueError('timestep_embed_f32: t fp32 [B] on device, out bf16 [B, dim] on device, both contiguous')
    _lib.call('da_timestep_embed_f32', t.data_ptr(), out.data_ptr(), t.numel(), out.shape[1], _stream())


# target kinds of da_add_noise_ex, by the reference's prediction_type names
NOISE_TARGETS = {'epsilon': 0, 'v_prediction': 1, 'sample': 2}


def add_noise_ex(x0, eps, t, xt, target, prediction_type='epsilon', sqrt_ac=None, sqrt_1mac=None):
    """Pixel-space noising (C = 1..8 channels): int64 ``t`` with the DDPM tables, or fp32 ``t`` (angles) with the tangent
    schedule computed in the kernel.  x0 / eps NCHW fp32; xt [B*H*W, 8] bf16 and target [B*H*W, 8] fp32."""
    if x0.dim() != 4:
        raise ValueError('add_noise_ex: x0/eps must be [B,C,H,W]')
    B, C = x0.shape[0], x0.shape[1]
    HW = x0.shape[2] * x0.shape[3]
    for z in (x0, eps):
        if z.dtype != F32 or not z.is_cuda or not z.is_contiguous() or z.shape != x0.shape:
            raise ValueError('add_noise_ex: x0/eps must be contiguous fp32 [B,C,H,W] device tensors')
    if not 1 <= C <= 8:
        raise ValueError(f'add_noise_ex: {C} channels (1..8 supported)')
    for z, dt in ((xt, BF16), (target, F32)):
        if z.dtype != dt or not z.is_cuda or not z.is_contiguous() or z.numel() != B * HW * 8 or z.data_ptr() % 16:
            raise ValueError('add_noise_ex: xt bf16 [B*HW,8], target fp32 [B*HW,8], contiguous on device')
    if not t.is_cuda or not t.is_contiguous() or t.numel() != B:
        raise ValueError('add_noise_ex: t must be a contiguous [B] device tensor')
    if prediction_type not in NOISE_TARGETS:
        raise ValueError(f'add_noise_ex: unknown prediction_type {prediction_type!r}')
    if t.dtype == F32:
        is_f32, pa, pb = 1, None, None
    elif t.dtype == torch.int64:
        if sqrt_ac is None or sqrt_1mac is None or int(sqrt_ac.numel()) != int(sqrt_1mac.numel()):
            raise ValueError('add_noise_ex: discrete t needs both sqrt(abar) tables')
        is_f32, pa, pb = 0, _vec(sqrt_ac, sqrt_ac.numel(), 'sqrt_ac'), _vec(sqrt_1mac, sqrt_1mac.numel(), 'sqrt_1mac')
    else:
        raise ValueError(f'add_noise_ex: t must be int64 (discrete) or fp32 (continuous), got {t.dtype}')
    _lib.call('da_add_noise_ex', x0.data_ptr(), eps.data_ptr(), t.data_ptr(), is_f32, pa, pb, xt.data_ptr(),
              target.data_ptr(), B, C, HW, NOISE_TARGETS[prediction_type], _stream())


def add_noise_rng(x0, seeds, t, xt, target, prediction_type='epsilon', sqrt_ac=None, sqrt_1mac=None, *, draw_t=True,
                  t_range=None, slots=None, n_slots=0, noise_offset=0.0, perturbation=0.0):
    """The noising of ``add_noise_ex`` with every draw made in the launch (``da_add_noise_rng``): no noise tensor, sample
    b's noise, offset, perturbation and timestep come from its own Philox key ``seeds[b]`` (uint64 [B] on the device).
    ``t`` int64 [B] (discrete, with both tables) or fp32 [B] (continuous) on the device: written with the drawn timesteps
    when ``draw_t``, else read.  ``t_range`` = (lo, hi): integers inside the table (default all of it), or fp32 values for
    continuous time (required).  ``slots`` int32 [B] on the device with ``n_slots``: timesteps stratified over n_slots."""
    if x0.dim() != 4:
        raise ValueError('add_noise_rng: x0 must be [B,C,H,W]')
    B, C = x0.shape[0], x0.shape[1]
    HW = x0.shape[2] * x0.shape[3]
    if x0.dtype != F32 or not x0.is_cuda or not x0.is_contiguous() or B < 1 or HW < 1 or HW > 2**31 - 1:
        raise ValueError('add_noise_rng: x0 must be a contiguous fp32 [B,C,H,W] device tensor with H W in 1..2^31 - 1')
    if not 1 <= C <= 8:
        raise ValueError(f'add_noise_rng: {C} channels (1..8 supported)')
    for z, dt in ((xt, BF16), (target, F32)):
        if z.dtype != dt or not z.is_cuda or not z.is_contiguous() or z.numel() != B * HW * 8 or z.data_ptr() % 16:
            raise ValueError('add_noise_rng: xt bf16 [B*HW,8], target fp32 [B*HW,8], contiguous on device')
    if not isinstance(seeds, torch.Tensor) or seeds.dtype != torch.uint64 or not seeds.is_cuda or not seeds.is_contiguous() \
            or tuple(seeds.shape) != (B,) or seeds.data_ptr() % 8:
        raise ValueError(f'add_noise_rng: seeds must be a contiguous uint64 [{B}] device tensor')
    if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous() or t.numel() != B:
        raise ValueError('add_noise_rng: t must be a contiguous [B] device tensor')
    if prediction_type not in NOISE_TARGETS:
        raise ValueError(f'add_noise_rng: unknown prediction_type {prediction_type!r}')
    noise_offset, perturbation = float(noise_offset), float(perturbation)
    if not math.isfinite(noise_offset) or not math.isfinite(perturbation):
        raise ValueError(f'add_noise_rng: noise_offset = {noise_offset}, perturbation = {perturbation} must be finite')
    if t.dtype == F32:
        is_f32, pa, pb, T = 1, None, None, 0
    elif t.dtype == torch.int64:
        if sqrt_ac is None or sqrt_1mac is None or int(sqrt_ac.numel()) != int(sqrt_1mac.numel()) or sqrt_ac.numel() < 1:
            raise ValueError('add_noise_rng: discrete t needs both sqrt(abar) tables')
        T = int(sqrt_ac.numel())
        is_f32, pa, pb = 0, _vec(sqrt_ac, T, 'sqrt_ac'), _vec(sqrt_1mac, T, 'sqrt_1mac')
    else:
        raise ValueError(f'add_noise_rng: t must be int64 (discrete) or fp32 (continuous), got {t.dtype}')
    n_slots = int(n_slots)
    if n_slots < 0 or (slots is None) != (n_slots == 0):
        raise ValueError(f'add_noise_rng: slots and n_slots >= 1 go together (n_slots = {n_slots})')
    if slots is not None and (not isinstance(slots, torch.Tensor) or slots.dtype != torch.int32 or not slots.is_cuda
                              or not slots.is_contiguous() or tuple(slots.shape) != (B,)):
        raise ValueError(f'add_noise_rng: slots must be a contiguous int32 [{B}] device tensor')
    lo = hi = 0.0
    if draw_t:
        if t_range is None:
            if is_f32:
                raise ValueError('add_noise_rng: continuous time needs t_range = (lo, hi)')
            t_range = (0, T)
        lo, hi = t_range
        if is_f32:
            lo, hi = float(lo), float(hi)
            if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi) or n_slots > 2**24 \
                    or any(struct.unpack('f', struct.pack('f', v))[0] != v for v in (lo, hi)):
                raise ValueError(f'add_noise_rng: t_range = ({lo}, {hi}) must be fp32 values with lo < hi; n_slots <= 2^24')
        else:
            if any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in (lo, hi)) or not 0 <= lo < hi <= T:
                raise ValueError(f'add_noise_rng: t_range = ({lo}, {hi}) must be integers with 0 <= lo < hi <= {T}')
            if n_slots * (hi - lo) >= 2**32:
                raise ValueError(f'add_noise_rng: n_slots * (hi - lo) = {n_slots * (hi - lo)} must stay below 2^32')
            lo, hi = float(lo), float(hi)
    _lib.call('da_add_noise_rng', x0.data_ptr(), seeds.data_ptr(), None if slots is None else slots.data_ptr(), n_slots,
              t.data_ptr(), is_f32, 1 if draw_t else 0, lo, hi, pa, pb, T, noise_offset, perturbation, xt.data_ptr(),
              target.data_ptr(), B, C, HW, NOISE_TARGETS[prediction_type], _stream())


IMAGE_INGEST_MAX_SIDE = 65535   # da_image_ingest skips larger sides; rejected here


def _image_ingest_args(fn, raw, off, hw, Rh, Rw, out, kind, host):
    """the checks the ingest entries share; returns B"""
    for z, dt, nm in ((raw, torch.uint8, 'raw uint8'), (off, torch.int64, 'off int64'), (hw, torch.int32, 'hw int32')):
        if not isinstance(z, torch.Tensor) or not z.is_cuda or z.dtype != dt or not z.is_contiguous():
            raise ValueError(f'{fn}: {nm} must be a contiguous device tensor')
    B = int(off.numel())
    if raw.dim() != 1 or off.dim() != 1 or B < 1 or tuple(hw.shape) != (B, 2):
        raise ValueError(f'{fn}: raw [nbytes], off [B], hw [B, 2] with B >= 1')
    if not (1 <= Rh <= 4096 and 1 <= Rw <= 4096):
        raise ValueError(f'{fn}: target {Rh} x {Rw} outside 1..4096' if Rh != Rw else f'{fn}: R = {Rh} outside 1..4096')
    if kind not in (0, 1):
        raise ValueError(f'{fn}: unknown out kind {kind!r} (0: bf16 NHWC-8, 1: fp32 NCHW)')
    dt, numel, align = ((BF16, B * Rh * Rw * 8, 16), (F32, B * 3 * Rh * Rw, 4))[kind]
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != dt or not out.is_contiguous() \
            or out.numel() != numel or out.data_ptr() % align:
        raise ValueError(f'{fn}: out must be a contiguous {dt} device tensor of {numel} elements, '
                         f'{align}-byte aligned (kind {kind})')
    if host is None:
        raise ValueError(f'{fn}: host=(off, hw) copies of the tables are required for the bounds check')
    h_off, h_hw = (torch.as_tensor(z) for z in host)
    if h_off.is_cuda or h_hw.is_cuda or h_off.numel() != B or tuple(h_hw.shape) != (B, 2):
        raise ValueError(f'{fn}: host=(off [B], hw [B, 2]) must be host tensors of the same shapes')
    h_off, h_hw = h_off.to(torch.int64), h_hw.to(torch.int64)
    if int(h_hw.min()) < 1 or int(h_hw.max()) > IMAGE_INGEST_MAX_SIDE:
        raise ValueError(f'{fn}: image sides must be in 1..{IMAGE_INGEST_MAX_SIDE}')
    end = h_off + 3 * h_hw[:, 0] * h_hw[:, 1]
    if int(h_off.min()) < 0 or int(end.max()) > raw.numel():
        raise ValueError(f'{fn}: the offset table runs outside the {raw.numel()}-byte buffer')
    return B


def image_ingest(raw, off, hw, R, out, kind, host=None):
    """LargestCenterSquare(R) + ToTensor + Normalize(0.5, 0.5) of packed RGB uint8 images (``da_image_ingest``).

    raw uint8 [nbytes], off int64 [B] (byte offsets, any alignment), hw int32 [B, 2] = (h, w): contiguous device tensors.
    out: kind 0 bf16 [B*R*R, 8] (NHWC-8, 16-byte aligned), kind 1 fp32 [B, 3, R, R].  ``host = (off, hw)`` are the host
    copies the collate function made of the two tables: sizes and ``off[b] + 3*h*w <= raw.numel()`` are checked on them,
    never by reading the device tables back.  They are required - the kernel trusts the tables."""
    R = int(R)
    B = _image_ingest_args('image_ingest', raw, off, hw, R, R, out, kind, host)
    _lib.call('da_image_ingest', raw.data_ptr(), off.data_ptr(), hw.data_ptr(), B, R, out.data_ptr(), int(kind), _stream())


def image_ingest_rect(raw, off, hw, Rh, Rw, out, kind, host=None):
    """``image_ingest`` for a target of ``Rh`` rows x ``Rw`` columns (``da_image_ingest_rect``): resize to cover, then the
    centre crop (``datasets.image_ingest.ingest_geometry`` with a pair).  out: kind 0 bf16 [B*Rh*Rw, 8], kind 1 fp32
    [B, 3, Rh, Rw]; everything else as ``image_ingest``, whose bits it gives at ``Rh == Rw``."""
    Rh, Rw = int(Rh), int(Rw)
    B = _image_ingest_args('image_ingest_rect', raw, off, hw, Rh, Rw, out, kind, host)
    _lib.call('da_image_ingest_rect', raw.data_ptr(), off.data_ptr(), hw.data_ptr(), B, Rh, Rw, out.data_ptr(), int(kind),
              _stream())


def image_ingest_aug(raw, off, hw, aug, Rh, Rw, out, kind, host=None):
    """``image_ingest_rect`` with a crop window and a horizontal flip per image (``da_image_ingest_aug``).  ``aug`` int32
    [B, 3] = (top, left, flip), a contiguous device tensor: origins in pixels of the resized image (``ingest_geometry``'s
    ``nh x nw``), ``out[Y][X] = resized[top + Y][left + X]``, and with ``flip = 1`` the same crop of the mirrored image.
    ``host = (off, hw, aug)``: on these copies the buffer bounds, ``0 <= top <= nh - Rh``, ``0 <= left <= nw - Rw`` and
    ``flip in {0, 1}`` are checked before anything is launched (the kernel clamps the origins besides).  The centre origins
    with flip 0 give ``image_ingest_rect``'s bits."""
    Rh, Rw = int(Rh), int(Rw)
    if host is None or len(host) != 3:
        raise ValueError('image_ingest_aug: host=(off, hw, aug) copies of the tables are required for the bounds check')
    B = _image_ingest_args('image_ingest_aug', raw, off, hw, Rh, Rw, out, kind, host[:2])
    if not isinstance(aug, torch.Tensor) or not aug.is_cuda or aug.dtype != torch.int32 or not aug.is_contiguous() \
            or tuple(aug.shape) != (B, 3):
        raise ValueError('image_ingest_aug: aug int32 [B, 3] must be a contiguous device tensor')
    h_aug = torch.as_tensor(host[2])
    if h_aug.is_cuda or tuple(h_aug.shape) != (B, 3):
        raise ValueError('image_ingest_aug: host aug [B, 3] must be a host tensor')
    h_aug, h_hw = h_aug.to(torch.int64), torch.as_tensor(host[1]).to(torch.int64)
    h, w = h_hw[:, 0], h_hw[:, 1]
    fit_w = w * Rh <= h * Rw   # ingest_geometry's cover rule, on the whole batch
    nw = torch.where(fit_w, torch.full_like(w, Rw), (Rh * w) // h)
    nh = torch.where(fit_w, (Rw * h) // w, torch.full_like(h, Rh))
    top, left, flip = h_aug[:, 0], h_aug[:, 1], h_aug[:, 2]
    if bool(((top < 0) | (top > nh - Rh) | (left < 0) | (left > nw - Rw)).any()):
        raise ValueError('image_ingest_aug: a crop origin lies outside [0, nh - Rh] x [0, nw - Rw] of its resized image')
    if bool(((flip != 0) & (flip != 1)).any()):
        raise ValueError('image_ingest_aug: flip must be 0 or 1')
    _lib.call('da_image_ingest_aug', raw.data_ptr(), off.data_ptr(), hw.data_ptr(), aug.data_ptr(), B, Rh, Rw,
              out.data_ptr(), int(kind), _stream())


def image_resize(raw, off, hw, Rh, Rw, out, kind, geometry, filter, range, host=None):
    """``image_ingest_rect`` with the transform as three switches (``da_image_resize``, the same kernel): ``geometry`` 0
    resize to cover + centre crop, 1 stretch each axis on its own; ``filter`` 0 the antialiased triangle filter (Pillow,
    ``F.interpolate(antialias=True)``), 1 two-tap bilinear (``F.interpolate(align_corners=False, antialias=False)``);
    ``range`` 0 ``v / 127.5 - 1``, 1 ``v / 255``.  ``(0, 0, 0)`` gives ``image_ingest_rect``'s bits.  Arguments, outputs and
    the host-side bounds check are ``image_ingest_rect``'s."""
    Rh, Rw = int(Rh), int(Rw)
    B = _image_ingest_args('image_resize', raw, off, hw, Rh, Rw, out, kind, host)
    for nm, val in (('geometry', geometry), ('filter', filter), ('range', range)):
        if val not in (0, 1):
            raise ValueError(f'image_resize: {nm} must be 0 or 1, got {val!r}')
    _lib.call('da_image_resize', raw.data_ptr(), off.data_ptr(), hw.data_ptr(), B, Rh, Rw, out.data_ptr(), int(kind),
              int(geometry), int(filter), int(range), _stream())


CLIP_MAX_PATCH, CLIP_MAX_SIZE = 32, 448   # da_clip_preprocess: one block stages a P x P patch
_CLIP_TABLES = {}   # (H, W, R, device) -> (xtab, ytab) int32 on the device


def clip_patch_cols(P: int) -> int:
    """columns of the patch matrix: 3 * P * P rounded up to the multiple of 8 da_gemm_nt needs (592 for P = 14)"""
    return (3 * P * P + 7) // 8 * 8


def clip_preprocess(images, R, P, out, kind, mean, std):
    """``CLIPImageProcessor`` of uint8 [B, 3, H, W] device images (``da_clip_preprocess``): Pillow's bicubic resize of the
    shorter side to R, centre crop, / 255, normalise.  out: kind 0 the patch matrix bf16 [B * ((R/P)**2 + 1), clip_patch_cols(P)]
    with zero class-token rows, kind 1 ``pixel_values`` fp32 [B, 3, R, R].  The integer tap tables come from
    ``metrics.clip_preprocess`` and are uploaded once per image size."""
    from .metrics.clip_preprocess import tables_for
    if not isinstance(images, torch.Tensor) or not images.is_cuda or images.dtype != torch.uint8 or images.dim() != 4 \
            or images.shape[1] != 3 or not images.is_contiguous() or images.shape[0] < 1:
        raise ValueError('clip_preprocess: images must be a contiguous uint8 [B, 3, H, W] device tensor')
    B, _, H, W = images.shape
    R, P = int(R), int(P)
    if not (1 <= P <= CLIP_MAX_PATCH and P <= R <= CLIP_MAX_SIZE and R % P == 0):
        raise ValueError(f'clip_preprocess: R = {R}, P = {P} (P <= {CLIP_MAX_PATCH}, R <= {CLIP_MAX_SIZE}, R % P == 0)')
    if not (1 <= H <= IMAGE_INGEST_MAX_SIDE and 1 <= W <= IMAGE_INGEST_MAX_SIDE):
        raise ValueError(f'clip_preprocess: image sides must be in 1..{IMAGE_INGEST_MAX_SIDE}')
    if kind not in (0, 1):
        raise ValueError(f'clip_preprocess: unknown out kind {kind!r} (0: bf16 patch matrix, 1: fp32 pixel_values)')
    dt, shape, align = ((BF16, (B * ((R // P) ** 2 + 1), clip_patch_cols(P)), 16), (F32, (B, 3, R, R), 4))[kind]
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != dt or not out.is_contiguous() \
            or tuple(out.shape) != shape or out.data_ptr() % align:
        raise ValueError(f'clip_preprocess: out must be a contiguous {dt} device tensor {shape}, {align}-byte aligned')
    key = (H, W, R, images.device)
    if key not in _CLIP_TABLES:
        _CLIP_TABLES[key] = tuple(torch.from_numpy(t.copy()).to(images.device) for t in tables_for(H, W, R))
    xtab, ytab = _CLIP_TABLES[key]
    f3 = ctypes.c_float * 3
    _lib.call('da_clip_preprocess', images.data_ptr(), B, H, W, R, P, xtab.data_ptr(), xtab.shape[1], ytab.data_ptr(),
              ytab.shape[1], f3(*map(float, mean)), f3(*map(float, std)), out.data_ptr(), int(kind), _stream())
    return out


def clip_score(img, txt, scores, state):
    """``da_clip_score``: scores[i] = 100 cos(img_i, txt_i); state[0] += their sum (index order), state[1] += B.  img / txt
    fp32 [B, D] device matrices with unit column stride (any row stride); scores fp32 [B]; state fp32 [2]."""
    for z, nm in ((img, 'img'), (txt, 'txt')):
        if z.dim() != 2 or z.dtype != F32 or not z.is_cuda or z.stride(1) != 1 or z.shape != img.shape:
            raise ValueError(f'clip_score: {nm} must be an fp32 [B, D] device matrix with unit column stride')
    B, D = img.shape
    if B < 1 or D < 1:
        raise ValueError('clip_score: empty batch')
    _lib.call('da_clip_score', img.data_ptr(), max(img.stride(0), D), txt.data_ptr(), max(txt.stride(0), D), B, D,
              _vec(scores, B, 'scores'), _vec(state, 2, 'state'), _stream())


INCEPTION_SIDE = 299   # da_inception_preprocess: the FID Inception's input side


def conv2d_tile_for(Cout: int) -> int:
    """the column tile (32 / 64 / 96) ``da_conv2d_relu_fwd`` picks for ``Cout``"""
    return int(_lib.load().da_conv2d_tile_for(int(Cout)))


def conv2d_relu_fwd(X, W, bias, Y, B, Hin, Win, kh, kw, stride=1, ph=0, pw=0, relu=True, tile_n=0):
    """``da_conv2d_relu_fwd``: Y[B*Hout*Wout, Cout] = act(conv(X[B*Hin*Win, Cin], W[Cout, kh*kw*Cin]) + bias).  X and Y are
    bf16 device matrices with unit column stride (column slices of wider buffers are fine), W contiguous bf16 in
    [Cout][kh][kw][Cin] order, bias fp32 [Cout] or None.  Returns (Hout, Wout)."""
    Cin, Cout = X.shape[1], Y.shape[1]
    if Hin + 2 * ph < kh or Win + 2 * pw < kw:
        raise ValueError(f'conv2d_relu_fwd: a {kh}x{kw} window does not fit {Hin}x{Win} padded by ({ph}, {pw})')
    Hout, Wout = (Hin + 2 * ph - kh) // stride + 1, (Win + 2 * pw - kw) // stride + 1
    if X.shape[0] != B * Hin * Win or Y.shape[0] != B * Hout * Wout:
        raise ValueError(f'conv2d_relu_fwd: X has {X.shape[0]} rows, Y {Y.shape[0]}; need {B * Hin * Win} and '
                         f'{B * Hout * Wout}')
    if W.dim() != 2 or W.dtype != BF16 or not W.is_cuda or not W.is_contiguous() or tuple(W.shape) != (Cout, kh * kw * Cin) \
            or W.data_ptr() % 16:
        raise ValueError(f'conv2d_relu_fwd: W must be contiguous bf16 [{Cout}, {kh * kw * Cin}] on the device, 16-byte aligned')
    px, ldx = _mat(X, name='X')
    py, ldy = _mat(Y, name='Y')
    pb = _vec(bias, Cout, 'bias')
    if pb % 16:
        raise ValueError('conv2d_relu_fwd: bias must be 16-byte aligned')
    with _Timed('conv_rect', 2.0 * B * Hout * Wout * Cout * kh * kw * Cin):
        _lib.call('da_conv2d_relu_fwd', px, ldx, W.data_ptr(), pb, py, ldy, B, Hin, Win, Hout, Wout, Cin, Cout, kh, kw,
                  int(stride), int(ph), int(pw), int(bool(relu)), int(tile_n), _stream())
    return Hout, Wout


def pool2d_fwd(X, Y, B, Hin, Win, stride, pad, kind):
    """``da_pool2d_fwd``: 3x3 max (kind 0) or average over the in-bounds taps (kind 1) of bf16 NHWC rows.  Returns
    (Hout, Wout)."""
    C = X.shape[1]
    if Hin + 2 * pad < 3 or Win + 2 * pad < 3:
        raise ValueError(f'pool2d_fwd: a 3x3 window does not fit {Hin}x{Win} padded by {pad}')
    Hout, Wout = (Hin + 2 * pad - 3) // stride + 1, (Win + 2 * pad - 3) // stride + 1
    if X.shape[0] != B * Hin * Win or tuple(Y.shape) != (B * Hout * Wout, C):
        raise ValueError(f'pool2d_fwd: X {tuple(X.shape)}, Y {tuple(Y.shape)}; need [{B * Hin * Win}, C] and '
                         f'[{B * Hout * Wout}, C]')
    px, ldx = _mat(X, name='X')
    py, ldy = _mat(Y, name='Y')
    _lib.call('da_pool2d_fwd', px, ldx, py, ldy, B, Hin, Win, Hout, Wout, C, int(stride), int(pad), int(kind), _stream())
    return Hout, Wout


def avgpool_global_f32(X, out, B, HW):
    """``da_avgpool_global_f32``: out[b, c] = mean over the HW rows of image b; X bf16 [B*HW, C], out fp32 [B, C]."""
    C = X.shape[1]
    if X.shape[0] != B * HW or out.dim() != 2 or tuple(out.shape) != (B, C) or out.dtype != F32 or not out.is_cuda \
            or out.stride(1) != 1:
        raise ValueError(f'avgpool_global_f32: X {tuple(X.shape)}, out {tuple(out.shape)} {out.dtype}')
    px, ldx = _mat(X, name='X')
    _lib.call('da_avgpool_global_f32', px, ldx, out.data_ptr(), max(out.stride(0), C), B, HW, C, _stream())
    return out


def inception_preprocess(images, out):
    """``da_inception_preprocess``: planar [B, 3, H, W] device images, uint8 levels or fp32 in [0, 1], through the TF1-style
    bilinear resize to 299 x 299 and (v - 128) / 128 into out bf16 [B * 299 * 299, 8] (channels 3..7 zero)."""
    if not isinstance(images, torch.Tensor) or not images.is_cuda or images.dtype not in (torch.uint8, F32) \
            or images.dim() != 4 or images.shape[1] != 3 or not images.is_contiguous() or images.shape[0] < 1:
        raise ValueError('inception_preprocess: images must be a contiguous uint8 or fp32 [B, 3, H, W] device tensor')
    B, _, H, W = images.shape
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError('inception_preprocess: image sides must be in 1..65535')
    n = B * INCEPTION_SIDE * INCEPTION_SIDE
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != BF16 or not out.is_contiguous() \
            or tuple(out.shape) != (n, 8) or out.data_ptr() % 16:
        raise ValueError(f'inception_preprocess: out must be a contiguous bf16 [{n}, 8] device tensor, 16-byte aligned')
    _lib.call('da_inception_preprocess', images.data_ptr(), int(images.dtype == F32), B, H, W, out.data_ptr(), _stream())
    return out


def feature_moments(F, fsum, cov, n):
    """``da_feature_moments``: fsum[d] += sum_b F[b, d], cov[d, e] += sum_b F[b, d] F[b, e], n[0] += B.  F fp32 [B, D] with
    unit column stride; fsum [D], cov [D, D], n [1]: contiguous float64 device tensors."""
    if F.dim() != 2 or F.dtype != F32 or not F.is_cuda or F.stride(1) != 1 or F.shape[0] < 1:
        raise ValueError('feature_moments: F must be an fp32 [B, D] device matrix with unit column stride')
    B, D = F.shape
    ldf = max(F.stride(0), D)
    if D % 8 or ldf % 4 or F.data_ptr() % 16:
        raise ValueError('feature_moments: D % 8 == 0, row stride % 4 == 0 and a 16-byte aligned base are required')
    for z, shape, nm in ((fsum, (D,), 'sum'), (cov, (D, D), 'cov'), (n, (1,), 'n')):
        if not isinstance(z, torch.Tensor) or z.dtype != torch.float64 or not z.is_cuda or not z.is_contiguous() \
                or tuple(z.shape) != shape:
            raise ValueError(f'feature_moments: {nm} must be a contiguous float64 device tensor {shape}')
    _lib.call('da_feature_moments', F.data_ptr(), ldf, B, D, fsum.data_ptr(), cov.data_ptr(), n.data_ptr(), _stream())


def _f32rows(x, name, cols=None):
    """an fp32 device matrix with unit column stride -> (rows, columns, row stride)"""
    if not isinstance(x, torch.Tensor) or x.dtype != F32:
        raise TypeError(f'{name}: need an fp32 tensor, got {x.dtype if isinstance(x, torch.Tensor) else type(x).__name__}')
    if x.dim() != 2 or not x.is_cuda or x.stride(1) != 1 or x.shape[0] < 1 or (cols is not None and x.shape[1] != cols):
        raise ValueError(f'{name}: need an fp32 [rows, {cols if cols is not None else "cols"}] device matrix with unit column '
                         f'stride, got {tuple(x.shape)} strides {x.stride()} on {x.device}')
    return x.shape[0], x.shape[1], max(x.stride(0), x.shape[1])


def fc_logits_f32(F, W, out):
    """``da_fc_logits_f32``: out[b, c] = sum_k F[b, k] W[c, k] in float64, rounded once to fp32 (no bias).  F fp32 [B, K] and
    out fp32 [B, C] with unit column stride (row strides free), W contiguous fp32 [C, K]; K % 4 == 0."""
    B, K, ldf = _f32rows(F, 'fc_logits_f32: F')
    C, _, _ = _f32rows(W, 'fc_logits_f32: W', K)
    _, _, ldo = _f32rows(out, 'fc_logits_f32: out', C)
    if out.shape[0] != B or not W.is_contiguous():
        raise ValueError(f'fc_logits_f32: F {tuple(F.shape)}, W {tuple(W.shape)} (contiguous), out {tuple(out.shape)}')
    if K % 4 or ldf % 4 or F.data_ptr() % 16 or W.data_ptr() % 16:
        raise ValueError('fc_logits_f32: K % 4 == 0, F row stride % 4 == 0 and 16-byte aligned F and W are required')
    _lib.call('da_fc_logits_f32', F.data_ptr(), ldf, W.data_ptr(), out.data_ptr(), ldo, B, K, C, _stream())
    return out


def _host_indices(idx, name):
    """the host copy of an index tensor: int32, on the CPU (the checks below read it without a device synchronisation)"""
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32:
        raise TypeError(f'{name}: need an int32 tensor, got {idx.dtype if isinstance(idx, torch.Tensor) else type(idx).__name__}')
    if idx.is_cuda:
        raise ValueError(f'{name}: pass the HOST tensor; it is range-checked here and uploaded afterwards')
    return idx.contiguous()


def inception_score(logits, perm, splits, scores=None):
    """``da_inception_score``: per-chunk Inception scores of rows ``perm`` of logits fp32 [N, C] (unit column stride, row
    stride free), chunked as ``torch.chunk(splits)`` does.  ``perm``: int32 [N] on the HOST; it must be a permutation of
    range(N) - checked here, before the upload, so that no out-of-range row reaches a launch.  Returns the float64 device
    vector of the chunks produced (a view of ``scores`` [splits] when that is given)."""
    N, C, ld = _f32rows(logits, 'inception_score: logits')
    perm = _host_indices(perm, 'inception_score: perm')
    if isinstance(splits, bool) or not isinstance(splits, int) or splits < 1:
        raise ValueError(f'inception_score: splits must be a positive int, got {splits!r}')
    if perm.dim() != 1 or perm.numel() != N or not torch.equal(perm.sort().values, torch.arange(N, dtype=torch.int32)):
        raise ValueError(f'inception_score: perm must be a permutation of range({N})')
    if not 1 <= C <= 4096:
        raise ValueError(f'inception_score: 1 <= C <= 4096, got {C}')
    if scores is None:
        scores = torch.empty(splits, device=logits.device, dtype=torch.float64)
    elif not isinstance(scores, torch.Tensor) or scores.dtype != torch.float64 or not scores.is_cuda \
            or not scores.is_contiguous() or tuple(scores.shape) != (splits,):
        raise ValueError(f'inception_score: scores must be a contiguous float64 device tensor [{splits}]')
    chunks = ctypes.c_int(0)
    dperm = perm.to(logits.device)
    _lib.call('da_inception_score', logits.data_ptr(), ld, dperm.data_ptr(), N, C, splits, scores.data_ptr(),
              ctypes.byref(chunks), _stream())
    return scores[:chunks.value]


def poly_mmd_workspace(subsets: int, m: int) -> int:
    """``da_poly_mmd_workspace``: float64 elements of workspace ``poly_mmd`` needs (0: the pair is rejected)"""
    return int(_lib.load().da_poly_mmd_workspace(int(subsets), int(m)))


def poly_mmd(Fr, Ff, idx_r, idx_f, degree=3, gamma=None, coef=1.0, out=None, ws=None):
    """``da_poly_mmd``: the polynomial-kernel MMD of torchmetrics' KID per subset.  Fr fp32 [Nr, D], Ff fp32 [Nf, D] (unit column
    stride, row stride % 4 == 0); idx_r, idx_f int32 [subsets, m] on the HOST, range-checked here before the upload;
    ``gamma=None`` is 1 / D.  Returns out, float64 [subsets] on the device."""
    Nr, D, ldr = _f32rows(Fr, 'poly_mmd: Fr')
    Nf, _, ldf = _f32rows(Ff, 'poly_mmd: Ff', D)
    idx_r, idx_f = _host_indices(idx_r, 'poly_mmd: idx_r'), _host_indices(idx_f, 'poly_mmd: idx_f')
    if idx_r.dim() != 2 or idx_r.shape != idx_f.shape or idx_r.shape[0] < 1:
        raise ValueError(f'poly_mmd: idx_r {tuple(idx_r.shape)} and idx_f {tuple(idx_f.shape)} must both be [subsets, m]')
    subsets, m = idx_r.shape
    for idx, n, nm in ((idx_r, Nr, 'idx_r'), (idx_f, Nf, 'idx_f')):
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
            raise ValueError(f'poly_mmd: {nm} must lie in [0, {n})')
    if isinstance(degree, bool) or not isinstance(degree, int) or not 1 <= degree <= 8:
        raise ValueError(f'poly_mmd: degree must be an int in 1..8, got {degree!r}')
    gamma = 1.0 / D if gamma is None else float(gamma)
    coef = float(coef)
    need = poly_mmd_workspace(subsets, m)
    if m < 2 or need == 0:
        raise ValueError(f'poly_mmd: need 2 <= m <= 65536 and subsets <= 65535, got m = {m}, subsets = {subsets}')
    if not (0.0 < gamma < float('inf')) or not (0.0 <= coef < float('inf')):
        raise ValueError(f'poly_mmd: gamma must be > 0 and coef >= 0, got {gamma}, {coef}')
    if D % 4 or ldr % 4 or ldf % 4 or Fr.data_ptr() % 16 or Ff.data_ptr() % 16:
        raise ValueError('poly_mmd: D % 4 == 0, row strides % 4 == 0 and 16-byte aligned stores are required')
    f64 = dict(device=Fr.device, dtype=torch.float64)
    if out is None:
        out = torch.empty(subsets, **f64)
    if ws is None:
        ws = torch.empty(need, **f64)
    for z, nm, n, exact in ((out, 'out', subsets, True), (ws, 'ws', need, False)):
        if not isinstance(z, torch.Tensor) or z.dtype != torch.float64 or not z.is_cuda or not z.is_contiguous() \
                or z.dim() != 1 or z.numel() < n or (exact and z.numel() != n):
            raise ValueError(f'poly_mmd: {nm} must be a contiguous float64 device vector of {"" if exact else ">= "}{n}')
    dr, df = idx_r.to(Fr.device), idx_f.to(Fr.device)
    _lib.call('da_poly_mmd', Fr.data_ptr(), ldr, Nr, Ff.data_ptr(), ldf, Nf, dr.data_ptr(), df.data_ptr(), subsets, m, D,
              degree, gamma, coef, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return out


def _rescale_operands(fn, factor, HW, npix):
    """``factor=`` / ``HW=`` of the four step wrappers (guidance rescale): the sample's pixel count, checked."""
    if HW is None or int(HW) < 1 or npix % int(HW):
        raise ValueError(f'{fn}: factor needs HW, the pixel count of one sample, dividing npix = {npix}; got {HW}')
    if factor.dtype != F32 or not factor.is_cuda or not factor.is_contiguous() or factor.numel() != npix // int(HW):
        raise ValueError(f'{fn}: factor must be a contiguous fp32 [{npix // int(HW)}] device tensor')
    return int(HW)


def guidance_rescale(pred, coef, factor, *, phi, HW, C, g_index):
    """The statistics pass of guidance rescale (``da_guidance_rescale``): factor[b] = phi std(pt) / std(m) + 1 - phi per
    sample, with m = pu + g (pt - pu) and g = coef[g_index] read on the device (3: the ``sampler_step`` rows, 5: the
    ``sampler_step_ms`` rows).  pred fp32 [2 npix, 8] (both guidance halves); factor fp32 [npix / HW]; phi in [0, 1]."""
    C, HW, g_index, phi = int(C), int(HW), int(g_index), float(phi)
    if not 1 <= C <= 8 or HW < 1 or not 0.0 <= phi <= 1.0:
        raise ValueError(f'guidance_rescale: C = {C} (1..8), HW = {HW} (>= 1), phi = {phi} (in [0, 1])')
    if pred.dim() != 2 or pred.shape[1] != 8 or pred.dtype != F32 or not pred.is_cuda or not pred.is_contiguous() \
            or pred.shape[0] < 2 or pred.shape[0] % (2 * HW) or pred.data_ptr() % 16:
        raise ValueError(f'guidance_rescale: pred must be a contiguous fp32 [2 B * {HW}, 8] device tensor, 16-byte aligned')
    npix = pred.shape[0] // 2
    if coef.dtype != F32 or not coef.is_cuda or not coef.is_contiguous() or coef.numel() not in (4, 8, 12) \
            or coef.data_ptr() % 16 or not 0 <= g_index < min(coef.numel(), 8):
        raise ValueError('guidance_rescale: coef must be 4, 8 or 12 contiguous fp32 on the device, 16-byte aligned, g_index inside')
    _rescale_operands('guidance_rescale', factor, HW, npix)
    _lib.call('da_guidance_rescale', pred.data_ptr(), coef.data_ptr(), g_index, phi, factor.data_ptr(), npix, HW, C,
              _stream())


def _sampler_step(ms, blend, pred, x, coef, x_out, xt_out, C, cfg, copies, factor, HW, *, noise=None, hist=None, known8=None,
                  eps8=None, mask=None, seeds=None):
    """The four step wrappers behind their signatures: the form is (``ms``: two-step, with ``hist`` and no ``noise``;
    ``blend``: masked, with ``known8`` / ``eps8`` / ``mask``), the checks are stated once and raise under the wrapper's name,
    and the call goes to that form's symbol, its ``_rs`` twin when ``factor`` is given.  With ``seeds`` (``sampler_step_rng``)
    the row is the wider one, there is no ``noise`` operand and the call goes to ``da_sampler_step_rng`` with the form as a
    mask."""
    rng = seeds is not None
    fn = 'sampler_step_rng' if rng else 'sampler_step' + ('_ms' if ms else '') + ('_blend' if blend else '')
    C, copies, cfg = int(C), int(copies), bool(cfg)
    if not 1 <= C <= 8 or copies not in (1, 2):
        raise ValueError(f'{fn}: C = {C} (1..8), copies = {copies} (1 or 2)')
    if x.dim() != 2 or x.shape[1] != 8 or x.shape[0] < 1:
        raise ValueError(f'{fn}: x must be [npix, 8]')
    npix = x.shape[0]
    mats = [(pred, (2 if cfg else 1) * npix, 'pred'), (x, npix, 'x')] + ([(hist, npix, 'hist')] if ms else []) \
        + [(x_out, npix, 'x_out')] + ([(known8, npix, 'known8'), (eps8, npix, 'eps8')] if blend else [])
    for z, rows, nm in mats:
        if z.dtype != F32 or not z.is_cuda or not z.is_contiguous() or tuple(z.shape) != (rows, 8) or z.data_ptr() % 16:
            raise ValueError(f'{fn}: {nm} must be a contiguous fp32 [{rows}, 8] device tensor, 16-byte aligned')
    if blend and (mask.dtype != F32 or not mask.is_cuda or not mask.is_contiguous() or tuple(mask.shape) != (npix,)
                  or mask.data_ptr() % 16):
        raise ValueError(f'{fn}: mask must be a contiguous fp32 [{npix}] device tensor, 16-byte aligned')
    # hist is written while the others are still being read
    if ms and hist.data_ptr() in [z.data_ptr() for z in (x, x_out, pred) + ((known8, eps8) if blend else ())]:
        raise ValueError(f'{fn}: hist must be a buffer of its own')
    ncoef = (12 if ms else 8) if rng else 8 if ms or blend else 4
    if coef.dtype != F32 or not coef.is_cuda or not coef.is_contiguous() or coef.numel() != ncoef or coef.data_ptr() % 16:
        raise ValueError(f'{fn}: coef must be {ncoef} contiguous fp32 on the device, 16-byte aligned')
    HW_arg, HW = HW, npix
    if noise is not None:
        if noise.dim() != 4 or noise.dtype != F32 or not noise.is_cuda or not noise.is_contiguous() \
                or noise.shape[1] != C or noise.shape[0] * noise.shape[2] * noise.shape[3] != npix or noise.data_ptr() % 16:
            raise ValueError(f'{fn}: noise must be a contiguous fp32 [B, {C}, H, W] device tensor over {npix} pixels')
        HW = noise.shape[2] * noise.shape[3]
    if xt_out is not None and (xt_out.dtype != BF16 or not xt_out.is_cuda or not xt_out.is_contiguous()
                               or tuple(xt_out.shape) != (copies * npix, 8) or xt_out.data_ptr() % 16):
        raise ValueError(f'{fn}: xt_out must be a contiguous bf16 [{copies * npix}, 8] device tensor')
    if factor is not None:
        if _rescale_operands(fn, factor, HW_arg, npix) != HW and noise is not None:
            raise ValueError(f'{fn}: HW = {HW_arg} is not the noise draw\'s {HW} pixels per sample')
        HW = int(HW_arg)
    ptr = lambda z: z.data_ptr() if z is not None else None  # noqa: E731
    if rng:
        if HW_arg is None or int(HW_arg) < 1 or npix % int(HW_arg):
            raise ValueError(f'{fn}: HW, the pixel count of one sample, must divide npix = {npix}; got {HW_arg}')
        HW = int(HW_arg)
        if not isinstance(seeds, torch.Tensor) or seeds.dtype != torch.uint64 or not seeds.is_cuda \
                or not seeds.is_contiguous() or tuple(seeds.shape) != (npix // HW,) or seeds.data_ptr() % 8:
            raise ValueError(f'{fn}: seeds must be a contiguous uint64 [{npix // HW}] device tensor')
        _lib.call('da_sampler_step_rng', ptr(pred), ptr(x), ptr(hist if ms else None), ptr(coef),
                  *((ptr(known8), ptr(eps8), ptr(mask)) if blend else (None, None, None)), ptr(factor), ptr(seeds),
                  ptr(x_out), ptr(xt_out), npix, HW, C, (1 if ms else 0) | (2 if blend else 0) | (4 if factor is not None else 0),
                  int(cfg), copies, _stream())
        return
    _lib.call('da_' + fn + ('_rs' if factor is not None else ''), ptr(pred), ptr(x), ptr(hist if ms else noise), ptr(coef),
              *((ptr(known8), ptr(eps8), ptr(mask)) if blend else ()), *((ptr(factor),) if factor is not None else ()),
              ptr(x_out), ptr(xt_out), npix, HW, C, int(cfg), copies, _stream())


def sampler_step(pred, x, coef, x_out, xt_out=None, noise=None, *, C, cfg, copies=1, factor=None, HW=None):
    """One sampling step after the U-Net call (``da_sampler_step``): guidance, the scheduler update with the device
    coefficients ``coef`` = {cx, cm, cn, guidance} and the next U-Net input.  With ``factor`` (fp32 [npix / HW], what
    ``guidance_rescale`` wrote; ``HW`` the pixel count of one sample) the guided prediction of sample b is multiplied by
    factor[b] first (``da_sampler_step_rs``); the other three step wrappers take the same two keywords.

    pred fp32 [(2 if cfg else 1) * npix, 8]; x / x_out fp32 [npix, 8] (x_out may be x); noise None or fp32 NCHW
    [B, C, H, W] with B * H * W = npix; xt_out None or bf16 [copies * npix, 8]."""
    _sampler_step(False, False, pred, x, coef, x_out, xt_out, C, cfg, copies, factor, HW, noise=noise)


def sampler_step_ms(pred, x, hist, coef, x_out, xt_out=None, *, C, cfg, copies=1, factor=None, HW=None):
    """One sampling step of a two-step scheduler after the U-Net call (``da_sampler_step_ms``): guidance, the data
    prediction, the update with the previous step's data prediction and the next U-Net input.  ``coef`` = {ax, am, kx, k0,
    k1, guidance, 0, 0} on the device (``DPMSolverMultistepScheduler.step_coefficients_ms``).

    pred fp32 [(2 if cfg else 1) * npix, 8]; x / x_out / hist fp32 [npix, 8] (x_out may be x; hist is read iff k1 != 0 and
    then overwritten with this step's data prediction); xt_out None or bf16 [copies * npix, 8]."""
    _sampler_step(True, False, pred, x, coef, x_out, xt_out, C, cfg, copies, factor, HW, hist=hist)


def sampler_step_blend(pred, x, coef, known8, eps8, mask, x_out, xt_out=None, noise=None, *, C, cfg, copies=1, factor=None,
                       HW=None):
    """``sampler_step`` for a masked sample (``da_sampler_step_blend``): with v what ``sampler_step`` stores and m the pixel's
    mask value, x_out = m v + (1 - m) (bA known8 + bS eps8).  ``coef`` = {cx, cm, cn, guidance, bA, bS, 0, 0} on the device.

    known8 / eps8 fp32 [npix, 8] and mask fp32 [npix] (what ``sampler_init`` writes); the rest as in ``sampler_step``."""
    _sampler_step(False, True, pred, x, coef, x_out, xt_out, C, cfg, copies, factor, HW, noise=noise, known8=known8, eps8=eps8,
                  mask=mask)


def sampler_step_ms_blend(pred, x, hist, coef, known8, eps8, mask, x_out, xt_out=None, *, C, cfg, copies=1, factor=None,
                          HW=None):
    """``sampler_step_ms`` for a masked sample (``da_sampler_step_ms_blend``): the same blend after the two-step update;
    ``hist`` receives the unblended data prediction.  ``coef`` = {ax, am, kx, k0, k1, guidance, bA, bS} on the device."""
    _sampler_step(True, True, pred, x, coef, x_out, xt_out, C, cfg, copies, factor, HW, hist=hist, known8=known8, eps8=eps8,
                  mask=mask)


def sampler_step_rng(pred, x, coef, seeds, x_out, xt_out=None, *, HW, C, cfg, copies=1, hist=None, known8=None, eps8=None,
                     mask=None, factor=None):
    """The stochastic step (``da_sampler_step_rng``): any form of the step with its noise term drawn inside the kernel from
    the per-image Philox streams of ``seeds`` (uint64 [npix / HW] on the device).  The form follows the operands: ``hist``
    makes it two-step, ``known8`` / ``eps8`` / ``mask`` blended, ``factor`` rescaled.  ``coef`` on the device is
    {cx, cm, cn, guidance, bA, bS, draw, 0} (first order) or {ax, am, kx, k0, k1, guidance, bA, bS, kn, draw, 0, 0}
    (two-step), ``draw`` a uint32 bit pattern (``stochastic_rows`` of ``sampling`` writes it through an int32 view).  With
    z = ``randn_philox(seeds, draw, 0, ...)`` the first-order forms give the bits of the deterministic wrapper fed z as
    ``noise``; a zero noise coefficient draws nothing."""
    ms, blend = hist is not None, mask is not None or known8 is not None or eps8 is not None
    if blend and (mask is None or known8 is None or eps8 is None):
        raise ValueError('sampler_step_rng: known8, eps8 and mask go together')
    if seeds is None:
        raise ValueError('sampler_step_rng: seeds is required')
    _sampler_step(ms, blend, pred, x, coef, x_out, xt_out, C, cfg, copies, factor, HW, hist=hist, known8=known8, eps8=eps8,
                  mask=mask, seeds=seeds)


def philox_seeds(seeds, B=None, device=None):
    """``seeds`` (a sequence or tensor of integers in [0, 2^64)) as the uint64 device tensor the Philox entries read; with
    ``B`` its length is checked.  ``ValueError`` for anything else, raised before the upload."""
    if isinstance(seeds, torch.Tensor):
        if seeds.dtype == torch.uint64 and (B is None or seeds.numel() == B) and seeds.dim() == 1:
            return seeds.to(device).contiguous() if device is not None else seeds.contiguous()
        seeds = seeds.tolist()
    try:
        vals = list(seeds)
    except TypeError:
        raise ValueError(f'seeds must be a sequence of integers, got {seeds!r}') from None
    import numbers
    if isinstance(seeds, (str, bytes)) or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in vals) \
            or any(not 0 <= int(v) < 2**64 for v in vals) or (B is not None and len(vals) != B):
        raise ValueError(f'seeds must be {B if B is not None else "a sequence of"} integers in [0, 2^64), got {seeds!r}')
    # through int64 bit patterns: torch builds no uint64 tensor from Python ints above 2^63 - 1
    t = torch.tensor([v - 2**64 if v >= 2**63 else v for v in map(int, vals)], dtype=torch.int64).view(torch.uint64)
    return t.to(device) if device is not None else t


def randn_philox(seeds, draw, stream, shape=None, *, out=None, kind=0):
    """Per-image counter-based normals (``da_randn_philox``), the unfused form of the step kernels' draw: fp32 NCHW
    [B, C, H, W] where image b's values depend on (seeds[b], draw, stream, pixel, channel) only.  ``seeds`` uint64 [B] on the
    device; ``draw`` in [0, 2^32); ``stream`` 0 (step noise) or 1 (initial latents); ``kind`` 1 writes the raw Philox words
    as bit patterns (C % 4 == 0).  Returns ``out`` (allocated with ``shape`` when not given)."""
    if out is None:
        if shape is None or len(shape) != 4:
            raise ValueError('randn_philox: shape must be (B, C, H, W)')
        out = torch.empty(tuple(int(v) for v in shape), device=seeds.device, dtype=F32)
    if out.dim() != 4 or out.dtype != F32 or not out.is_cuda or not out.is_contiguous() or out.data_ptr() % 16 \
            or out.numel() < 1 or not 1 <= out.shape[1] <= 8:
        raise ValueError('randn_philox: out must be a contiguous fp32 [B, C, H, W] device tensor with C in 1..8')
    B, C, H, W = out.shape
    draw, stream, kind = int(draw), int(stream), int(kind)
    if not 0 <= draw < 2**32 or stream not in (0, 1) or kind not in (0, 1) or (kind == 1 and C % 4) or H * W > 2**31 - 1:
        raise ValueError(f'randn_philox: draw = {draw} (uint32), stream = {stream} (0 or 1), kind = {kind} (0, or 1 with C % 4 == 0)')
    if not isinstance(seeds, torch.Tensor) or seeds.dtype != torch.uint64 or not seeds.is_cuda or not seeds.is_contiguous() \
            or tuple(seeds.shape) != (B,) or seeds.data_ptr() % 8:
        raise ValueError(f'randn_philox: seeds must be a contiguous uint64 [{B}] device tensor')
    _lib.call('da_randn_philox', seeds.data_ptr(), draw, stream, out.data_ptr(), B, C, H, W, kind, _stream())
    return out


def sampler_init(known, noise, coef, x, xt=None, *, known8=None, eps8=None, mask_px=None, mask=None, copies=1):
    """The start of a sample that begins from an image (``da_sampler_init``): x = a0 known + s0 noise in NHWC-8 with its bf16
    copies, and for a masked sample the NHWC-8 relayouts of both operands and the mask's f x f box mean.

    known / noise fp32 NCHW [B, C, H, W]; coef = {a0, s0, 0, 0} on the device; x fp32 [B H W, 8]; xt None or bf16
    [copies * B H W, 8]; known8 / eps8 None (both) or fp32 [B H W, 8]; mask_px None or fp32 [B, f H, f W] with f a power of
    two in 1..16, and mask fp32 [B H W] given iff mask_px is."""
    copies = int(copies)
    if known.dim() != 4 or not 1 <= known.shape[1] <= 8 or known.numel() < 1 or copies not in (1, 2):
        raise ValueError(f'sampler_init: known must be [B, C, H, W] with C in 1..8, copies = {copies} (1 or 2)')
    B, C, H, W = known.shape
    npix = B * H * W
    for z, nm in ((known, 'known'), (noise, 'noise')):
        if z.dtype != F32 or not z.is_cuda or not z.is_contiguous() or z.shape != known.shape or z.data_ptr() % 16:
            raise ValueError(f'sampler_init: {nm} must be a contiguous fp32 {tuple(known.shape)} device tensor, 16-byte aligned')
    if coef.dtype != F32 or not coef.is_cuda or not coef.is_contiguous() or coef.numel() != 4 or coef.data_ptr() % 16:
        raise ValueError('sampler_init: coef must be 4 contiguous fp32 on the device, 16-byte aligned')
    if (known8 is None) != (eps8 is None) or (mask_px is None) != (mask is None):
        raise ValueError('sampler_init: known8 goes with eps8, mask_px with mask')
    for z, nm in ((x, 'x'), (known8, 'known8'), (eps8, 'eps8')):
        if z is not None and (z.dtype != F32 or not z.is_cuda or not z.is_contiguous() or tuple(z.shape) != (npix, 8)
                              or z.data_ptr() % 16):
            raise ValueError(f'sampler_init: {nm} must be a contiguous fp32 [{npix}, 8] device tensor, 16-byte aligned')
    if xt is not None and (xt.dtype != BF16 or not xt.is_cuda or not xt.is_contiguous()
                           or tuple(xt.shape) != (copies * npix, 8) or xt.data_ptr() % 16):
        raise ValueError(f'sampler_init: xt must be a contiguous bf16 [{copies * npix}, 8] device tensor')
    f = 1
    if mask_px is not None:
        f = mask_factor(tuple(mask_px.shape), B, H, W, 'sampler_init')
        if mask_px.dtype != F32 or not mask_px.is_cuda or not mask_px.is_contiguous() or mask_px.data_ptr() % 16:
            raise ValueError(f'sampler_init: mask_px must be a contiguous fp32 [{B}, f {H}, f {W}] device tensor, 16-byte aligned')
        if mask.dtype != F32 or not mask.is_cuda or not mask.is_contiguous() or tuple(mask.shape) != (npix,) \
                or mask.data_ptr() % 16:
            raise ValueError(f'sampler_init: mask must be a contiguous fp32 [{npix}] device tensor, 16-byte aligned')
    _lib.call('da_sampler_init', known.data_ptr(), noise.data_ptr(), mask_px.data_ptr() if mask_px is not None else None,
              coef.data_ptr(), known8.data_ptr() if known8 is not None else None,
              eps8.data_ptr() if eps8 is not None else None, mask.data_ptr() if mask is not None else None, x.data_ptr(),
              xt.data_ptr() if xt is not None else None, B, H, W, C, f, copies, _stream())


def mask_factor(shape, B, H, W, who='mask_px'):
    """f of a pixel mask [B, f H, f W] over a [B, ., H, W] state: a power of two in 1..16 (``ValueError`` otherwise)."""
    if len(shape) != 3 or shape[0] != B or H < 1 or W < 1 or shape[1] % H or shape[2] % W or shape[1] // H != shape[2] // W \
            or shape[1] // H not in (1, 2, 4, 8, 16):
        raise ValueError(f'{who}: mask_px must be [{B}, f * {H}, f * {W}] with f a power of two in 1..16, got {tuple(shape)}')
    return shape[1] // H


def add_noise(x0, eps, t, sqrt_ac, sqrt_1mac, xt, target, v_pred):
    B = x0.shape[0]
    HW = x0.shape[2] * x0.shape[3]
    for z in (x0, eps):
        if z.dtype != F32 or not z.is_contiguous() or z.shape[1] != 4 or z.shape != x0.shape:
            raise ValueError('add_noise: x0/eps must be contiguous fp32 [B,4,H,W]')
    if xt.dtype != BF16 or xt.numel() != B * HW * 8 or target.dtype != F32 or target.numel() != B * HW * 8:
        raise ValueError('add_noise: xt bf16 [B*HW,8], target fp32 [B*HW,8]')
    if int(sqrt_ac.numel()) != int(sqrt_1mac.numel()):
        raise ValueError('add_noise: table mismatch')
    _lib.call('da_add_noise', x0.data_ptr(), eps.data_ptr(), t.data_ptr(), sqrt_ac.data_ptr(), sqrt_1mac.data_ptr(),
              xt.data_ptr(), target.data_ptr(), B, HW, int(v_pred), _stream())


def mse_loss(pred, target, dpred, loss, scratch, total_pix, grad_coef, weight, accumulate):
    if pred.dtype != F32 or target.dtype != F32 or dpred.dtype != BF16:
        raise ValueError('mse_loss: dtypes')
    if pred.numel() != total_pix * 8 or target.numel() != total_pix * 8 or dpred.numel() != total_pix * 8:
        raise ValueError('mse_loss: sizes')
    _lib.call('da_mse_loss', pred.data_ptr(), target.data_ptr(), dpred.data_ptr(), loss.data_ptr(),
              _f32buf(scratch, 1024), total_pix, float(grad_coef), float(weight), int(accumulate), _stream())


def mse_loss_c(pred, target, dpred, loss, scratch, total_pix, C, grad_coef, weight, accumulate):
    """``mse_loss`` over the first C (1..8) channels of NHWC(8) tensors; dpred is 0 in the pad channels."""
    for z, dt in ((pred, F32), (target, F32), (dpred, BF16)):
        if z.dtype != dt or not z.is_cuda or not z.is_contiguous() or z.numel() != total_pix * 8 or z.data_ptr() % 16:
            raise ValueError('mse_loss_c: pred / target fp32 and dpred bf16, contiguous [total_pix, 8] on device')
    if loss.dtype != F32 or not loss.is_cuda or not 1 <= int(C) <= 8:
        raise ValueError('mse_loss_c: loss fp32 on device, 1 <= C <= 8')
    _lib.call('da_mse_loss_c', pred.data_ptr(), target.data_ptr(), dpred.data_ptr(), loss.data_ptr(),
              _f32buf(scratch, 1024), total_pix, int(C), float(grad_coef), float(weight), int(accumulate), _stream())


def mse_loss_w(pred, target, dpred, loss, scratch, total_pix, C, HW, t, wtab, grad_coef, weight, accumulate):
    """``mse_loss_c`` with a weight per sample (``da_mse_loss_w``): sample b = pixel // HW weighs wtab[t[b]] in the loss and
    in dpred.  t int64 [total_pix / HW] and wtab fp32 [T] on the device; a timestep outside the table is clamped into it."""
    for z, dt in ((pred, F32), (target, F32), (dpred, BF16)):
        if z.dtype != dt or not z.is_cuda or not z.is_contiguous() or z.numel() != total_pix * 8 or z.data_ptr() % 16:
            raise ValueError('mse_loss_w: pred / target fp32 and dpred bf16, contiguous [total_pix, 8] on device')
    if loss.dtype != F32 or not loss.is_cuda or not 1 <= int(C) <= 8:
        raise ValueError('mse_loss_w: loss fp32 on device, 1 <= C <= 8')
    HW = int(HW)
    if HW < 1 or total_pix < 1 or total_pix % HW:
        raise ValueError(f'mse_loss_w: total_pix = {total_pix} must be a positive multiple of HW = {HW}')
    if t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous() or t.numel() != total_pix // HW:
        raise ValueError(f'mse_loss_w: t must be a contiguous int64 [{total_pix // HW}] device tensor')
    if wtab.dtype != F32 or not wtab.is_cuda or not wtab.is_contiguous() or wtab.dim() != 1 or wtab.numel() < 1:
        raise ValueError('mse_loss_w: wtab must be a contiguous fp32 [T] device tensor')
    _lib.call('da_mse_loss_w', pred.data_ptr(), target.data_ptr(), dpred.data_ptr(), loss.data_ptr(), _f32buf(scratch, 1024),
              total_pix, int(C), HW, t.data_ptr(), wtab.data_ptr(), int(wtab.numel()), float(grad_coef), float(weight),
              int(accumulate), _stream())


def adamw(p, g, m, v, shadow, lr, beta1, beta2, eps, wd, step, grad_scale, ema=None, ema_smoothing=0.0):
    n = p.numel()
    for z in (p, g, m, v):
        if z.dtype != F32 or not z.is_contiguous() or z.numel() != n:
            raise ValueError('adamw: fp32 contiguous flat buffers of equal size required')
    if shadow.dtype != BF16 or shadow.numel() != n:
        raise ValueError('adamw: shadow')
    if ema is not None and (ema.dtype != F32 or not ema.is_contiguous() or ema.numel() != n):
        raise ValueError('adamw: ema buffer')
    _lib.call('da_adamw', p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), shadow.data_ptr(),
              ema.data_ptr() if ema is not None else 0, float(ema_smoothing), n, float(lr),
              float(beta1), float(beta2), float(eps), float(wd), int(step), float(grad_scale), _stream())


GRAD_STATS_WORDS = 8   # struct DaGradStats: fp32 sumsq, norm, grad_mult, finite; int32 skipped_steps; 3 reserved


def segment_sumsq_scratch_floats(n_chunks: int) -> int:
    return int(_lib.load().da_segment_sumsq_scratch_floats(int(n_chunks)))


def segment_sumsq(x, tables, chunk_partials, seg_sumsq, stats=None, grad_scale=1.0, max_norm=0.0):
    """Sum of squares of every segment of the flat fp32 buffer ``x`` (tables: models.unet.SumsqTables on the device) into
    ``seg_sumsq`` [n_segs], and into ``stats`` (fp32[8], struct DaGradStats) the total, the global norm times grad_scale, the
    gradient multiplier of torch's clip_grad_norm_ rule and the finite flag.  Enqueued on the current stream, no sync."""
    nc, ns = len(tables.chunks), len(tables.segs)
    if tables.chunk_desc is None or not tables.chunk_desc.is_cuda:
        raise ValueError('segment_sumsq: tables not on the device (SumsqTables.to(device))')
    if x.dtype != F32 or not x.is_contiguous() or not x.is_cuda or x.numel() < tables.extent:
        raise ValueError(f'segment_sumsq: x must be a contiguous fp32 device buffer of >= {tables.extent} elements')
    if seg_sumsq.dtype != F32 or not seg_sumsq.is_contiguous() or seg_sumsq.numel() < ns or not seg_sumsq.is_cuda:
        raise ValueError(f'segment_sumsq: seg_sumsq must be contiguous fp32[>= {ns}] on the device')
    if stats is not None and (stats.dtype != F32 or not stats.is_contiguous() or stats.numel() < GRAD_STATS_WORDS or not stats.is_cuda):
        raise ValueError(f'segment_sumsq: stats must be contiguous fp32[{GRAD_STATS_WORDS}] on the device')
    _lib.call('da_segment_sumsq', x.data_ptr(), tables.chunk_desc.data_ptr(), nc, tables.seg_desc.data_ptr(), ns,
              _f32buf(chunk_partials, segment_sumsq_scratch_floats(nc), 'chunk_partials'), seg_sumsq.data_ptr(),
              stats.data_ptr() if stats is not None else 0, float(grad_scale), float(max_norm), _stream())


def adamw_dev(p, g, m, v, shadow, lr, beta1, beta2, eps, wd, step, stats, ema=None, ema_smoothing=0.0):
    """``adamw`` with the gradient multiplier read from ``stats[2]`` on the device; when ``stats[3] == 0`` (a non-finite
    gradient) the kernel writes nothing.  ``step`` is the host's step number either way."""
    n = p.numel()
    for z in (p, g, m, v):
        if z.dtype != F32 or not z.is_contiguous() or z.numel() != n:
            raise ValueError('adamw_dev: fp32 contiguous flat buffers of equal size required')
    if shadow.dtype != BF16 or shadow.numel() != n:
        raise ValueError('adamw_dev: shadow')
    if ema is not None and (ema.dtype != F32 or not ema.is_contiguous() or ema.numel() != n):
        raise ValueError('adamw_dev: ema buffer')
    if stats.dtype != F32 or not stats.is_contiguous() or stats.numel() < GRAD_STATS_WORDS or not stats.is_cuda:
        raise ValueError(f'adamw_dev: stats must be contiguous fp32[{GRAD_STATS_WORDS}] on the device')
    _lib.call('da_adamw_dev', p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), shadow.data_ptr(),
              ema.data_ptr() if ema is not None else 0, float(ema_smoothing), n, float(lr),
              float(beta1), float(beta2), float(eps), float(wd), int(step), stats.data_ptr(), _stream())


def cast_f32_bf16(src, dst):
    if src.dtype != F32 or dst.dtype != BF16 or src.numel() != dst.numel() or not src.is_contiguous():
        raise ValueError('cast: bad args')
    _lib.call('da_cast_f32_bf16', src.data_ptr(), dst.data_ptr(), src.numel(), _stream())


def transpose_weight(src, dst, N, T, C):
    if src.dtype != BF16 or dst.dtype != BF16 or src.numel() != N * T * C or dst.numel() != N * T * C:
        raise ValueError('transpose_weight: bad args')
    _lib.call('da_transpose_weight', src.data_ptr(), dst.data_ptr(), N, T, C, _stream())


def transpose_weights_batched(src_base, dst_base, desc, ntensors, total_blocks):
    if src_base.dtype != BF16 or dst_base.dtype != BF16 or desc.dtype != torch.uint8 or not desc.is_cuda:
        raise ValueError('transpose_weights_batched: bad args')
    _lib.call('da_transpose_weights_batched', src_base.data_ptr(), dst_base.data_ptr(), desc.data_ptr(), int(ntensors),
              int(total_blocks), _stream())


def _lora_check(name, adapters, *bufs):
    if adapters.table is None or not adapters.table.is_cuda:
        raise ValueError(f'{name}: the adapter layout is not on the device (LoRAAdapters.to(device))')
    for z, n, what in bufs:
        if z.dtype != F32 or not z.is_cuda or not z.is_contiguous() or z.numel() < n:
            raise ValueError(f'{name}: {what} must be a contiguous fp32 device buffer of >= {n} elements')


def lora_merge(master, adapters, shadow, vout=None):
    """shadow = bf16(master + s B A) on the row ranges of ``adapters`` (diffusion_amd.lora.LoRAAdapters on the device), one
    launch; ``vout`` (fp32, may be ``master``) receives the unrounded value.  Follow it with refresh_transposed()."""
    _lora_check('lora_merge', adapters, (master, adapters.master_extent, 'master'), (adapters.params, adapters.total, 'params'))
    if shadow.dtype != BF16 or not shadow.is_cuda or not shadow.is_contiguous() or shadow.numel() < adapters.master_extent:
        raise ValueError('lora_merge: shadow must be a contiguous bf16 device buffer as long as the master')
    if vout is not None:
        _lora_check('lora_merge', adapters, (vout, adapters.master_extent, 'vout'))
    _lib.call('da_lora_merge', master.data_ptr(), adapters.params.data_ptr(), adapters.table.data_ptr(), len(adapters.items),
              adapters.tiles()[0], shadow.data_ptr(), vout.data_ptr() if vout is not None else 0, _stream())


def lora_project(grad, adapters):
    """adapters.grad <- (dA = s B^T dW, dB = s dW A^T) of every item from the dense weight gradient in ``grad``: one launch
    that overwrites the adapter gradient buffer, every sum in a fixed order."""
    _lora_check('lora_project', adapters, (grad, adapters.master_extent, 'grad'), (adapters.params, adapters.total, 'params'),
                (adapters.grad, adapters.total, 'adapter grad'))
    _, da, db = adapters.tiles()
    _lib.call('da_lora_project', grad.data_ptr(), adapters.params.data_ptr(), adapters.table.data_ptr(),
              len(adapters.items), da, db, adapters.grad.data_ptr(), _stream())
