"""da_lora_merge and da_lora_project on the MI355X against float64, on raw item tables (tests/lora_reference.py).

Shapes: a ragged small matrix (40 x 32), one square (320 x 320), a 3x3-convolution shape (256 x 9*64), a fused qkv storage
(3*128 x 128) adapted as three row-range items and a fused kv storage (2*320 x 128) as two - all in ONE launch, at offsets
that are no multiple of a tile, with an untouched storage between them; ranks 1, 3, 4, 16, 128 (odd, below / at / above the
32-wide LDS chunk).  The bounds are derived, not measured: bf16 half-ulp plus the fp32 chain for the merge, the fp32 fmaf
chain for the projection.  One further test puts the item at the end of a 0.6 G-float buffer, where byte offsets cross 2 GiB.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import lora_reference as lr  # noqa: E402

pytestmark = pytest.mark.gpu

RANKS = (1, 3, 4, 16, 128)
# (rows of the storage, K, row ranges adapted)
STORAGES = [(40, 32, [(0, 40)]), (320, 320, [(0, 320)]), (96, 64, []), (256, 9 * 64, [(0, 256)]),
            (3 * 128, 128, [(0, 128), (128, 128), (256, 128)]), (2 * 320, 128, [(0, 320), (320, 320)])]
SCALE = 0.75


def _table(r, dev, w_base=0, seed=0):
    """Rows, the table on the device, host master / dW / adapter values; storages 100 floats apart from w_base + 36."""
    rng = np.random.default_rng(1000 * r + seed)
    rows, regions = [], []
    off, aoff = w_base + 36, 64
    for n_all, K, ranges in STORAGES:
        for row0, N in ranges:
            a_off = aoff
            aoff += -(-(r * K) // 64) * 64 + 64
            b_off = aoff
            aoff += -(-(N * r) // 64) * 64
            rows.append((off + row0 * K, a_off, b_off, N, K, r, SCALE))
        regions.append((off, n_all * K))
        off += n_all * K + 100
    extent = off
    host = {'W': rng.uniform(-1, 1, extent - w_base).astype(np.float32), 'dW': rng.standard_normal(extent - w_base).astype(np.float32),
            'P': rng.uniform(-1, 1, aoff).astype(np.float32)}
    tab = lr.RawTable(rows, aoff, extent, dev)
    tab.params.copy_(torch.from_numpy(host['P']))
    return tab, host, regions


def _views(row, host, w_base=0):
    w_off, a_off, b_off, N, K, r, s = row
    W = host['W'][w_off - w_base:w_off - w_base + N * K].reshape(N, K)
    dW = host['dW'][w_off - w_base:w_off - w_base + N * K].reshape(N, K)
    A = host['P'][a_off:a_off + r * K].reshape(r, K)
    B = host['P'][b_off:b_off + N * r].reshape(N, r)
    return W, dW, A, B


def _bf16_bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize('r', RANKS)
def test_merge_against_float64(dev, r):
    from diffusion_amd import ops
    tab, host, regions = _table(r, dev)
    master = torch.from_numpy(host['W']).to(dev)
    shadow = torch.full((tab.master_extent,), -7.0, device=dev, dtype=torch.bfloat16)
    vout = torch.full((tab.master_extent,), -7.0, device=dev, dtype=torch.float32)
    ops.lora_merge(master, tab, shadow, vout=vout)
    torch.cuda.synchronize()
    got, v = shadow.float().cpu().numpy().astype(np.float64), vout.cpu()
    touched = np.zeros(tab.master_extent, dtype=bool)
    for row in tab.rows:
        w_off, _, _, N, K, _, s = row
        W, _, A, B = _views(row, host)
        ref, mag = lr.merge_ref64(W, A, B, s)
        err = np.abs(got[w_off:w_off + N * K].reshape(N, K) - ref)
        bound = lr.merge_bound(ref, mag, r)
        assert (err <= bound).all(), f'item {row[3:6]}: worst excess {(err - bound).max():.3g} at {np.unravel_index((err - bound).argmax(), err.shape)}'
        # the fp32 output is the value before the rounding: within the fp32 chain, and it casts to the bf16 output's bits
        verr = np.abs(v[w_off:w_off + N * K].numpy().astype(np.float64).reshape(N, K) - ref)
        assert (verr <= (r + 2) * 2.0 ** -24 * mag).all()
        touched[w_off:w_off + N * K] = True
    cast = torch.empty_like(shadow)
    ops.cast_f32_bf16(vout, cast)
    t = torch.from_numpy(touched).to(dev)
    assert torch.equal(_bf16_bits(cast)[t], _bf16_bits(shadow)[t])
    # nothing outside the row ranges is written: gaps, the storage without an item
    assert (shadow[~t].float() == -7.0).all() and (vout[~t] == -7.0).all()
    assert torch.equal(master.cpu(), torch.from_numpy(host['W']))


@pytest.mark.parametrize('r', (1, 16, 128))
def test_merge_with_zero_B_is_the_cast_and_in_place_fuse_matches(dev, r):
    from diffusion_amd import ops
    tab, host, _ = _table(r, dev)
    master = torch.from_numpy(host['W']).to(dev)
    master[tab.rows[0][0]] = -0.0
    cast = torch.empty(tab.master_extent, device=dev, dtype=torch.bfloat16)
    ops.cast_f32_bf16(master, cast)
    keep = tab.params.clone()
    for _, _, b_off, N, _, _, _ in tab.rows:
        tab.params[b_off:b_off + N * r] = 0
    shadow = cast.clone().fill_(3.0)
    ops.lora_merge(master, tab, shadow)
    t = torch.zeros(tab.master_extent, dtype=torch.bool, device=dev)
    for w_off, _, _, N, K, _, _ in tab.rows:
        t[w_off:w_off + N * K] = True
    assert torch.equal(_bf16_bits(shadow)[t], _bf16_bits(cast)[t])
    # vout may be the master itself (fuse): the fused master casts to the merged shadow's bits
    tab.params.copy_(keep)
    ops.lora_merge(master, tab, shadow)
    fused = master.clone()
    sh2 = torch.empty_like(shadow)
    ops.lora_merge(fused, tab, sh2, vout=fused)
    ops.cast_f32_bf16(fused, cast)
    assert torch.equal(_bf16_bits(sh2)[t], _bf16_bits(shadow)[t]) and torch.equal(_bf16_bits(cast)[t], _bf16_bits(shadow)[t])
    assert torch.equal(fused[~t], master[~t])


@pytest.mark.parametrize('r', RANKS)
def test_project_against_float64_and_bit_identical_runs(dev, r):
    from diffusion_amd import ops
    tab, host, _ = _table(r, dev)
    grad = torch.from_numpy(host['dW']).to(dev)
    tab.grad.fill_(float('nan'))     # the launch overwrites: nothing of the old contents survives in an adapter tensor
    ops.lora_project(grad, tab)
    torch.cuda.synchronize()
    first = tab.grad.clone()
    got = first.cpu().numpy().astype(np.float64)
    for row in tab.rows:
        _, a_off, b_off, N, K, _, s = row
        _, dW, A, B = _views(row, host)
        dA, dB, magA, magB = lr.project_ref64(dW, A, B, s)
        ea = np.abs(got[a_off:a_off + r * K].reshape(r, K) - dA)
        eb = np.abs(got[b_off:b_off + N * r].reshape(N, r) - dB)
        assert (ea <= lr.project_bound(magA, N)).all(), f'dA of item {row[3:6]}: worst {ea.max():.3g}'
        assert (eb <= lr.project_bound(magB, K)).all(), f'dB of item {row[3:6]}: worst {eb.max():.3g}'
    tab.grad.zero_()
    ops.lora_project(grad, tab)
    own = torch.zeros(tab.total, dtype=torch.bool, device=dev)
    for _, a_off, b_off, N, K, _, _ in tab.rows:
        own[a_off:a_off + r * K] = True
        own[b_off:b_off + N * r] = True
    assert torch.equal(tab.grad[own].view(torch.int32), first[own].view(torch.int32))
    assert (tab.grad[~own] == 0).all()                     # alignment gaps of the adapter buffer are never written
    ops.set_option('reserve_cus', 8)
    try:
        tab.grad.zero_()
        ops.lora_project(grad, tab)
        torch.cuda.synchronize()
    finally:
        ops.set_option('reserve_cus', 0)
    assert torch.equal(tab.grad[own].view(torch.int32), first[own].view(torch.int32))


def test_bad_arguments_are_rejected(dev):
    from diffusion_amd import ops
    from diffusion_amd.lora import pack_items
    tab, host, _ = _table(4, dev)
    master = torch.from_numpy(host['W']).to(dev)
    shadow = torch.zeros(tab.master_extent, device=dev, dtype=torch.bfloat16)
    for r in (0, 129):
        with pytest.raises(ValueError):
            pack_items([(0, 0, 64, 8, 8, r, 1.0)])
    with pytest.raises(ValueError):
        ops.lora_merge(master[:100], tab, shadow)
    with pytest.raises(ValueError):
        ops.lora_merge(master, tab, shadow.float())
    p, t = tab.params.data_ptr(), tab.table.data_ptr()
    for bad in [(master.data_ptr(), p, t, 0, 5, shadow.data_ptr(), 0, 0), (master.data_ptr(), p, t, 1, 0, shadow.data_ptr(), 0, 0),
                (0, p, t, 1, 5, shadow.data_ptr(), 0, 0), (master.data_ptr(), p, t, 1, 5, 0, 0, 0),
                (master.data_ptr() + 2, p, t, 1, 5, shadow.data_ptr(), 0, 0)]:
        with pytest.raises(RuntimeError, match='DA_ERR_SHAPE'):
            ops._lib.call('da_lora_merge', *bad)
    g = tab.grad.data_ptr()
    for bad in [(master.data_ptr(), p, t, 0, 1, 1, g, 0), (master.data_ptr(), p, t, 1, 0, 1, g, 0),
                (master.data_ptr(), p, t, 1, 1, 0, g, 0), (master.data_ptr(), p, t, 1, 1, 1, 0, 0),
                (master.data_ptr(), p, t, 1, 1, 1, p, 0)]:
        with pytest.raises(RuntimeError, match='DA_ERR_SHAPE'):
            ops._lib.call('da_lora_project', *bad)


def test_item_past_two_gib(dev):
    """A flat buffer of 0.6 G floats with the only item in its last rows: every byte offset of the item (fp32 master and
    gradient: past 2 GiB; the bf16 shadow: past 1 GiB) needs 64-bit address arithmetic.  Only the item's region and a band in
    front of it are initialised and checked.  About 3.6 GiB of HBM."""
    from diffusion_amd import ops
    total, N, K, r, s = 600_000_000, 320, 320, 16, 0.5
    w_off = total - N * K - 7
    assert w_off * 4 > 2 ** 31
    rng = np.random.default_rng(5)
    W, dW = rng.uniform(-1, 1, (N, K)).astype(np.float32), rng.standard_normal((N, K)).astype(np.float32)
    A, B = rng.uniform(-1, 1, (r, K)).astype(np.float32), rng.uniform(-1, 1, (N, r)).astype(np.float32)
    tab = lr.RawTable([(w_off, 64, 64 + r * K, N, K, r, s)], 64 + r * K + N * r, total, dev)
    tab.params[64:64 + r * K] = torch.from_numpy(A).to(dev).flatten()
    tab.params[64 + r * K:] = torch.from_numpy(B).to(dev).flatten()
    big = torch.empty(total, device=dev, dtype=torch.float32)
    shadow = torch.empty(total, device=dev, dtype=torch.bfloat16)
    band = slice(w_off - 4096, w_off)
    shadow[band] = 5.0
    shadow[w_off + N * K:] = 5.0
    big[w_off:w_off + N * K] = torch.from_numpy(dW).to(dev).flatten()
    ops.lora_project(big, tab)
    dA, dB, magA, magB = lr.project_ref64(dW, A, B, s)
    got = tab.grad.cpu().numpy().astype(np.float64)
    assert (np.abs(got[64:64 + r * K].reshape(r, K) - dA) <= lr.project_bound(magA, N)).all()
    assert (np.abs(got[64 + r * K:].reshape(N, r) - dB) <= lr.project_bound(magB, K)).all()
    big[w_off:w_off + N * K] = torch.from_numpy(W).to(dev).flatten()
    big[band] = 9.0
    ops.lora_merge(big, tab, shadow, vout=big)
    torch.cuda.synchronize()
    ref, mag = lr.merge_ref64(W, A, B, s)
    out = shadow[w_off:w_off + N * K].float().cpu().numpy().astype(np.float64).reshape(N, K)
    assert (np.abs(out - ref) <= lr.merge_bound(ref, mag, r)).all()
    v = big[w_off:w_off + N * K].cpu().numpy().astype(np.float64).reshape(N, K)
    assert (np.abs(v - ref) <= (r + 2) * 2.0 ** -24 * mag).all()
    assert (shadow[band].float() == 5.0).all() and (shadow[w_off + N * K:].float() == 5.0).all() and (big[band] == 9.0).all()
