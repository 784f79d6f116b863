"""CPU-only tests: the C-ABI library loads and exports every symbol include/diffusion_amd.h declares (no compute),
host logic (flat layout, mini-Hydra, schedulers, dataloader contract, LR schedule), and that the product path fails
loudly without a GPU instead of falling back."""
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, 'include', 'diffusion_amd.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(?:int|long)\s+(da_\w+)\s*\(', src)))


def test_header_symbols_exported_and_bound():
    from diffusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = _lib.load()
    syms = _declared_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in include/diffusion_amd.h but not exported'
    assert sorted(_lib.SIGNATURES) == syms, set(_lib.SIGNATURES) ^ set(syms)


def test_header_arity_matches_ctypes_signatures():
    from diffusion_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'diffusion_amd.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name, args in re.findall(r'\b(?:int|long)\s+(da_\w+)\s*\(([^;]*?)\)\s*;', src, flags=re.S):
        n = len([a for a in args.split(',') if a.strip()])
        assert n == len(_lib.SIGNATURES[name]), (name, n, len(_lib.SIGNATURES[name]))


def test_set_option_keys_and_ranges(tmp_path):
    """da_set_option is host-only state: every documented key is accepted, unknown keys and out-of-range values are rejected
    (DA_ERR_SHAPE), and DA_SET_OPTIONS applies / rejects the same way at library load (checked in a child process)."""
    import subprocess
    import sys
    from diffusion_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'diffusion_amd.h')).read()
    doc = hdr[hdr.index('/* tuning / test hooks'):hdr.index('int da_set_option')]
    keys = re.findall(r'^ \*   "([a-z0-9_]+)"', doc, flags=re.M)
    assert {'gn_resident', 'gn_resident_form', 'reserve_cus', 'grad_overwrite', 'gemm_nt_persist_conv', 'gemm_nt_ws', 'gemm_nt_de',
            'attn_fused_bwd', 'gemm_tn_ring', 'gemm_nt_stream'} <= set(keys)
    defaults = {'gn_resident': 192, 'gn_resident_min_slab': 65536, 'gemm_nt_persist': -1, 'gemm_nt_dispatch': 1, 'gemm_nt_korder': 1, 'gemm_nt_splitk': 1,
                'gemm_nt_persist_conv': 1, 'gemm_nt_de': 1, 'gemm_nt_ws': 1, 'attn_fused_bwd': 1}
    for k in keys:
        assert lib.da_set_option(k.encode(), defaults.get(k, 0)) == 0, k
    assert lib.da_set_option(b'no_such_option', 1) != 0
    assert lib.da_set_option(b'reserve_cus', 129) != 0 and lib.da_set_option(b'reserve_cus', -1) != 0
    assert lib.da_set_option(b'gn_resident', -1) != 0 and lib.da_set_option(b'gn_resident_form', 3) != 0
    code = 'from diffusion_amd import _lib; _lib.load(); print("loaded")'
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ok = subprocess.run([sys.executable, '-c', code], cwd=root, env=dict(os.environ, DA_SET_OPTIONS='gn_resident=0,reserve_cus=8'),
                        capture_output=True, text=True)
    assert ok.returncode == 0 and 'loaded' in ok.stdout, ok.stderr
    bad = subprocess.run([sys.executable, '-c', code], cwd=root, env=dict(os.environ, DA_SET_OPTIONS='gn_resident=0,bogus=1'),
                         capture_output=True, text=True)
    assert bad.returncode != 0 and 'DA_SET_OPTIONS' in bad.stderr


def test_kernel_spill_budget():
    """The build leaves each object's register report (csrc/<file>.ru.txt, -Rpass-analysis=kernel-resource-usage).  No kernel of
    the library may spill except the four recorded ones (2 VGPRs each, outside their inner loops): a template edit that pushed
    the persistent linear form of gemm_nt2 from 0 to 7 spills cost 6-16 % on its shapes and no numerical test noticed."""
    import glob
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'diffusion_amd', 'csrc')
    reports = sorted(glob.glob(os.path.join(csrc, '*.ru.txt')))
    if len(reports) < 7:   # fresh checkout (the reports are git-ignored): compile them into a scratch directory, link nothing
        import subprocess
        import tempfile
        tmp = tempfile.mkdtemp(prefix='da_ru_')
        r = subprocess.run(['make', '-C', csrc, 'ru', f'RU_DIR={tmp}', '-j4'], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        reports = sorted(glob.glob(os.path.join(tmp, '*.ru.txt')))
    assert len(reports) >= 7
    allowed = {   # mangled-name fragment -> spilled VGPRs allowed
        'gemm_nt2_kernelILi4ELi5ELi4ELi4ELi64ELb0ELi0ELb0ELi16ELb1E': 2,     # persistent 3x3 convolution form
        'gemm_nt2_kernelILi4ELi5ELi4ELi4ELi64ELb0ELi0ELb0ELi16ELb1ELb1ELb1E': 5,   # ... with the direct epilogue + residual (none in the K loop)
        'gemm_nt2_kernelILi4ELi5ELi4ELi4ELi64ELb0ELi0ELb1ELi16ELb1ELb1ELb1E': 13,  # linear form, direct epilogue + residual: opt-in only (gemm_nt_de = 3)
        'gemm_nt2_kernelILi4ELi5ELi4ELi4ELi64ELb0ELi2ELb1ELi16ELb1E': 2,     # fused GEGLU backward
        'attn_bwd_fused_kernelILi8E': 1,     # 8-wave form of the one-kernel attention backward: opt-in only (attn_fused_bwd = 2)
        'gn_res_bwd_kernelILi11ELb1ELi1024E': 2, 'gn_res_bwd_kernelILi11ELb0ELi1024E': 2}
    seen = 0
    for f in reports:
        txt = open(f).read()
        names = re.findall(r'Function Name: (\S+)', txt)
        spills = [int(x) for x in re.findall(r'VGPRs Spill: (\d+)', txt)]
        assert len(names) == len(spills) and names, f
        for n, sp in zip(names, spills):
            seen += 1
            budget = max([v for k, v in allowed.items() if k in n] or [0])
            assert sp <= budget, f'{n}: {sp} spilled VGPRs (budget {budget}) in {os.path.basename(f)}'
    assert seen > 100


def test_fastdiv_exact_at_the_admitted_bounds():
    """csrc/common.hpp FastDiv: q = (n * (2^40 // d + 1)) >> 40.  The launchers admit n < 2^24 with n * d < 2^40
    (gemm_nt_v2.hip persistent forms, gemm_tn.hip); inside that range the quotient must be exact, and just outside
    it must be able to fail - otherwise the guard is not the binding one."""
    import random

    def fdiv(n, d):
        return ((n * ((1 << 40) // d + 1)) & ((1 << 64) - 1)) >> 40

    rnd = random.Random(5)
    ds = [1, 2, 3, 7, 32 * 32, 64 * 64, 96 * 96, 65535, 65536, 65537, 99991, 512 * 512, (1 << 20) - 1, 1 << 20]
    ds += [rnd.randrange(1, 1 << 22) for _ in range(200)]
    for d in ds:
        nmax = min((1 << 24) - 1, ((1 << 40) - 1) // d)
        cand = {0, 1, d - 1, d, d + 1, nmax, nmax - 1} | {k * d - 1 for k in range(1, 50)} | {k * d for k in range(1, 50)}
        cand |= {nmax - (nmax % d) - 1, nmax - (nmax % d)} | {rnd.randrange(0, nmax + 1) for _ in range(300)}
        for n in cand:
            if 0 <= n <= nmax:
                assert fdiv(n, d) == n // d, (n, d)
    # beyond n * d < 2^40 the formula does go wrong (d = 512*512 output pixels, n just under 2^24)
    d = 512 * 512
    assert any(fdiv(k * d - 1, d) != (k * d - 1) // d for k in range(1, 64))


def test_groupnorm_plan_table_of_the_edge_tests():
    """da_groupnorm_plan_for (host only) reports for every shape of tests/test_norm_edges_gpu.py's GN_CASES the instantiation
    its table names, under every forced form; the table covers every forward NL, every backward (threads, NL) pair, peers8
    on and off, one and several parts, line-aligned and unaligned slabs.  The query leaves the options as they were."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_norm_edges_gpu as E
    from diffusion_amd import ops
    fwd, bwd, peers8, parts, aligned = set(), set(), set(), set(), set()
    for entry in E.GN_CASES:
        for form in E.FORMS:
            for b in (False, True):
                p = E.gn_plan(ops, entry[0], form, b)
                assert E.plan_label(p) == E.gn_target(entry, form, b), (entry[0], form, b, p)
                if p['form'] == 'resident':
                    (bwd if b else fwd).add((p['threads'], p['nl']))
                    peers8.add(p['peers8'])
                    parts.add(min(p['parts'], 2))
                    aligned.add(p['cw'] * 2 % 128 == 0 and E.row_stride(entry[0][2], entry[0][4]) % 64 == 0)
    assert fwd == {(1024, nl) for nl in (1, 2, 3, 4, 6, 8, 11, 16, 21)}
    assert bwd == {(1024, nl) for nl in (1, 2, 3, 4, 6, 8, 11)} | {(768, 11), (768, 14)}
    assert peers8 == {0, 1} and parts == {1, 2} and aligned == {False, True}
    cpg = {C // G for (B, HW, C, G, *_), *_ in E.GN_CASES}
    assert {1, 2, 3, 5, 8, 10, 15, 20, 30, 40, 60, 80} <= cpg
    assert {HW for (B, HW, *_), *_ in E.GN_CASES} >= {1, 7, 16, 17, 1000}
    # B = 1, HW = 1000 under the default options (restored by the forced forms): the multi-pass form with 62 chunks of
    # 17 pixels, the last three empty
    p = ops.groupnorm_plan(1, 1000, 320, 32, 336, 336)
    assert p['form'] == 'multipass' and p['nchunks'] == 62 and 59 * -(-1000 // 62) >= 1000
    with pytest.raises(ValueError):
        ops.groupnorm_plan(1, 16, 320, 30)   # C % G != 0: rejected like the entry points


def test_gemm_edge_case_tables():
    """tests/test_gemm_edges_gpu.py pins the kernel form of every case: da_gemm_nt_variant_for / da_gemm_tn_variant_for
    (host only) must report the variant its table names under the case's options, so a dispatch change cannot move a
    case unnoticed.  For the forms no query reports, each case meets the eligibility condition its table states.  The
    queries leave the options as they were."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_gemm_edges_gpu as E
    from diffusion_amd import _lib, ops
    seen = set()
    for case in E.NT_CASES:
        cid, g, N, Cin, opts, want, epi, form = case
        G = E.geom(ops, g)
        M, K = G.B * G.Hout * G.Wout, G.ksize * G.ksize * Cin
        if want is not None:
            assert E.nt_variant(ops, case) == want, (cid, E.nt_variant(ops, case))
            seen.add(want)
        if form == 'pconv':   # launch_v2: 3x3 mode 0, N % 320 == 0, tiles > 256 - reserve_cus, a ragged last row tile
            tiles = -(-M // 256) * (N // 320)
            assert G.ksize == 3 and G.mode == 0 and N % 320 == 0 and tiles > 256 - opts.get('reserve_cus', 0), cid
            assert M % 256 != 0, cid
        if form.endswith('-early'):   # the 16-wave forms take ksize 1 through the early-issue persistent walk
            assert G.ksize == 1 and opts['gemm_nt_variant'] in (12, 14, 15, 18), cid
        if form == 'ws':   # da_gemm_nt_ws_try: K 320 (BN 320, N <= 1280) / 640 (BN 128), whole 32-row tiles, enough tiles
            bn = 320 if K == 320 else 128
            assert K in (320, 640) and M % 32 == 0 and N % bn == 0 and N // bn <= 8, cid
            assert (M // 32) * (N // bn) >= 8 * (256 - opts['reserve_cus']) and not {'rb', 'a', 'f32'} & set(epi.split('+'))
        if form == 'stream':   # da_gemm_nt_v3_try: K % 64 == 0, K >= 320, bf16 out, alpha 1, no row bias
            assert K % 64 == 0 and K >= 320 and not {'rb', 'a', 'f32'} & set(epi.split('+')), cid
    assert seen == {1, 4, 5, 10, 11, 12, 14, 15, 16, 18}
    forms = {c[7] for c in E.NT_CASES}
    assert {'pconv', 'splitk', 'ws', 'stream', 'v12-early', 'v14-early', 'v15-early', 'v18-early'} <= forms
    assert {0, 1, 3} <= {c[4].get('gemm_nt_de', 1) for c in E.NT_CASES}
    assert {0, 1} <= {c[4].get('gemm_nt_korder', 1) for c in E.NT_CASES if c[3] in (320, 1280) and c[1][0] == 'conv'}
    modes = {E.geom(ops, c[1]).mode for c in E.NT_CASES}
    assert modes == {0, 1, 2, 3, 4}
    tn_seen = set()
    for case in E.TN_CASES:
        cid, g, N, Cin, opts, want, use_ws, use_db, form = case
        assert E.tn_variant(ops, case) == want, (cid, E.tn_variant(ops, case))
        tn_seen.add(form)
        G = E.geom(ops, g)
        M = G.B * G.Hout * G.Wout
        if form == 'v1':
            assert M <= 256, cid      # one pixel split
        if form in ('v1slab', 'v1atomic'):
            assert M > 256 and use_ws == (form == 'v1slab'), cid
        if form in ('v2slab', 'v2atomic'):
            assert M >= 1024 and use_ws == (form == 'v2slab'), cid
        if form.startswith('ring'):
            assert G.ksize == 1 and G.mode == 0 and want == 3, cid
    assert tn_seen == {'v1', 'v1slab', 'v1atomic', 'v2', 'fast', 'v2slab', 'v2atomic', 'ring4', 'ring5'}
    assert _lib.load().da_gemm_nt_variant_for(4096, 1280, 2880, 320, 0) == ops._lib.load().da_gemm_nt_variant_for(
        4096, 1280, 2880, 320, 0)   # defaults restored


def test_gemm_edge_gather_matches_conv2d():
    """the explicit gather of tests/test_gemm_edges_gpu.py, times the weights, equals the float64 convolution it stands
    for in every mode: 0 (pad 1, and 1x1), 1 (stride 2, pad 1, odd sizes too), 2 (dgrad of stride 2), 3 (nearest-2x
    upsample), 4 (stride 2, bottom / right pad)"""
    import sys
    import torch.nn.functional as F
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_gemm_edges_gpu as E
    from diffusion_amd import ops
    g = torch.Generator().manual_seed(3)
    Cin, Co = 8, 16
    for kind, B, H, W in (('conv', 2, 1, 1), ('conv', 2, 3, 5), ('c1', 2, 3, 5), ('down', 2, 4, 6), ('down', 2, 3, 5),
                          ('down', 1, 1, 1), ('dgrad', 2, 4, 6), ('dgrad', 1, 2, 2), ('up', 2, 1, 1), ('up', 2, 3, 5),
                          ('vae', 2, 4, 6), ('vae', 1, 2, 2)):
        G = E.geom(ops, (kind, B, H, W))
        k = G.ksize
        x = torch.randn(B, Cin, G.Hin, G.Win, generator=g, dtype=torch.float64)
        w = torch.randn(Co, Cin, k, k, generator=g, dtype=torch.float64)
        if kind in ('conv', 'c1'):
            ref = F.conv2d(x, w, padding=k // 2)
        elif kind == 'down':
            ref = F.conv2d(x, w, stride=2, padding=1)
        elif kind == 'up':
            ref = F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, padding=1)
        elif kind == 'vae':
            ref = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)
        else:   # dgrad: the gradient of a stride-2 conv (weights w2 [Cin, Co]) wrt its input, weights flipped + transposed
            w2 = torch.randn(Cin, Co, 3, 3, generator=g, dtype=torch.float64)
            ref = F.conv_transpose2d(x, w2, stride=2, padding=1, output_padding=1)
            w = w2.flip(2, 3).transpose(0, 1)    # [Co, Cin, 3, 3]: Wt[co][r][s][ci] = w2[ci][co][2-r][2-s]
        assert tuple(ref.shape[2:]) == (G.Hout, G.Wout), (kind, ref.shape, G.Hout, G.Wout)
        X = x.permute(0, 2, 3, 1).reshape(-1, Cin)
        Wm = w.permute(0, 2, 3, 1).reshape(Co, -1)
        got = (E.gather(X, G) @ Wm.t()).view(B, G.Hout, G.Wout, Co).permute(0, 3, 1, 2)
        assert torch.allclose(got, ref, rtol=0, atol=1e-12), kind


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.models.unet import UNetConfig, UNetHIP
    from diffusion_amd import ops
    with pytest.raises(RuntimeError):
        stable_diffusion_2(pretrained=False, precomputed_latents=True)
    with pytest.raises(RuntimeError):
        UNetHIP(UNetConfig.tiny(), device='cpu')
    a = torch.zeros(8, 8, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.add(a, a, a)  # host tensors are rejected before any launch
    # the product package never imports the oracle
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'diffusion_amd')):
        for f in files:
            if f.endswith('.py'):
                assert 'oracle' not in open(os.path.join(dirpath, f)).read().replace('# oracle', ''), f


def test_flat_layout_covers_manifest():
    from oracle import unet_oracle as O
    from diffusion_amd.models.unet import UNetConfig, build_layout
    for ocfg, cfg in ((O.UNetConfig.sd2_base(), UNetConfig.sd2_base()), (O.UNetConfig.tiny(), UNetConfig.tiny())):
        fp, resnets, toffs, ttotal = build_layout(cfg)
        man = dict(O.param_manifest(ocfg))
        keys = [k for k, _, _ in fp.views]
        assert sorted(keys) == sorted(man), 'diffusers key set mismatch'
        assert len(resnets) == 22 and ttotal == sum(c for _, _, c in resnets)
        # storages are disjoint, aligned, in increasing order
        end = 0
        for name, st in fp.storages.items():
            assert st.off >= end and st.off % fp.ALIGN == 0, name
            end = st.off + st.numel
        assert end <= fp.total
    # view shapes on the tiny config (cheap to materialise on the host)
    cfg = UNetConfig.tiny()
    fp, *_ = build_layout(cfg)
    flat = torch.arange(fp.total, dtype=torch.float64)  # exact integers (fp32 is not above 2^24)
    man = dict(O.param_manifest(O.UNetConfig.tiny()))
    seen = torch.zeros(fp.total, dtype=torch.int32)
    for key, sname, fn in fp.views:
        st = fp.storages[sname]
        v = fn(flat[st.off:st.off + st.numel].view(st.shape))
        assert tuple(v.shape) == tuple(man[key]), key
        seen[v.reshape(-1).long()] += 1
    assert int(seen.max()) == 1, 'two parameters alias the same storage element'
    assert int(seen.sum()) == O.param_count(O.UNetConfig.tiny())
    # conv weights are channels-last views: OIHW logical shape over OHWI memory
    k = 'down_blocks.0.resnets.0.conv1.weight'
    st = fp.storages[k]
    v = dict((a, (b, c)) for a, b, c in fp.views)[k][1](flat[st.off:st.off + st.numel].view(st.shape))
    assert v.stride() == (9 * 64, 1, 3 * 64, 64)


def test_up_block_channels():
    from diffusion_amd.models.unet import UNetConfig, up_block_resnet_channels
    cfg = UNetConfig.sd2_base()
    cat = [[sum(up_block_resnet_channels(cfg, i, j)[:2]) for j in range(3)] for i in range(4)]
    assert cat == [[2560, 2560, 2560], [2560, 2560, 1920], [1920, 1280, 960], [960, 640, 640]]


def test_hydra_lite(tmp_path):
    from diffusion_amd import hydra_lite as h
    cfg = h.load_config(os.path.join(ROOT, 'yamls', 'hydra-yamls', 'SD-2-base-256.yaml'),
                        ['batch_size=512', 'dataset.train_dataset.shuffle=false', 'trainer.max_duration=7ba'])
    assert cfg.dataset.train_batch_size == 512 and cfg.dataset.train_dataset.batch_size == 512
    assert cfg.dataset.train_dataset.shuffle is False and cfg.trainer.max_duration == '7ba'
    assert cfg.trainer.seed == 17 and cfg.trainer.device_train_microbatch_size == 'auto'
    assert h.resolve_target('diffusion.models.models.stable_diffusion_2').__module__ == 'diffusion_amd.models.models'
    assert h.resolve_target('composer.Trainer').__name__ == 'Trainer'
    assert h.resolve_target('torch.optim.AdamW').__name__ == 'FusedAdamW'
    assert h.resolve_target('composer.callbacks.lr_monitor.LRMonitor').__name__ == 'NoOpCallback'
    sched = h.instantiate(cfg.scheduler)
    assert sched(0) == 0.0 and abs(sched(5000) - 0.5) < 1e-9 and sched(10000) == 1.0 and sched(10 ** 6) == 1.0
    dl = h.instantiate(cfg.dataset.train_dataset, batch_size=4, num_workers=0, _recursive_=False)
    batch = next(iter(dl))
    assert batch['image_latents'].shape == (4, 4, 32, 32) and batch['image_latents'].dtype == torch.float16
    assert batch['caption_latents'].shape == (4, 77, 1024) and batch['captions'].shape == (4, 77)
    mets = h.instantiate(cfg.model.val_metrics)
    assert mets[0].__class__.__name__ == 'MeanSquaredError'
    # partial + nested interpolation
    p = tmp_path / 'c.yaml'
    p.write_text('a: 3\nb:\n  c: ${a}\n  s: "x${a}y"\nobj:\n  _target_: builtins.dict\n  k: ${b.c}\n')
    c2 = h.load_config(str(p))
    assert c2.b.c == 3 and c2.b.s == 'x3y' and h.instantiate(c2.obj) == {'k': 3}
    assert h.instantiate(c2.obj, _partial_=True)(z=1) == {'k': 3, 'z': 1}


def test_reference_yaml_loads_unmodified():
    # the reference's yamls/hydra-yamls/SD-2-base-256.yaml, stored verbatim as a fixture
    ref = os.path.join(ROOT, 'tests', 'golden', 'reference_SD-2-base-256.yaml')
    from diffusion_amd import hydra_lite as h
    cfg = h.load_config(ref, ['dataset.train_dataset.num_workers=0'])
    assert cfg.optimizer.lr == 1e-4 and cfg.optimizer.weight_decay == 0.01
    assert h.resolve_target(cfg.model._target_).__name__ == 'stable_diffusion_2'
    assert h.resolve_target(cfg.dataset.train_dataset._target_).__name__ == 'build_streaming_laion_dataloader'
    assert h.resolve_target(cfg.trainer._target_).__name__ == 'Trainer'


def test_schedulers_match_oracle():
    from oracle import unet_oracle as O
    from diffusion_amd.models.schedulers import DDIMScheduler, DDPMScheduler
    s, o = DDPMScheduler(), O.DDPMSchedule()
    assert torch.equal(s.alphas_cumprod, o.alphas_cumprod) and len(s) == 1000 and s.num_train_timesteps == 1000
    g = torch.Generator().manual_seed(0)
    x, n, t = torch.randn(3, 4, 8, 8, generator=g), torch.randn(3, 4, 8, 8, generator=g), torch.tensor([0, 500, 999])
    assert torch.allclose(s.add_noise(x, n, t), o.add_noise(x, n, t))
    assert torch.allclose(s.get_velocity(x, n, t), o.get_velocity(x, n, t))
    d = DDIMScheduler()
    d.set_timesteps(50)
    assert d.timesteps[0].item() == 981 and d.timesteps[-1].item() == 1 and len(d.timesteps) == 50
    # with the true noise as model output, a DDIM step lands exactly on the less-noisy interpolation
    t0 = int(d.timesteps[0]); xt = s.add_noise(x, n, torch.full((3,), t0))
    prev = d.step(n, t0, xt)['prev_sample']
    tp = t0 - 20
    assert torch.allclose(prev, s.add_noise(x, n, torch.full((3,), tp)), atol=1e-4)


def test_metric_shim_and_dataloader_local(tmp_path):
    import numpy as np
    from diffusion_amd.models.composer_shim import MeanSquaredError
    from diffusion_amd.datasets.laion.laion import build_streaming_laion_dataloader
    m = MeanSquaredError()
    a, b = torch.randn(4, 5), torch.randn(4, 5)
    m.update(a, b); m.update(a, b)
    assert abs(m.compute().item() - torch.nn.functional.mse_loss(a, b).item()) < 1e-6
    d = tmp_path / 'shards'; d.mkdir()
    np.savez(d / 's0.npz', caption_latents=np.random.randn(6, 77 * 1024).astype(np.float16),
             latents_256=np.random.randn(6, 4 * 32 * 32).astype(np.float16))
    dl = build_streaming_laion_dataloader(remote=str(d), local=str(d), batch_size=3, resize_size=256, shuffle=False)
    bt = next(iter(dl))
    assert bt['image_latents'].shape == (3, 4, 32, 32) and bt['caption_latents'].shape == (3, 77, 1024)
    with pytest.raises(ValueError):
        build_streaming_laion_dataloader(remote=['a', 'b'], local=['a'], batch_size=1)
    # `local` alone as a plain string (the shipped YAML leaves `remote:` blank) reads that directory ...
    dl = build_streaming_laion_dataloader(remote=None, local=str(d), batch_size=2, resize_size=256, shuffle=False)
    assert len(dl.dataset) == 6 and torch.equal(next(iter(dl))['image_latents'], bt['image_latents'][:2])
    # ... and a mistyped / missing directory is an error, never a silent fall-back to synthetic noise
    with pytest.raises(FileNotFoundError):
        build_streaming_laion_dataloader(remote=None, local=str(d) + '-typo', batch_size=2)
    with pytest.raises(FileNotFoundError):
        build_streaming_laion_dataloader(remote='', local=[str(d), str(tmp_path / 'nope')], batch_size=2)
    with pytest.raises(ValueError):
        build_streaming_laion_dataloader(remote='s3://bucket/laion', local=None, batch_size=2)
    # both empty -> the seeded synthetic dataset; shuffle is honoured and changes from epoch to epoch
    syn = build_streaming_laion_dataloader(remote=None, local='', batch_size=4, num_samples=32, shuffle=True, seed=5)
    e0 = torch.cat([b['image_latents'][:, 0, 0, 0] for b in syn])
    e1 = torch.cat([b['image_latents'][:, 0, 0, 0] for b in syn])
    seq = build_streaming_laion_dataloader(remote=None, local=None, batch_size=4, num_samples=32, shuffle=False, seed=5)
    s0 = torch.cat([b['image_latents'][:, 0, 0, 0] for b in seq])
    assert not torch.equal(e0, s0) and not torch.equal(e0, e1)
    assert torch.equal(e0.sort().values, s0.sort().values) and torch.equal(e1.sort().values, s0.sort().values)
    assert torch.equal(s0, torch.cat([b['image_latents'][:, 0, 0, 0] for b in seq]))


def test_mds_reader_roundtrip(tmp_path):
    """MDS shards with the column set of scripts/precompute_latents.py:252-272 (subset) -> dataloader batch dict."""
    import numpy as np
    from diffusion_amd.datasets.mds import MDSDirectory, write_mds
    from diffusion_amd.datasets.laion.laion import build_streaming_laion_dataloader
    rng = np.random.default_rng(0)
    cols = {'punsafe': 'float64', 'caption': 'str', 'width': 'int32', 'height': 'int32', 'jpg': 'bytes', 'hash': 'int64',
            'caption_latents': 'bytes', 'latents_256': 'bytes', 'latents_512': 'bytes'}
    samples = []
    for i in range(7):
        samples.append({'punsafe': 0.1 * i, 'caption': f'a photo number {i} \u00e9', 'width': 300 + i, 'height': 280,
                        'jpg': bytes(rng.integers(0, 255, 50 + i, dtype=np.uint8)), 'hash': -i,
                        'caption_latents': rng.standard_normal((77, 1024)).astype(np.float16).tobytes(),
                        'latents_256': rng.standard_normal((4, 32, 32)).astype(np.float16).tobytes(),
                        'latents_512': b''})   # image smaller than 512: empty bytes (precompute_latents.py:305-306)
    d = str(tmp_path / 'mds')
    write_mds(d, cols, samples, samples_per_shard=3)   # 3 shards: 3 + 3 + 1
    md = MDSDirectory(d)
    assert len(md) == 7 and len(md.shards) == 3
    for i in (0, 2, 3, 6):
        got = md.get(i)
        assert got['caption'] == samples[i]['caption'] and got['jpg'] == samples[i]['jpg']
        assert int(got['width']) == 300 + i and int(got['hash']) == -i and abs(float(got['punsafe']) - 0.1 * i) < 1e-12
        assert got['latents_256'] == samples[i]['latents_256'] and got['latents_512'] == b''
    dl = build_streaming_laion_dataloader(remote=d, local=d, batch_size=3, resize_size=256, shuffle=False, num_workers=0)
    b = next(iter(dl))
    assert b['image_latents'].shape == (3, 4, 32, 32) and b['image_latents'].dtype == torch.float16
    assert b['caption_latents'].shape == (3, 77, 1024) and b['captions'].shape == (3, 77)
    ref = torch.from_numpy(np.frombuffer(samples[1]['latents_256'], np.float16).copy()).reshape(4, 32, 32)
    assert torch.equal(b['image_latents'][1], ref)
    # no sample holds 512-px latents: a clear error, not an IndexError from inside a worker
    dl512 = build_streaming_laion_dataloader(remote=d, local=d, batch_size=1, resize_size=512, num_workers=0, shuffle=False)
    with pytest.raises(RuntimeError, match='have no latents_512'):
        next(iter(dl512))


def test_mds_samples_without_latents_are_skipped(tmp_path):
    """b'' in latents_512 (image smaller than 512 px, precompute_latents.py:303-306) must not abort the epoch: the loader
    substitutes the next sample that has latents."""
    import numpy as np
    from diffusion_amd.datasets.mds import write_mds
    from diffusion_amd.datasets.laion.laion import build_streaming_laion_dataloader
    rng = np.random.default_rng(1)
    cols = {'caption': 'str', 'caption_latents': 'bytes', 'latents_256': 'bytes', 'latents_512': 'bytes'}
    have = [True, False, False, True, True, False, True, False]
    samples = [{'caption': f'c{i}', 'caption_latents': rng.standard_normal((77, 1024)).astype(np.float16).tobytes(),
                'latents_256': rng.standard_normal((4, 32, 32)).astype(np.float16).tobytes(),
                'latents_512': rng.standard_normal((4, 64, 64)).astype(np.float16).tobytes() if h else b''}
               for i, h in enumerate(have)]
    d = str(tmp_path / 'mds')
    write_mds(d, cols, samples, samples_per_shard=3)
    dl = build_streaming_laion_dataloader(remote=None, local=d, batch_size=4, resize_size=512, shuffle=False, num_workers=0)
    got = torch.cat([b['image_latents'] for b in dl])
    assert got.shape == (8, 4, 64, 64)
    nxt = [0, 3, 3, 3, 4, 6, 6, 0]   # index -> next index (cyclic) holding 512-px latents
    for i, j in enumerate(nxt):
        ref = torch.from_numpy(np.frombuffer(samples[j]['latents_512'], np.float16).copy()).reshape(4, 64, 64)
        assert torch.equal(got[i], ref), (i, j)
    assert dl.dataset.datasets[0].skipped == 5


def test_mds_reader_on_byte_level_fixture(tmp_path):
    """A shard assembled BYTE BY BYTE with ``struct`` from the published MDS layout - independently of
    diffusion_amd.datasets.mds.write_mds - with the column set of scripts/precompute_latents.py:252-272: columns sorted
    by name, per-sample uint32 size prefix for every variable-size column, the JSON config blob between the offset table
    and the samples, absolute offsets, and b'' for latents_512 of an image below 512 px (:303-306)."""
    import json
    import struct
    import numpy as np
    from diffusion_amd.datasets.mds import MDSDirectory
    from diffusion_amd.datasets.laion.laion import build_streaming_laion_dataloader
    columns = {'punsafe': 'float64', 'pwatermark': 'float64', 'similarity': 'float64', 'caption': 'str', 'url': 'str',
               'key': 'str', 'status': 'str', 'error_message': 'str', 'width': 'int32', 'height': 'int32',
               'original_width': 'int32', 'original_height': 'int32', 'exif': 'str', 'jpg': 'bytes', 'hash': 'int64',
               'aesthetic_score': 'float64', 'caption_latents': 'bytes', 'latents_256': 'bytes', 'latents_512': 'bytes'}
    names = sorted(columns)
    encs = [columns[n] for n in names]
    fixed = {'float64': 8, 'int32': 4, 'int64': 8}
    sizes = [fixed.get(e) for e in encs]
    pack = {'float64': lambda v: struct.pack('<d', v), 'int32': lambda v: struct.pack('<i', v),
            'int64': lambda v: struct.pack('<q', v), 'str': lambda v: v.encode('utf-8'), 'bytes': lambda v: v}
    rng = np.random.default_rng(7)
    rows = []
    for i in range(5):
        big = i % 2 == 0
        rows.append({'punsafe': 0.01 * i, 'pwatermark': 0.5, 'similarity': 0.3, 'caption': f'caf\u00e9 {i}', 'url': f'http://x/{i}',
                     'key': f'{i:09d}', 'status': 'success', 'error_message': '', 'width': 600 if big else 300,
                     'height': 512 if big else 280, 'original_width': 1200, 'original_height': 900, 'exif': '{}',
                     'jpg': bytes(rng.integers(0, 255, 40 + i, dtype=np.uint8)), 'hash': -123456789012 - i,
                     'aesthetic_score': 5.5, 'caption_latents': rng.standard_normal((77, 1024)).astype('<f2').tobytes(),
                     'latents_256': rng.standard_normal((4, 32, 32)).astype('<f2').tobytes(),
                     'latents_512': rng.standard_normal((4, 64, 64)).astype('<f2').tobytes() if big else b''})
    blobs = []
    for r in rows:
        payload = [pack[e](r[n]) for n, e in zip(names, encs)]
        head = b''.join(struct.pack('<I', len(p)) for p, s in zip(payload, sizes) if s is None)
        blobs.append(head + b''.join(payload))
    config = json.dumps({'column_encodings': encs, 'column_names': names, 'column_sizes': sizes, 'compression': None,
                         'format': 'mds', 'hashes': [], 'size_limit': 1 << 28, 'version': 2}, sort_keys=True).encode()
    n = len(blobs)
    first = 4 + 4 * (n + 1) + len(config)
    offsets, pos = [], first
    for b in blobs:
        offsets.append(pos)
        pos += len(b)
    offsets.append(pos)
    shard = struct.pack('<I', n) + struct.pack(f'<{n + 1}I', *offsets) + config + b''.join(blobs)
    d = tmp_path / 'mds'
    d.mkdir()
    (d / 'shard.00000.mds').write_bytes(shard)
    index = {'version': 2, 'shards': [{'column_encodings': encs, 'column_names': names, 'column_sizes': sizes,
                                       'compression': None, 'format': 'mds', 'hashes': [],
                                       'raw_data': {'basename': 'shard.00000.mds', 'bytes': len(shard), 'hashes': {}},
                                       'samples': n, 'size_limit': 1 << 28, 'version': 2, 'zip_data': None}]}
    (d / 'index.json').write_text(json.dumps(index))
    md = MDSDirectory(str(d))
    assert len(md) == 5
    for i, r in enumerate(rows):
        got = md.get(i)
        assert set(got) == set(columns)
        for k, v in r.items():
            if isinstance(v, float):
                assert float(got[k]) == v, k
            elif isinstance(v, int):
                assert int(got[k]) == v, k
            else:
                assert got[k] == v, k
    dl = build_streaming_laion_dataloader(remote=None, local=str(d), batch_size=5, resize_size=256, shuffle=False, num_workers=0)
    b = next(iter(dl))
    assert torch.equal(b['image_latents'][3], torch.from_numpy(np.frombuffer(rows[3]['latents_256'], '<f2').copy()).reshape(4, 32, 32))
    assert torch.equal(b['caption_latents'][4], torch.from_numpy(np.frombuffer(rows[4]['caption_latents'], '<f2').copy()).reshape(77, 1024))
    # 512 px: samples 1 and 3 hold b'' and are replaced by the next sample that has latents
    dl5 = build_streaming_laion_dataloader(remote=None, local=str(d), batch_size=5, resize_size=512, shuffle=False, num_workers=0)
    b5 = next(iter(dl5))
    for i, j in enumerate([0, 2, 2, 4, 4]):
        assert torch.equal(b5['image_latents'][i], torch.from_numpy(np.frombuffer(rows[j]['latents_512'], '<f2').copy()).reshape(4, 64, 64))


def test_resumable_loader_skips_at_index_level_and_reshuffles_per_epoch():
    """a resumed run must continue INSIDE its epoch.  The loader's next iterator is epoch e minus its first k
    batches (no sample loaded for them), the single-process shuffle is a pure function of (seed, epoch)."""
    from diffusion_amd.datasets.laion.laion import build_streaming_laion_dataloader

    def fingerprints(dl):
        return [[float(v) for v in b['image_latents'][:, 0, 0, 0]] for b in dl]

    mk = lambda: build_streaming_laion_dataloader(remote=None, local=None, batch_size=4, num_samples=24, shuffle=True,
                                                  seed=3, num_workers=0)
    a = mk()
    assert len(a) == 6
    e0, e1 = fingerprints(a), fingerprints(a)
    assert e0 != e1 and sorted(sum(e0, [])) == sorted(sum(e1, []))      # reshuffled, same samples
    b = mk()
    b.set_epoch(0, skip_batches=4)
    assert fingerprints(b) == e0[4:]                                       # rest of epoch 0 ...
    assert fingerprints(b) == e1                                           # ... then epoch 1 in full
    c = mk()
    c.set_epoch(1)
    assert fingerprints(c) == e1

    class Counting(torch.utils.data.Dataset):
        def __init__(self):
            self.loaded = []

        def __len__(self):
            return 20

        def __getitem__(self, i):
            self.loaded.append(i)
            return torch.tensor(i)

    from diffusion_amd.datasets.laion.laion import EpochDataLoader, ResumableBatchSampler
    ds = Counting()
    dl = EpochDataLoader(dataset=ds, batch_sampler=ResumableBatchSampler(torch.utils.data.SequentialSampler(ds), 5, True))
    dl.set_epoch(0, skip_batches=2)
    got = [x.tolist() for x in dl]
    assert got == [[10, 11, 12, 13, 14], [15, 16, 17, 18, 19]] and ds.loaded == list(range(10, 20))


# ---- predicates of tests/test_pointwise_edges_gpu.py
def _pointwise_edges():
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_pointwise_edges_gpu as P
    return P


def test_pointwise_edge_rne_helper_rounds_once():
    """rne_bf16 (float64 -> bf16 on the bit pattern) agrees with the fp32 -> bf16 conversion on every fp32 that is a bf16
    value or exactly on a tie between two, denormals, +-0 and the overflow tie included; unlike a conversion through
    fp32, it rounds a float64 just above a tie up."""
    P = _pointwise_edges()
    hi = torch.arange(65536, dtype=torch.int32)
    hi = hi[((hi >> 7) & 0xFF) != 0xFF]
    for low in (0x0000, 0x8000):                                   # the bf16 value itself; the tie above it (in magnitude)
        x = ((hi << 16) | low).view(torch.float32)
        assert torch.equal(P.rne_bf16(x.double()).view(torch.int16), x.to(torch.bfloat16).view(torch.int16)), hex(low)
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40, -(1.0 + 2.0 ** -8 + 2.0 ** -40), 1.0 + 2.0 ** -8, 2.0 ** -140,
                      3.0e38, 3.4e38, float('inf'), -float('inf')], dtype=torch.float64)
    want = torch.tensor([1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7), 1.0, 0.0, 3.0041e38, float('inf'), float('inf'),
                         -float('inf')], dtype=torch.float64).to(torch.bfloat16)
    assert torch.equal(P.rne_bf16(x), want), (P.rne_bf16(x), want)
    assert float(x[0].to(torch.float32).to(torch.bfloat16)) == 1.0   # the double rounding the helper avoids
    assert bool(torch.isnan(P.rne_bf16(torch.tensor([float('nan')], dtype=torch.float64))).all())
    # needed_delta is the smallest delta the sandwich accepts: 0 for the rounded value, and just enough otherwise
    r = torch.tensor([1.0 + 2.0 ** -9, 1.0 + 2.0 ** -9, -3.0], dtype=torch.float64)
    out = torch.tensor([1.0, 1.0 + 2.0 ** -7, -3.0], dtype=torch.float64).to(torch.bfloat16)
    need = P.needed_delta(out, r)
    assert need.tolist() == [0.0, 2.0 ** -8 - 2.0 ** -9, 0.0]
    assert bool(P.sandwich_ok(out, r, need * 1.001).all()) and not bool(P.sandwich_ok(out, r, need * 0.999)[1])


def _emulated_formulas():
    """common.hpp's activation formulas and quick-GELU in numpy fp32 (fmaf: one rounding of the float64 result)"""
    import numpy as np
    f = np.float32

    def fma(a, b, c):
        return (a.astype(np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f)

    def sigmoid(x):
        return f(1) / (f(1) + np.exp2(f(-1.4426950408889634) * x))

    def silu(x):
        return x * sigmoid(x)

    def dsilu(x):
        s = sigmoid(x)
        return s * fma(x, f(1) - s, f(1))

    def phi(x):
        z = np.abs(x) * f(0.70710678118654752)
        t = f(1) / fma(z, f(0.3275911), f(1))
        poly = fma(t, f(1.061405429), f(-1.453152027))
        for c in (1.421413741, -0.284496736, 0.254829592):
            poly = fma(poly, t, f(c))
        poly = poly * t
        e = np.exp2(-(z * z) * f(1.4426950408889634))
        er = np.copysign(fma(-poly, e, f(1)), x)
        return fma(er, f(0.5), f(0.5)), e

    def gelu(x):
        return x * phi(x)[0]

    def dgelu(x):
        cdf, e = phi(x)
        return fma(x * f(0.39894228040143268), e, cdf)

    def qgelu(x):
        return x / (f(1) + np.exp(f(-1.702) * x))

    return {'silu': silu, 'dsilu': dsilu, 'gelu': gelu, 'dgelu': dgelu, 'qgelu': qgelu}


def test_pointwise_edge_sandwich_accepts_the_fp32_formulas_and_rejects_other_functions():
    """Over all 65,280 finite bf16 inputs the sandwich predicate, at HALF the delta the GPU module allows, accepts a numpy
    fp32 emulation of each activation formula rounded to bf16; it rejects tanh-GELU and x * sigmoid(1.702 x) in place of
    erf-GELU, and a sigmoid rounded to bf16 before the multiply - so it is sharp enough to tell functions apart.
    quick-GELU's worst element is the same in the emulation and on the device (0.58783 of its unit), so a bound of twice
    the device's figure, rounded down, leaves the emulation a factor 1.9999 instead of 2."""
    import numpy as np
    P = _pointwise_edges()
    xb = P.all_finite_bf16()
    x = xb.double()
    xf = xb.float().numpy()
    E = _emulated_formulas()
    cases = {   # name: (float64 result, delta at the module's constants, slack)
        'silu': (P.silu64(x), P.BOUNDS['silu.c'] * P.unit_silu(x), P.slack_sigmoid(x)),
        'dsilu': (P.dsilu64(x), P.BOUNDS['dsilu.c'] * P.unit_dsilu(x), (1 + x.abs()) * P.TINY),
        'qgelu': (P.qgelu64(x), P.BOUNDS['qgelu.c'] * P.unit_qgelu(x), P.slack_sigmoid(x)),
        'gelu': (P.gelu64(x), P.delta_gelu(x), None),
        'dgelu': (P.dgelu64(x), P.delta_gelu(x) / x.abs().clamp(min=1), None),
    }
    with np.errstate(all='ignore'):
        for name, (r, delta, slack) in cases.items():
            got32 = torch.from_numpy(E[name](xf))
            assert not bool(torch.isnan(got32).any()), name
            out = got32.to(torch.bfloat16)
            ok = P.sandwich_ok(out, r, delta / (1.999 if name == 'qgelu' else 2) + (slack if slack is not None else 0))
            assert bool(ok.all()), (name, int((~ok).sum()), xb[~ok][:4], out[~ok][:4], r[~ok][:4])
            err = (got32.double() - r).abs()
            if slack is not None:
                err = (err - slack).clamp(min=0)
            print(name, 'fp32 error / delta:', float((err / delta.clamp(min=1e-300))[delta > 0].max()),
                  'smallest accepting delta / delta:', P.needed_c(out, r, delta, slack))
        g = torch.from_numpy(E['gelu'](xf))
        assert bool(P.gelu_exact_beyond_16(xb, g.to(torch.bfloat16)).all())
        d = torch.from_numpy(E['dgelu'](xf)).double()
        assert bool(((d == 1) | (x <= 16)).all()) and bool(((d == 0) | (x >= -16)).all())
    tanh_gelu = 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))
    assert not bool(P.sandwich_ok(P.rne_bf16(tanh_gelu), P.gelu64(x), P.delta_gelu(x)).all())
    assert not bool(P.sandwich_ok(P.rne_bf16(P.qgelu64(x)), P.gelu64(x), P.delta_gelu(x)).all())
    early = x * P.rne_bf16(torch.sigmoid(x)).double()
    assert not bool(P.sandwich_ok(P.rne_bf16(early), P.silu64(x),
                                  P.BOUNDS['silu.c'] * P.unit_silu(x) + P.slack_sigmoid(x)).all())


def test_pointwise_edge_transposed_weight_reference_is_the_dgrad_weight():
    """src.view(N, T, C).permute(2, 1, 0).flip(1) - the reference of the weight-shadow tests - is, for T = 9, the weight
    with which a 3x3 convolution over dY gives the input gradient (the flipped-kernel identity), in float64"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(5)
    N, C, B, H, W = 6, 4, 2, 5, 3
    w = torch.randn(N, C, 3, 3, generator=g, dtype=torch.float64)           # conv weight [out, in, r, s]
    dy = torch.randn(B, N, H, W, generator=g, dtype=torch.float64)
    src = w.permute(0, 2, 3, 1).reshape(N, 9, C)                            # kernel layout [N][T][C]
    dst = src.view(N, 9, C).permute(2, 1, 0).flip(1)                        # [C][T][N]
    wt = dst.reshape(C, 3, 3, N).permute(0, 3, 1, 2)                        # back to [out = C, in = N, r, s]
    assert torch.allclose(F.conv2d(dy, wt, padding=1), F.conv_transpose2d(dy, w, padding=1), rtol=0, atol=1e-12)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, padding=1).backward(dy)
    assert torch.allclose(F.conv2d(dy, wt, padding=1), x.grad, rtol=0, atol=1e-12)


def test_pointwise_edge_batched_tables_cover_both_paths_and_ragged_tiles():
    """the descriptor tables of the batched weight-shadow test: T = 1 and 9, N and C of 8, 64, 72, 320 and 1280 (ragged
    64-tiles), and the scalar path by C = 4 and by N = 12; total_blocks follows refresh_transposed's formula"""
    P = _pointwise_edges()
    assert sorted(P.BATCHED_TABLES) == [1, 2, 3, 5, 8] and all(len(v) == k for k, v in P.BATCHED_TABLES.items())
    tensors = [t for table in P.BATCHED_TABLES.values() for t in table]
    assert {t[1] for t in tensors} == {1, 9}
    assert {8, 64, 72, 320, 1280} <= {t[0] for t in tensors} and {8, 64, 72, 320, 1280} <= {t[2] for t in tensors}
    assert any(t[2] == 4 for t in tensors) and any(t[0] == 12 for t in tensors)
    for table in P.BATCHED_TABLES.values():
        desc, rows, total, ns, nd = P.batched_layout(table)
        assert len(desc) == 32 * len(table)
        assert total == sum(T * ((N + 63) // 64) * ((C + 63) // 64) for N, T, C in table)
        assert [r[5] for r in rows] == sorted(r[5] for r in rows) and rows[0][5] == 0
        assert all(r[0] % 8 == 0 and r[1] % 8 == 0 for r in rows)
        assert all(rows[i][1] + rows[i][2] * rows[i][3] * rows[i][4] + P.GAP <= rows[i + 1][1] for i in range(len(rows) - 1))
        shifted = P.batched_layout(table, shift_tensor=0, shift=4)[1]
        assert shifted[0][0] % 8 == 4 and shifted[0][1] % 8 == 4
