"""Interleaved A/B of two builds of the library in ONE process (same box, same clocks - MI355X devices differ by several
per cent, so numbers from different gpurun boxes are not comparable).

  python tools/lib_ab.py <old.so> attn [cand.so ...]   attention forward / backward at the U-Net's shapes
  python tools/lib_ab.py <old.so> tn [B]               weight-gradient GEMM at the U-Net's shapes (batch B, default 256)
  python tools/lib_ab.py <old.so> nt [B]               forward / dgrad GEMM (convs, linears with bias + residual, fused GEGLU)
  python tools/lib_ab.py <old.so> gn                   GroupNorm(+SiLU) forward / backward at the U-Net's shapes
  python tools/lib_ab.py <old.so> pw                   the strided-map, noising and loss kernels of pointwise.hip, bit for bit
  python tools/lib_ab.py <old.so> smp                  the ten entries of sampler.hip (eight steps, init, guidance rescale), bit for bit
  python tools/lib_ab.py <old.so> norms [bits|time]    every entry of norms.hip (GroupNorm under each forced form, LayerNorm, the
                                                       column sums): bit for bit at the edge shapes, then timed at the U-Net's
With candidates, each is timed against <old.so>; without, the shipped library is the candidate.

<old.so> is any earlier build, e.g.  git show <rev>:diffusion_amd/csrc/attention.hip > /tmp/a.hip ; hipcc ... -o tools/_ab/old.so
(built .so files are git-ignored but travel to the GPU box)."""
import ctypes as C
import ctypes as _ct
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusion_amd import _lib  # noqa: E402


def load(path):
    lib = C.CDLL(path)
    for name, argtypes in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = _lib._RESTYPES.get(name, C.c_int)
    return lib


def timeit(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / reps   # us


def ab(fa, fb, reps=5, rounds=5):
    fa(); fb(); torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timeit(fa, reps))
        tb.append(timeit(fb, reps))
    return sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]


def main():
    what = sys.argv[2]
    cands = [a for a in sys.argv[3:] if a.endswith('.so')] or [_lib.LIB_PATH]
    if what == 'attn' and len(cands) > 1:
        for c in cands:
            print(f'==== {os.path.basename(c)} vs {os.path.basename(sys.argv[1])}', flush=True)
            run(load(sys.argv[1]), load(c), what)
        return
    run(load(sys.argv[1]), load(cands[0]), what)


def run(old, new, what):
    # DA_AB_OLD_OPTS="key=val,key=val": da_set_option calls applied to <old.so> only (each .so has its own option globals),
    # so a copy of the shipped library with an option flipped can serve as the baseline of a run-time switch
    for kv in filter(None, os.environ.get('DA_AB_OLD_OPTS', '').split(',')):
        k_, v_ = kv.split('=')
        old.da_set_option.argtypes = [_ct.c_char_p, _ct.c_int]
        assert old.da_set_option(k_.encode(), int(v_)) == 0, kv
    for kv in filter(None, os.environ.get('DA_AB_NEW_OPTS', '').split(',')):   # the same for the candidate
        k_, v_ = kv.split('=')
        new.da_set_option.argtypes = [_ct.c_char_p, _ct.c_int]
        assert new.da_set_option(k_.encode(), int(v_)) == 0, kv
    dev = torch.device('cuda')
    BF = torch.bfloat16
    st = torch.cuda.current_stream().cuda_stream
    if what == 'attn':
        shapes = [(256, 5, 1024, 1024), (256, 10, 256, 256), (256, 20, 64, 64), (256, 5, 1024, 77), (256, 10, 256, 77),
                  (64, 5, 4096, 4096), (64, 10, 1024, 1024), (64, 5, 4096, 77), (16, 5, 9216, 9216)]
        for B, H, Nq, Nk in shapes:
            Cc = H * 64
            q = torch.randn(B * Nq, Cc, device=dev).to(BF); k = torch.randn(B * Nk, Cc, device=dev).to(BF)
            v = torch.randn(B * Nk, Cc, device=dev).to(BF); do = torch.randn(B * Nq, Cc, device=dev).to(BF)
            outs = []
            for lib in (old, new):
                O = torch.empty_like(q); L2 = torch.empty(B * H * Nq, device=dev); D = torch.empty_like(L2)
                dQ = torch.empty_like(q); dK = torch.empty_like(k); dV = torch.empty_like(v)
                outs.append((O, L2, D, dQ, dK, dV))

            def fwd(lib, o):
                rc = lib.da_attn_fwd(q.data_ptr(), Cc, k.data_ptr(), Cc, v.data_ptr(), Cc, o[0].data_ptr(), Cc, o[1].data_ptr(), B, H,
                                     Nq, Nk, 0.125, st)
                assert rc == 0

            def bwd(lib, o):
                rc = lib.da_attn_bwd(q.data_ptr(), Cc, k.data_ptr(), Cc, v.data_ptr(), Cc, o[0].data_ptr(), Cc, do.data_ptr(), Cc,
                                     o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), Cc, o[4].data_ptr(), Cc, o[5].data_ptr(), Cc,
                                     B, H, Nq, Nk, 0.125, st)
                assert rc == 0
            fa, fb = ab(lambda: fwd(old, outs[0]), lambda: fwd(new, outs[1]))
            ba, bb = ab(lambda: bwd(old, outs[0]), lambda: bwd(new, outs[1]))
            rel = lambda a, b: ((a.float() - b.float()).norm() / (b.float().norm() + 1e-30)).item()
            fl = 4.0 * B * H * Nq * Nk * 64
            print(f'attn B={B} H={H} Nq={Nq} Nk={Nk}: fwd {fa:7.0f} -> {fb:7.0f} us ({fl / fb / 1e6:5.0f} TF/s, {100 * (fa / fb - 1):+5.1f} %)  '
                  f'bwd {ba:7.0f} -> {bb:7.0f} us ({2 * fl / bb / 1e6:5.0f} TF/s, {100 * (ba / bb - 1):+5.1f} %)  '
                  f'O equal {torch.equal(outs[0][0], outs[1][0])}  rel dQ {rel(outs[1][3], outs[0][3]):.1e} dK {rel(outs[1][4], outs[0][4]):.1e} '
                  f'dV {rel(outs[1][5], outs[0][5]):.1e}', flush=True)
            del q, k, v, do, outs
    elif what == 'tn':
        Bt = int(sys.argv[3]) if len(sys.argv) > 3 and sys.argv[3].isdigit() else 256
        ws = torch.empty(32 * 1024 * 1024, device=dev)
        # (M-per-image, N, Cin, H, W, ksize): linears, GEGLU projections, convs of the three levels
        shapes = [(1024, 320, 320, 1, 1, 1), (256, 640, 640, 1, 1, 1), (64, 1280, 1280, 1, 1, 1), (1024, 960, 320, 1, 1, 1),
                  (1024, 2560, 320, 1, 1, 1), (1024, 320, 1280, 1, 1, 1), (256, 5120, 640, 1, 1, 1), (256, 1920, 640, 1, 1, 1), (256, 640, 2560, 1, 1, 1), (64, 10240, 1280, 1, 1, 1),
                  (1024, 320, 320, 32, 32, 3), (256, 640, 640, 16, 16, 3), (64, 1280, 1280, 8, 8, 3), (16, 1280, 1280, 4, 4, 3),
                  (1024, 320, 640, 32, 32, 3), (64, 1280, 2560, 8, 8, 3)]
        for hw, N, Cin, H, W, ks in shapes:
            M = Bt * hw
            dy = torch.randn(M, N, device=dev).to(BF); x = torch.randn(M, Cin, device=dev).to(BF)
            dws = [torch.zeros(N * ks * ks * Cin, device=dev) for _ in range(2)]
            dbs = [torch.zeros(N, device=dev) for _ in range(2)]
            scr = torch.empty(256 * N * 2 + 1024, device=dev)
            geom = (Bt * hw, 1, 1, 1, 1) if ks == 1 else None

            def run(lib, dw, db):
                hin, win = (1, 1) if ks == 1 else (H, W)
                rc = lib.da_gemm_tn_wgrad(dy.data_ptr(), N, x.data_ptr(), Cin, dw.data_ptr(), db.data_ptr(), scr.data_ptr(), M, N, Cin,
                                          hin, win, hin, win, ks, 0, ws.data_ptr(), ws.numel(), st)
                assert rc == 0
            ta, tb = ab(lambda: run(old, dws[0], dbs[0]), lambda: run(new, dws[1], dbs[1]))
            for t_ in dws + dbs:
                t_.zero_()
            run(old, dws[0], dbs[0]); run(new, dws[1], dbs[1]); torch.cuda.synchronize()
            rel = ((dws[0] - dws[1]).norm() / dws[0].norm()).item()
            relb = ((dbs[0] - dbs[1]).norm() / dbs[0].norm()).item()
            fl = 2.0 * M * N * ks * ks * Cin
            print(f'tn M={M} N={N} Kt={ks * ks * Cin} k{ks}: {ta:7.0f} -> {tb:7.0f} us ({fl / tb / 1e6:5.0f} TF/s, {100 * (ta / tb - 1):+5.1f} %) '
                  f'rel dW {rel:.1e} db {relb:.1e}', flush=True)
            del dy, x, dws
    elif what == 'nt':
        Bt = int(sys.argv[3]) if len(sys.argv) > 3 and sys.argv[3].isdigit() else 256
        ws = torch.empty(32 * 1024 * 1024, device=dev)
        # (pixels per image, N, Cin, H, W, ksize, residual)
        shapes = [(1024, 320, 320, 32, 32, 3, 0), (1024, 320, 320, 32, 32, 3, 1), (256, 640, 640, 16, 16, 3, 0), (64, 1280, 1280, 8, 8, 3, 1),
                  (16, 1280, 1280, 4, 4, 3, 0), (1024, 320, 960, 32, 32, 3, 0), (1024, 320, 320, 1, 1, 1, 1), (1024, 320, 320, 1, 1, 1, 0),
                  (1024, 960, 320, 1, 1, 1, 0), (256, 640, 640, 1, 1, 1, 1), (256, 640, 640, 1, 1, 1, 0), (64, 1280, 1280, 1, 1, 1, 1),
                  (1024, 320, 1280, 1, 1, 1, 1), (256, 640, 2560, 1, 1, 1, 1)]
        if os.environ.get('DA_AB_ONLY_LINEAR'):
            shapes = [s_ for s_ in shapes if s_[5] == 1]
        for hw, N, Cin, H, W, ks, res in shapes:
            M = Bt * hw
            a = torch.randn(M, Cin, device=dev).to(BF); w = (torch.randn(N, ks * ks * Cin, device=dev) * 0.05).to(BF)
            bias = torch.randn(N, device=dev); r = torch.randn(M, N, device=dev).to(BF)
            outs = [torch.empty(M, N, device=dev, dtype=BF) for _ in range(2)]
            hin, win = (1, 1) if ks == 1 else (H, W)

            def run(lib, o):
                rc = lib.da_gemm_nt(a.data_ptr(), Cin, w.data_ptr(), o.data_ptr(), N, bias.data_ptr(), 0, 0, r.data_ptr() if res else 0,
                                    N if res else 0, M, N, ks * ks * Cin, Cin, hin, win, hin, win, ks, 0, 0, 1.0, ws.data_ptr(), ws.numel(), st)
                assert rc == 0
            ta, tb = ab(lambda: run(old, outs[0]), lambda: run(new, outs[1]))
            fl = 2.0 * M * N * ks * ks * Cin
            print(f'nt M={M} N={N} K={ks * ks * Cin} k{ks} res{res}: {ta:7.0f} -> {tb:7.0f} us ({fl / tb / 1e6:5.0f} TF/s, {100 * (ta / tb - 1):+5.1f} %) '
                  f'equal {torch.equal(outs[0], outs[1])}', flush=True)
            del a, w, r, outs
        for hw, C in (() if os.environ.get('DA_AB_ONLY_LINEAR') else ((1024, 320), (256, 640), (64, 1280))):   # fused GEGLU forward / backward of the feed-forward
            M = Bt * hw
            inner = 4 * C
            a = torch.randn(M, C, device=dev).to(BF); w = (torch.randn(2 * inner, C, device=dev) * 0.05).to(BF)
            bias = torch.randn(2 * inner, device=dev)
            F = [torch.empty(M, 2 * inner, device=dev, dtype=BF) for _ in range(2)]
            G = [torch.empty(M, inner, device=dev, dtype=BF) for _ in range(2)]

            def fw(lib, i):
                assert lib.da_gemm_nt_geglu(a.data_ptr(), C, w.data_ptr(), F[i].data_ptr(), 2 * inner, G[i].data_ptr(), inner, bias.data_ptr(),
                                            M, inner, C, st) == 0
            ta, tb = ab(lambda: fw(old, 0), lambda: fw(new, 1))
            fl = 2.0 * M * 2 * inner * C
            print(f'geglu fwd M={M} C={C}: {ta:7.0f} -> {tb:7.0f} us ({fl / tb / 1e6:5.0f} TF/s, {100 * (ta / tb - 1):+5.1f} %) '
                  f'equal {torch.equal(F[0], F[1]) and torch.equal(G[0], G[1])}', flush=True)
            dy = torch.randn(M, C, device=dev).to(BF); wt = (torch.randn(inner, C, device=dev) * 0.05).to(BF)
            dF = [torch.empty(M, 2 * inner, device=dev, dtype=BF) for _ in range(2)]

            def bw(lib, i):
                assert lib.da_gemm_nt_geglu_bwd(dy.data_ptr(), C, wt.data_ptr(), F[0].data_ptr(), 2 * inner, dF[i].data_ptr(), 2 * inner, M,
                                                inner, C, st) == 0
            ta, tb = ab(lambda: bw(old, 0), lambda: bw(new, 1))
            fl = 2.0 * M * inner * C
            print(f'geglu bwd M={M} C={C}: {ta:7.0f} -> {tb:7.0f} us ({fl / tb / 1e6:5.0f} TF/s, {100 * (ta / tb - 1):+5.1f} %) '
                  f'equal {torch.equal(dF[0], dF[1])}', flush=True)
            del a, w, F, G, dy, wt, dF
    elif what == 'gn':
        B, G = 256, 32
        for HW, Cc in ((1024, 320), (1024, 960), (256, 640), (256, 1920), (64, 1280), (64, 2560), (16, 1280)):
            M = B * HW
            x = torch.randn(M, Cc, device=dev).to(BF); dy = torch.randn(M, Cc, device=dev).to(BF)
            gamma = torch.randn(Cc, device=dev); beta = torch.randn(Cc, device=dev)
            nsc = int(new.da_norm_scratch_floats(B, HW, Cc))
            bufs = []
            for _ in range(2):
                bufs.append(dict(y=torch.empty_like(x), dx=torch.empty_like(x), mr=torch.empty(B * G * 2, device=dev),
                                 ss=torch.empty(B * Cc * 2, device=dev), coef=torch.empty(B * G * 2, device=dev),
                                 sc=torch.empty(nsc, device=dev), dg=torch.zeros(Cc, device=dev), db=torch.zeros(Cc, device=dev)))

            def fwd(lib, b):
                assert lib.da_groupnorm_fwd(x.data_ptr(), Cc, b['y'].data_ptr(), Cc, gamma.data_ptr(), beta.data_ptr(), b['mr'].data_ptr(),
                                            b['ss'].data_ptr(), b['sc'].data_ptr(), B, HW, Cc, G, 1e-5, 1, st) == 0

            def bwd(lib, b):
                assert lib.da_groupnorm_bwd(x.data_ptr(), Cc, dy.data_ptr(), Cc, 0, 0, b['dx'].data_ptr(), Cc, gamma.data_ptr(), beta.data_ptr(),
                                            b['mr'].data_ptr(), b['dg'].data_ptr(), b['db'].data_ptr(), b['coef'].data_ptr(), b['sc'].data_ptr(),
                                            B, HW, Cc, G, 1, st) == 0
            fa, fb = ab(lambda: fwd(old, bufs[0]), lambda: fwd(new, bufs[1]))
            ba, bb = ab(lambda: bwd(old, bufs[0]), lambda: bwd(new, bufs[1]))
            nb = M * Cc * 2
            rel = lambda a, b: ((a.float() - b.float()).norm() / (b.float().norm() + 1e-30)).item()
            print(f'gn HW={HW} C={Cc}: fwd {fa:7.1f} -> {fb:7.1f} us ({3 * nb / fb / 1e6:5.2f} TB/s, {100 * (fa / fb - 1):+5.1f} %)  '
                  f'bwd {ba:7.1f} -> {bb:7.1f} us ({5 * nb / bb / 1e6:5.2f} TB/s, {100 * (ba / bb - 1):+5.1f} %)  '
                  f'rel y {rel(bufs[1]["y"], bufs[0]["y"]):.1e} dx {rel(bufs[1]["dx"], bufs[0]["dx"]):.1e}', flush=True)
            del x, dy, bufs
    elif what == 'pw':
        # the strided-map, noising and loss kernels of pointwise.hip.  Most of these launches take microseconds, so the
        # launches per timed window are calibrated per row to ~30 ms of the old build (5 launches would time the clock)
        bits = lambda t: t.view(torch.int16 if t.dtype == BF else torch.int32)   # noqa: E731
        spread = {}

        def row(op, label, call, outs):
            """call(lib, o) launches on the output tensors o; outs = (the old build's, the new build's)"""
            fa, fb = (lambda: call(old, outs[0])), (lambda: call(new, outs[1]))
            fa(); fb(); torch.cuda.synchronize()
            reps = max(5, min(20000, int(30e3 / max(timeit(fa, 20), 1e-3))))
            ta, tb = ab(fa, fb, reps=reps, rounds=7)
            equal = all(torch.equal(bits(x), bits(y)) for x, y in zip(*outs))
            pct = 100 * (ta / tb - 1)
            spread.setdefault(op, []).append(pct)
            print(f'pw {op:14s} {label:28s}: {ta:8.2f} -> {tb:8.2f} us ({pct:+5.1f} %, {reps} launches / window)  '
                  f'equal bits {equal}', flush=True)

        def mat(M, Cc):
            return torch.randn(M, Cc, device=dev).to(BF)

        def two(*shape, dtype=BF):
            return tuple([torch.empty(*shape, device=dev, dtype=dtype)] for _ in range(2))

        def strided(name, ins, Cc):
            """an entry point of the map: (pointer, ld) per operand, then M, C"""
            flat = [v for t_ in ins for v in (t_.data_ptr(), t_.stride(0))]
            return lambda lib, o: _ok(getattr(lib, name)(*flat, o[0].data_ptr(), o[0].stride(0), ins[0].shape[0], Cc, st))

        def _ok(rc):
            assert rc == 0, rc

        for M, Cc in ((262144, 320), (65536, 640), (16384, 1280), (4096, 1280)):
            a, b = mat(M, Cc), mat(M, Cc)
            row('add', f'{M}x{Cc}', strided('da_add', (a, b), Cc), two(M, Cc))
            row('copy2d', f'{M}x{Cc}', strided('da_copy2d', (a,), Cc), two(M, Cc))
            if Cc == 640:     # a skip gradient: one operand is a column slice of the concat buffer's gradient
                cat = mat(M, 2 * Cc)
                row('add', f'{M}x{Cc} b = [:, {Cc}:] of {2 * Cc}', strided('da_add', (a, cat[:, Cc:]), Cc), two(M, Cc))
                del cat
            del a, b
        x, dy = mat(256, 1280), mat(256, 1280)
        row('silu_fwd', '256x1280', strided('da_silu_fwd', (x,), 1280), two(256, 1280))
        row('silu_bwd', '256x1280', strided('da_silu_bwd', (x, dy), 1280), two(256, 1280))
        x = mat(19712, 4096)
        row('gelu_fwd', '19712x4096', strided('da_gelu_fwd', (x,), 4096), two(19712, 4096))
        x = mat(19712, 3072)
        row('quick_gelu_fwd', '19712x3072', strided('da_quick_gelu_fwd', (x,), 3072), two(19712, 3072))
        del x, dy
        for M, Cc in ((262144, 320), (65536, 640), (16384, 1280)):      # the shapes of tools/pw_bench.py
            inner = 4 * Cc
            proj, dout = mat(M, 2 * inner), mat(M, inner)
            row('geglu_fwd', f'{M}x{inner}', strided('da_geglu_fwd', (proj,), inner), two(M, inner))
            row('geglu_bwd', f'{M}x{inner}', strided('da_geglu_bwd', (proj, dout), inner), two(M, 2 * inner))
            del proj, dout
        betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
        ac = torch.cumprod(1 - betas, 0)
        sa, s1 = ac.sqrt().float().to(dev), (1 - ac).sqrt().float().to(dev)
        for B, side in ((256, 32), (64, 64)):
            HW = side * side
            x0, eps = torch.randn(B, 4, HW, device=dev), torch.randn(B, 4, HW, device=dev)
            t = torch.randint(0, 1000, (B,), device=dev)
            for v_pred in (0, 1):
                outs = tuple([torch.empty(B * HW, 8, device=dev, dtype=BF), torch.empty(B * HW, 8, device=dev)] for _ in range(2))
                row('add_noise', f'B={B} 4x{side}x{side} v_pred={v_pred}',
                    lambda lib, o: _ok(lib.da_add_noise(x0.data_ptr(), eps.data_ptr(), t.data_ptr(), sa.data_ptr(), s1.data_ptr(),
                                                        o[0].data_ptr(), o[1].data_ptr(), B, HW, v_pred, st)), outs)
        pix = 262144
        pred, target = torch.randn(pix, 8, device=dev), torch.randn(pix, 8, device=dev)
        outs = tuple([torch.empty(pix, 8, device=dev, dtype=BF), torch.empty(1, device=dev), torch.empty(1024, device=dev)]
                     for _ in range(2))
        row('mse_loss', f'{pix} pixels',
            lambda lib, o: _ok(lib.da_mse_loss(pred.data_ptr(), target.data_ptr(), o[0].data_ptr(), o[1].data_ptr(),
                                               o[2].data_ptr(), pix, 2.0 / (4 * pix), 1.0, 0, st)), outs)
        for op, pcts in spread.items():     # with the same build on both sides this is the op's noise
            print(f'pw spread {op:14s}: new slower by at most {max(0.0, -min(pcts)):4.1f} %, largest |difference| '
                  f'{max(abs(v) for v in pcts):4.1f} %', flush=True)
    elif what == 'smp':
        # the ten entries of sampler.hip: every output buffer bit for bit at small edge shapes (one line per entry and
        # size, every operand combination behind it), then bits and time at the two state sizes generate() uses most
        import itertools
        bits = lambda t: t.view(torch.int16 if t.dtype == BF else torch.int32)   # noqa: E731  (NaN-proof)
        ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        gen = torch.Generator(device=dev).manual_seed(5)
        rnd = lambda *shape: torch.randn(*shape, device=dev, generator=gen)   # noqa: E731
        steps = [(ms, blend, rs) for rs in (0, 1) for blend in (0, 1) for ms in (0, 1)]
        name = lambda ms, blend, rs: 'da_sampler_step' + '_ms' * ms + '_blend' * blend + '_rs' * rs   # noqa: E731

        def operands(npix, HW, Cc, cfg, k1):
            """the inputs of one step, shared by both builds; masks hold exact 0, exact 1 and fractions, factor != 1"""
            B = npix // HW
            mask = torch.rand(npix, device=dev, generator=gen)
            mask[0::3], mask[1::3] = 0.0, 1.0
            return dict(pred=rnd((2 if cfg else 1) * npix, 8), x=rnd(npix, 8), noise=rnd(B, Cc, HW, 1), hist=rnd(npix, 8),
                        known8=rnd(npix, 8), eps8=rnd(npix, 8), mask=mask,
                        factor=0.5 + torch.rand(B, device=dev, generator=gen),
                        coef1=torch.tensor([0.9, 0.1, 0.3, 3.0, 0.8, 0.6, 0.0, 0.0], device=dev),    # cx cm cn g bA bS
                        coef2=torch.tensor([0.9, -0.4, 0.5, 0.4, k1, 3.0, 0.8, 0.6], device=dev))   # ax am kx k0 k1 g bA bS

        def step_call(ms, blend, rs, ops_, npix, HW, Cc, cfg, copies, noise, o):
            """o = (x, x_out, hist, xt_out or None): this build's own buffers (x_out is x when in place)"""
            x, x_out, hist, xt = o
            args = [ptr(ops_['pred']), ptr(x), ptr(hist) if ms else (ptr(ops_['noise']) if noise else None),
                    ptr(ops_['coef2'] if ms else ops_['coef1'])]
            if blend:
                args += [ptr(ops_['known8']), ptr(ops_['eps8']), ptr(ops_['mask'])]
            if rs:
                args += [ptr(ops_['factor'])]
            return lambda lib: getattr(lib, name(ms, blend, rs))(*args, ptr(x_out), ptr(xt), npix, HW, Cc, cfg, copies, st)

        def step_bufs(ops_, npix, copies, inplace, with_xt, nan_hist):
            """fresh buffers per build: outputs start from a sentinel, so a stray or a missing store shows too"""
            out = []
            for _ in range(2):
                x = ops_['x'].clone()
                hist = torch.full_like(ops_['hist'], float('nan')) if nan_hist else ops_['hist'].clone()
                out.append((x, x if inplace else torch.full_like(x, 7.0), hist,
                            torch.full((copies * npix, 8), 7.0, device=dev, dtype=BF) if with_xt else None))
            return out

        def same(oa, ob):
            return all(torch.equal(bits(p), bits(q)) for p, q in zip(oa, ob) if p is not None)

        ok_all = True
        for (ms, blend, rs), (npix, HW) in itertools.product(steps, ((1, 1), (255, 85), (257, 257), (260, 130))):
            n_cases, bad = 0, []
            # `order`: the noise draw given or NULL (first-order forms); k1 = 0 over a NaN history or k1 != 0 (two-step)
            for Cc, cfg, copies, with_xt, inplace, order in itertools.product((1, 3, 4, 8), (0, 1), (1, 2), (1, 0), (1, 0), (1, 0)):
                ops_ = operands(npix, HW, Cc, cfg, k1=0.25 if order else 0.0)
                ba, bb = step_bufs(ops_, npix, copies, inplace, with_xt, nan_hist=bool(ms and not order))
                ra = step_call(ms, blend, rs, ops_, npix, HW, Cc, cfg, copies, order, ba)(old)
                rb = step_call(ms, blend, rs, ops_, npix, HW, Cc, cfg, copies, order, bb)(new)
                n_cases += 1
                if ra != 0 or rb != 0 or not same(ba, bb):
                    bad.append((Cc, cfg, copies, with_xt, inplace, order, ra, rb))
            ok_all &= not bad
            print(f'smp {name(ms, blend, rs)[3:]:26s} npix={npix:3d} HW={HW:3d}: {n_cases} cases (C 1/3/4/8, cfg, copies, xt_out / NULL, '
                  f'in / out of place, {"k1 = 0 over NaN hist / k1 != 0" if ms else "noise / NULL"}): x_out xt_out'
                  f'{" hist" if ms else ""}  equal bits {not bad}' + (f'  FIRST DIFFERENCES {bad[:4]}' if bad else ''), flush=True)
        for (B, H, W), f in itertools.product(((1, 1, 1), (3, 5, 17), (1, 1, 257), (2, 10, 13)), (1, 2)):
            n_cases, bad = 0, []
            for Cc, copies, with_xt, with_mask, with_k8 in itertools.product((1, 3, 4, 8), (1, 2), (1, 0), (1, 0), (1, 0)):
                npix = B * H * W
                known, noise = rnd(B, Cc, H, W), rnd(B, Cc, H, W)
                mask_px = torch.rand(B, f * H, f * W, device=dev, generator=gen).round_(decimals=1) if with_mask else None
                coef = torch.tensor([0.8, 0.6, 0.0, 0.0], device=dev)
                bufs = [[torch.full((npix, 8), 7.0, device=dev) if with_k8 else None, torch.full((npix, 8), 7.0, device=dev) if with_k8 else None,
                         torch.full((npix,), 7.0, device=dev) if with_mask else None, torch.full((npix, 8), 7.0, device=dev),
                         torch.full((copies * npix, 8), 7.0, device=dev, dtype=BF) if with_xt else None] for _ in range(2)]
                rcs = [lib.da_sampler_init(ptr(known), ptr(noise), ptr(mask_px), ptr(coef), *[ptr(t_) for t_ in o], B, H, W, Cc, f,
                                           copies, st) for lib, o in zip((old, new), bufs)]
                n_cases += 1
                if rcs != [0, 0] or not same(*bufs):
                    bad.append((Cc, copies, with_xt, with_mask, with_k8, rcs))
            ok_all &= not bad
            print(f'smp {"sampler_init":26s} B={B} {H}x{W} f={f}: {n_cases} cases (C 1/3/4/8, copies, xt / NULL, mask / NULL, known8 + eps8 / '
                  f'NULL): known8 eps8 mask x xt  equal bits {not bad}' + (f'  FIRST DIFFERENCES {bad[:4]}' if bad else ''), flush=True)
        for npix, HW in ((1, 1), (255, 85), (257, 257), (260, 130)):
            n_cases, bad = 0, []
            for Cc, g_index in itertools.product((1, 3, 4, 8), (3, 5)):
                ops_ = operands(npix, HW, Cc, 1, 0.25)
                fac = [torch.full((npix // HW,), 7.0, device=dev) for _ in range(2)]
                rcs = [lib.da_guidance_rescale(ptr(ops_['pred']), ptr(ops_['coef2']), g_index, 0.7, ptr(o), npix, HW, Cc, st)
                       for lib, o in zip((old, new), fac)]
                n_cases += 1
                if rcs != [0, 0] or not same(fac[:1], fac[1:]):
                    bad.append((Cc, g_index, rcs))
            ok_all &= not bad
            print(f'smp {"guidance_rescale":26s} npix={npix:3d} HW={HW:3d}: {n_cases} cases (C 1/3/4/8, g_index 3 / 5): factor  '
                  f'equal bits {not bad}' + (f'  FIRST DIFFERENCES {bad[:4]}' if bad else ''), flush=True)

        # the workload: B = 16 at 32 x 32 and 64 x 64 latents, C = 4, under guidance, in place, as the sampler launches it.
        # A launch takes microseconds, so launches per window are calibrated as in `pw`; the rows of the four passes are an
        # entry's samples for its closing "smp spread" line (with the same build on both sides: its noise)
        spread = {}

        def row(op, label, fa, fb, outs):
            fa(); fb(); torch.cuda.synchronize()
            equal = same(*outs)      # after ONE launch each on equal buffers; the timed launches then iterate in place
            reps = max(5, min(20000, int(30e3 / max(timeit(fa, 20), 1e-3))))
            ta, tb = ab(fa, fb, reps=reps, rounds=7)
            pct = 100 * (ta / tb - 1)
            spread.setdefault(op, []).append(pct)
            print(f'smp {op:26s} {label:24s}: {ta:8.2f} -> {tb:8.2f} us ({pct:+5.1f} %, {reps} launches / window)  '
                  f'equal bits {equal}', flush=True)
            return equal

        for rep, side in itertools.product((1, 2, 3, 4), (32, 64)):
            B, Cc, HW = 16, 4, side * side
            npix, label = B * HW, f'B={B} {Cc}x{side}x{side} pass {rep}'
            ops_ = operands(npix, HW, Cc, 1, 0.25)
            # contracting rows: thousands of in-place launches stay finite
            ops_['coef1'] = torch.tensor([0.9, 0.1, 0.0, 3.0, 0.8, 0.6, 0.0, 0.0], device=dev)
            ops_['coef2'] = torch.tensor([0.5, 0.1, 0.5, 0.3, 0.1, 3.0, 0.8, 0.6], device=dev)
            for ms, blend, rs in steps:
                ba, bb = step_bufs(ops_, npix, 2, True, True, False)
                ca = step_call(ms, blend, rs, ops_, npix, HW, Cc, 1, 2, 0, ba)
                cb = step_call(ms, blend, rs, ops_, npix, HW, Cc, 1, 2, 0, bb)
                ok_all &= row(name(ms, blend, rs)[3:], label, lambda: ca(old), lambda: cb(new), (ba, bb))
            known, noise = rnd(B, Cc, side, side), rnd(B, Cc, side, side)
            mask_px = torch.rand(B, 8 * side, 8 * side, device=dev, generator=gen).round_()
            coef = torch.tensor([0.8, 0.6, 0.0, 0.0], device=dev)
            bufs = [[torch.full((npix, 8), 7.0, device=dev), torch.full((npix, 8), 7.0, device=dev), torch.full((npix,), 7.0, device=dev),
                     torch.full((npix, 8), 7.0, device=dev), torch.full((2 * npix, 8), 7.0, device=dev, dtype=BF)] for _ in range(2)]
            init = lambda lib, o: lib.da_sampler_init(ptr(known), ptr(noise), ptr(mask_px), ptr(coef), *[ptr(t_) for t_ in o], B,   # noqa: E731
                                                      side, side, Cc, 8, 2, st)
            ok_all &= row('sampler_init', label, lambda: init(old, bufs[0]), lambda: init(new, bufs[1]), bufs)
            fac = [[torch.full((B,), 7.0, device=dev)] for _ in range(2)]
            gr = lambda lib, o: lib.da_guidance_rescale(ptr(ops_['pred']), ptr(ops_['coef2']), 5, 0.7, ptr(o[0]), npix, HW, Cc, st)   # noqa: E731
            ok_all &= row('guidance_rescale', label, lambda: gr(old, fac[0]), lambda: gr(new, fac[1]), fac)
        for op, pcts in spread.items():     # with the same build on both sides this is the entry's noise
            print(f'smp spread {op:26s}: new slower by at most {max(0.0, -min(pcts)):4.1f} %, largest |difference| '
                  f'{max(abs(v) for v in pcts):4.1f} %', flush=True)
        print(f'smp every comparison equal bits {ok_all}', flush=True)
        if not ok_all:
            raise SystemExit(1)
    elif what == 'norms':
        norms(old, new, dev, st, sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] in ('bits', 'time') else 'all')
    else:
        raise SystemExit(__doc__)


def norms(old, new, dev, st, part):
    """every entry of norms.hip: all output buffers bit for bit at the edge shapes (part 'bits'), then time at the workload's
    shapes (part 'time'); 'all' runs both.  Outputs start from a sentinel, so a stray or a missing store shows too."""
    import itertools
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    from test_norm_edges_gpu import FORMS, GN_CASES, LN5_RPW, row_stride
    BF = torch.bfloat16
    bits = lambda t: t.view(torch.int16 if t.dtype == BF else torch.int32)   # noqa: E731  (NaN-proof)
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    gen = torch.Generator(device=dev).manual_seed(9)
    libs = (old, new)

    def rnd(*shape, dtype=torch.float32):
        return torch.randn(*shape, device=dev, generator=gen).to(dtype)

    def sent(*shape, dtype=torch.float32):
        return torch.full(shape, 7.0, device=dev, dtype=dtype)

    def opt(key, value, only=libs):
        for lib in only:
            lib.da_set_option.argtypes = [_ct.c_char_p, _ct.c_int]
            assert lib.da_set_option(key.encode(), int(value)) == 0, key

    def view(t, ld):
        """t [rows, C] as a column view at 8 of a [rows, ld] buffer (the other columns: sentinel)"""
        buf = sent(t.shape[0], ld, dtype=BF)
        buf[:, 8:8 + t.shape[1]] = t
        return buf[:, 8:8 + t.shape[1]]

    def same(a, b, skip=()):
        return [k for k in a if k not in skip and not torch.equal(bits(a[k]), bits(b[k]))]

    # ---- the calls: o = this build's own output buffers (whole strided buffers, so pad columns are compared too)
    def gn_bufs(B, HW, C, G, ld, prior):
        n = int(new.da_norm_scratch_floats(B, HW, C))
        return dict(y=sent(B * HW, ld, dtype=BF), mean_rstd=sent(B * G * 2), scale_shift=sent(B * C * 2), scratch_f=sent(n),
                    dx=sent(B * HW, ld, dtype=BF), coef=sent(B * G * 2), scratch_b=sent(n),
                    dgamma=prior[0].clone() if prior else sent(C), dbeta=prior[1].clone() if prior else sent(C))

    def gn_fwd(lib, o, x, gamma, beta, B, HW, C, G, ld, eps, silu):
        return lib.da_groupnorm_fwd(ptr(x), ld, o['y'].data_ptr() + 16, ld, ptr(gamma), ptr(beta), ptr(o['mean_rstd']),
                                    ptr(o['scale_shift']), ptr(o['scratch_f']), B, HW, C, G, eps, silu, st)

    def gn_bwd(lib, o, x, dy, r, gamma, beta, B, HW, C, G, ld, silu):
        return lib.da_groupnorm_bwd(ptr(x), ld, ptr(dy), ld, ptr(r), ld if r is not None else 0, o['dx'].data_ptr() + 16, ld, ptr(gamma),
                                    ptr(beta), ptr(o['mean_rstd']), ptr(o['dgamma']), ptr(o['dbeta']), ptr(o['coef']),
                                    ptr(o['scratch_b']), B, HW, C, G, silu, st)

    def ln_bufs(M, C, prior):
        return dict(y=sent(M, C, dtype=BF), mean_rstd=sent(2 * M), dx=sent(M, C, dtype=BF), scratch=sent(1024 * C * 2),
                    dgamma=prior[0].clone() if prior else sent(C), dbeta=prior[1].clone() if prior else sent(C))

    def ln_fwd(lib, o, x, gamma, beta, M, C):
        return lib.da_layernorm_fwd(ptr(x), C, ptr(o['y']), C, ptr(gamma), ptr(beta), ptr(o['mean_rstd']), M, C, 1e-5, st)

    def ln_bwd(lib, o, x, dy, r, gamma, M, C):
        return lib.da_layernorm_bwd(ptr(x), C, ptr(dy), C, ptr(r), C if r is not None else 0, ptr(o['dx']), C, ptr(gamma),
                                    ptr(o['mean_rstd']), ptr(o['dgamma']), ptr(o['dbeta']), ptr(o['scratch']), M, C, st)

    def colsum(lib, o, x, M, C):
        return lib.da_colsum_accum(ptr(x), C, ptr(o['out']), ptr(o['scratch']), M, C, st)

    def image_colsum(lib, o, x, B, HW, C):
        return lib.da_image_colsum(ptr(x), C, ptr(o['out']), C, ptr(o['db']), ptr(o['scratch']), B, HW, C, st)

    ok_all = True

    def report(label, n_cases, names, bad):
        nonlocal ok_all
        ok_all &= not bad
        print(f'norms {label}: {n_cases} cases: {names}  equal bits {not bad}' + (f'  FIRST DIFFERENCES {bad[:4]}' if bad else ''),
              flush=True)

    if part in ('all', 'bits'):
        # GroupNorm: the cases and strides of the edge tests under each forced form; gradients added onto a prior and written
        for form, (case, _, _) in itertools.product(FORMS, GN_CASES):
            B, HW, C, G, aligned, eps, silu, radd = case
            ld = row_stride(C, aligned)
            opt('gn_resident', FORMS[form][0]); opt('gn_resident_form', FORMS[form][1]); opt('gn_resident_min_slab', 0)
            x, dy = view(rnd(B * HW, C, dtype=BF), ld), view(rnd(B * HW, C, dtype=BF), ld)
            r = view(rnd(B * HW, C, dtype=BF), ld) if radd else None
            gamma, beta, prior = 1 + 0.25 * rnd(C), 0.25 * rnd(C), (rnd(C), rnd(C))
            bad = []
            for overwrite in (0, 1):
                opt('grad_overwrite', overwrite)
                oa, ob = (gn_bufs(B, HW, C, G, ld, None if overwrite else prior) for _ in libs)
                rcs = [gn_fwd(lib, o, x, gamma, beta, B, HW, C, G, ld, eps, silu) for lib, o in zip(libs, (oa, ob))]
                rcs += [gn_bwd(lib, o, x, dy, r, gamma, beta, B, HW, C, G, ld, silu) for lib, o in zip(libs, (oa, ob))]
                torch.cuda.synchronize()
                # scale_shift is exempt from the comparison: the new build must leave the sentinel
                diff = same(oa, ob, skip=('scale_shift',)) + ([] if torch.equal(ob['scale_shift'], sent(B * C * 2)) else ['scale_shift written'])
                if any(rcs) or diff:
                    bad.append((overwrite, rcs, diff))
            opt('grad_overwrite', 0)
            report(f'groupnorm {form:9s} {case}', 2, 'y mean_rstd dx coef dgamma dbeta scratch (grad_overwrite 0 / 1), scale_shift left alone', bad)
        opt('gn_resident', 192); opt('gn_resident_form', 0); opt('gn_resident_min_slab', 64 * 1024)
        # LayerNorm: the *5 kernels around the rows of a wave and past the capped grids, the generic ones at lane tails
        ln_shapes = [(M, C) for C, rpw in LN5_RPW.items() for M in sorted({1, rpw - 1, rpw + 1, 4 * rpw + 1, 65539} - {0})]
        ln_shapes += [(M, C) for C in (8, 64, 1024, 1536) for M in (1, 5, 4097)]
        for M, C in ln_shapes:
            x, dy, radd_t, gamma, beta, prior = rnd(M, C, dtype=BF), rnd(M, C, dtype=BF), rnd(M, C, dtype=BF), 1 + 0.25 * rnd(C), rnd(C), (rnd(C), rnd(C))
            bad = []
            for r, overwrite in itertools.product((None, radd_t), (0, 1)):
                opt('grad_overwrite', overwrite)
                oa, ob = (ln_bufs(M, C, None if overwrite else prior) for _ in libs)
                rcs = [ln_fwd(lib, o, x, gamma, beta, M, C) for lib, o in zip(libs, (oa, ob))]
                rcs += [ln_bwd(lib, o, x, dy, r, gamma, M, C) for lib, o in zip(libs, (oa, ob))]
                torch.cuda.synchronize()
                if any(rcs) or same(oa, ob):
                    bad.append((r is not None, overwrite, rcs, same(oa, ob)))
            opt('grad_overwrite', 0)
            report(f'layernorm M={M} C={C}', 4, 'y mean_rstd dx dgamma dbeta scratch (Radd / none, grad_overwrite 0 / 1)', bad)
        # column sums: every loop, tail, z-slab and lane fold
        for M, C in ((1, 8), (63, 24), (12416, 16), (16421, 24), (16, 10240)):
            x, prior, bad = rnd(M, C, dtype=BF), rnd(C), []
            for overwrite in (0, 1):
                opt('grad_overwrite', overwrite)
                oa, ob = (dict(out=sent(C) if overwrite else prior.clone(), scratch=sent(256 * C * 2)) for _ in libs)
                rcs = [colsum(lib, o, x, M, C) for lib, o in zip(libs, (oa, ob))]
                torch.cuda.synchronize()
                if any(rcs) or same(oa, ob):
                    bad.append((overwrite, rcs, same(oa, ob)))
            opt('grad_overwrite', 0)
            report(f'colsum_accum M={M} C={C}', 2, 'out scratch (grad_overwrite 0 / 1)', bad)
        for B, HW, C in ((1, 1, 8), (65, 512, 16), (130, 16, 4104)):
            x, prior, bad = rnd(B * HW, C, dtype=BF), rnd(C), []
            for with_db, overwrite in itertools.product((1, 0), (0, 1)):
                opt('grad_overwrite', overwrite)
                oa, ob = (dict(out=sent(B, C, dtype=BF), db=(sent(C) if overwrite else prior.clone()) if with_db else None,
                               scratch=sent(int(new.da_norm_scratch_floats(B, HW, C)))) for _ in libs)
                rcs = [image_colsum(lib, o, x, B, HW, C) for lib, o in zip(libs, (oa, ob))]
                torch.cuda.synchronize()
                diff = same({k: v for k, v in oa.items() if v is not None}, ob)
                if any(rcs) or diff:
                    bad.append((with_db, overwrite, rcs, diff))
            opt('grad_overwrite', 0)
            report(f'image_colsum B={B} HW={HW} C={C}', 4, 'out db scratch (db / NULL, grad_overwrite 0 / 1)', bad)
        print(f'norms every comparison equal bits {ok_all}', flush=True)
        if not ok_all:
            raise SystemExit(1)
    if part in ('all', 'time'):
        # the workload: launches per window calibrated as in `pw`, 7 windows, 4 passes; an entry's rows are its samples for
        # the closing "norms spread" line (with the same build on both sides: its noise)
        spread = {}

        def row(op, label, fa, fb):
            fa(); fb(); torch.cuda.synchronize()
            reps = max(5, min(20000, int(30e3 / max(timeit(fa, 20), 1e-3))))
            ta, tb = ab(fa, fb, reps=reps, rounds=7)
            pct = 100 * (ta / tb - 1)
            spread.setdefault(op, []).append(pct)
            print(f'norms {op:20s} {label:30s}: {ta:8.2f} -> {tb:8.2f} us ({pct:+5.1f} %, {reps} launches / window)', flush=True)

        def ok(rc):
            assert rc == 0, rc

        for rep in (1, 2, 3, 4):
            B, G = 256, 32
            for HW, C in ((1024, 320), (1024, 960), (256, 640), (256, 1920), (64, 1280), (64, 2560), (16, 1280)):
                x, dy, r = rnd(B * HW, C, dtype=BF), rnd(B * HW, C, dtype=BF), rnd(B * HW, C, dtype=BF)
                gamma, beta = 1 + 0.25 * rnd(C), 0.25 * rnd(C)
                oa, ob = (gn_bufs(B, HW, C, G, C, None) for _ in libs)
                for tag, res in (('', 192), (' mp', 0)):      # the default options, then the multi-pass kernels
                    opt('gn_resident', res)
                    label = f'B={B} HW={HW} C={C} pass {rep}'

                    def fwd(lib, o):
                        ok(lib.da_groupnorm_fwd(ptr(x), C, ptr(o['y']), C, ptr(gamma), ptr(beta), ptr(o['mean_rstd']), ptr(o['scale_shift']),
                                                ptr(o['scratch_f']), B, HW, C, G, 1e-5, 1, st))

                    def bwd(lib, o, radd):
                        ok(lib.da_groupnorm_bwd(ptr(x), C, ptr(dy), C, ptr(radd), C if radd is not None else 0, ptr(o['dx']), C, ptr(gamma),
                                                ptr(beta), ptr(o['mean_rstd']), ptr(o['dgamma']), ptr(o['dbeta']), ptr(o['coef']),
                                                ptr(o['scratch_b']), B, HW, C, G, 1, st))
                    row('gn_fwd' + tag, label, lambda: fwd(old, oa), lambda: fwd(new, ob))
                    row('gn_bwd' + tag, label, lambda: bwd(old, oa, None), lambda: bwd(new, ob, None))
                    row('gn_bwd_radd' + tag, label, lambda: bwd(old, oa, r), lambda: bwd(new, ob, r))
                opt('gn_resident', 192)
                del x, dy, r, oa, ob
            for M, C in ((262144, 320), (65536, 640), (16384, 1280)):
                x, dy, gamma, beta = rnd(M, C, dtype=BF), rnd(M, C, dtype=BF), 1 + 0.25 * rnd(C), rnd(C)
                oa, ob = (ln_bufs(M, C, None) for _ in libs)
                label = f'{M}x{C} pass {rep}'
                row('ln_fwd', label, lambda: ok(ln_fwd(old, oa, x, gamma, beta, M, C)), lambda: ok(ln_fwd(new, ob, x, gamma, beta, M, C)))
                row('ln_bwd', label, lambda: ok(ln_bwd(old, oa, x, dy, None, gamma, M, C)), lambda: ok(ln_bwd(new, ob, x, dy, None, gamma, M, C)))
                ca, cb = (dict(out=sent(C), scratch=sent(256 * C * 2)) for _ in libs)
                row('colsum_accum', label, lambda: ok(colsum(old, ca, x, M, C)), lambda: ok(colsum(new, cb, x, M, C)))
                del x, dy, oa, ob
            for B, HW, C in ((256, 1024, 320), (256, 64, 1280)):
                x = rnd(B * HW, C, dtype=BF)
                oa, ob = (dict(out=sent(B, C, dtype=BF), db=sent(C), scratch=sent(int(new.da_norm_scratch_floats(B, HW, C)))) for _ in libs)
                row('image_colsum', f'B={B} HW={HW} C={C} pass {rep}', lambda: ok(image_colsum(old, oa, x, B, HW, C)),
                    lambda: ok(image_colsum(new, ob, x, B, HW, C)))
                del x
        for op, pcts in spread.items():
            med = sorted(pcts)[len(pcts) // 2]
            print(f'norms spread {op:20s}: median {med:+5.1f} %, rows {min(pcts):+5.1f} ... {max(pcts):+5.1f} % ({len(pcts)} rows)', flush=True)


if __name__ == '__main__':
    main()
