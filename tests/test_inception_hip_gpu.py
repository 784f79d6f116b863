"""InceptionV3HIP (models/inception_hip.py) against the plain torch.nn FID Inception of tests/inception_reference.py.

The reference module is random-init (He) with live BatchNorm statistics (gamma in [0.5, 1.5], beta, mean ~ N(0, 0.1), variance
in [0.5, 2]); the input is two 64 x 96 uint8 images of different kinds.  A collapsed random tower would pass anything, so the
reference alone must first show that the two images' features differ by rel-L2 > 0.1 and that the features' standard
deviation over the 2048 dimensions exceeds 1e-3 of their mean magnitude (measured on the CPU: 0.58 and 1.4).

(a) launch by launch: every convolution and pool of the HIP walk against float64 of that one launch on the walk's own bf16
    input and the tower's own folded bf16 weights / fp32 bias.  Convolutions: the per-element bound of
    tests/test_conv_rect_gpu.py's float cases with its measured c2 (tests/conv_rect_reference.py).  Pools: the maximum is
    exact; the average is the float64 average within 9 fp32 roundings (8 additions of non-negative values, one division: 9 * 2^-24 relative), rounded once.
(b) the 11 Mixed outputs and the 2048-d features against the fp32 CPU run of the whole reference by rel-L2.  The bar is what
    torch's own bf16 run of the same module on the GPU achieves against that fp32 reference: the HIP tower may be at most
    2x that, per output.  Measured on an MI355X: see DESIGN.md section 4.8 (recorded through tests/parity_margins.py).
"""
import pytest
import torch

import conv_rect_reference as CT
import inception_reference as IR
import parity_margins

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


@pytest.fixture(scope='module')
def setup(dev):
    from diffusion_amd.models.inception_hip import InceptionV3HIP
    net = IR.seeded_module()
    images = IR.seeded_images()
    x = torch.from_numpy(IR.preprocess_f64(images.numpy())).float()
    with torch.no_grad():
        feats, mixed = net(x)
    tower = InceptionV3HIP(net.state_dict(), dev)
    return net, images, x, feats, mixed, tower


def test_reference_is_not_collapsed(setup):
    _, _, _, feats, mixed, _ = setup
    d = ((feats[0] - feats[1]).norm() / feats[0].norm()).item()
    spread = (feats.std(dim=1) / feats.abs().mean(dim=1)).min().item()
    print(f'feature rel-L2 between the two images {d:.3f}; std / mean magnitude {spread:.3f}')
    assert d > 0.1 and spread > 1e-3
    assert all(bool((m > 0).any()) for m in mixed)


def rne_bf16(x):
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 256.0), e - 8)


def test_launch_by_launch(setup, dev):
    _, images, _, _, _, tower = setup
    B = images.shape[0]
    P = tower.plan
    c2 = max(CT.BOUNDS.values())
    seen = {'conv': 0, 'pool': 0}
    worst = {'conv_c2': 0.0, 'unit': None}

    def trace(op, X, Y):
        torch.cuda.synchronize()
        if op[0] == 'conv':
            unit, src = op[1], op[2]
            cin, cout, kh, kw, s, ph, pw = P.units[unit]
            side = P.bufs[src][0]
            W, bias = tower.units[unit]
            ref, absprod = CT.reference(X.float(), W.float(), bias, (B, side, side, kh, kw, s, ph, pw), True)
            K = kh * kw * cin
            err = (Y.double() - ref).abs()
            assert bool(torch.isfinite(err).all()), unit
            over = (err - CT.ulp_bf16(ref)).clamp(min=0) / (2.0 ** -24 * K * absprod).clamp(min=1e-300)
            if over.max().item() > worst['conv_c2']:
                worst['conv_c2'], worst['unit'] = over.max().item(), unit
            assert bool((Y > 0).any()), f'{unit}: all-zero output'
        else:
            _, kind, s, p, src, dst, col = op
            side, C = P.bufs[src]
            x = X.cpu().double().view(B, side, side, C).permute(0, 3, 1, 2).contiguous()   # the CPU's float64 pools
            y = Y.cpu().double()
            if kind == 0:
                ref = torch.nn.functional.max_pool2d(x, 3, stride=s, padding=p)
            else:
                ref = torch.nn.functional.avg_pool2d(x, 3, stride=s, padding=p, count_include_pad=False)
            ref = ref.permute(0, 2, 3, 1).reshape(y.shape)
            if kind == 0:
                assert torch.equal(y, ref), f'max pool {src}'
            else:
                assert bool((x >= 0).all())   # post-ReLU: partial sums never exceed the total
                a = 9 * 2.0 ** -24
                lo, hi = rne_bf16(ref * (1 - a)), rne_bf16(ref * (1 + a))
                bad = (y < lo) | (y > hi)
                if bool(bad.any()):
                    i = tuple(bad.nonzero()[0].tolist())
                    raise AssertionError(f'avg pool {src}: {int(bad.sum())} outside one rounding, first {i}: got {y[i].item()!r}, '
                                         f'float64 {ref[i].item()!r}, interval [{lo[i].item()!r}, {hi[i].item()!r}]')
        seen[op[0]] += 1

    tower(images, trace=trace)
    assert seen == {'conv': 94, 'pool': 13}
    print(f'launch by launch: worst conv c2 {worst["conv_c2"]:.3e} at {worst["unit"]} (bound {c2:.3e})')
    parity_margins.record('inception_launches', tolerances={'conv_c2': c2}, **worst)
    assert worst['conv_c2'] <= c2, f'{worst["unit"]}: c2 {worst["conv_c2"]:.3e} > {c2:.3e}'


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_tower_against_fp32_reference_within_2x_of_bf16_torch(setup, dev):
    net, images, x, feats, mixed, tower = setup
    B = images.shape[0]
    got = {}
    f_hip = tower(images)
    # the Mixed buffers are distinct and written once per walk: read them after it
    for name, ref in zip(IR.MIXED, mixed):
        side, C = tower.plan.bufs[name]
        got[name] = tower._buffers(B)[name].float().view(B, side, side, C).permute(0, 3, 1, 2).cpu()
    got['pool3'] = f_hip.cpu()
    import copy
    net16 = copy.deepcopy(net).to(dev, BF)
    with torch.no_grad():
        f16, m16 = net16(x.to(dev, BF))
    torch.cuda.synchronize()
    bf = {name: m.float().cpu() for name, m in zip(IR.MIXED, m16)}
    bf['pool3'] = f16.float().cpu()
    refs = dict(zip(IR.MIXED, mixed))
    refs['pool3'] = feats
    hip_rel, bf_rel = {}, {}
    for name in list(IR.MIXED) + ['pool3']:
        hip_rel[name], bf_rel[name] = _rel(got[name], refs[name]), _rel(bf[name], refs[name])
        print(f'{name}: HIP {hip_rel[name]:.3e}, bf16 torch {bf_rel[name]:.3e}, ratio {hip_rel[name] / bf_rel[name]:.2f}')
    parity_margins.record('inception_tower', tolerances={'hip_over_bf16_torch': 2.0},
                          **{f'hip_{k}': v for k, v in hip_rel.items()}, **{f'bf16_torch_{k}': v for k, v in bf_rel.items()})
    for name in hip_rel:
        assert hip_rel[name] <= 2.0 * bf_rel[name], (name, hip_rel[name], bf_rel[name])
    # the two images keep their distance through the HIP tower
    assert _rel(got['pool3'][0], got['pool3'][1]) > 0.1


def test_chunked_walk_and_float_input_match(setup, dev):
    """max_batch chunks give the bits of the one-batch walk per image; fp32 images (k + 0.5) / 255 give the uint8 features"""
    from diffusion_amd.models.inception_hip import InceptionV3HIP
    net, images, _, _, _, tower = setup
    imgs3 = torch.cat([images, images[:1]])
    whole = tower(imgs3).cpu()
    small = InceptionV3HIP(net.state_dict(), dev, max_batch=2)
    assert torch.equal(small(imgs3).cpu(), whole)
    # buffers are allocated once per batch size: the chunk of 2 and the rest of 1 each keep theirs over a second call
    kept = {B: bufs['x'].data_ptr() for B, bufs in small._bufs.items()}
    assert set(kept) == {1, 2}
    assert torch.equal(small(imgs3).cpu(), whole) and kept == {B: bufs['x'].data_ptr() for B, bufs in small._bufs.items()}
    as_float = (images.float() + 0.5) / 255.0
    assert torch.equal(tower(as_float).cpu(), whole[:2])


def test_strict_loader(setup, dev, tmp_path):
    from diffusion_amd.models import inception_hip as IH
    net, images, _, _, _, tower = setup
    sd = net.state_dict()
    path = tmp_path / 'inception.pth'
    torch.save(sd, path)
    loaded = IH.load_state_dict_file(str(path))
    assert set(loaded) == set(sd)
    assert torch.equal(IH.InceptionV3HIP(loaded, dev)(images).cpu(), tower(images).cpu())
    for drop in ('Mixed_6c.branch7x7dbl_3.bn.running_var', 'Conv2d_1a_3x3.conv.weight'):
        torch.save({k: v for k, v in sd.items() if k != drop}, path)
        with pytest.raises(RuntimeError):
            IH.load_state_dict_file(str(path))
    bad = dict(sd)
    bad['Mixed_7a.branch3x3_2.conv.weight'] = bad['Mixed_7a.branch3x3_2.conv.weight'][:, :, :1]
    torch.save(bad, path)
    with pytest.raises(RuntimeError):
        IH.load_state_dict_file(str(path))
