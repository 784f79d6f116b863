"""Shared by tests/test_conv_rect_gpu.py, tests/test_inception_hip_gpu.py and tests/test_fid_host.py: the float64 reference of
da_conv2d_relu_fwd (an explicit gather, then one matrix product), the per-element bound of its float cases and the case
tables of the exact cases."""
import torch

F64 = torch.float64

# one c2 for the three input kinds, at most 2x the worst measured on MI355X: randn 3.5e-05, rows 0
# (every element within one ulp), cancel 1.86e-03 (1x1 on 64 channels: at small K the K-proportional term is small and
# a cancelling sum shows the fp32 roundings), the launches of the Inception walk 3.9e-04.  da_gemm_nt's own: 2.5e-03
BOUNDS = {'randn.c2': 3.7e-03, 'rows.c2': 3.7e-03, 'cancel.c2': 3.7e-03}


def out_size(H, W, kh, kw, s, ph, pw):
    return (H + 2 * ph - kh) // s + 1, (W + 2 * pw - kw) // s + 1


def gather(X, B, H, W, kh, kw, s, ph, pw):
    """X [B*H*W, Cin] float -> float64 [B*Hout*Wout, kh*kw*Cin]"""
    dev = X.device
    Ho, Wo = out_size(H, W, kh, kw, s, ph, pw)
    b = torch.arange(B, device=dev).view(B, 1, 1, 1, 1)
    ih = (torch.arange(Ho, device=dev) * s - ph).view(1, Ho, 1, 1, 1) + torch.arange(kh, device=dev).view(1, 1, 1, kh, 1)
    iw = (torch.arange(Wo, device=dev) * s - pw).view(1, 1, Wo, 1, 1) + torch.arange(kw, device=dev).view(1, 1, 1, 1, kw)
    ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
    idx = torch.where(ok, (b * H + ih) * W + iw, torch.full_like(b, B * H * W)).reshape(B * Ho * Wo, kh * kw)
    Xz = torch.cat([X.double(), torch.zeros(1, X.shape[1], dtype=F64, device=dev)])
    return Xz[idx].reshape(B * Ho * Wo, kh * kw * X.shape[1])


def reference(X, Wt, bias, geo, relu):
    Ag = gather(X, *geo)
    ref = Ag @ Wt.double().t()
    absprod = Ag.abs() @ Wt.double().abs().t()
    if bias is not None:
        ref = ref + bias.double()
        absprod = absprod + bias.double().abs()
    return (ref.clamp(min=0) if relu else ref), absprod


def ulp_bf16(ref):
    _, e = torch.frexp(ref)
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - 8))


# (name, kh, kw, stride, ph, pw, ((H, W), ...)): the last size of a padded form is smaller than the form's reach
FORMS = [
    ('3x3s2', 3, 3, 2, 0, 0, ((9, 7), (8, 10))),
    ('3x3', 3, 3, 1, 0, 0, ((5, 7),)),
    ('3x3p1', 3, 3, 1, 1, 1, ((5, 7), (1, 2))),
    ('1x1', 1, 1, 1, 0, 0, ((3, 5),)),
    ('5x5p2', 5, 5, 1, 2, 2, ((6, 9), (2, 3))),
    ('1x7p03', 1, 7, 1, 0, 3, ((5, 9), (4, 3))),
    ('7x1p30', 7, 1, 1, 3, 0, ((9, 5), (2, 5))),
    ('1x3p01', 1, 3, 1, 0, 1, ((4, 6), (3, 1))),
    ('3x1p10', 3, 1, 1, 1, 0, ((6, 4), (1, 3))),
]
CINS, COUTS = (8, 48, 80, 160, 448), (32, 80, 192, 448)


def _exact_cases():
    cases, k = [], 0
    for name, kh, kw, s, ph, pw, sizes in FORMS:
        for H, W in sizes:
            for Cin in CINS:
                if kh * kw * Cin > 4032:
                    continue
                Cout, B, relu, tile = COUTS[k % 4], (1, 3)[(k // 4) % 2], bool((k // 2) % 2), (0, 32, 0, 64, 0, 96)[k % 6]
                cases.append((f'{name}-{H}x{W}-b{B}-c{Cin}-n{Cout}-r{int(relu)}-t{tile}', (B, H, W, kh, kw, s, ph, pw), Cin, Cout,
                              relu, tile))
                k += 1
    return cases


EXACT_CASES = _exact_cases()
# each tile width, Cout below / at / past it; 3 images of 11 x 13 = 429 rows = 3 row tiles + 45
TILE_CASES = [(f'tile{t}-n{n}', (3, 11, 13, 3, 3, 1, 1, 1), 48, n, True, t)
              for t in (32, 64, 96) for n in (t - 8, t, t + 8)]
LARGE_CASE = [('large-449x453-c8-n448', (1, 449, 453, 3, 3, 2, 0, 0), 8, 448, True, 0)]
