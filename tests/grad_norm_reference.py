"""Shared by tests/test_grad_norm_host.py and tests/test_grad_norm_gpu.py (not collected by pytest): hand-made segment
layouts, the float64 reference, a numpy emulation of da_segment_sumsq's three-stage summation order, and the bounds both
modules assert."""
import numpy as np

from diffusion_amd.models.unet import SUMSQ_CHUNK as CH, SumsqTables

GAP = 64   # FlatParams.ALIGN: storages start at multiples of 64 floats, the words in between belong to nobody

# Relative error of a segment's (and the total's) fp32 sum of squares against float64 of the same fp32 inputs.
# Worst case of the order: a chunk partial is 8 sequential fp32 adds per lane component, 2 adds over the 4 components, head
# and tail (2), 6 butterfly levels and 3 adds over the waves = 21 roundings plus one for each square = 22 x 2^-24 = 1.3e-6;
# stages 2 and 3 add in fp64 and round once each.  Rounding errors of random data add like a random walk, far below that:
# measured on the MI355X (profiles/grad_norm_margins.json) the worst case is 7.86e-8 per segment and 5.97e-8 for a total;
# asserted: 2 x measured, rounded down.
SEG_REL_BOUND = 1.5e-7
TOTAL_REL_BOUND = 1.1e-7

EXACT_SIZES = [1, 3, 4, 5, 63, 64, 65, CH - 1, CH, CH + 1, 2 * CH + 5, 262144]


def gapped_layout(sizes, shifts=None):
    """Segments of the given sizes at 64-float aligned offsets (as FlatParams lays storages out), each start moved by
    shifts[i] floats (default 0), with at least one gap word between neighbours.  Returns ([(off, n)], total length)."""
    segs, off = [], 0
    for i, n in enumerate(sizes):
        sh = shifts[i] if shifts else 0
        segs.append((off + sh, n))
        off = -(-(off + sh + n + 1) // GAP) * GAP
    return segs, off


def fill(segs, total, values):
    """float32 buffer of `total` words: NaN everywhere, values[i] (float32 array) in segment i."""
    x = np.full(total, np.nan, dtype=np.float32)
    for (off, n), v in zip(segs, values):
        assert v.dtype == np.float32 and v.shape == (n,)
        x[off:off + n] = v
    return x


def reference(x, segs):
    """float64 sums of squares of the fp32 words actually stored: per segment and their total."""
    per = np.array([np.sum(x[o:o + n].astype(np.float64)**2) for o, n in segs])
    return per, float(np.sum(per))


def _butterfly(v):
    """The xor butterfly of wave_sum over 64 lanes (offsets 32 .. 1); every lane ends with the same value."""
    v = v.copy()
    o = 32
    while o:
        v = v + v[np.arange(64) ^ o]
        o >>= 1
    return v[0]


def emulate_chunk(x, off, n):
    """fp32 partial of one chunk in the kernel's order (products rounded separately: the GPU contracts them into FMAs)."""
    f = np.float32
    head = min((4 - (off & 3)) & 3, n)
    nvec = (n - head) >> 2
    tail = n - head - 4 * nvec
    body = x[off + head:off + head + 4 * nvec].reshape(nvec, 4)
    rounds = -(-nvec // 256) if nvec else 0
    pad = np.zeros((rounds * 256, 4), dtype=f)
    pad[:nvec] = body
    acc = np.zeros((256, 4), dtype=f)
    for k in range(rounds):
        v = pad[k * 256:(k + 1) * 256]
        acc = acc + v * v
    s = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
    h = np.zeros(256, dtype=f)
    h[:head] = x[off:off + head]
    s = s + h * h
    t = np.zeros(256, dtype=f)
    t[:tail] = x[off + head + 4 * nvec:off + n]
    s = s + t * t
    w = [_butterfly(s[i * 64:(i + 1) * 64]) for i in range(4)]
    return f(f(f(w[0] + w[1]) + w[2]) + w[3])


def _strided_f64(vals, lanes):
    a = np.zeros(lanes, dtype=np.float64)
    for i, v in enumerate(vals):
        a[i % lanes] += np.float64(v)
    return a


def emulate(x, segs):
    """(seg_sumsq fp32 [n_segs], total fp32) in the order of the three launches."""
    tb = SumsqTables(segs)
    partial = np.array([emulate_chunk(x, off, n) for off, n, _ in tb.chunks], dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        seg = np.array([np.float32(_butterfly(_strided_f64(partial[first:first + cnt], 64))) for first, cnt in tb.segs],
                       dtype=np.float32)
        a = _strided_f64(seg, 256)
        w = [_butterfly(a[i * 64:(i + 1) * 64]) for i in range(4)]
        return seg, np.float32(((w[0] + w[1]) + w[2]) + w[3])


def float_case_values(rng, sizes):
    """The float cases of both modules: N(0,1) at per-segment scales 1e-3 .. 1e3, then a segment holding a few 1e18 (squares
    finite in fp32) among N(0,1), then one whose squares underflow to 0 (1e-30), as float32."""
    scales = np.logspace(-3, 3, num=len(sizes))
    vals = [(rng.standard_normal(n) * s).astype(np.float32) for n, s in zip(sizes, scales)]
    big = rng.standard_normal(1000).astype(np.float32)
    big[[7, 500, 999]] = 1e18
    tiny = np.full(300, 1e-30, dtype=np.float32)
    return vals + [big, tiny], list(sizes) + [1000, 300]


def clip_reference(sumsq32, grad_scale, max_norm):
    """torch.nn.utils.clip_grad_norm_'s formula in float64 from the fp32 total: (norm, multiplier).  Where the norm is at or
    under the threshold the formula still gives max_norm / (norm + 1e-6) < 1 for norm within 1e-6 of it; the record is
    exactly grad_scale there (the tests assert equality in those cases, the formula in the others)."""
    norm = float(np.sqrt(np.float64(sumsq32))) * grad_scale
    coef = 1.0 if max_norm <= 0 else min(1.0, max_norm / (norm + 1e-6))
    return norm, grad_scale * coef
