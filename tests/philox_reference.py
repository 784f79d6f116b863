"""NumPy restatement of the stochastic samplers' noise stream (csrc/philox.hpp): Philox4x32-10 and Box-Muller.

    key     = (seed & 0xffffffff, seed >> 32)        the image's own uint64 seed
    counter = (pix, draw, stream, block)             pix = h W + w; stream 0: step noise, 1: initial latents; block = c // 4
    (r0, r1) -> channels 4 block + {0, 1},  (r2, r3) -> channels 4 block + {2, 3}; for a pair (ra, rb)
    u = ((ra >> 9) + 0.5) 2^-23,  theta = 2 pi (rb >> 8) 2^-24,  z_even = sqrt(-2 ln u) cos theta,  z_odd = ... sin theta

The words are integers (the device must match them bit for bit); the normals are float64 here, or the same formula in
float32 (``dtype=np.float32``), which is how the fp32-against-float64 error of the formula itself is measured."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

# (counter, key, output): the Random123 known-answer vectors of philox4x32-10
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK, MASK, MASK, MASK), (MASK, MASK), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(counter, key):
    """counter: four broadcastable uint64 arrays holding 32-bit values; key: two Python ints.  Returns four uint64 arrays of
    32-bit words."""
    c0, c1, c2, c3 = [np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2        # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(MASK), p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def box_muller(ra, rb, dtype=np.float64):
    ra, rb = np.asarray(ra, dtype=np.uint64), np.asarray(rb, dtype=np.uint64)
    f = dtype
    u = ((ra >> np.uint64(9)).astype(f) + f(0.5)) * f(2.0**-23)
    theta = f(2.0 * np.pi) * ((rb >> np.uint64(8)).astype(f) * f(2.0**-24))
    r = np.sqrt(f(-2.0) * np.log(u))
    return r * np.cos(theta), r * np.sin(theta)


def words(seed, draw, stream, C, H, W):
    """The raw words behind image ``seed``'s [C, H, W] draw: uint32 [4 ceil(C / 4), H, W]."""
    seed = int(seed)
    assert 0 <= seed < 2**64
    key = (seed & MASK, seed >> 32)
    pix = np.arange(H * W, dtype=np.uint64)
    out = []
    for blk in range((C + 3) // 4):
        out += list(philox4x32_10((pix, np.uint64(int(draw) & MASK), np.uint64(stream), np.uint64(blk)), key))
    return np.stack(out).astype(np.uint32).reshape(-1, H, W)


def randn(seeds, draw, stream, C, H, W, dtype=np.float64):
    """The normals [B, C, H, W] of the images seeded ``seeds`` (what da_randn_philox writes with kind 0)."""
    res = []
    for seed in seeds:
        r = words(seed, draw, stream, C, H, W)
        z = []
        for blk in range(r.shape[0] // 4):
            ze, zo = box_muller(r[4 * blk], r[4 * blk + 1], dtype)
            z += [ze, zo]
            ze, zo = box_muller(r[4 * blk + 2], r[4 * blk + 3], dtype)
            z += [ze, zo]
        res.append(np.stack(z[:C]))
    return np.stack(res)
