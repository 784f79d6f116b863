// The noise stream of the stochastic samplers: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel Random Numbers: As Easy as
// 1, 2, 3", SC'11) and Box-Muller, in plain 32-bit integer and fp32 arithmetic.  One call serves one pixel of one image and four
// channels of it:
//   key     = (seed & 0xffffffff, seed >> 32)          the image's own uint64 seed
//   counter = (pix, draw, stream, block)               pix = h W + w; stream 0: step noise, 1: initial latents; block = c / 4
//   (r0, r1) -> channels 4 block + {0, 1},  (r2, r3) -> channels 4 block + {2, 3}
// tests/philox_reference.py restates all of it in NumPy; the words are bit-exact against it, the normals within 2e-5.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace philox {

constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;  // the round multipliers
constexpr uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;  // the Weyl constants the key is bumped by

// ten rounds; the key is bumped between rounds (nine times)
__device__ __forceinline__ void words(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                      uint32_t r[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  r[0] = c0, r[1] = c1, r[2] = c2, r[3] = c3;
}

// One Box-Muller pair: u = ((ra >> 9) + 0.5) 2^-23 is exact and lies in (0, 1); theta / pi = (rb >> 8) 2^-23 is exact too, so
// sincospif sees the angle without a rounded 2 pi.  The accurate logf / sincospif / sqrtf: no fast-math intrinsic.
__device__ __forceinline__ void pair(uint32_t ra, uint32_t rb, float& z_even, float& z_odd) {
  const float u = ((float)(ra >> 9) + 0.5f) * 0x1p-23f;
  const float t = (float)(rb >> 8) * 0x1p-23f;
  float sn, cs;
  sincospif(t, &sn, &cs);
  const float r = sqrtf(-2.0f * logf(u));
  z_even = r * cs;
  z_odd = r * sn;
}

// the four normals of channel block `block` at pixel `pix` of the image seeded `seed`
__device__ __forceinline__ void normals(uint64_t seed, uint32_t pix, uint32_t draw, uint32_t stream, uint32_t block,
                                        float z[4]) {
  uint32_t r[4];
  words(pix, draw, stream, block, (uint32_t)seed, (uint32_t)(seed >> 32), r);
  pair(r[0], r[1], z[0], z[1]);
  pair(r[2], r[3], z[2], z[3]);
}

// v + k z with the product and the sum each rounded, never contracted into an FMA: how a draw is added wherever the result
// is defined as the torch expression v + k * z (the two-step samplers' noise term, the training noise's offset and
// perturbation terms)
__device__ __forceinline__ float add_scaled_unfused(float v, float k, float z) {
#pragma clang fp contract(off)
  const float kz = k * z;
  return v + kz;
}

}  // namespace philox
