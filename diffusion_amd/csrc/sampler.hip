// One launch per denoising step of generate(): classifier-free guidance, the scheduler update and the next U-Net input.
// Every step of the DDIM (eta = 0) and continuous-time (ODE / Euler-Maruyama) schedulers is linear in (sample, model
// output, noise draw), so the host reduces a step to three coefficients (step_coefficients of the schedulers) and this
// kernel applies them to the sampler's state, which stays in the U-Net's own layout (NHWC-8 fp32) between steps:
//   m     = cfg ? pu + g (pt - pu) : p          (the reference's operation order)
//   x_out = cx x + cm m (+ cn z)                fp32, channels C..7 exactly 0
//   xt    = bf16(x_out)                         written `copies` times: both guidance halves of the next U-Net batch
// The coefficients are read from device memory, so the launch can sit in a captured graph and the host only copies the
// step's 16-byte row.  HBM-bound: one work item is one pixel, 16-byte accesses along the channel axis; the noise draw is
// read where torch.randn left it (NCHW, as da_add_noise reads eps).
// A sample that starts from an image (image-to-image, inpainting) adds da_sampler_init, the start of a partial schedule in
// one launch, and the blended forms of both steps: outside a per-pixel mask the state is replaced by the known sample
// re-noised to the level of the next timestep.
// The step is the product {first-order, two-step} x {plain, blended} x {plain, rescaled}: eight C entries, and behind them
// ONE kernel body (sampler_step_kernel<MS, BLEND, RS>) and ONE host path (step<MS, BLEND, RS>: the argument rules and the
// launch).  What a form does not use is an empty operand struct and code under `if constexpr`, so the plain instantiations
// are the kernels they were before the other forms existed.
// A ninth entry, da_sampler_step_rng, is any of the eight forms with the noise term drawn inside the kernel (RNG: philox.hpp,
// keyed by the image's seed, the step's draw number and the pixel), so a stochastic step is one launch, can sit in a captured
// graph (the draw number is device data like the coefficients) and gives an image the same noise in any batch.
#include "common.hpp"
#include "diffusion_amd.h"
#include "philox.hpp"

namespace {

constexpr int SMP_BLOCK = 256;
// the unmasked step kernels keep the compiler's default bound (and with it their code); the masked forms and the init kernel
// hold more operands per pixel and are bounded by the block they are launched with, or they would spill
constexpr int SMP_MAX_BLOCK = 1024;
#define GRID_STRIDE(i, n) \
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

// The blend of the masked forms, per pixel with its mask value m (broadcast over the channels) and the step's (bA, bS):
//   kn    = bA known8 + bS eps8                 the known sample at the noise level of the next timestep
//   x_out = m v + (1 - m) kn                    in exactly this form
// m == 1 gives v's bits (1 v + 0 kn), m == 0 gives kn's (0 v + 1 kn) and (bA, bS) = (1, 0) makes kn known8's bits, whichever
// product the compiler folds into an FMA: the other one is an exact 0 or the exact operand either way.
template <bool BLEND>
struct Blend {
  const float *known8, *eps8, *mask;
};
template <>
struct Blend<false> {};  // the unmasked kernels: the operand list they always had

// Guidance rescale (Lin et al., arXiv:2305.08891, section 3.4): the guided prediction m of sample b is multiplied by
// factor[b] (guidance_rescale_kernel below writes it) before the scheduler update.  hw is the sample's pixel count.
template <bool RS>
struct Rescale {
  const float* factor;
  int hw;
};
template <>
struct Rescale<false> {};  // the plain kernels: the operand list and the arithmetic they always had

// The operand only one order of the step has.  First order: the noise draw (NCHW, NULL without one) and HW, the pixel count
// of one sample, which indexes it.  Two-step: the previous step's data prediction, read iff k1 != 0 and then overwritten.
template <bool MS>
struct Form {
  const float* noise;
  int HW;
};
template <>
struct Form<true> {
  float* hist;
};

// The in-kernel draw: one uint64 seed per sample, and HW, the sample's pixel count (a pixel's counter is its index in its
// own image).  The row of an RNG form is wider: first order {cx, cm, cn, guidance, bA, bS, draw, 0}, two-step {ax, am, kx, k0,
// k1, guidance, bA, bS, kn, draw, 0, 0}; draw is a uint32 bit pattern in a float slot.
template <bool RNG>
struct Rng {
  const uint64_t* seeds;
  int HW;
};
template <>
struct Rng<false> {};  // the eight entries without it: the operand list and the code they always had

// v + k z with the product and the sum each rounded (philox.hpp): the two-step forms' noise term is defined as the torch
// expression x += kn * z on the deterministic update, so it must not contract into an FMA
using philox::add_scaled_unfused;

// The step, every form of it.  First order (MS = false), coef = {cx, cm, cn, guidance} and, BLEND, {bA, bS, 0, 0} after it:
//   m     = cfg ? pu + g (pt - pu) : p
//   v     = cx x + cm m (+ cn z)
// Two-step (MS: DPM-Solver++ 2M, one operand wider), coef = {ax, am, kx, k0, k1, guidance, bA, bS}: the host reduces a step
// to five coefficients (DPMSolverMultistepScheduler.step_coefficients_ms) and the kernel carries the previous step's data
// prediction in `hist`:
//   m     = cfg ? pu + g (pt - pu) : p
//   d     = ax x + am m                         the data prediction x0 of this step
//   v     = kx x + k0 d (+ k1 hist)             k1 == 0 (a first-order step): hist is not read, it may hold anything
//   hist  = d
// k1 comes from device memory like the rest, so one captured launch serves first- and second-order steps alike.
// RNG (any form): z is philox::normals(seed of the pixel's sample, pixel in the sample, draw, stream 0) and
//   v    += cn z  (first order: what the noise operand does)      v = v + kn z  (two-step: add_scaled_unfused)
// drawn iff the coefficient is not 0, which is uniform across the launch; hist keeps the noise-free data prediction.
// Every form: RS multiplies m by the sample's factor first, BLEND replaces v by m v + (1 - m) kn last, and
//   x_out = v,  xt = bf16(v)                    channels C..7 of x_out, xt and hist exactly 0
// every load of a pixel comes before its first store, and a pixel is read and written by one thread only: x_out may be x
template <bool MS, bool BLEND, bool RS, bool RNG = false>
__global__ void __launch_bounds__((BLEND || RS || RNG) ? SMP_BLOCK : SMP_MAX_BLOCK)
    sampler_step_kernel(const float* pred, const float* x, Form<MS> fm, const float* coef, float* x_out, bf16* xt_out,
                        long npix, int C, int cfg, int copies, Blend<BLEND> bl, Rescale<RS> rs, Rng<RNG> rg) {
  const f32x4 ka = *reinterpret_cast<const f32x4*>(coef);
  f32x4 kb = {0, 0, 0, 0};  // the second half of the row: the first-order form has (and reads) one only when blended or RNG
  if constexpr (MS || BLEND || RNG) kb = *reinterpret_cast<const f32x4*>(coef + 4);
  float kn_z = 0.f;     // the noise coefficient of an RNG form and its draw number, bit-cast after the vector load
  uint32_t draw = 0;
  if constexpr (RNG && MS) {
    const f32x4 kc = *reinterpret_cast<const f32x4*>(coef + 8);
    kn_z = kc[0], draw = __float_as_uint(kc[1]);
  } else if constexpr (RNG) {
    kn_z = ka[2], draw = __float_as_uint(kb[2]);
  }
  const bool draws = RNG && kn_z != 0.0f;  // uniform across the launch
  const float c0 = ka[0], c1 = ka[1];  // {cx, cm} or {ax, am}
  const float cn = ka[2], kx = ka[2], k0 = ka[3], k1 = kb[0];
  const float g = MS ? kb[1] : ka[3], bA = MS ? kb[2] : kb[0], bS = MS ? kb[3] : kb[1];
  const bool second = MS && k1 != 0.0f;  // uniform across the launch
  GRID_STRIDE(i, npix) {
    const f32x4 x0 = *reinterpret_cast<const f32x4*>(x + i * 8), x1 = *reinterpret_cast<const f32x4*>(x + i * 8 + 4);
    const f32x4 p0 = *reinterpret_cast<const f32x4*>(pred + i * 8), p1 = *reinterpret_cast<const f32x4*>(pred + i * 8 + 4);
    f32x4 q0 = p0, q1 = p1;
    if (cfg) {  // uniform: rows [npix, 2 npix) are the conditional half
      q0 = *reinterpret_cast<const f32x4*>(pred + (npix + i) * 8);
      q1 = *reinterpret_cast<const f32x4*>(pred + (npix + i) * 8 + 4);
    }
    f32x4 h0 = {0, 0, 0, 0}, h1 = {0, 0, 0, 0};
    if constexpr (MS) {
      if (second) {
        h0 = *reinterpret_cast<const f32x4*>(fm.hist + i * 8);
        h1 = *reinterpret_cast<const f32x4*>(fm.hist + i * 8 + 4);
      }
    }
    float kn[8] = {0, 0, 0, 0, 0, 0, 0, 0}, mk = 1.f;
    if constexpr (BLEND) {
      const f32x4 n0 = *reinterpret_cast<const f32x4*>(bl.known8 + i * 8),
                  n1 = *reinterpret_cast<const f32x4*>(bl.known8 + i * 8 + 4);
      const f32x4 e0 = *reinterpret_cast<const f32x4*>(bl.eps8 + i * 8), e1 = *reinterpret_cast<const f32x4*>(bl.eps8 + i * 8 + 4);
      mk = bl.mask[i];
#pragma unroll
      for (int c = 0; c < 8; ++c) kn[c] = bA * (c < 4 ? n0[c & 3] : n1[c & 3]) + bS * (c < 4 ? e0[c & 3] : e1[c & 3]);
    }
    long b = 0;
    int pix = 0;
    if constexpr (!MS && !RNG) {  // where the pixel's noise draw is
      b = i / fm.HW;
      pix = (int)(i - b * fm.HW);
    }
    float fac = 1.f;
    if constexpr (RS) fac = rs.factor[i / rs.hw];
    float z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (RNG) {
      if (draws) {
        const long bz = i / rg.HW;
        const uint32_t pz = (uint32_t)(i - bz * rg.HW);
        const uint64_t seed = rg.seeds[bz];
        philox::normals(seed, pz, draw, 0u, 0u, z);
        if (C > 4) philox::normals(seed, pz, draw, 0u, 1u, z + 4);  // uniform
      }
    }
    float o[8] = {0, 0, 0, 0, 0, 0, 0, 0}, d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c < C) {
        const float xv = c < 4 ? x0[c & 3] : x1[c & 3], pu = c < 4 ? p0[c & 3] : p1[c & 3];
        float m = pu;
        if (cfg) {
          const float pt = c < 4 ? q0[c & 3] : q1[c & 3];
          m = pu + g * (pt - pu);
        }
        if constexpr (RS) m *= fac;
        const float dv = c0 * xv + c1 * m;  // first order: the update itself; two-step: the data prediction
        float v = dv;
        if constexpr (MS) {
          v = kx * xv + k0 * dv;
          if (second) v += k1 * (c < 4 ? h0[c & 3] : h1[c & 3]);
          if constexpr (RNG) {
            if (draws) v = add_scaled_unfused(v, kn_z, z[c]);
          }
        } else if constexpr (RNG) {
          if (draws) v += cn * z[c];
        } else {
          if (fm.noise) v += cn * fm.noise[(b * C + c) * fm.HW + pix];
        }
        if constexpr (BLEND) v = mk * v + (1.f - mk) * kn[c];  // the history keeps the unblended data prediction
        if constexpr (MS) d[c] = dv;
        o[c] = v;
      }
    }
    if constexpr (MS) {
      *reinterpret_cast<f32x4*>(fm.hist + i * 8) = f32x4{d[0], d[1], d[2], d[3]};
      *reinterpret_cast<f32x4*>(fm.hist + i * 8 + 4) = f32x4{d[4], d[5], d[6], d[7]};
    }
    *reinterpret_cast<f32x4*>(x_out + i * 8) = f32x4{o[0], o[1], o[2], o[3]};
    *reinterpret_cast<f32x4*>(x_out + i * 8 + 4) = f32x4{o[4], o[5], o[6], o[7]};
    if (xt_out) {
      bf16x8 t;
#pragma unroll
      for (int c = 0; c < 8; ++c) t[c] = f2bf(o[c]);
      st8(xt_out + i * 8, t);
      if (copies == 2) st8(xt_out + (npix + i) * 8, t);
    }
  }
}

// The start of a partial schedule in one launch: the known (clean, scaled) sample and the noise draw, both NCHW as torch
// left them, go to the state's layout, the pixel mask to one value per state pixel, and the state starts at the noise level
// of the first executed timestep:
//   known8 = known, eps8 = noise                bit-exact relayouts (written iff known8 is given; eps8 goes with it)
//   mask   = (1 / f^2) sum of the f x f block   row by row, left to right: a fixed order; 1 / f^2 is exact (f = 2^k)
//   x      = a0 known + s0 noise,  xt = bf16(x) written `copies` times
// One work item is one state pixel; channels C..7 of every [., 8] output are exactly 0.
__global__ void __launch_bounds__(SMP_BLOCK)
    sampler_init_kernel(const float* known, const float* noise, const float* mask_px, const float* coef, float* known8,
                        float* eps8, float* mask, float* x, bf16* xt, long npix, int H, int W, int C, int f, int copies) {
  const f32x4 k = *reinterpret_cast<const f32x4*>(coef);
  const float a0 = k[0], s0 = k[1];
  const int HW = H * W;
  const float inv = 1.f / (float)(f * f);
  GRID_STRIDE(i, npix) {
    const long b = i / HW;
    const int pix = (int)(i - b * HW);
    float kv[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ev[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c < C) {
        kv[c] = known[(b * C + c) * HW + pix];
        ev[c] = noise[(b * C + c) * HW + pix];
        o[c] = a0 * kv[c] + s0 * ev[c];
      }
    }
    if (mask_px) {
      const int h = pix / W, w = pix - h * W;
      const float* blk = mask_px + ((b * H + h) * f) * ((long)W * f) + (long)w * f;
      float sum = 0.f;
      for (int dy = 0; dy < f; ++dy)
        for (int dx = 0; dx < f; ++dx) sum += blk[dy * ((long)W * f) + dx];
      mask[i] = sum * inv;
    }
    if (known8) {
      *reinterpret_cast<f32x4*>(known8 + i * 8) = f32x4{kv[0], kv[1], kv[2], kv[3]};
      *reinterpret_cast<f32x4*>(known8 + i * 8 + 4) = f32x4{kv[4], kv[5], kv[6], kv[7]};
      *reinterpret_cast<f32x4*>(eps8 + i * 8) = f32x4{ev[0], ev[1], ev[2], ev[3]};
      *reinterpret_cast<f32x4*>(eps8 + i * 8 + 4) = f32x4{ev[4], ev[5], ev[6], ev[7]};
    }
    *reinterpret_cast<f32x4*>(x + i * 8) = f32x4{o[0], o[1], o[2], o[3]};
    *reinterpret_cast<f32x4*>(x + i * 8 + 4) = f32x4{o[4], o[5], o[6], o[7]};
    if (xt) {
      bf16x8 t;
#pragma unroll
      for (int c = 0; c < 8; ++c) t[c] = f2bf(o[c]);
      st8(xt + i * 8, t);
      if (copies == 2) st8(xt + (npix + i) * 8, t);
    }
  }
}

// The statistics pass of guidance rescale: with pt the conditional half and m = pu + g (pt - pu), per sample b over its C
// valid channels and HW pixels
//   factor[b] = phi * std(pt) / std(m) + (1 - phi)          1 when std(m) == 0
// One workgroup of 1024 threads per sample and no second launch: a sample is 256-768 KiB of pred, a few microseconds for one
// CU beside a U-Net call of milliseconds, and a batch fills as many CUs as it has samples.  Both sums run in double on data
// shifted by the sample's first value (sum (x - k), sum (x - k)^2: no cancellation however large |mean| / std is), pred is
// read once, and the order is fixed: a thread's pixels in sequence, the wave butterfly, the 16 wave partials in wave order.
constexpr int GR_BLOCK = 1024;
__global__ void __launch_bounds__(GR_BLOCK)
    guidance_rescale_kernel(const float* pred, const float* coef, int g_index, float phi, float* factor, long npix, int HW,
                            int C) {
  __shared__ double sh[GR_BLOCK / 64][4];
  const float g = coef[g_index];
  const float* pu_s = pred + (long)blockIdx.x * HW * 8;
  const float* pt_s = pu_s + npix * 8;
  // m itself is formed in double from the fp32 operands: the statistics then carry no rounding of m, which matters for
  // samples of a few values; the step kernels' fp32 m differs from it by one rounding per element
  const double gd = (double)g, kt = (double)pt_s[0], km = (double)pu_s[0] + gd * ((double)pt_s[0] - (double)pu_s[0]);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};  // sum (pt - kt), sum (pt - kt)^2, sum (m - km), sum (m - km)^2
  for (int p = threadIdx.x; p < HW; p += GR_BLOCK) {
    const f32x4 p0 = *reinterpret_cast<const f32x4*>(pu_s + (long)p * 8), q0 = *reinterpret_cast<const f32x4*>(pt_s + (long)p * 8);
    f32x4 p1 = {0.f, 0.f, 0.f, 0.f}, q1 = {0.f, 0.f, 0.f, 0.f};
    if (C > 4) {  // uniform
      p1 = *reinterpret_cast<const f32x4*>(pu_s + (long)p * 8 + 4);
      q1 = *reinterpret_cast<const f32x4*>(pt_s + (long)p * 8 + 4);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c < C) {
        const float pu = c < 4 ? p0[c & 3] : p1[c & 3], pt = c < 4 ? q0[c & 3] : q1[c & 3];
        const double m = (double)pu + gd * ((double)pt - (double)pu);
        const double dt = (double)pt - kt, dm = m - km;
        acc[0] += dt;
        acc[1] += dt * dt;
        acc[2] += dm;
        acc[3] += dm * dm;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int w = 0; w < GR_BLOCK / 64; ++w)
      for (int k = 0; k < 4; ++k) s[k] += sh[w][k];
    const double n = (double)HW * (double)C;
    const double vt = s[1] - s[0] * s[0] / n, vm = s[3] - s[2] * s[2] / n;  // n var; the count cancels in the ratio
    double f = 1.0;
    if (vm > 0.0) f = (double)phi * sqrt((vt > 0.0 ? vt : 0.0) / vm) + (1.0 - (double)phi);
    factor[blockIdx.x] = (float)f;
  }
}

// one work item per pixel: ceil(npix / 256) blocks of 256, capped (the kernels stride over the rest)
unsigned pixel_grid(long npix) {
  const long blocks = (npix + SMP_BLOCK - 1) / SMP_BLOCK;
  return (unsigned)(blocks > 16384 ? 16384 : blocks);
}

// What a step entry was called with: the operands every form has, then the ones a form may have (NULL where it has none).
struct StepArgs {
  const float *pred, *x, *coef;
  float* x_out;
  void* xt_out;
  long npix;
  int HW, C, cfg, copies;
  hipStream_t s;
  const float* noise = nullptr;  // first order, optional
  float* hist = nullptr;         // two-step
  const float *known8 = nullptr, *eps8 = nullptr, *mask = nullptr;  // BLEND
  const float* factor = nullptr;                                    // RS
  const uint64_t* seeds = nullptr;                                  // RNG
};

// The argument rules of every step entry, each stated once, and the launch.
template <bool MS, bool BLEND, bool RS, bool RNG = false>
int step(const StepArgs& a) {
  // shapes; the two-step forms check HW like the rest, though only their RS forms read it
  if (a.npix <= 0 || a.HW <= 0 || (a.npix % a.HW) || a.C < 1 || a.C > 8 || (a.copies != 1 && a.copies != 2))
    return DA_ERR_SHAPE;
  // required: the common operands and the form's own; noise and xt_out are optional
  if (!a.pred || !a.x || !a.coef || !a.x_out) return DA_ERR_SHAPE;
  if (MS && !a.hist) return DA_ERR_SHAPE;
  if (BLEND && (!a.known8 || !a.eps8 || !a.mask)) return DA_ERR_SHAPE;
  if (RS && !a.factor) return DA_ERR_SHAPE;
  if (RNG && !a.seeds) return DA_ERR_SHAPE;
  // alignment: 16 bytes for every pointer given (the optional ones included), 4 for factor, 8 for seeds
  const uintptr_t ptrs = (uintptr_t)a.pred | (uintptr_t)a.x | (uintptr_t)a.coef | (uintptr_t)a.x_out | (uintptr_t)a.xt_out |
                         (uintptr_t)a.noise | (uintptr_t)a.hist | (uintptr_t)a.known8 | (uintptr_t)a.eps8 | (uintptr_t)a.mask;
  if ((ptrs & 15) || ((uintptr_t)a.factor & 3) || ((uintptr_t)a.seeds & 7)) return DA_ERR_SHAPE;
  Form<MS> fm;
  if constexpr (MS) fm = {a.hist};
  else fm = {a.noise, a.HW};
  Blend<BLEND> bl;
  if constexpr (BLEND) bl = {a.known8, a.eps8, a.mask};
  Rescale<RS> rs;
  if constexpr (RS) rs = {a.factor, a.HW};
  Rng<RNG> rg;
  if constexpr (RNG) rg = {a.seeds, a.HW};
  hipLaunchKernelGGL((sampler_step_kernel<MS, BLEND, RS, RNG>), dim3(pixel_grid(a.npix)), dim3(SMP_BLOCK), 0, a.s, a.pred,
                     a.x, fm, a.coef, a.x_out, (bf16*)a.xt_out, a.npix, a.C, a.cfg ? 1 : 0, a.copies, bl, rs, rg);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// da_randn_philox: one work item per (sample, pixel, channel block), NCHW stores (coalesced along the pixels of a channel)
__global__ void __launch_bounds__(SMP_BLOCK)
    randn_philox_kernel(const uint64_t* seeds, uint32_t draw, uint32_t stream, float* out, long nitem, int nblk, int C, int HW,
                        int kind) {
  GRID_STRIDE(i, nitem) {
    const long bk = i / HW;  // sample * nblk + block
    const uint32_t pix = (uint32_t)(i - bk * HW);
    const long b = bk / nblk;
    const uint32_t blk = (uint32_t)(bk - b * nblk);
    const uint64_t seed = seeds[b];
    float z[4];
    if (kind == 0) {  // uniform
      philox::normals(seed, pix, draw, stream, blk, z);
    } else {
      uint32_t r[4];
      philox::words(pix, draw, stream, blk, (uint32_t)seed, (uint32_t)(seed >> 32), r);
#pragma unroll
      for (int j = 0; j < 4; ++j) z[j] = __uint_as_float(r[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = (int)blk * 4 + j;
      if (c < C) out[(b * C + c) * HW + pix] = z[j];
    }
  }
}

}  // namespace

extern "C" int da_randn_philox(const unsigned long long* seeds, unsigned draw, unsigned stream, float* out, int B, int C,
                               int H, int W, int kind, hipStream_t s) {
  DA_CLEAR_ERR();
  if (B <= 0 || H <= 0 || W <= 0 || C < 1 || C > 8 || (long)H * W > 0x7fffffffL) return DA_ERR_SHAPE;
  if (stream > 1u || (kind != 0 && kind != 1) || (kind == 1 && (C % 4))) return DA_ERR_SHAPE;
  if (!seeds || !out || ((uintptr_t)seeds & 7) || ((uintptr_t)out & 15)) return DA_ERR_SHAPE;
  const int nblk = (C + 3) / 4, HW = H * W;
  const long nitem = (long)B * nblk * HW;
  hipLaunchKernelGGL(randn_philox_kernel, dim3(pixel_grid(nitem)), dim3(SMP_BLOCK), 0, s,
                     reinterpret_cast<const uint64_t*>(seeds), (uint32_t)draw, (uint32_t)stream, out, nitem, nblk, C, HW, kind);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// ---- the stochastic step: one entry, the form as a mask, the same StepArgs and step<...> with RNG on
extern "C" int da_sampler_step_rng(const float* pred, const float* x, float* hist, const float* coef, const float* known8,
                                   const float* eps8, const float* mask, const float* factor,
                                   const unsigned long long* seeds, float* x_out, void* xt_out, long npix, int HW, int C,
                                   int form, int cfg, int copies, hipStream_t s) {
  DA_CLEAR_ERR();
  if (form < 0 || form > 7) return DA_ERR_SHAPE;
  StepArgs a{pred, x, coef, x_out, xt_out, npix, HW, C, cfg, copies, s};
  a.seeds = reinterpret_cast<const uint64_t*>(seeds);
  if (form & 1) a.hist = hist;
  if (form & 2) a.known8 = known8, a.eps8 = eps8, a.mask = mask;
  if (form & 4) a.factor = factor;
  switch (form) {
    case 0: return step<false, false, false, true>(a);
    case 1: return step<true, false, false, true>(a);
    case 2: return step<false, true, false, true>(a);
    case 3: return step<true, true, false, true>(a);
    case 4: return step<false, false, true, true>(a);
    case 5: return step<true, false, true, true>(a);
    case 6: return step<false, true, true, true>(a);
    default: return step<true, true, true, true>(a);
  }
}

// ---- the eight step entries: the call's operands into a StepArgs, then step<MS, BLEND, RS>
extern "C" int da_sampler_step(const float* pred, const float* x, const float* noise, const float* coef, float* x_out,
                               void* xt_out, long npix, int HW, int C, int cfg, int copies, hipStream_t s) {
  DA_CLEAR_ERR();
  StepArgs a{pred, x, coef, x_out, xt_out, npix, HW, C, cfg, copies, s};
  a.noise = noise;
  return step<false, false, false>(a);
}

extern "C" int da_sampler_step_ms(const float* pred, const float* x, float* hist, const float* coef, float* x_out,
                                  void* xt_out, long npix, int HW, int C, int cfg, int copies, hipStream_t s) {
  DA_CLEAR_ERR();
  StepArgs a{pred, x, coef, x_out, xt_out, npix, HW, C, cfg, copies, s};
  a.hist = hist;
  return step<true, false, false>(a);
}

extern "C" int da_sampler_step_blend(const float* pred, const float* x, const float* noise, const float* coef,
                                     const float* known8, const float* eps8, const float* mask, float* x_out, void* xt_out,
                                     long npix, int HW, int C, int cfg, int copies, hipStream_t s) {
  DA_CLEAR_ERR();
  StepArgs a{pred, x, coef, x_out, xt_out, npix, HW, C, cfg, copies, s};
  a.noise = noise, a.known8 = known8, a.eps8 = eps8, a.mask = mask;
  return step<false, true, false>(a);
}

extern "C" int da_sampler_step_ms_blend(const float* pred, const float* x, float* hist, const float* coef,
                                        const float* known8, const float* eps8, const float* mask, float* x_out,
                                        void* xt_out, long npix, int HW, int C, int cfg, int copies, hipStream_t s) {
  DA_CLEAR_ERR();
  StepArgs a{pred, x, coef, x_out, xt_out, npix, HW, C, cfg, copies, s};
  a.hist = hist, a.known8 = known8, a.eps8 = eps8, a.mask = mask;
  return step<true, true, false>(a);
}

extern "C" int da_guidance_rescale(const float* pred, const float* coef, int g_index, float phi, float* factor, long npix,
                                   int HW, int C, hipStream_t s) {
  DA_CLEAR_ERR();
  if (npix <= 0 || HW <= 0 || (npix % HW) || C < 1 || C > 8 || g_index < 0 || g_index > 7) return DA_ERR_SHAPE;
  if (!(phi >= 0.f && phi <= 1.f) || !pred || !coef || !factor) return DA_ERR_SHAPE;
  if ((((uintptr_t)pred | (uintptr_t)coef) & 15) || ((uintptr_t)factor & 3)) return DA_ERR_SHAPE;
  if (npix / HW > 0x7fffffffL) return DA_ERR_SHAPE;
  hipLaunchKernelGGL(guidance_rescale_kernel, dim3((unsigned)(npix / HW)), dim3(GR_BLOCK), 0, s, pred, coef, g_index, phi,
                     factor, npix, HW, C);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// ---- the four step forms with guidance rescale: `factor` fp32 [npix / HW] (4-byte aligned) multiplies m
extern "C" int da_sampler_step_rs(const float* pred, const float* x, const float* noise, const float* coef,
                                  const float* factor, float* x_out, void* xt_out, long npix, int HW, int C, int cfg,
                                  int copies, hipStream_t s) {
  DA_CLEAR_ERR();
  StepArgs a{pred, x, coef, x_out, xt_out, npix, HW, C, cfg, copies, s};
  a.noise = noise, a.factor = factor;
  return step<false, false, true>(a);
}

extern "C" int da_sampler_step_ms_rs(const float* pred, const float* x, float* hist, const float* coef, const float* factor,
                                     float* x_out, void* xt_out, long npix, int HW, int C, int cfg, int copies,
                                     hipStream_t s) {
  DA_CLEAR_ERR();
  StepArgs a{pred, x, coef, x_out, xt_out, npix, HW, C, cfg, copies, s};
  a.hist = hist, a.factor = factor;
  return step<true, false, true>(a);
}

extern "C" int da_sampler_step_blend_rs(const float* pred, const float* x, const float* noise, const float* coef,
                                        const float* known8, const float* eps8, const float* mask, const float* factor,
                                        float* x_out, void* xt_out, long npix, int HW, int C, int cfg, int copies,
                                        hipStream_t s) {
  DA_CLEAR_ERR();
  StepArgs a{pred, x, coef, x_out, xt_out, npix, HW, C, cfg, copies, s};
  a.noise = noise, a.known8 = known8, a.eps8 = eps8, a.mask = mask, a.factor = factor;
  return step<false, true, true>(a);
}

extern "C" int da_sampler_step_ms_blend_rs(const float* pred, const float* x, float* hist, const float* coef,
                                           const float* known8, const float* eps8, const float* mask, const float* factor,
                                           float* x_out, void* xt_out, long npix, int HW, int C, int cfg, int copies,
                                           hipStream_t s) {
  DA_CLEAR_ERR();
  StepArgs a{pred, x, coef, x_out, xt_out, npix, HW, C, cfg, copies, s};
  a.hist = hist, a.known8 = known8, a.eps8 = eps8, a.mask = mask, a.factor = factor;
  return step<true, true, true>(a);
}

extern "C" int da_sampler_init(const float* known, const float* noise, const float* mask_px, const float* coef,
                               float* known8, float* eps8, float* mask, float* x, void* xt, int B, int H, int W, int C,
                               int f, int copies, hipStream_t s) {
  DA_CLEAR_ERR();
  if (B <= 0 || H <= 0 || W <= 0 || C < 1 || C > 8 || (copies != 1 && copies != 2)) return DA_ERR_SHAPE;
  if (f < 1 || f > 16 || (f & (f - 1))) return DA_ERR_SHAPE;
  if ((long)H * W > (1L << 23)) return DA_ERR_SHAPE;  // pix, and pix times f^2, stay in an int
  if (!known || !noise || !coef || !x) return DA_ERR_SHAPE;
  if (!mask_px != !mask || !known8 != !eps8) return DA_ERR_SHAPE;
  if ((((uintptr_t)known | (uintptr_t)noise | (uintptr_t)mask_px | (uintptr_t)coef | (uintptr_t)known8 | (uintptr_t)eps8 |
        (uintptr_t)mask | (uintptr_t)x | (uintptr_t)xt) & 15))
    return DA_ERR_SHAPE;
  const long npix = (long)B * H * W;
  hipLaunchKernelGGL(sampler_init_kernel, dim3(pixel_grid(npix)), dim3(SMP_BLOCK), 0, s, known, noise, mask_px, coef, known8,
                     eps8, mask, x, (bf16*)xt, npix, H, W, C, f, copies);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
