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
// re-noised to the level of the next timestep.  The unmasked kernels are the BLEND = false instantiations of the same
// bodies.
#include "common.hpp"
#include "diffusion_amd.h"

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

// every load of a pixel comes before its first store, and a pixel is read and written by one thread only: x_out may be x
// BLEND: coef is the row widened to eight floats, {cx, cm, cn, guidance, bA, bS, 0, 0}
template <bool BLEND, bool RS = false>
__global__ void __launch_bounds__((BLEND || RS) ? SMP_BLOCK : SMP_MAX_BLOCK)
    sampler_step_kernel(const float* pred, const float* x, const float* noise, const float* coef, float* x_out, bf16* xt_out,
                        long npix, int HW, int C, int cfg, int copies, Blend<BLEND> bl, Rescale<RS> rs) {
  const f32x4 k = *reinterpret_cast<const f32x4*>(coef);
  const float cx = k[0], cm = k[1], cn = k[2], g = k[3];
  float bA = 0.f, bS = 0.f;
  if constexpr (BLEND) {
    const f32x4 kb = *reinterpret_cast<const f32x4*>(coef + 4);
    bA = kb[0], bS = kb[1];
  }
  GRID_STRIDE(i, npix) {
    const f32x4 x0 = *reinterpret_cast<const f32x4*>(x + i * 8), x1 = *reinterpret_cast<const f32x4*>(x + i * 8 + 4);
    const f32x4 p0 = *reinterpret_cast<const f32x4*>(pred + i * 8), p1 = *reinterpret_cast<const f32x4*>(pred + i * 8 + 4);
    f32x4 q0 = p0, q1 = p1;
    if (cfg) {  // uniform: rows [npix, 2 npix) are the conditional half
      q0 = *reinterpret_cast<const f32x4*>(pred + (npix + i) * 8);
      q1 = *reinterpret_cast<const f32x4*>(pred + (npix + i) * 8 + 4);
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
    const long b = i / HW;
    const int pix = (int)(i - b * HW);
    float fac = 1.f;
    if constexpr (RS) fac = rs.factor[i / rs.hw];
    float o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
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
        float v = cx * xv + cm * m;
        if (noise) v += cn * noise[(b * C + c) * HW + pix];
        if constexpr (BLEND) v = mk * v + (1.f - mk) * kn[c];
        o[c] = v;
      }
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

// The two-step (DPM-Solver++ 2M) form of the same launch: one operand wider.  The host reduces a step to five coefficients
// (DPMSolverMultistepScheduler.step_coefficients_ms) and the kernel carries the previous step's data prediction in `hist`:
//   m     = cfg ? pu + g (pt - pu) : p
//   d     = ax x + am m                         the data prediction x0 of this step
//   v     = kx x + k0 d (+ k1 hist)             k1 == 0 (a first-order step): hist is not read, it may hold anything
//   hist  = d,  x_out = v,  xt = bf16(v)        channels C..7 of all three exactly 0
// k1 comes from device memory like the rest, so one captured launch serves first- and second-order steps alike.
// every load of a pixel comes before its first store, and a pixel is read and written by one thread only: x_out may be x
// BLEND: coef = {ax, am, kx, k0, k1, guidance, bA, bS}
template <bool BLEND, bool RS = false>
__global__ void __launch_bounds__((BLEND || RS) ? SMP_BLOCK : SMP_MAX_BLOCK)
    sampler_step_ms_kernel(const float* pred, const float* x, float* hist, const float* coef, float* x_out, bf16* xt_out,
                           long npix, int C, int cfg, int copies, Blend<BLEND> bl, Rescale<RS> rs) {
  const f32x4 ka = *reinterpret_cast<const f32x4*>(coef), kb = *reinterpret_cast<const f32x4*>(coef + 4);
  const float ax = ka[0], am = ka[1], kx = ka[2], k0 = ka[3], k1 = kb[0], g = kb[1];
  const float bA = kb[2], bS = kb[3];  // the row's two free slots; read by the blended form only
  const bool second = k1 != 0.0f;  // uniform across the launch
  GRID_STRIDE(i, npix) {
    const f32x4 x0 = *reinterpret_cast<const f32x4*>(x + i * 8), x1 = *reinterpret_cast<const f32x4*>(x + i * 8 + 4);
    const f32x4 p0 = *reinterpret_cast<const f32x4*>(pred + i * 8), p1 = *reinterpret_cast<const f32x4*>(pred + i * 8 + 4);
    f32x4 q0 = p0, q1 = p1;
    if (cfg) {  // uniform: rows [npix, 2 npix) are the conditional half
      q0 = *reinterpret_cast<const f32x4*>(pred + (npix + i) * 8);
      q1 = *reinterpret_cast<const f32x4*>(pred + (npix + i) * 8 + 4);
    }
    f32x4 h0 = {0, 0, 0, 0}, h1 = {0, 0, 0, 0};
    if (second) {
      h0 = *reinterpret_cast<const f32x4*>(hist + i * 8);
      h1 = *reinterpret_cast<const f32x4*>(hist + i * 8 + 4);
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
    float fac = 1.f;
    if constexpr (RS) fac = rs.factor[i / rs.hw];
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
        const float dv = ax * xv + am * m;
        float v = kx * xv + k0 * dv;
        if (second) v += k1 * (c < 4 ? h0[c & 3] : h1[c & 3]);
        if constexpr (BLEND) v = mk * v + (1.f - mk) * kn[c];  // the history keeps the unblended data prediction
        d[c] = dv;
        o[c] = v;
      }
    }
    *reinterpret_cast<f32x4*>(hist + i * 8) = f32x4{d[0], d[1], d[2], d[3]};
    *reinterpret_cast<f32x4*>(hist + i * 8 + 4) = f32x4{d[4], d[5], d[6], d[7]};
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

template <bool BLEND, bool RS>
int launch_step(const float* pred, const float* x, const float* noise, const float* coef, float* x_out, void* xt_out,
                long npix, int HW, int C, int cfg, int copies, Blend<BLEND> bl, Rescale<RS> rs, hipStream_t s) {
  long blocks = (npix + SMP_BLOCK - 1) / SMP_BLOCK;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL((sampler_step_kernel<BLEND, RS>), dim3((unsigned)blocks), dim3(SMP_BLOCK), 0, s, pred, x, noise, coef,
                     x_out, (bf16*)xt_out, npix, HW, C, cfg ? 1 : 0, copies, bl, rs);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
template <bool BLEND, bool RS>
int launch_step_ms(const float* pred, const float* x, float* hist, const float* coef, float* x_out, void* xt_out, long npix,
                   int C, int cfg, int copies, Blend<BLEND> bl, Rescale<RS> rs, hipStream_t s) {
  long blocks = (npix + SMP_BLOCK - 1) / SMP_BLOCK;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL((sampler_step_ms_kernel<BLEND, RS>), dim3((unsigned)blocks), dim3(SMP_BLOCK), 0, s, pred, x, hist, coef,
                     x_out, (bf16*)xt_out, npix, C, cfg ? 1 : 0, copies, bl, rs);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// the argument rules every step entry shares; `extra` ORs the form's own pointers, `need` is false when one of them is NULL
bool step_args_ok(const float* pred, const float* x, const float* coef, float* x_out, void* xt_out, long npix, int HW, int C,
                  int copies, uintptr_t extra, bool need) {
  if (npix <= 0 || HW <= 0 || (npix % HW) || C < 1 || C > 8 || (copies != 1 && copies != 2)) return false;
  if (!pred || !x || !coef || !x_out || !need) return false;
  return !((((uintptr_t)pred | (uintptr_t)x | (uintptr_t)coef | (uintptr_t)x_out | (uintptr_t)xt_out | extra) & 15));
}

}  // namespace

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
  if (!step_args_ok(pred, x, coef, x_out, xt_out, npix, HW, C, copies, (uintptr_t)noise, factor != nullptr) ||
      ((uintptr_t)factor & 3))
    return DA_ERR_SHAPE;
  return launch_step<false, true>(pred, x, noise, coef, x_out, xt_out, npix, HW, C, cfg, copies, Blend<false>{},
                                  Rescale<true>{factor, HW}, s);
}

extern "C" int da_sampler_step_ms_rs(const float* pred, const float* x, float* hist, const float* coef, const float* factor,
                                     float* x_out, void* xt_out, long npix, int HW, int C, int cfg, int copies,
                                     hipStream_t s) {
  DA_CLEAR_ERR();
  if (!step_args_ok(pred, x, coef, x_out, xt_out, npix, HW, C, copies, (uintptr_t)hist, hist && factor) ||
      ((uintptr_t)factor & 3))
    return DA_ERR_SHAPE;
  return launch_step_ms<false, true>(pred, x, hist, coef, x_out, xt_out, npix, C, cfg, copies, Blend<false>{},
                                     Rescale<true>{factor, HW}, s);
}

extern "C" int da_sampler_step_blend_rs(const float* pred, const float* x, const float* noise, const float* coef,
                                        const float* known8, const float* eps8, const float* mask, const float* factor,
                                        float* x_out, void* xt_out, long npix, int HW, int C, int cfg, int copies,
                                        hipStream_t s) {
  DA_CLEAR_ERR();
  if (!step_args_ok(pred, x, coef, x_out, xt_out, npix, HW, C, copies,
                    (uintptr_t)noise | (uintptr_t)known8 | (uintptr_t)eps8 | (uintptr_t)mask,
                    known8 && eps8 && mask && factor) ||
      ((uintptr_t)factor & 3))
    return DA_ERR_SHAPE;
  return launch_step<true, true>(pred, x, noise, coef, x_out, xt_out, npix, HW, C, cfg, copies,
                                 Blend<true>{known8, eps8, mask}, Rescale<true>{factor, HW}, s);
}

extern "C" int da_sampler_step_ms_blend_rs(const float* pred, const float* x, float* hist, const float* coef,
                                           const float* known8, const float* eps8, const float* mask, const float* factor,
                                           float* x_out, void* xt_out, long npix, int HW, int C, int cfg, int copies,
                                           hipStream_t s) {
  DA_CLEAR_ERR();
  if (!step_args_ok(pred, x, coef, x_out, xt_out, npix, HW, C, copies,
                    (uintptr_t)hist | (uintptr_t)known8 | (uintptr_t)eps8 | (uintptr_t)mask,
                    hist && known8 && eps8 && mask && factor) ||
      ((uintptr_t)factor & 3))
    return DA_ERR_SHAPE;
  return launch_step_ms<true, true>(pred, x, hist, coef, x_out, xt_out, npix, C, cfg, copies,
                                    Blend<true>{known8, eps8, mask}, Rescale<true>{factor, HW}, s);
}

extern "C" int da_sampler_step(const float* pred, const float* x, const float* noise, const float* coef, float* x_out,
                               void* xt_out, long npix, int HW, int C, int cfg, int copies, hipStream_t s) {
  DA_CLEAR_ERR();
  if (npix <= 0 || HW <= 0 || (npix % HW) || C < 1 || C > 8 || (copies != 1 && copies != 2)) return DA_ERR_SHAPE;
  if (!pred || !x || !coef || !x_out) return DA_ERR_SHAPE;
  if ((((uintptr_t)pred | (uintptr_t)x | (uintptr_t)noise | (uintptr_t)coef | (uintptr_t)x_out | (uintptr_t)xt_out) & 15))
    return DA_ERR_SHAPE;
  long blocks = (npix + SMP_BLOCK - 1) / SMP_BLOCK;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(sampler_step_kernel<false>, dim3((unsigned)blocks), dim3(SMP_BLOCK), 0, s, pred, x, noise, coef, x_out,
                     (bf16*)xt_out, npix, HW, C, cfg ? 1 : 0, copies, Blend<false>{}, Rescale<false>{});
  DA_CHECK_LAUNCH();
  return DA_OK;
}

extern "C" int da_sampler_step_ms(const float* pred, const float* x, float* hist, const float* coef, float* x_out,
                                  void* xt_out, long npix, int HW, int C, int cfg, int copies, hipStream_t s) {
  DA_CLEAR_ERR();
  if (npix <= 0 || HW <= 0 || (npix % HW) || C < 1 || C > 8 || (copies != 1 && copies != 2)) return DA_ERR_SHAPE;
  if (!pred || !x || !hist || !coef || !x_out) return DA_ERR_SHAPE;
  if ((((uintptr_t)pred | (uintptr_t)x | (uintptr_t)hist | (uintptr_t)coef | (uintptr_t)x_out | (uintptr_t)xt_out) & 15))
    return DA_ERR_SHAPE;
  long blocks = (npix + SMP_BLOCK - 1) / SMP_BLOCK;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(sampler_step_ms_kernel<false>, dim3((unsigned)blocks), dim3(SMP_BLOCK), 0, s, pred, x, hist, coef,
                     x_out, (bf16*)xt_out, npix, C, cfg ? 1 : 0, copies, Blend<false>{}, Rescale<false>{});
  DA_CHECK_LAUNCH();
  return DA_OK;
}

extern "C" int da_sampler_step_blend(const float* pred, const float* x, const float* noise, const float* coef,
                                     const float* known8, const float* eps8, const float* mask, float* x_out, void* xt_out,
                                     long npix, int HW, int C, int cfg, int copies, hipStream_t s) {
  DA_CLEAR_ERR();
  if (npix <= 0 || HW <= 0 || (npix % HW) || C < 1 || C > 8 || (copies != 1 && copies != 2)) return DA_ERR_SHAPE;
  if (!pred || !x || !coef || !known8 || !eps8 || !mask || !x_out) return DA_ERR_SHAPE;
  if ((((uintptr_t)pred | (uintptr_t)x | (uintptr_t)noise | (uintptr_t)coef | (uintptr_t)known8 | (uintptr_t)eps8 |
        (uintptr_t)mask | (uintptr_t)x_out | (uintptr_t)xt_out) & 15))
    return DA_ERR_SHAPE;
  long blocks = (npix + SMP_BLOCK - 1) / SMP_BLOCK;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(sampler_step_kernel<true>, dim3((unsigned)blocks), dim3(SMP_BLOCK), 0, s, pred, x, noise, coef, x_out,
                     (bf16*)xt_out, npix, HW, C, cfg ? 1 : 0, copies, Blend<true>{known8, eps8, mask}, Rescale<false>{});
  DA_CHECK_LAUNCH();
  return DA_OK;
}

extern "C" int da_sampler_step_ms_blend(const float* pred, const float* x, float* hist, const float* coef,
                                        const float* known8, const float* eps8, const float* mask, float* x_out,
                                        void* xt_out, long npix, int HW, int C, int cfg, int copies, hipStream_t s) {
  DA_CLEAR_ERR();
  if (npix <= 0 || HW <= 0 || (npix % HW) || C < 1 || C > 8 || (copies != 1 && copies != 2)) return DA_ERR_SHAPE;
  if (!pred || !x || !hist || !coef || !known8 || !eps8 || !mask || !x_out) return DA_ERR_SHAPE;
  if ((((uintptr_t)pred | (uintptr_t)x | (uintptr_t)hist | (uintptr_t)coef | (uintptr_t)known8 | (uintptr_t)eps8 |
        (uintptr_t)mask | (uintptr_t)x_out | (uintptr_t)xt_out) & 15))
    return DA_ERR_SHAPE;
  long blocks = (npix + SMP_BLOCK - 1) / SMP_BLOCK;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(sampler_step_ms_kernel<true>, dim3((unsigned)blocks), dim3(SMP_BLOCK), 0, s, pred, x, hist, coef,
                     x_out, (bf16*)xt_out, npix, C, cfg ? 1 : 0, copies, Blend<true>{known8, eps8, mask}, Rescale<false>{});
  DA_CHECK_LAUNCH();
  return DA_OK;
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
  long blocks = (npix + SMP_BLOCK - 1) / SMP_BLOCK;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(sampler_init_kernel, dim3((unsigned)blocks), dim3(SMP_BLOCK), 0, s, known, noise, mask_px, coef, known8,
                     eps8, mask, x, (bf16*)xt, npix, H, W, C, f, copies);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
