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
#include "common.hpp"
#include "diffusion_amd.h"

namespace {

constexpr int SMP_BLOCK = 256;
#define GRID_STRIDE(i, n) \
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

// every load of a pixel comes before its first store, and a pixel is read and written by one thread only: x_out may be x
__global__ void sampler_step_kernel(const float* pred, const float* x, const float* noise, const float* coef,
                                    float* x_out, bf16* xt_out, long npix, int HW, int C, int cfg, int copies) {
  const f32x4 k = *reinterpret_cast<const f32x4*>(coef);
  const float cx = k[0], cm = k[1], cn = k[2], g = k[3];
  GRID_STRIDE(i, npix) {
    const f32x4 x0 = *reinterpret_cast<const f32x4*>(x + i * 8), x1 = *reinterpret_cast<const f32x4*>(x + i * 8 + 4);
    const f32x4 p0 = *reinterpret_cast<const f32x4*>(pred + i * 8), p1 = *reinterpret_cast<const f32x4*>(pred + i * 8 + 4);
    f32x4 q0 = p0, q1 = p1;
    if (cfg) {  // uniform: rows [npix, 2 npix) are the conditional half
      q0 = *reinterpret_cast<const f32x4*>(pred + (npix + i) * 8);
      q1 = *reinterpret_cast<const f32x4*>(pred + (npix + i) * 8 + 4);
    }
    const long b = i / HW;
    const int pix = (int)(i - b * HW);
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
        float v = cx * xv + cm * m;
        if (noise) v += cn * noise[(b * C + c) * HW + pix];
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
__global__ void sampler_step_ms_kernel(const float* pred, const float* x, float* hist, const float* coef, float* x_out,
                                       bf16* xt_out, long npix, int C, int cfg, int copies) {
  const f32x4 ka = *reinterpret_cast<const f32x4*>(coef), kb = *reinterpret_cast<const f32x4*>(coef + 4);
  const float ax = ka[0], am = ka[1], kx = ka[2], k0 = ka[3], k1 = kb[0], g = kb[1];
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
        const float dv = ax * xv + am * m;
        float v = kx * xv + k0 * dv;
        if (second) v += k1 * (c < 4 ? h0[c & 3] : h1[c & 3]);
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

}  // namespace

extern "C" int da_sampler_step(const float* pred, const float* x, const float* noise, const float* coef, float* x_out,
                               void* xt_out, long npix, int HW, int C, int cfg, int copies, hipStream_t s) {
  DA_CLEAR_ERR();
  if (npix <= 0 || HW <= 0 || (npix % HW) || C < 1 || C > 8 || (copies != 1 && copies != 2)) return DA_ERR_SHAPE;
  if (!pred || !x || !coef || !x_out) return DA_ERR_SHAPE;
  if ((((uintptr_t)pred | (uintptr_t)x | (uintptr_t)noise | (uintptr_t)coef | (uintptr_t)x_out | (uintptr_t)xt_out) & 15))
    return DA_ERR_SHAPE;
  long blocks = (npix + SMP_BLOCK - 1) / SMP_BLOCK;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(sampler_step_kernel, dim3((unsigned)blocks), dim3(SMP_BLOCK), 0, s, pred, x, noise, coef, x_out,
                     (bf16*)xt_out, npix, HW, C, cfg ? 1 : 0, copies);
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
  hipLaunchKernelGGL(sampler_step_ms_kernel, dim3((unsigned)blocks), dim3(SMP_BLOCK), 0, s, pred, x, hist, coef, x_out,
                     (bf16*)xt_out, npix, C, cfg ? 1 : 0, copies);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
