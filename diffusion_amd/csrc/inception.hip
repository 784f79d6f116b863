// The thin kernels of the FID metric's Inception-v3 tower (models/inception_hip.py, metrics/fid.py): 3x3 pooling, the global
// average, the TF1-style resize to 299 x 299 and the float64 feature moments.  The convolutions are csrc/conv_rect.hip.
// Every reduction here runs in a fixed order inside one thread: two runs give identical bits.
#include "common.hpp"
#include "diffusion_amd.h"

namespace {

constexpr int IN_THREADS = 256;
constexpr int IN_SIDE = 299;

// one thread per (output pixel, 8-channel vector)
template <int KIND>
__global__ __launch_bounds__(IN_THREADS) void pool3_kernel(const bf16* __restrict__ X, long ldx, bf16* __restrict__ Y, long ldy,
                                                           int Hin, int Win, int Hout, int Wout, int C8, int stride, int pad,
                                                           long total) {
  const long g = (long)blockIdx.x * IN_THREADS + threadIdx.x;
  if (g >= total) return;
  const int c = (int)(g % C8);
  const long m = g / C8;
  const int ow = (int)(m % Wout);
  const long q = m / Wout;
  const int oh = (int)(q % Hout);
  const long b = q / Hout;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = KIND == 0 ? -INFINITY : 0.0f;
  int cnt = 0;
  for (int i = 0; i < 3; ++i) {
    const int ih = oh * stride - pad + i;
    if ((unsigned)ih >= (unsigned)Hin) continue;
    for (int j = 0; j < 3; ++j) {
      const int iw = ow * stride - pad + j;
      if ((unsigned)iw >= (unsigned)Win) continue;
      const bf16x8 v = ld8(X + ((b * Hin + ih) * Win + iw) * ldx + c * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = KIND == 0 ? fmaxf(acc[e], bf2f(v[e])) : acc[e] + bf2f(v[e]);
      ++cnt;
    }
  }
  bf16x8 o;
  const float n = (float)cnt;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = f2bf(KIND == 0 ? acc[e] : acc[e] / n);
  st8(Y + m * ldy + c * 8, o);
}

// one thread per (image, 8-channel vector): rows in index order
__global__ __launch_bounds__(IN_THREADS) void avg_global_kernel(const bf16* __restrict__ X, long ldx, float* __restrict__ out,
                                                                long ldo, int HW, int C8, int total) {
  const int g = blockIdx.x * IN_THREADS + threadIdx.x;
  if (g >= total) return;
  const int c = g % C8, b = g / C8;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
  const bf16* p = X + (long)b * HW * ldx + c * 8;
  for (int r = 0; r < HW; ++r) {
    const bf16x8 v = ld8(p + (long)r * ldx);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += bf2f(v[e]);
  }
  const float n = (float)HW;
  float* o = out + (long)b * ldo + c * 8;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = acc[e] / n;
}

template <typename T>
DEVINL float level(T v);
template <>
DEVINL float level<unsigned char>(unsigned char v) { return (float)v; }
template <>
DEVINL float level<float>(float v) { return floorf(fminf(fmaxf(255.0f * v, 0.0f), 255.0f)); }   // (x * 255).byte()

// one thread per output pixel.  src = dst * scale in fp32 (no half-pixel offset), lo = floor, hi = min(lo + 1, n - 1),
// lerp along x on both rows, then along y, each as lo + (hi - lo) * d without contraction.
template <typename T>
__global__ __launch_bounds__(IN_THREADS) void incep_pre_kernel(const T* __restrict__ src, int H, int W, float sy, float sx,
                                                               bf16* __restrict__ out, long total) {
  const long g = (long)blockIdx.x * IN_THREADS + threadIdx.x;
  if (g >= total) return;
  const int ox = (int)(g % IN_SIDE);
  const long q = g / IN_SIDE;
  const int oy = (int)(q % IN_SIDE);
  const long b = q / IN_SIDE;
  const float fx = __fmul_rn((float)ox, sx), fy = __fmul_rn((float)oy, sy);
  const int x0 = min((int)fx, W - 1), y0 = min((int)fy, H - 1);
  const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
  const float dx = fx - (float)x0, dy = fy - (float)y0;
  bf16x8 o = zero8();
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const T* p = src + (b * 3 + c) * (long)H * W;
    const float a00 = level<T>(p[(long)y0 * W + x0]), a01 = level<T>(p[(long)y0 * W + x1]);
    const float a10 = level<T>(p[(long)y1 * W + x0]), a11 = level<T>(p[(long)y1 * W + x1]);
    const float r0 = __fadd_rn(a00, __fmul_rn(a01 - a00, dx)), r1 = __fadd_rn(a10, __fmul_rn(a11 - a10, dx));
    const float v = __fadd_rn(r0, __fmul_rn(r1 - r0, dy));
    o[c] = f2bf((v - 128.0f) / 128.0f);
  }
  st8(out + g * 8, o);
}

// cov: one thread owns a 4 x 4 patch of the D x D matrix and walks the batch in order; the product of two fp32 values is
// exact in fp64, so each step is one rounding of the running sum.
__global__ __launch_bounds__(IN_THREADS) void moments_cov_kernel(const float* __restrict__ F, long ldf, int B, int D4,
                                                                 double* __restrict__ cov) {
  const int e4 = blockIdx.x * 16 + (threadIdx.x & 15), d4 = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (e4 >= D4 || d4 >= D4) return;
  const long D = 4L * D4;
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = cov[(4L * d4 + i) * D + 4 * e4 + j];
  for (int b = 0; b < B; ++b) {
    const f32x4 fd = *reinterpret_cast<const f32x4*>(F + b * ldf + 4 * d4);
    const f32x4 fe = *reinterpret_cast<const f32x4*>(F + b * ldf + 4 * e4);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] += (double)fd[i] * (double)fe[j];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) cov[(4L * d4 + i) * D + 4 * e4 + j] = acc[i][j];
}

__global__ __launch_bounds__(IN_THREADS) void moments_sum_kernel(const float* __restrict__ F, long ldf, int B, int D,
                                                                 double* __restrict__ sum, double* __restrict__ n) {
  const int d = blockIdx.x * IN_THREADS + threadIdx.x;
  if (d == 0) n[0] += (double)B;
  if (d >= D) return;
  double acc = sum[d];
  for (int b = 0; b < B; ++b) acc += (double)F[b * ldf + d];
  sum[d] = acc;
}

}  // namespace

extern "C" int da_pool2d_fwd(const void* X, long ldx, void* Y, long ldy, int B, int Hin, int Win, int Hout, int Wout, int C,
                             int stride, int pad, int kind, hipStream_t s) {
  DA_CLEAR_ERR();
  if (!X || !Y || B < 1 || Hin < 1 || Win < 1 || C < 8 || C % 8 || ldx < C || ldy < C || ldx % 8 || ldy % 8)
    return DA_ERR_SHAPE;
  if ((stride != 1 && stride != 2) || (pad != 0 && pad != 1) || (kind != 0 && kind != 1)) return DA_ERR_SHAPE;
  if (Hin > 65535 || Win > 65535 || Hin + 2 * pad < 3 || Win + 2 * pad < 3) return DA_ERR_SHAPE;
  if (Hout != (Hin + 2 * pad - 3) / stride + 1 || Wout != (Win + 2 * pad - 3) / stride + 1) return DA_ERR_SHAPE;
  if (((uintptr_t)X | (uintptr_t)Y) & 15) return DA_ERR_SHAPE;
  const long total = (long)B * Hout * Wout * (C / 8), blocks = (total + IN_THREADS - 1) / IN_THREADS;
  if (blocks > 0x7fffffffL) return DA_ERR_SHAPE;
  const bf16* x = static_cast<const bf16*>(X);
  bf16* y = static_cast<bf16*>(Y);
  if (kind == 0)
    hipLaunchKernelGGL(pool3_kernel<0>, dim3((unsigned)blocks), dim3(IN_THREADS), 0, s, x, ldx, y, ldy, Hin, Win, Hout, Wout,
                       C / 8, stride, pad, total);
  else
    hipLaunchKernelGGL(pool3_kernel<1>, dim3((unsigned)blocks), dim3(IN_THREADS), 0, s, x, ldx, y, ldy, Hin, Win, Hout, Wout,
                       C / 8, stride, pad, total);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

extern "C" int da_avgpool_global_f32(const void* X, long ldx, float* out, long ldo, int B, int HW, int C, hipStream_t s) {
  DA_CLEAR_ERR();
  if (!X || !out || B < 1 || HW < 1 || C < 8 || C % 8 || ldx < C || ldx % 8 || ldo < C) return DA_ERR_SHAPE;
  if (((uintptr_t)X & 15) || ((uintptr_t)out & 3)) return DA_ERR_SHAPE;
  const long total = (long)B * (C / 8);
  if (total > 0x7fffffffL - IN_THREADS || (long)B * HW > 0x7fffffffL) return DA_ERR_SHAPE;
  hipLaunchKernelGGL(avg_global_kernel, dim3((unsigned)((total + IN_THREADS - 1) / IN_THREADS)), dim3(IN_THREADS), 0, s,
                     static_cast<const bf16*>(X), ldx, out, ldo, HW, C / 8, (int)total);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

extern "C" int da_inception_preprocess(const void* src, int src_kind, int B, int H, int W, void* out, hipStream_t s) {
  DA_CLEAR_ERR();
  if (!src || !out || B < 1 || H < 1 || W < 1 || H > 65535 || W > 65535 || (src_kind != 0 && src_kind != 1))
    return DA_ERR_SHAPE;
  if (((uintptr_t)out & 15) || (src_kind == 1 && ((uintptr_t)src & 3))) return DA_ERR_SHAPE;
  const long total = (long)B * IN_SIDE * IN_SIDE, blocks = (total + IN_THREADS - 1) / IN_THREADS;
  if (blocks > 0x7fffffffL) return DA_ERR_SHAPE;
  const float sy = (float)((double)H / IN_SIDE), sx = (float)((double)W / IN_SIDE);
  bf16* o = static_cast<bf16*>(out);
  if (src_kind == 0)
    hipLaunchKernelGGL(incep_pre_kernel<unsigned char>, dim3((unsigned)blocks), dim3(IN_THREADS), 0, s,
                       static_cast<const unsigned char*>(src), H, W, sy, sx, o, total);
  else
    hipLaunchKernelGGL(incep_pre_kernel<float>, dim3((unsigned)blocks), dim3(IN_THREADS), 0, s,
                       static_cast<const float*>(src), H, W, sy, sx, o, total);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

extern "C" int da_feature_moments(const float* F, long ldf, int B, int D, double* sum, double* cov, double* n,
                                  hipStream_t s) {
  DA_CLEAR_ERR();
  if (!F || !sum || !cov || !n || B < 1 || D < 8 || D % 8 || D > 16384 || ldf < D || ldf % 4) return DA_ERR_SHAPE;
  if (((uintptr_t)F & 15) || (((uintptr_t)sum | (uintptr_t)cov | (uintptr_t)n) & 7)) return DA_ERR_SHAPE;
  const int D4 = D / 4, g = (D4 + 15) / 16;
  hipLaunchKernelGGL(moments_sum_kernel, dim3((unsigned)((D + IN_THREADS - 1) / IN_THREADS)), dim3(IN_THREADS), 0, s, F,
                     ldf, B, D, sum, n);
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(moments_cov_kernel, dim3((unsigned)g, (unsigned)g), dim3(IN_THREADS), 0, s, F, ldf, B, D4, cov);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
