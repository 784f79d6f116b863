// HBM-bound pointwise / small kernels of the U-Net training step:
// GEGLU, SiLU, strided add / copy (skip-connection concat), nearest-2x upsample fwd/bwd, sinusoidal
// timestep embedding, forward-diffusion noising (NCHW fp32 -> NHWC-8 bf16), fused MSE loss + gradient,
// fused AdamW (fp32 master + moments, bf16 shadow write), weight-shadow transpose for dgrad.
// All use 16-B vector accesses along the contiguous (channel) axis and grid-stride loops.  GEGLU, SiLU, the two GELUs, add and
// copy are instances of one kernel, map2d_kernel<Op, NIN, NOUT>, behind one launcher; the 4-channel latent loss runs the
// general mse_partial_c_kernel at C = 4.
#include <cmath>

#include "common.hpp"
#include "diffusion_amd.h"
#include "philox.hpp"

namespace {

constexpr int PW_BLOCK = 256;
inline int pw_blocks(long n) {
  long b = (n + PW_BLOCK - 1) / PW_BLOCK;
  if (b > 16384) b = 16384;
  if (b < 1) b = 1;
  return (int)b;
}
#define GRID_STRIDE(i, n) \
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

// ---- the strided map: the eight pointwise entry points whose work item is 16 bytes of every operand at [row, 8 v], each
// operand at its own row stride.  All NIN loads come before the first store, so an output may be one of the inputs.
template <int NIN, int NOUT>
struct Map2dArgs {
  const bf16* in[NIN];
  long ldi[NIN];
  bf16* out[NOUT];
  long ldo[NOUT];
  int nvec;
  long total;
};
template <typename Op, int NIN, int NOUT>
__global__ void map2d_kernel(Map2dArgs<NIN, NOUT> p) {
  GRID_STRIDE(i, p.total) {
    long row = i / p.nvec;
    int v = (int)(i - row * p.nvec);
    bf16x8 x[NIN], y[NOUT];
#pragma unroll
    for (int k = 0; k < NIN; ++k) x[k] = ld8(p.in[k] + row * p.ldi[k] + 8 * v);
    Op::apply(x, y);
#pragma unroll
    for (int k = 0; k < NOUT; ++k) st8(p.out[k] + row * p.ldo[k] + 8 * v, y[k]);
  }
}

// Op::apply(x, y): whole 16-byte vectors in and out, so a copy never passes through fp32
// ---- GEGLU: out = a * gelu(g), in = [a | g]: the gate half is a second operand at in + Cout with the same stride
struct GegluFwd {  // x = {a, g}
  static DEVINL void apply(const bf16x8* x, bf16x8* y) {
#pragma unroll
    for (int e = 0; e < 8; ++e) y[0][e] = f2bf(bf2f(x[0][e]) * gelu_f(bf2f(x[1][e])));
  }
};
struct GegluBwd {  // x = {a, g, dout}, y = {da, dg}
  static DEVINL void apply(const bf16x8* x, bf16x8* y) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float gf = bf2f(x[1][e]), df = bf2f(x[2][e]);
      y[0][e] = f2bf(df * gelu_f(gf));
      y[1][e] = f2bf(df * bf2f(x[0][e]) * dgelu_f(gf));
    }
  }
};
// ---- SiLU on a 2-D strided tensor
struct SiluFwd {
  static DEVINL void apply(const bf16x8* x, bf16x8* y) {
#pragma unroll
    for (int e = 0; e < 8; ++e) y[0][e] = f2bf(silu_f(bf2f(x[0][e])));
  }
};
struct SiluBwd {  // x = {x, dy}
  static DEVINL void apply(const bf16x8* x, bf16x8* y) {
#pragma unroll
    for (int e = 0; e < 8; ++e) y[0][e] = f2bf(bf2f(x[1][e]) * dsilu_f(bf2f(x[0][e])));
  }
};
// ---- erf-GELU on a 2-D strided tensor (the text encoder's MLP activation; forward only - the encoder is frozen)
struct GeluFwd {
  static DEVINL void apply(const bf16x8* x, bf16x8* y) {
#pragma unroll
    for (int e = 0; e < 8; ++e) y[0][e] = f2bf(gelu_f(bf2f(x[0][e])));
  }
};
// ---- quick-GELU x * sigmoid(1.702 x) (CLIP ViT-L/14's MLP activation, hidden_act = "quick_gelu"); forward only
struct QuickGeluFwd {
  static DEVINL void apply(const bf16x8* x, bf16x8* y) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float f = bf2f(x[0][e]);
      y[0][e] = f2bf(f / (1.0f + expf(-1.702f * f)));
    }
  }
};
// ---- strided add / copy
struct Add {
  static DEVINL void apply(const bf16x8* x, bf16x8* y) {
#pragma unroll
    for (int e = 0; e < 8; ++e) y[0][e] = f2bf(bf2f(x[0][e]) + bf2f(x[1][e]));
  }
};
struct Copy2d {
  static DEVINL void apply(const bf16x8* x, bf16x8* y) { y[0] = x[0]; }
};

// ---- nearest 2x upsample (NHWC)
__global__ void upsample2x_fwd_kernel(const bf16* x, bf16* y, int H, int W, int nvec, long total_out) {
  GRID_STRIDE(i, total_out) {
    long pix = i / nvec;
    int v = (int)(i - pix * nvec);
    int W2 = 2 * W, H2 = 2 * H;
    int ow = (int)(pix % W2);
    long t = pix / W2;
    int oh = (int)(t % H2);
    long b = t / H2;
    long src = (b * H + (oh >> 1)) * W + (ow >> 1);
    st8(y + pix * (long)(nvec * 8) + 8 * v, ld8(x + src * (long)(nvec * 8) + 8 * v));
  }
}
__global__ void upsample2x_bwd_kernel(const bf16* dy, bf16* dx, int H, int W, int nvec, long total_in) {
  GRID_STRIDE(i, total_in) {
    long pix = i / nvec;
    int v = (int)(i - pix * nvec);
    int w = (int)(pix % W);
    long t = pix / W;
    int h = (int)(t % H);
    long b = t / H;
    const long C = (long)nvec * 8;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int dh = 0; dh < 2; ++dh)
#pragma unroll
      for (int dw = 0; dw < 2; ++dw) {
        long src = (b * 2 * H + 2 * h + dh) * 2 * W + 2 * w + dw;
        bf16x8 d = ld8(dy + src * C + 8 * v);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += bf2f(d[e]);
      }
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(acc[e]);
    st8(dx + pix * C + 8 * v, o);
  }
}

// ---- sinusoidal timestep embedding: [cos(t f_i) | sin(t f_i)], f_i = 10000^(-i/half)
// T = long long (discrete DDPM steps) or float (continuous time): an integer-valued float t gives the same bits
template <typename T>
__global__ void timestep_embed_kernel(const T* t, bf16* out, int B, int dim) {
  const int half = dim >> 1;
  GRID_STRIDE(i, (long)B * half) {
    int b = (int)(i / half), k = (int)(i - (long)b * half);
    float f = expf(-9.210340371976184f * (float)k / (float)half);
    float a = (float)t[b] * f;
    out[(long)b * dim + k] = f2bf(cosf(a));
    out[(long)b * dim + half + k] = f2bf(sinf(a));
  }
}

// ---- forward diffusion: x_t = sqrt(ac[t]) x0 + sqrt(1-ac[t]) eps ; target = eps or v
// inputs NCHW fp32 [B,4,HW]; outputs NHWC with the 4 channels padded to 8 (pad = 0).  Not the C = 4 case of the general
// kernel below: here the compiler fuses a x + (s n) into an FMA, there it adds two rounded products, and among millions of
// pixels a few bf16 x_t differ by that (the v target is unfused in both); without the run-time channel count a launch at
// the U-Net's sizes also takes 5.2 us against 6.0 us (MI355X)
__global__ void add_noise_kernel(const float* x0, const float* eps, const long long* t, const float* sqrt_ac,
                                 const float* sqrt_1mac, bf16* xt, float* target, int HW, long total_pix,
                                 int v_pred) {
  GRID_STRIDE(i, total_pix) {
    long b = i / HW;
    int pix = (int)(i - b * HW);
    const float a = sqrt_ac[t[b]], s = sqrt_1mac[t[b]];
    bf16x8 o = zero8();
    float tg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float x = x0[(b * 4 + c) * HW + pix], n = eps[(b * 4 + c) * HW + pix];
      o[c] = f2bf(a * x + s * n);
      tg[c] = v_pred ? (a * n - s * x) : n;
    }
    st8(xt + i * 8, o);
    *reinterpret_cast<f32x4*>(target + i * 8) = f32x4{tg[0], tg[1], tg[2], tg[3]};
    *reinterpret_cast<f32x4*>(target + i * 8 + 4) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// ---- one channel of the general forward diffusion, shared by add_noise_ex_kernel and add_noise_rng_kernel: x_t = a x + s n_xt
// and the target (0: the noise n_tg, 1: v = a n_tg - s x, 2: x).  Every product and every sum is rounded on its own: the
// bits add_noise_ex_kernel has always had (its multiplies compile to packed ones, which never fused), now stated
DEVINL void noise_channel(float a, float s, float x, float n_xt, float n_tg, int kind, float& v, float& tg) {
#pragma clang fp contract(off)
  const float ax = a * x, sn = s * n_xt;
  v = ax + sn;
  if (kind == 1) {
    const float an = a * n_tg, sx = s * x;
    tg = an - sx;
  } else {
    tg = kind == 2 ? x : n_tg;
  }
}

// ---- general forward diffusion: C (1..8) channels, discrete (int64 t + sqrt(abar) tables) or continuous (fp32 angle t:
// cos t x0 + sin t eps) noising; target eps, v or x0.  inputs NCHW fp32 [B,C,HW]; outputs NHWC-8 (pad channels = 0)
template <bool CONT>
__global__ void add_noise_ex_kernel(const float* x0, const float* eps, const void* tv, const float* sqrt_ac,
                                    const float* sqrt_1mac, bf16* xt, float* target, int C, int HW, long total_pix,
                                    int kind) {
  GRID_STRIDE(i, total_pix) {
    long b = i / HW;
    int pix = (int)(i - b * HW);
    float a, s;
    if (CONT) {
      const float tt = static_cast<const float*>(tv)[b];
      a = cosf(tt);
      s = sinf(tt);
    } else {
      const long long tt = static_cast<const long long*>(tv)[b];
      a = sqrt_ac[tt];
      s = sqrt_1mac[tt];
    }
    bf16x8 o = zero8();
    float tg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c < C) {
        float x = x0[(b * C + c) * HW + pix], n = eps[(b * C + c) * HW + pix], v;
        noise_channel(a, s, x, n, n, kind, v, tg[c]);
        o[c] = f2bf(v);
      }
    }
    st8(xt + i * 8, o);
    *reinterpret_cast<f32x4*>(target + i * 8) = f32x4{tg[0], tg[1], tg[2], tg[3]};
    *reinterpret_cast<f32x4*>(target + i * 8 + 4) = f32x4{tg[4], tg[5], tg[6], tg[7]};
  }
}

// ---- the same noising with every draw made in the launch (da_add_noise_rng): per sample b the key is seeds[b], the stream 0,
// and the draw number says what a draw is for: 0 the noise n, 1 the perturbation z2, 2 the per-channel offset zc (pixel 0),
// 3 the timestep (pixel 0, block 0, word r0).  A thread owns a pixel: it recomputes its sample's timestep and offset draws
// (a few hundred integer and fp32 operations) and shares nothing with another thread, so nothing in the launch waits.
struct NoiseRngArgs {
  const float* x0;
  const uint64_t* seeds;
  const int* slot;  // NULL: plain uniform timesteps
  void* t;          // written when draw_t, else read
  const float *sqrt_ac, *sqrt_1mac;
  bf16* xt;
  float* target;
  long total_pix;
  long long t_lo, t_hi;  // discrete range
  float tf_lo, tf_hi;    // continuous range
  float noise_offset, perturbation;
  int n_slots, draw_t, C, HW, kind;
};
// the slot of sample b, held inside [0, n_slots): a slot from device memory can never carry a timestep out of the table
DEVINL uint32_t noise_slot(const NoiseRngArgs& p, long b) {
  const int sl = p.slot[b];
  return (uint32_t)(sl < 0 ? 0 : (sl >= p.n_slots ? p.n_slots - 1 : sl));
}
// t_lo + ((slot 2^32 + r0) R) / (n_slots 2^32): the division by 2^32 first (a shift), then a 32-bit one, which is the same
// floor; the host admits n_slots R < 2^32 only, so the product stays below 2^64 and its upper half below 2^32
DEVINL long long draw_timestep(const NoiseRngArgs& p, long b, uint32_t r0) {
  const uint64_t R = (uint64_t)(p.t_hi - p.t_lo);
  if (!p.slot) return p.t_lo + (long long)(((uint64_t)r0 * R) >> 32);
  const uint64_t num = (((uint64_t)noise_slot(p, b) << 32) | r0) * R;
  return p.t_lo + (long long)((uint32_t)(num >> 32) / (uint32_t)p.n_slots);
}
DEVINL float draw_time(const NoiseRngArgs& p, long b, uint32_t r0) {
#pragma clang fp contract(off)
  float u = (float)(r0 >> 8) * 0x1p-24f;
  if (p.slot) {
    const float su = (float)noise_slot(p, b) + u;
    u = su / (float)p.n_slots;
  }
  const float span = p.tf_hi - p.tf_lo;
  const float du = span * u;
  return p.tf_lo + du;
}
template <bool CONT>
__global__ void __launch_bounds__(PW_BLOCK) add_noise_rng_kernel(NoiseRngArgs p) {
  const int C = p.C, HW = p.HW;
  GRID_STRIDE(i, p.total_pix) {
    const long b = i / HW;
    const uint32_t pix = (uint32_t)(i - b * HW);
    const uint64_t seed = p.seeds[b];
    uint32_t r[4] = {0, 0, 0, 0};
    if (p.draw_t) philox::words(0u, 3u, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);  // uniform
    float a, s;
    if (CONT) {
      float* tp = static_cast<float*>(p.t);
      const float tt = p.draw_t ? draw_time(p, b, r[0]) : tp[b];
      if (p.draw_t && pix == 0) tp[b] = tt;
      a = cosf(tt);
      s = sinf(tt);
    } else {
      long long* tp = static_cast<long long*>(p.t);
      const long long tt = p.draw_t ? draw_timestep(p, b, r[0]) : tp[b];
      if (p.draw_t && pix == 0) tp[b] = tt;
      a = p.sqrt_ac[tt];
      s = p.sqrt_1mac[tt];
    }
    float n1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, n2[8];
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (4 * k < C) philox::normals(seed, pix, 0u, 0u, (uint32_t)k, n1 + 4 * k);
    if (p.noise_offset != 0.f) {  // uniform
#pragma unroll
      for (int k = 0; k < 2; ++k)
        if (4 * k < C) {
          float zc[4];
          philox::normals(seed, 0u, 2u, 0u, (uint32_t)k, zc);
#pragma unroll
          for (int j = 0; j < 4; ++j) n1[4 * k + j] = philox::add_scaled_unfused(n1[4 * k + j], p.noise_offset, zc[j]);
        }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) n2[c] = n1[c];
    if (p.perturbation != 0.f) {  // uniform
#pragma unroll
      for (int k = 0; k < 2; ++k)
        if (4 * k < C) {
          float z2[4];
          philox::normals(seed, pix, 1u, 0u, (uint32_t)k, z2);
#pragma unroll
          for (int j = 0; j < 4; ++j) n2[4 * k + j] = philox::add_scaled_unfused(n1[4 * k + j], p.perturbation, z2[j]);
        }
    }
    bf16x8 o = zero8();
    float tg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c < C) {
        float v;
        noise_channel(a, s, p.x0[(b * C + c) * HW + pix], n2[c], n1[c], p.kind, v, tg[c]);
        o[c] = f2bf(v);
      }
    }
    st8(p.xt + i * 8, o);
    *reinterpret_cast<f32x4*>(p.target + i * 8) = f32x4{tg[0], tg[1], tg[2], tg[3]};
    *reinterpret_cast<f32x4*>(p.target + i * 8 + 4) = f32x4{tg[4], tg[5], tg[6], tg[7]};
  }
}

// ---- sum over the block: wave butterfly, one partial per wave in LDS, thread 0 adds them in wave order (valid in thread 0)
DEVINL float block_sum(float acc) {
  __shared__ float sh[PW_BLOCK / 64];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  float s = 0.f;
  if (threadIdx.x == 0)
    for (int w = 0; w < PW_BLOCK / 64; ++w) s += sh[w];
  return s;
}

// ---- MSE loss over the C (1..8) valid channels of NHWC-8 tensors, and its gradient; dpred is exactly 0 in the pad channels
__global__ void mse_partial_c_kernel(const float* pred, const float* target, bf16* dpred, float* partial,
                                     long total_pix, int C, float grad_coef) {
  float acc = 0.f;
  GRID_STRIDE(i, total_pix) {
    // each square is rounded to fp32 and then added, never fused into an FMA: these are the bits the 4-channel latent loss
    // has always had (its former kernel of its own compiled to packed multiplies), whatever the compiler would choose here
#pragma clang fp contract(off)
    const f32x4 p0 = *reinterpret_cast<const f32x4*>(pred + i * 8), q0 = *reinterpret_cast<const f32x4*>(target + i * 8);
    f32x4 p1 = {0.f, 0.f, 0.f, 0.f}, q1 = {0.f, 0.f, 0.f, 0.f};
    if (C > 4) {  // uniform: the 4-channel (latent) loss reads the lower 16 bytes of a pixel only
      p1 = *reinterpret_cast<const f32x4*>(pred + i * 8 + 4);
      q1 = *reinterpret_cast<const f32x4*>(target + i * 8 + 4);
    }
    bf16x8 g = zero8();
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c < C) {
        float d = (c < 4 ? p0[c & 3] : p1[c & 3]) - (c < 4 ? q0[c & 3] : q1[c & 3]);
        acc += d * d;
        g[c] = f2bf(d * grad_coef);
      }
    }
    st8(dpred + i * 8, g);
  }
  const float s = block_sum(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
// ---- the same loss with a weight per sample, looked up by the sample's timestep: w = wtab[t[pix / HW]] (Min-SNR weighting).
// A sample boundary may fall anywhere in a block or in a thread's grid-stride sequence: the weight is looked up per pixel.
// A timestep outside [0, T) is clamped into the table.  dpred = (d * w) * grad_coef and acc += w * (d * d), each product
// rounded on its own: with a table of ones these are the bits of mse_partial_c_kernel.
__global__ void mse_partial_w_kernel(const float* pred, const float* target, bf16* dpred, float* partial, long total_pix,
                                     int C, int HW, const long long* t, const float* wtab, int T, float grad_coef) {
  float acc = 0.f;
  GRID_STRIDE(i, total_pix) {
#pragma clang fp contract(off)
    long long ts = t[i / HW];
    ts = ts < 0 ? 0 : (ts >= T ? T - 1 : ts);
    const float w = wtab[ts];
    const f32x4 p0 = *reinterpret_cast<const f32x4*>(pred + i * 8), q0 = *reinterpret_cast<const f32x4*>(target + i * 8);
    f32x4 p1 = {0.f, 0.f, 0.f, 0.f}, q1 = {0.f, 0.f, 0.f, 0.f};
    if (C > 4) {  // uniform
      p1 = *reinterpret_cast<const f32x4*>(pred + i * 8 + 4);
      q1 = *reinterpret_cast<const f32x4*>(target + i * 8 + 4);
    }
    bf16x8 g = zero8();
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c < C) {
        float d = (c < 4 ? p0[c & 3] : p1[c & 3]) - (c < 4 ? q0[c & 3] : q1[c & 3]);
        acc += w * (d * d);
        g[c] = f2bf((d * w) * grad_coef);
      }
    }
    st8(dpred + i * 8, g);
  }
  const float s = block_sum(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ void mse_finalize_kernel(const float* partial, int n, float* loss, float inv_count, float weight,
                                    int accumulate) {
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) acc += partial[i];
  float s = block_sum(acc);
  if (threadIdx.x == 0) {
    s = s * inv_count * weight;
    loss[0] = accumulate ? loss[0] + s : s;
  }
}

// ---- fused AdamW (torch.optim.AdamW semantics), flat buffers; writes the bf16 compute shadow.  One kernel text, two
// instantiations, so da_adamw and da_adamw_dev cannot drift: GS = float takes the gradient multiplier as an argument;
// GS = const float* reads it from the device record of the gradient-norm pass (gradnorm.hip, DaGradStats as fp32 words:
// [2] the multiplier, [3] 0.0 = a non-finite gradient: touch nothing).
template <typename GS>
__global__ void adamw_kernel(float* p, const float* g, float* m, float* v, bf16* shadow, float* ema, float ema_s,
                             long n, float lr, float b1, float b2, float eps, float wd, float inv_bc1,
                             float inv_sqrt_bc2, GS gs) {
  float gscale;
  if constexpr (__is_same(GS, float)) {
    gscale = gs;
  } else {
    if (gs[3] == 0.f) return;
    gscale = gs[2];
  }
  GRID_STRIDE(i4, (n + 3) / 4) {
    long i = i4 * 4;
    if (i + 3 < n) {
      f32x4 pp = *reinterpret_cast<f32x4*>(p + i), gg = *reinterpret_cast<const f32x4*>(g + i);
      f32x4 mm = *reinterpret_cast<f32x4*>(m + i), vv = *reinterpret_cast<f32x4*>(v + i);
      bf16x4 sh;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float gr = gg[e] * gscale;
        float w = pp[e] * (1.f - lr * wd);
        mm[e] = b1 * mm[e] + (1.f - b1) * gr;
        vv[e] = b2 * vv[e] + (1.f - b2) * gr * gr;
        float denom = sqrtf(vv[e]) * inv_sqrt_bc2 + eps;
        w -= lr * inv_bc1 * mm[e] / denom;
        pp[e] = w;
        sh[e] = f2bf(w);
      }
      if (ema) {  // EMA of the weights fused into the same pass (ema = s*ema + (1-s)*w_new)
        f32x4 ee = *reinterpret_cast<f32x4*>(ema + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) ee[e] = ema_s * ee[e] + (1.f - ema_s) * pp[e];
        *reinterpret_cast<f32x4*>(ema + i) = ee;
      }
      *reinterpret_cast<f32x4*>(p + i) = pp;
      *reinterpret_cast<f32x4*>(m + i) = mm;
      *reinterpret_cast<f32x4*>(v + i) = vv;
      *reinterpret_cast<bf16x4*>(shadow + i) = sh;
    } else {
      for (long j = i; j < n; ++j) {
        float gr = g[j] * gscale;
        float w = p[j] * (1.f - lr * wd);
        float mj = b1 * m[j] + (1.f - b1) * gr;
        float vj = b2 * v[j] + (1.f - b2) * gr * gr;
        w -= lr * inv_bc1 * mj / (sqrtf(vj) * inv_sqrt_bc2 + eps);
        p[j] = w; m[j] = mj; v[j] = vj; shadow[j] = f2bf(w);
        if (ema) ema[j] = ema_s * ema[j] + (1.f - ema_s) * w;
      }
    }
  }
}

__global__ void cast_f32_bf16_kernel(const float* s, bf16* d, long n) {
  GRID_STRIDE(i, n) d[i] = f2bf(s[i]);
}

// ---- dgrad weight shadow: dst[c][T-1-t][n] = src[n][t][c]   (taps flipped, channel roles swapped)
__global__ void transpose_weight_kernel(const bf16* src, bf16* dst, int N, int T, int C) {
  __shared__ bf16 tile[32][33];
  const int t = blockIdx.z;
  const int n0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int j = ty; j < 32; j += 8) {
    int n = n0 + j, c = c0 + tx;
    tile[j][tx] = (n < N && c < C) ? src[((long)n * T + t) * C + c] : (bf16)0.f;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    int c = c0 + j, n = n0 + tx;
    if (c < C && n < N) dst[((long)c * T + (T - 1 - t)) * N + n] = tile[tx][j];
  }
}

// ---- all dgrad weight shadows in ONE launch: descriptor table {src_off, dst_off, N, T, C, first_block} per tensor
struct TransposeDesc {
  long src_off, dst_off;
  int N, T, C, first_block;
};
// 64 x 64 tiles, 16-B accesses on both sides (the 32 x 32 scalar version moved 64-B row segments and spent most of a
// 2-KiB tile's time in the descriptor search: 2.2 ms per step for 1.7 GB each way)
__global__ __launch_bounds__(256) void transpose_weights_batched_kernel(const bf16* src_base, bf16* dst_base,
                                                                        const TransposeDesc* desc, int ntensors) {
  __shared__ __attribute__((aligned(16))) bf16 tile[64][72];
  // binary search: last tensor whose first_block <= blockIdx.x
  int lo = 0, hi = ntensors - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (desc[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const TransposeDesc d = desc[lo];
  int b = blockIdx.x - d.first_block;
  const int tc = (d.C + 63) / 64, tn = (d.N + 63) / 64;
  const int t = b / (tc * tn);
  b -= t * tc * tn;
  const int n0 = (b / tc) * 64, c0 = (b % tc) * 64;
  const bf16* src = src_base + d.src_off;
  bf16* dst = dst_base + d.dst_off;
  const bool vec = !(d.C & 7) && !(d.N & 7) && !(d.src_off & 7) && !(d.dst_off & 7);
  if (vec) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = threadIdx.x + 256 * i;
      const int row = idx >> 3, ch = (idx & 7) * 8;
      const int n = n0 + row, c = c0 + ch;
      bf16x8 v = zero8();
      if (n < d.N && c < d.C) v = ld8(src + ((long)n * d.T + t) * d.C + c);
      *reinterpret_cast<bf16x8*>(&tile[row][ch]) = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = threadIdx.x + 256 * i;
      const int crow = idx >> 3, nch = (idx & 7) * 8;
      const int c = c0 + crow, n = n0 + nch;
      if (c < d.C && n < d.N) {
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = tile[nch + e][crow];
        st8(dst + ((long)c * d.T + (d.T - 1 - t)) * d.N + n, o);
      }
    }
  } else {
    for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
      const int row = idx >> 6, col = idx & 63;
      const int n = n0 + row, c = c0 + col;
      tile[row][col] = (n < d.N && c < d.C) ? src[((long)n * d.T + t) * d.C + c] : (bf16)0.f;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
      const int crow = idx >> 6, ncol = idx & 63;
      const int c = c0 + crow, n = n0 + ncol;
      if (c < d.C && n < d.N) dst[((long)c * d.T + (d.T - 1 - t)) * d.N + n] = tile[ncol][crow];
    }
  }
}

}  // namespace

// The eight map entry points: C and every row stride a multiple of 8 elements, then one launch
template <typename Op, int NIN, int NOUT>
int map2d_launch(const void* const (&in)[NIN], const long (&ldi)[NIN], void* const (&out)[NOUT],
                 const long (&ldo)[NOUT], int M, int C, hipStream_t s) {
  DA_CLEAR_ERR();
  if (M <= 0 || C <= 0 || (C & 7)) return DA_ERR_SHAPE;
  Map2dArgs<NIN, NOUT> p;
  for (int k = 0; k < NIN; ++k) {
    if (ldi[k] & 7) return DA_ERR_SHAPE;
    p.in[k] = (const bf16*)in[k];
    p.ldi[k] = ldi[k];
  }
  for (int k = 0; k < NOUT; ++k) {
    if (ldo[k] & 7) return DA_ERR_SHAPE;
    p.out[k] = (bf16*)out[k];
    p.ldo[k] = ldo[k];
  }
  p.nvec = C >> 3;
  p.total = (long)M * p.nvec;
  hipLaunchKernelGGL((map2d_kernel<Op, NIN, NOUT>), dim3(pw_blocks(p.total)), dim3(PW_BLOCK), 0, s, p);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

extern "C" int da_geglu_fwd(const void* in, long ldi, void* out, long ldo, int M, int Cout, hipStream_t s) {
  return map2d_launch<GegluFwd, 2, 1>({in, (const bf16*)in + Cout}, {ldi, ldi}, {out}, {ldo}, M, Cout, s);
}
extern "C" int da_geglu_bwd(const void* in, long ldi, const void* dout, long lddo, void* din, long lddi, int M,
                            int Cout, hipStream_t s) {
  return map2d_launch<GegluBwd, 3, 2>({in, (const bf16*)in + Cout, dout}, {ldi, ldi, lddo}, {din, (bf16*)din + Cout},
                                      {lddi, lddi}, M, Cout, s);
}
extern "C" int da_silu_fwd(const void* x, long ldx, void* y, long ldy, int M, int C, hipStream_t s) {
  return map2d_launch<SiluFwd, 1, 1>({x}, {ldx}, {y}, {ldy}, M, C, s);
}
extern "C" int da_gelu_fwd(const void* x, long ldx, void* y, long ldy, int M, int C, hipStream_t s) {
  return map2d_launch<GeluFwd, 1, 1>({x}, {ldx}, {y}, {ldy}, M, C, s);
}
extern "C" int da_quick_gelu_fwd(const void* x, long ldx, void* y, long ldy, int M, int C, hipStream_t s) {
  return map2d_launch<QuickGeluFwd, 1, 1>({x}, {ldx}, {y}, {ldy}, M, C, s);
}
extern "C" int da_silu_bwd(const void* x, long ldx, const void* dy, long lddy, void* dx, long lddx, int M, int C,
                           hipStream_t s) {
  return map2d_launch<SiluBwd, 2, 1>({x, dy}, {ldx, lddy}, {dx}, {lddx}, M, C, s);
}
extern "C" int da_add(const void* a, long lda, const void* b, long ldb, void* o, long ldo, int M, int C,
                      hipStream_t s) {
  return map2d_launch<Add, 2, 1>({a, b}, {lda, ldb}, {o}, {ldo}, M, C, s);
}
extern "C" int da_copy2d(const void* a, long lda, void* o, long ldo, int M, int C, hipStream_t s) {
  return map2d_launch<Copy2d, 1, 1>({a}, {lda}, {o}, {ldo}, M, C, s);
}
extern "C" int da_upsample2x_fwd(const void* x, void* y, int B, int H, int W, int C, hipStream_t s) {
  DA_CLEAR_ERR();
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 7)) return DA_ERR_SHAPE;
  long total = (long)B * 4 * H * W * (C >> 3);
  hipLaunchKernelGGL(upsample2x_fwd_kernel, dim3(pw_blocks(total)), dim3(PW_BLOCK), 0, s, (const bf16*)x, (bf16*)y,
                     H, W, C >> 3, total);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
extern "C" int da_upsample2x_bwd(const void* dy, void* dx, int B, int H, int W, int C, hipStream_t s) {
  DA_CLEAR_ERR();
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 7)) return DA_ERR_SHAPE;
  long total = (long)B * H * W * (C >> 3);
  hipLaunchKernelGGL(upsample2x_bwd_kernel, dim3(pw_blocks(total)), dim3(PW_BLOCK), 0, s, (const bf16*)dy, (bf16*)dx,
                     H, W, C >> 3, total);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
extern "C" int da_timestep_embed(const long long* t, void* out, int B, int dim, hipStream_t s) {
  DA_CLEAR_ERR();
  if (B <= 0 || dim <= 0 || (dim & 1)) return DA_ERR_SHAPE;
  hipLaunchKernelGGL(timestep_embed_kernel<long long>, dim3(pw_blocks((long)B * dim / 2)), dim3(PW_BLOCK), 0, s, t,
                     (bf16*)out, B, dim);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
extern "C" int da_timestep_embed_f32(const float* t, void* out, int B, int dim, hipStream_t s) {
  DA_CLEAR_ERR();
  if (B <= 0 || dim <= 0 || (dim & 1)) return DA_ERR_SHAPE;
  hipLaunchKernelGGL(timestep_embed_kernel<float>, dim3(pw_blocks((long)B * dim / 2)), dim3(PW_BLOCK), 0, s, t,
                     (bf16*)out, B, dim);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
extern "C" int da_add_noise(const float* x0, const float* eps, const long long* t, const float* sqrt_ac,
                            const float* sqrt_1mac, void* xt, float* target, int B, int HW, int v_pred,
                            hipStream_t s) {
  DA_CLEAR_ERR();
  if (B <= 0 || HW <= 0 || !t || !sqrt_ac || !sqrt_1mac) return DA_ERR_SHAPE;
  if (((uintptr_t)xt & 15) || ((uintptr_t)target & 15)) return DA_ERR_SHAPE;
  long total = (long)B * HW;
  hipLaunchKernelGGL(add_noise_kernel, dim3(pw_blocks(total)), dim3(PW_BLOCK), 0, s, x0, eps, t, sqrt_ac, sqrt_1mac,
                     (bf16*)xt, target, HW, total, v_pred);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
extern "C" int da_add_noise_ex(const float* x0, const float* eps, const void* t, int t_is_f32, const float* sqrt_ac,
                               const float* sqrt_1mac, void* xt, float* target, int B, int C, int HW, int target_kind,
                               hipStream_t s) {
  DA_CLEAR_ERR();
  if (B <= 0 || HW <= 0 || C < 1 || C > 8 || target_kind < 0 || target_kind > 2 || !t) return DA_ERR_SHAPE;
  if (!t_is_f32 && (!sqrt_ac || !sqrt_1mac)) return DA_ERR_SHAPE;
  if (((uintptr_t)xt & 15) || ((uintptr_t)target & 15)) return DA_ERR_SHAPE;
  long total = (long)B * HW;
  if (t_is_f32)
    hipLaunchKernelGGL(add_noise_ex_kernel<true>, dim3(pw_blocks(total)), dim3(PW_BLOCK), 0, s, x0, eps, t, sqrt_ac,
                       sqrt_1mac, (bf16*)xt, target, C, HW, total, target_kind);
  else
    hipLaunchKernelGGL(add_noise_ex_kernel<false>, dim3(pw_blocks(total)), dim3(PW_BLOCK), 0, s, x0, eps, t, sqrt_ac,
                       sqrt_1mac, (bf16*)xt, target, C, HW, total, target_kind);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
extern "C" int da_add_noise_rng(const float* x0, const unsigned long long* seeds, const int* slot, int n_slots, void* t,
                                int t_is_f32, int draw_t, double t_lo, double t_hi, const float* sqrt_ac,
                                const float* sqrt_1mac, int T, float noise_offset, float perturbation, void* xt,
                                float* target, int B, int C, int HW, int target_kind, hipStream_t s) {
  DA_CLEAR_ERR();
  if (B <= 0 || HW <= 0 || C < 1 || C > 8 || target_kind < 0 || target_kind > 2) return DA_ERR_SHAPE;
  if (!x0 || !seeds || !t || !xt || !target) return DA_ERR_SHAPE;
  if (((uintptr_t)seeds & 7) || ((uintptr_t)xt & 15) || ((uintptr_t)target & 15) || ((uintptr_t)x0 & 3) ||
      ((uintptr_t)t & (t_is_f32 ? 3 : 7)) || ((uintptr_t)slot & 3))
    return DA_ERR_SHAPE;
  if (!t_is_f32 && (!sqrt_ac || !sqrt_1mac || T < 1)) return DA_ERR_SHAPE;
  if (!std::isfinite(noise_offset) || !std::isfinite(perturbation)) return DA_ERR_SHAPE;
  if (n_slots < 0 || (slot != nullptr) != (n_slots > 0)) return DA_ERR_SHAPE;
  NoiseRngArgs p{};
  if (draw_t) {
    if (!(t_lo < t_hi) || !std::isfinite(t_lo) || !std::isfinite(t_hi)) return DA_ERR_SHAPE;
    if (t_is_f32) {
      // slot + u must be exact up to its one rounding: slots below 2^24
      if ((double)(float)t_lo != t_lo || (double)(float)t_hi != t_hi || n_slots > (1 << 24)) return DA_ERR_SHAPE;
      p.tf_lo = (float)t_lo, p.tf_hi = (float)t_hi;
    } else {
      if (t_lo != std::floor(t_lo) || t_hi != std::floor(t_hi) || t_lo < 0 || t_hi > (double)T) return DA_ERR_SHAPE;
      p.t_lo = (long long)t_lo, p.t_hi = (long long)t_hi;
      if ((uint64_t)n_slots * (uint64_t)(p.t_hi - p.t_lo) >= (1ull << 32)) return DA_ERR_SHAPE;
    }
  }
  p.x0 = x0, p.seeds = reinterpret_cast<const uint64_t*>(seeds), p.slot = slot, p.t = t;
  p.sqrt_ac = sqrt_ac, p.sqrt_1mac = sqrt_1mac, p.xt = (bf16*)xt, p.target = target;
  p.total_pix = (long)B * HW;
  p.noise_offset = noise_offset, p.perturbation = perturbation;
  p.n_slots = n_slots, p.draw_t = draw_t ? 1 : 0, p.C = C, p.HW = HW, p.kind = target_kind;
  if (t_is_f32)
    hipLaunchKernelGGL(add_noise_rng_kernel<true>, dim3(pw_blocks(p.total_pix)), dim3(PW_BLOCK), 0, s, p);
  else
    hipLaunchKernelGGL(add_noise_rng_kernel<false>, dim3(pw_blocks(p.total_pix)), dim3(PW_BLOCK), 0, s, p);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
// both MSE entry points: each computes the reciprocal of its count its own way (they differ in the last bit for some sizes)
static int mse_launch(const float* pred, const float* target, void* dpred, float* loss, float* scratch, long total_pix,
                      int C, float grad_coef, float inv_count, float weight, int accumulate, hipStream_t s) {
  DA_CLEAR_ERR();
  if (total_pix <= 0 || C < 1 || C > 8) return DA_ERR_SHAPE;
  if ((((uintptr_t)pred | (uintptr_t)target | (uintptr_t)dpred) & 15)) return DA_ERR_SHAPE;
  int blocks = pw_blocks(total_pix);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(mse_partial_c_kernel, dim3(blocks), dim3(PW_BLOCK), 0, s, pred, target, (bf16*)dpred, scratch,
                     total_pix, C, grad_coef);
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(mse_finalize_kernel, dim3(1), dim3(PW_BLOCK), 0, s, scratch, blocks, loss, inv_count, weight,
                     accumulate);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
extern "C" int da_mse_loss(const float* pred, const float* target, void* dpred, float* loss, float* scratch,
                           long total_pix, float grad_coef, float weight, int accumulate, hipStream_t s) {
  return mse_launch(pred, target, dpred, loss, scratch, total_pix, 4, grad_coef, 1.0f / (4.0f * (float)total_pix), weight,
                    accumulate, s);
}
extern "C" int da_mse_loss_c(const float* pred, const float* target, void* dpred, float* loss, float* scratch,
                             long total_pix, int C, float grad_coef, float weight, int accumulate, hipStream_t s) {
  return mse_launch(pred, target, dpred, loss, scratch, total_pix, C, grad_coef,
                    (float)(1.0 / ((double)C * (double)total_pix)), weight, accumulate, s);
}
extern "C" int da_mse_loss_w(const float* pred, const float* target, void* dpred, float* loss, float* scratch,
                             long total_pix, int C, int HW, const long long* t, const float* wtab, int T, float grad_coef,
                             float weight, int accumulate, hipStream_t s) {
  DA_CLEAR_ERR();
  if (total_pix <= 0 || C < 1 || C > 8 || HW <= 0 || (total_pix % HW) || T <= 0 || !t || !wtab) return DA_ERR_SHAPE;
  if ((((uintptr_t)pred | (uintptr_t)target | (uintptr_t)dpred) & 15)) return DA_ERR_SHAPE;
  int blocks = pw_blocks(total_pix);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(mse_partial_w_kernel, dim3(blocks), dim3(PW_BLOCK), 0, s, pred, target, (bf16*)dpred, scratch,
                     total_pix, C, HW, t, wtab, T, grad_coef);
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(mse_finalize_kernel, dim3(1), dim3(PW_BLOCK), 0, s, scratch, blocks, loss,
                     (float)(1.0 / ((double)C * (double)total_pix)), weight, accumulate);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
extern "C" int da_adamw(float* p, const float* g, float* m, float* v, void* shadow, float* ema, float ema_smoothing,
                        long n, float lr, float beta1, float beta2, float eps, float wd, int step, float grad_scale,
                        hipStream_t s) {
  DA_CLEAR_ERR();
  if (n <= 0 || step <= 0) return DA_ERR_SHAPE;
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) || ((uintptr_t)shadow & 7))
    return DA_ERR_SHAPE;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  hipLaunchKernelGGL(adamw_kernel<float>, dim3(pw_blocks((n + 3) / 4)), dim3(PW_BLOCK), 0, s, p, g, m, v, (bf16*)shadow,
                     ema, ema_smoothing, n,
                     lr, beta1, beta2, eps, wd, (float)(1.0 / bc1), (float)(1.0 / sqrt(bc2)), grad_scale);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
extern "C" int da_adamw_dev(float* p, const float* g, float* m, float* v, void* shadow, float* ema, float ema_smoothing,
                            long n, float lr, float beta1, float beta2, float eps, float wd, int step, const float* stats,
                            hipStream_t s) {
  DA_CLEAR_ERR();
  if (n <= 0 || step <= 0 || !stats) return DA_ERR_SHAPE;
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) || ((uintptr_t)shadow & 7) ||
      ((uintptr_t)stats & 3))
    return DA_ERR_SHAPE;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  hipLaunchKernelGGL(adamw_kernel<const float*>, dim3(pw_blocks((n + 3) / 4)), dim3(PW_BLOCK), 0, s, p, g, m, v,
                     (bf16*)shadow, ema, ema_smoothing, n, lr, beta1, beta2, eps, wd, (float)(1.0 / bc1),
                     (float)(1.0 / sqrt(bc2)), stats);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
extern "C" int da_cast_f32_bf16(const float* src, void* dst, long n, hipStream_t s) {
  DA_CLEAR_ERR();
  if (n <= 0) return DA_ERR_SHAPE;
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(pw_blocks(n)), dim3(PW_BLOCK), 0, s, src, (bf16*)dst, n);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
extern "C" int da_transpose_weight(const void* src, void* dst, int N, int T, int C, hipStream_t s) {
  DA_CLEAR_ERR();
  if (N <= 0 || T <= 0 || C <= 0) return DA_ERR_SHAPE;
  hipLaunchKernelGGL(transpose_weight_kernel, dim3((C + 31) / 32, (N + 31) / 32, T), dim3(256), 0, s,
                     (const bf16*)src, (bf16*)dst, N, T, C);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

extern "C" int da_transpose_weights_batched(const void* src_base, void* dst_base, const void* desc, int ntensors,
                                            int total_blocks, hipStream_t s) {
  DA_CLEAR_ERR();
  if (ntensors <= 0 || total_blocks <= 0) return DA_ERR_SHAPE;
  hipLaunchKernelGGL(transpose_weights_batched_kernel, dim3(total_blocks), dim3(256), 0, s, (const bf16*)src_base,
                     (bf16*)dst_base, (const TransposeDesc*)desc, ntensors);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
