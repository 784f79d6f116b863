// CLIP score on the device: the image preprocessing of the reference's CLIPImageProcessor and the score reduction.
//
// da_clip_preprocess.  Resize of the shorter side to R with PIL's bicubic filter, centre crop to R x R, * 1/255 and the
// per-channel (x - mean) / std, of planar uint8 [B, 3, H, W] images, written straight into the patch matrix the vision
// tower's patch-embedding GEMM reads (or as the reference's fp32 `pixel_values`).
//
// Arithmetic.  Pillow resamples 8-bit images in two passes, horizontal then vertical, with 22-bit fixed-point tap weights,
// and rounds and clamps to a uint8 level after EACH pass: level = clamp((2^21 + sum k * v) >> 22, 0, 255) in int32.  The
// host builds the weights exactly as Pillow does (metrics/clip_preprocess.py: one row {lo, count, k[count]} per cropped
// output index and axis) and the kernel does integer arithmetic only, so the levels are Pillow's by construction; no
// filter centre is evaluated here.  The 256 possible levels go through one fp32 table per channel, (l * (1/255) - mean) /
// std, which both output kinds read.
//
// Staging.  One 256-thread block owns one P x P patch of one image, i.e. one row of the patch matrix.  The source rows its
// vertical windows span are walked in chunks of CLIP_ROWS: the horizontal pass of (row, channel, patch column) goes into
// an LDS cache as rounded uint8 levels; after a barrier every thread adds the rows of the chunk that fall into the
// windows of its (at most CLIP_ACC) outputs.  Tap counts are loop bounds.  Table entries are clamped to the image before
// use: every read is at row < H, column < W of its own image whatever the tables hold.
#include "common.hpp"
#include "diffusion_amd.h"

namespace {

constexpr int CLIP_THREADS = 256;
constexpr int CLIP_MAX_P = 32;     // patch side: 3 * P * P outputs per block, CLIP_ACC accumulators per thread
constexpr int CLIP_MAX_R = 448;
constexpr int CLIP_MAX_SIDE = 65535;
constexpr int CLIP_ROWS = 128;     // source rows per chunk of the horizontal-pass cache
constexpr int CLIP_ACC = 3 * CLIP_MAX_P * CLIP_MAX_P / CLIP_THREADS;
constexpr int CLIP_PREC = 22;      // Pillow's PRECISION_BITS for 8-bit images

DEVINL int clip8(int acc) {
  const int v = (acc + (1 << (CLIP_PREC - 1))) >> CLIP_PREC;   // arithmetic shift, as Pillow's clip8
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(CLIP_THREADS) void clip_preprocess_kernel(const unsigned char* __restrict__ src, int H, int W,
                                                                       int R, int P, const int* __restrict__ xtab, int xld,
                                                                       const int* __restrict__ ytab, int yld, float m0,
                                                                       float m1, float m2, float r0, float r1, float r2,
                                                                       void* __restrict__ out, int kind, int Kp) {
  __shared__ float s_lut[3][256];
  __shared__ int s_x[CLIP_MAX_P][2], s_y[CLIP_MAX_P][2];   // clamped {lo, count} of the patch's columns / rows
  __shared__ unsigned char s_row[CLIP_ROWS][3][CLIP_MAX_P];
  __shared__ unsigned char s_lvl[3 * CLIP_MAX_P * CLIP_MAX_P];
  const int t = threadIdx.x;
  const int G = R / P, Np = G * G;
  const int b = blockIdx.x / Np, patch = blockIdx.x - b * Np;
  const int py = patch / G, px = patch - py * G;
  const int PP = P * P, n_out = 3 * PP;
  for (int i = t; i < 3 * 256; i += CLIP_THREADS) {
    const int c = i >> 8;
    const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? r0 : (c == 1 ? r1 : r2);
    s_lut[c][i & 255] = ((float)(i & 255) * (1.0f / 255.0f) - mean) / sd;
  }
  if (t < 2 * P) {
    const int a = t >= P, j = a ? t - P : t;   // a = 0: columns, 1: rows
    const int* row = a ? ytab + (long)(py * P + j) * yld : xtab + (long)(px * P + j) * xld;
    const int n_in = a ? H : W, ld = a ? yld : xld;
    const int lo = min(max(row[0], 0), n_in - 1);
    const int cnt = min(max(row[1], 0), min(n_in - lo, ld - 2));
    (a ? s_y : s_x)[j][0] = lo;
    (a ? s_y : s_x)[j][1] = cnt;
  }
  __syncthreads();
  int vlo = H, vhi = 0;
  for (int j = 0; j < P; ++j) {
    vlo = min(vlo, s_y[j][0]);
    vhi = max(vhi, s_y[j][0] + s_y[j][1]);
  }
  int acc[CLIP_ACC];
#pragma unroll
  for (int j = 0; j < CLIP_ACC; ++j) acc[j] = 0;
  const unsigned char* img = src + (long)b * 3 * H * W;
  for (int v0 = vlo; v0 < vhi; v0 += CLIP_ROWS) {
    const int rows = min(vhi - v0, CLIP_ROWS);
    for (int i = t; i < rows * 3 * P; i += CLIP_THREADS) {   // horizontal pass: (source row r, channel c, patch column ix)
      const int ix = i % P, rc = i / P, c = rc % 3, r = rc / 3;
      const int lo = s_x[ix][0], cnt = s_x[ix][1];
      const int* k = xtab + (long)(px * P + ix) * xld + 2;
      const unsigned char* p = img + ((long)c * H + (v0 + r)) * W + lo;
      int h = 0;
      for (int u = 0; u < cnt; ++u) h += k[u] * (int)p[u];
      s_row[r][c][ix] = (unsigned char)clip8(h);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CLIP_ACC; ++j) {   // vertical pass: output (c, iy, ix) = column t + 256 j of the matrix row
      const int o = t + j * CLIP_THREADS;
      if (o < n_out) {
        const int c = o / PP, rem = o - c * PP, iy = rem / P, ix = rem - iy * P;
        const int lo = s_y[iy][0], hi = lo + s_y[iy][1];
        const int* k = ytab + (long)(py * P + iy) * yld + 2 - lo;
        const int v1 = min(hi, v0 + rows);
        int a = acc[j];
        for (int v = max(lo, v0); v < v1; ++v) a += k[v] * (int)s_row[v - v0][c][ix];
        acc[j] = a;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < CLIP_ACC; ++j) {
    const int o = t + j * CLIP_THREADS;
    if (o < n_out) s_lvl[o] = (unsigned char)clip8(acc[j]);
  }
  __syncthreads();
  if (kind == 0) {
    bf16* rowp = static_cast<bf16*>(out) + ((long)b * (Np + 1) + 1 + patch) * Kp;
    for (int g = t; g < Kp / 8; g += CLIP_THREADS) {
      bf16x8 o = zero8();
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int col = g * 8 + e;
        if (col < n_out) o[e] = f2bf(s_lut[col / PP][s_lvl[col]]);
      }
      st8(rowp + g * 8, o);
    }
    if (patch == 0) {   // the class-token slot of this image: exact zeros
      bf16* cls = static_cast<bf16*>(out) + (long)b * (Np + 1) * Kp;
      for (int g = t; g < Kp / 8; g += CLIP_THREADS) st8(cls + g * 8, zero8());
    }
  } else {
    float* of = static_cast<float*>(out) + (long)b * 3 * R * R;
    for (int o = t; o < n_out; o += CLIP_THREADS) {
      const int c = o / PP, rem = o - c * PP, iy = rem / P, ix = rem - iy * P;
      of[((long)c * R + (py * P + iy)) * R + px * P + ix] = s_lut[c][s_lvl[o]];
    }
  }
}

// One workgroup: wave w of round n takes pair 4 n + w (lane-strided partial sums, then a butterfly: the order is a function
// of D alone); after a barrier thread 0 adds the round's scores to the running sum in index order.
__global__ __launch_bounds__(CLIP_THREADS) void clip_score_kernel(const float* __restrict__ a, long lda,
                                                                  const float* __restrict__ b, long ldb, int B, int D,
                                                                  float* __restrict__ scores, float* __restrict__ state) {
  constexpr int WAVES = CLIP_THREADS / 64;
  __shared__ float s_sc[WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float sum = 0.0f;
  for (int i0 = 0; i0 < B; i0 += WAVES) {
    const int i = i0 + w;
    if (i < B) {
      const float* pa = a + (long)i * lda;
      const float* pb = b + (long)i * ldb;
      float dot = 0.0f, na = 0.0f, nb = 0.0f;
      for (int d = lane; d < D; d += 64) {
        const float x = pa[d], y = pb[d];
        dot = fmaf(x, y, dot);
        na = fmaf(x, x, na);
        nb = fmaf(y, y, nb);
      }
      dot = wave_sum(dot);
      na = wave_sum(na);
      nb = wave_sum(nb);
      const float sc = 100.0f * dot / (sqrtf(na) * sqrtf(nb));   // no epsilon, no per-sample clamp
      if (lane == 0) {
        scores[i] = sc;
        s_sc[w] = sc;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int j = 0; j < min(WAVES, B - i0); ++j) sum += s_sc[j];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    state[0] += sum;
    state[1] += (float)B;
  }
}

}  // namespace

extern "C" int da_clip_preprocess(const unsigned char* src, int B, int H, int W, int R, int P, const int* xtab, int xld,
                                  const int* ytab, int yld, const float* mean, const float* std, void* out, int out_kind,
                                  hipStream_t s) {
  DA_CLEAR_ERR();
  if (B < 1 || !src || !xtab || !ytab || !mean || !std || !out || (out_kind != 0 && out_kind != 1)) return DA_ERR_SHAPE;
  if (H < 1 || W < 1 || H > CLIP_MAX_SIDE || W > CLIP_MAX_SIDE) return DA_ERR_SHAPE;
  if (P < 1 || P > CLIP_MAX_P || R < P || R > CLIP_MAX_R || R % P) return DA_ERR_SHAPE;
  if (xld < 3 || yld < 3) return DA_ERR_SHAPE;
  if ((uintptr_t)out & (out_kind == 0 ? 15 : 3)) return DA_ERR_SHAPE;
  const int G = R / P, Kp = (3 * P * P + 7) / 8 * 8;
  const long blocks = (long)B * G * G;
  if (blocks > 0x7fffffffL) return DA_ERR_SHAPE;
  hipLaunchKernelGGL(clip_preprocess_kernel, dim3((unsigned)blocks), dim3(CLIP_THREADS), 0, s, src, H, W, R, P, xtab, xld,
                     ytab, yld, mean[0], mean[1], mean[2], std[0], std[1], std[2], out, out_kind, Kp);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

extern "C" int da_clip_score(const float* img, long ldi, const float* txt, long ldt, int B, int D, float* scores,
                             float* state, hipStream_t s) {
  DA_CLEAR_ERR();
  if (B < 1 || D < 1 || ldi < D || ldt < D || !img || !txt || !scores || !state) return DA_ERR_SHAPE;
  if (((uintptr_t)img | (uintptr_t)txt | (uintptr_t)scores | (uintptr_t)state) & 3) return DA_ERR_SHAPE;
  hipLaunchKernelGGL(clip_score_kernel, dim3(1), dim3(CLIP_THREADS), 0, s, img, ldi, txt, ldt, B, D, scores, state);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
