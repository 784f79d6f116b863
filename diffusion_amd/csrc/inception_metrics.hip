// The kernels behind the Inception score and the Kernel Inception Distance (metrics/inception_score.py, metrics/kid.py):
// the 2048 -> 1008 logits head, the per-split score from stored logits and the polynomial-kernel MMD of row subsets of two
// feature stores.  Every sum is float64 and runs in an order fixed by the launch geometry alone (no atomics): two runs give
// identical bits.  Rows are addressed through index vectors with 64-bit offsets; the indices are validated on the host
// (ops.py) before they are uploaded.
#include "common.hpp"
#include "diffusion_amd.h"

namespace {

constexpr int IM_THREADS = 256;
constexpr int IM_WAVES = IM_THREADS / 64;
constexpr int IS_MAX_C = 4096;   // the marginal lives in LDS: 8 bytes per class

typedef double f64x4 __attribute__((ext_vector_type(4)));

// xor butterflies: fp addition commutes, so every lane ends with the same bits
DEVINL double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
DEVINL double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// ---------------------------------------------------------------------------------------------------------------- head
// one wave per class c and group of FC_B rows: lane l owns k = 4 l + 256 j in order, fp64 FMAs (the product of two fp32
// values is exact in fp64), one butterfly, one rounding to fp32.  W is read once per row group.
constexpr int FC_B = 8;

__global__ __launch_bounds__(IM_THREADS) void fc_logits_kernel(const float* __restrict__ F, long ldf,
                                                               const float* __restrict__ W, float* __restrict__ out,
                                                               long ldo, int B, int K, int C) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = blockIdx.x * IM_WAVES + wave, b0 = blockIdx.y * FC_B;
  if (c >= C) return;
  double acc[FC_B];
#pragma unroll
  for (int j = 0; j < FC_B; ++j) acc[j] = 0.0;
  const float* w = W + (long)c * K;
  for (int k = lane * 4; k < K; k += 256) {
    const f32x4 wv = *reinterpret_cast<const f32x4*>(w + k);
#pragma unroll
    for (int j = 0; j < FC_B; ++j) {
      if (b0 + j >= B) break;
      const f32x4 fv = *reinterpret_cast<const f32x4*>(F + (long)(b0 + j) * ldf + k);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[j] = fma((double)fv[e], (double)wv[e], acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < FC_B; ++j) {
    if (b0 + j >= B) break;
    const double s = wave_sum_d(acc[j]);
    if (lane == 0) out[(long)(b0 + j) * ldo + c] = (float)s;
  }
}

// ----------------------------------------------------------------------------------------------------- Inception score
// log sum_c exp(x_c) of one row by one wave: max, then the sum of exp(x - max), lanes striding the classes
DEVINL double row_lse(const float* __restrict__ row, int C, int lane) {
  double mx = -INFINITY;
  for (int c = lane; c < C; c += 64) mx = fmax(mx, (double)row[c]);
  mx = wave_max_d(mx);
  double s = 0.0;
  for (int c = lane; c < C; c += 64) s += exp((double)row[c] - mx);
  return mx + log(wave_sum_d(s));
}

// one workgroup per chunk of `chunk` rows (the last may be short).  Marginal: rows go through LDS-sized tiles; a wave
// computes each row's log-sum-exp, then the thread that owns class c adds p_ic over the tile's rows in order.  KL: a wave
// per row (rows w, w + 4, ... in order), lanes striding the classes; the four wave sums are added in wave order.
__global__ __launch_bounds__(IM_THREADS) void inception_score_kernel(const float* __restrict__ L, long ld,
                                                                     const int* __restrict__ perm, int N, int C, int chunk,
                                                                     double* __restrict__ scores) {
  extern __shared__ double lm[];   // [C]: sum_i p_ic, then log m_c
  __shared__ double lse_t[IM_THREADS];
  __shared__ double part[IM_WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int i0 = blockIdx.x * chunk, n = min(chunk, N - i0);
  const int* pm = perm + i0;
  for (int c = tid; c < C; c += IM_THREADS) lm[c] = 0.0;
  for (int t0 = 0; t0 < n; t0 += IM_THREADS) {
    const int nt = min(IM_THREADS, n - t0);
    __syncthreads();
    for (int r = wave; r < nt; r += IM_WAVES) {
      const double lse = row_lse(L + (long)pm[t0 + r] * ld, C, lane);
      if (lane == 0) lse_t[r] = lse;
    }
    __syncthreads();
    for (int c = tid; c < C; c += IM_THREADS) {
      double a = lm[c];
      for (int r = 0; r < nt; ++r) a += exp((double)L[(long)pm[t0 + r] * ld + c] - lse_t[r]);
      lm[c] = a;
    }
  }
  __syncthreads();
  for (int c = tid; c < C; c += IM_THREADS) lm[c] = log(lm[c] / (double)n);   // -inf where every p_ic is 0: never used
  __syncthreads();
  double kl = 0.0;
  for (int r = wave; r < n; r += IM_WAVES) {
    const float* row = L + (long)pm[r] * ld;
    const double lse = row_lse(row, C, lane);
    double a = 0.0;
    for (int c = lane; c < C; c += 64) {
      const double lp = (double)row[c] - lse, p = exp(lp);
      if (p > 0.0) a += p * (lp - lm[c]);
    }
    kl += wave_sum_d(a);
  }
  if (lane == 0) part[wave] = kl;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < IM_WAVES; ++w) s += part[w];
    scores[blockIdx.x] = exp(s / (double)n);
  }
}

// ------------------------------------------------------------------------------------------------------ polynomial MMD
// One workgroup per 64 x 64 tile of one Gram block of one subset: XY (all T x T tiles), XX and YY (the T (T + 1) / 2 tiles
// on and above the diagonal; a tile above it counts twice).  Both operands' rows are gathered through idx into LDS as
// fp32, MM_K columns at a time; each of the four waves owns a 32 x 32 quarter as 2 x 2 v_mfma_f64_16x16x4_f64 blocks and
// converts fp32 -> fp64 (exact) on the LDS read.  The epilogue raises gamma <x, y> + coef to the degree, skips rows and
// columns past m and the diagonal of XX / YY, and leaves the tile's sum in ws[subset][tile].
constexpr int MM_T = 64, MM_K = 32, MM_LD = MM_K + 4;   // row pitch 36 floats: the 16 rows x 4 k of one operand read hit
                                                        // 64 distinct banks, and rows stay 16-byte aligned

__host__ __device__ inline long mmd_tiles(int T) { return (long)T * T + (long)T * (T + 1); }

__global__ __launch_bounds__(IM_THREADS) void poly_mmd_tile_kernel(const float* __restrict__ Fr, long ldr,
                                                                   const float* __restrict__ Ff, long ldf,
                                                                   const int* __restrict__ idx_r,
                                                                   const int* __restrict__ idx_f, int m, int D, int T,
                                                                   int degree, double gamma, double coef,
                                                                   double* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float As[MM_T * MM_LD];
  __shared__ __attribute__((aligned(16))) float Bs[MM_T * MM_LD];
  __shared__ double part[IM_WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int t = blockIdx.x, s = blockIdx.y;
  int kind, ti, tj;   // kind 0: XY, 1: XX, 2: YY
  if (t < T * T) {
    kind = 0, ti = t / T, tj = t % T;
  } else {
    const int tri = T * (T + 1) / 2;
    int u = t - T * T;
    kind = 1 + u / tri;
    u %= tri;
    ti = 0;
    while (u >= T - ti) u -= T - ti, ++ti;
    tj = ti + u;
  }
  const float* FA = kind == 2 ? Ff : Fr;
  const float* FB = kind == 1 ? Fr : Ff;
  const long lda = kind == 2 ? ldf : ldr, ldb = kind == 1 ? ldr : ldf;
  const int* ia = (kind == 2 ? idx_f : idx_r) + (long)s * m;
  const int* ib = (kind == 1 ? idx_r : idx_f) + (long)s * m;

  // staging: thread -> float4 column c4 of rows r and r + 32 of both operands; rows past m read as zero
  const int c4 = (tid & 7) * 4, r = tid >> 3;
  const float* pa[2];
  const float* pb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int ra = ti * MM_T + r + 32 * h, rb = tj * MM_T + r + 32 * h;
    pa[h] = ra < m ? FA + (long)ia[ra] * lda + c4 : nullptr;
    pb[h] = rb < m ? FB + (long)ib[rb] * ldb + c4 : nullptr;
  }
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  f32x4 ga[2], gb[2];
  auto fetch = [&](int kc) {
    const bool in = kc + c4 < D;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      ga[h] = in && pa[h] ? *reinterpret_cast<const f32x4*>(pa[h] + kc) : zero;
      gb[h] = in && pb[h] ? *reinterpret_cast<const f32x4*>(pb[h] + kc) : zero;
    }
  };

  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32, lr = lane & 15, lk = lane >> 4;
  f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

  fetch(0);
  for (int kc = 0; kc < D; kc += MM_K) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *reinterpret_cast<f32x4*>(&As[(r + 32 * h) * MM_LD + c4]) = ga[h];
      *reinterpret_cast<f32x4*>(&Bs[(r + 32 * h) * MM_LD + c4]) = gb[h];
    }
    __syncthreads();
    if (kc + MM_K < D) fetch(kc + MM_K);
#pragma unroll
    for (int kk = 0; kk < MM_K; kk += 4) {
      // A: lane holds A[row lane & 15][k lane >> 4]; B: B[k lane >> 4][col lane & 15] = Y[col][k]
      double a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = (double)As[(wr + 16 * i + lr) * MM_LD + kk + lk];
        b[i] = (double)Bs[(wc + 16 * i + lr) * MM_LD + kk + lk];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg (not the f32 forms' 4 * (lane >> 4) + reg)
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = ti * MM_T + wr + 16 * i + lk + 4 * e, col = tj * MM_T + wc + 16 * j + lr;
        if (row < m && col < m && (kind == 0 || row != col)) {
          const double base = gamma * acc[i][j][e] + coef;
          double p = base;
          for (int d = 1; d < degree; ++d) p *= base;
          sum += p;
        }
      }
  sum = wave_sum_d(sum);
  if (lane == 0) part[wave] = sum;
  __syncthreads();
  if (tid == 0) {
    double v = 0.0;
    for (int w = 0; w < IM_WAVES; ++w) v += part[w];
    ws[(long)s * mmd_tiles(T) + t] = (kind != 0 && tj > ti) ? 2.0 * v : v;
  }
}

// one thread per subset adds its tiles in index order
__global__ __launch_bounds__(IM_THREADS) void poly_mmd_finalize_kernel(const double* __restrict__ ws, int subsets, int m,
                                                                       int T, double* __restrict__ out) {
  const int s = blockIdx.x * IM_THREADS + threadIdx.x;
  if (s >= subsets) return;
  const long sq = (long)T * T, tri = (long)T * (T + 1) / 2;
  const double* w = ws + (long)s * mmd_tiles(T);
  double sxy = 0.0, sxx = 0.0, syy = 0.0;
  for (long t = 0; t < sq; ++t) sxy += w[t];
  for (long t = 0; t < tri; ++t) sxx += w[sq + t];
  for (long t = 0; t < tri; ++t) syy += w[sq + tri + t];
  const double dm = (double)m;
  out[s] = (sxx + syy) / (dm * (dm - 1.0)) - 2.0 * sxy / (dm * dm);
}

}  // namespace

extern "C" int da_fc_logits_f32(const float* F, long ldf, const float* W, float* out, long ldo, int B, int K, int C,
                                hipStream_t s) {
  DA_CLEAR_ERR();
  if (!F || !W || !out || B < 1 || C < 1 || K < 4 || K % 4 || ldf < K || ldf % 4 || ldo < C) return DA_ERR_SHAPE;
  if ((((uintptr_t)F | (uintptr_t)W) & 15) || ((uintptr_t)out & 3)) return DA_ERR_SHAPE;
  const long gy = ((long)B + FC_B - 1) / FC_B;
  if (gy > 65535) return DA_ERR_SHAPE;
  hipLaunchKernelGGL(fc_logits_kernel, dim3((unsigned)((C + IM_WAVES - 1) / IM_WAVES), (unsigned)gy), dim3(IM_THREADS), 0, s,
                     F, ldf, W, out, ldo, B, K, C);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

extern "C" int da_inception_score(const float* logits, long ld, const int* perm, int N, int C, int splits, double* scores,
                                  int* chunks, hipStream_t s) {
  DA_CLEAR_ERR();
  if (!logits || !perm || !scores || !chunks || N < 1 || C < 1 || C > IS_MAX_C || splits < 1 || ld < C) return DA_ERR_SHAPE;
  if ((((uintptr_t)logits | (uintptr_t)perm) & 3) || ((uintptr_t)scores & 7)) return DA_ERR_SHAPE;
  const int chunk = (int)(((long)N + splits - 1) / splits), n_chunks = (N + chunk - 1) / chunk;
  hipLaunchKernelGGL(inception_score_kernel, dim3((unsigned)n_chunks), dim3(IM_THREADS), (size_t)C * sizeof(double), s,
                     logits, ld, perm, N, C, chunk, scores);
  DA_CHECK_LAUNCH();
  *chunks = n_chunks;
  return DA_OK;
}

extern "C" long da_poly_mmd_workspace(int subsets, int m) {
  if (subsets < 1 || subsets > 65535 || m < 2 || m > 65536) return 0;
  return (long)subsets * mmd_tiles((m + MM_T - 1) / MM_T);
}

extern "C" int da_poly_mmd(const float* Fr, long ldr, int Nr, const float* Ff, long ldf, int Nf, const int* idx_r,
                           const int* idx_f, int subsets, int m, int D, int degree, double gamma, double coef, double* out,
                           double* ws, long ws_doubles, hipStream_t s) {
  DA_CLEAR_ERR();
  if (!Fr || !Ff || !idx_r || !idx_f || !out || !ws || Nr < 1 || Nf < 1) return DA_ERR_SHAPE;
  const long need = da_poly_mmd_workspace(subsets, m);
  if (need == 0 || ws_doubles < need) return DA_ERR_SHAPE;
  if (D < 4 || D % 4 || ldr < D || ldf < D || ldr % 4 || ldf % 4 || degree < 1 || degree > 8) return DA_ERR_SHAPE;
  if (!(gamma > 0.0) || !(coef >= 0.0) || !(gamma < INFINITY) || !(coef < INFINITY)) return DA_ERR_SHAPE;
  if ((((uintptr_t)Fr | (uintptr_t)Ff) & 15) || (((uintptr_t)idx_r | (uintptr_t)idx_f) & 3) ||
      (((uintptr_t)out | (uintptr_t)ws) & 7))
    return DA_ERR_SHAPE;
  const int T = (m + MM_T - 1) / MM_T;
  hipLaunchKernelGGL(poly_mmd_tile_kernel, dim3((unsigned)mmd_tiles(T), (unsigned)subsets), dim3(IM_THREADS), 0, s, Fr, ldr,
                     Ff, ldf, idx_r, idx_f, m, D, T, degree, gamma, coef, ws);
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(poly_mmd_finalize_kernel, dim3((unsigned)((subsets + IM_THREADS - 1) / IM_THREADS)), dim3(IM_THREADS), 0,
                     s, ws, subsets, m, T, out);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
