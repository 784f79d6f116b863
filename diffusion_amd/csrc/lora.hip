// LoRA adapters on the merged-shadow path (include/diffusion_amd.h: da_lora_merge, da_lora_project).
//
// An adapted matrix W [N][K] (a contiguous row range of one storage of the flat buffers, ld = K) carries A [r][K] and
// B [N][r] in a flat fp32 adapter buffer.  Three small fp32 products, all on the f32-input MFMA (32x32x2), whose result is
// a k-ordered fmaf chain: every output element is owned by one lane of one workgroup and summed in ascending index order
// from 0, so the bits are a function of the item table alone - no atomics, no split reductions, nothing that depends on
// the grid or on how many CUs run it.
//   merge     shadow[n][k] = bf16(master[n][k] + s * sum_j B[n][j] A[j][k])        tile 32 x 128, j in LDS chunks of 32
//   dA        dA[j][k]     = s * sum_n B[n][j] dW[n][k]                            tile 32 x 128, n in LDS chunks of 32
//   dB        dB[n][j]     = s * sum_k dW[n][k] A[j][k]                            tile 32 x 128, k in LDS chunks of 32
// Operands go through LDS with zeros staged for everything outside the matrix or past r (an odd r, the ragged last tile):
// memory is never padded.  Speed is secondary here (a few GFLOP per optimizer step); the kernels are not pipelined.
#include "common.hpp"
#include "diffusion_amd.h"

struct LoraItem {   // struct DaLoraItem of include/diffusion_amd.h
  long long w_off, a_off, b_off;
  int N, K, r;
  float scale;
  int first_merge, first_da, first_db, reserved;
};
static_assert(sizeof(LoraItem) == sizeof(DaLoraItem), "item layout");

#define LORA_THREADS 256
#define LORA_TN 128   // output columns of a tile: 4 waves x 32
#define LORA_KC 32    // reduction chunk staged in LDS

// last item whose first tile of family F (0 merge, 1 dA, 2 dB) is <= tile
template <int F>
DEVINL int lora_first(const LoraItem& it) { return F == 0 ? it.first_merge : F == 1 ? it.first_da : it.first_db; }
template <int F>
DEVINL int lora_find(const LoraItem* items, int n, int tile) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (lora_first<F>(items[mid]) <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// One 32 x 32 product chunk: acc[i][c] += sum_{q < 32} L[i][q] * R[q][c], q ascending (two per MFMA).  ls / rs: the strides
// of q in the two LDS images, li / rc: this lane's row of L and column of R.
DEVINL f32x16 lora_chunk(const float* L, int li, int ls, const float* R, int rc, int rs, int qn, f32x16 acc) {
  const int h = threadIdx.x >> 5 & 1;
  for (int q = 0; q < qn; q += 2)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(L[li + (q + h) * ls], R[rc + (q + h) * rs], acc, 0, 0, 0);
  return acc;
}

// row of accumulator register g in the 32 x 32 C/D map (column = lane & 31)
DEVINL int lora_row(int g) { return (g & 3) + 8 * (g >> 2) + 4 * (threadIdx.x >> 5 & 1); }

__global__ __launch_bounds__(LORA_THREADS) void lora_merge_kernel(const float* master, const float* ad,
                                                                  const LoraItem* items, int n_items, bf16* shadow,
                                                                  float* vout) {
  __shared__ float Bs[32][LORA_KC + 1];       // [n][j]
  __shared__ float As[LORA_KC][LORA_TN];      // [j][k]
  const LoraItem it = items[lora_find<0>(items, n_items, blockIdx.x)];
  const int local = blockIdx.x - it.first_merge;
  const int kt = (it.K + LORA_TN - 1) / LORA_TN;
  const int n0 = (local / kt) * 32, k0 = (local % kt) * LORA_TN;
  const float* A = ad + it.a_off;
  const float* B = ad + it.b_off;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  f32x16 acc;
#pragma unroll
  for (int g = 0; g < 16; ++g) acc[g] = 0.f;
  for (int j0 = 0; j0 < it.r; j0 += LORA_KC) {
    if (j0) __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = t + LORA_THREADS * q, i = e >> 5, jj = e & 31;
      Bs[i][jj] = (n0 + i < it.N && j0 + jj < it.r) ? B[(long long)(n0 + i) * it.r + j0 + jj] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int e = t + LORA_THREADS * q, jj = e >> 7, c = e & 127;
      As[jj][c] = (j0 + jj < it.r && k0 + c < it.K) ? A[(long long)(j0 + jj) * it.K + k0 + c] : 0.f;
    }
    __syncthreads();
    const int qn = min(LORA_KC, (it.r - j0 + 1) & ~1);
    acc = lora_chunk(&Bs[0][0], (lane & 31) * (LORA_KC + 1), 1, &As[0][0], w * 32 + (lane & 31), LORA_TN, qn, acc);
  }
  const int k = k0 + w * 32 + (lane & 31);
  if (k >= it.K) return;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int n = n0 + lora_row(g);
    if (n >= it.N) continue;
    const long long idx = it.w_off + (long long)n * it.K + k;
    const float m = master[idx];
    // a zero sum leaves the master's own bits (-0 included): B = 0 is exactly da_cast_f32_bf16
    const float v = acc[g] == 0.f ? m : fmaf(it.scale, acc[g], m);
    shadow[idx] = f2bf(v);
    if (vout) vout[idx] = v;
  }
}

// blocks [0, tiles_da): dA tiles; the rest: dB tiles
__global__ __launch_bounds__(LORA_THREADS) void lora_project_kernel(const float* grad, const float* ad,
                                                                    const LoraItem* items, int n_items, int tiles_da,
                                                                    float* adg) {
  __shared__ float Ls[32 * (LORA_KC + 1)];       // dA: B chunk [n][j] (stride 32); dB: dW chunk [n][k] (stride 33)
  __shared__ float Rs[LORA_TN * (LORA_KC + 1)];   // dA: dW chunk [n][k] (stride 128); dB: A chunk [j][k] (stride 33)
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  f32x16 acc;
#pragma unroll
  for (int g = 0; g < 16; ++g) acc[g] = 0.f;
  if ((int)blockIdx.x < tiles_da) {
    const LoraItem it = items[lora_find<1>(items, n_items, blockIdx.x)];
    const int local = blockIdx.x - it.first_da;
    const int kt = (it.K + LORA_TN - 1) / LORA_TN;
    const int j0 = (local / kt) * 32, k0 = (local % kt) * LORA_TN;
    const float* B = ad + it.b_off;
    const float* dW = grad + it.w_off;
    for (int c0 = 0; c0 < it.N; c0 += LORA_KC) {
      if (c0) __syncthreads();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = t + LORA_THREADS * q, nn = e >> 5, jj = e & 31;
        Ls[nn * 32 + jj] = (c0 + nn < it.N && j0 + jj < it.r) ? B[(long long)(c0 + nn) * it.r + j0 + jj] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int e = t + LORA_THREADS * q, nn = e >> 7, c = e & 127;
        Rs[nn * LORA_TN + c] = (c0 + nn < it.N && k0 + c < it.K) ? dW[(long long)(c0 + nn) * it.K + k0 + c] : 0.f;
      }
      __syncthreads();
      const int qn = min(LORA_KC, (it.N - c0 + 1) & ~1);
      acc = lora_chunk(Ls, lane & 31, 32, Rs, w * 32 + (lane & 31), LORA_TN, qn, acc);
    }
    const int k = k0 + w * 32 + (lane & 31);
    if (k >= it.K) return;
    float* dA = adg + it.a_off;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int j = j0 + lora_row(g);
      if (j < it.r) dA[(long long)j * it.K + k] = it.scale * acc[g];
    }
    return;
  }
  const int tile = blockIdx.x - tiles_da;
  const LoraItem it = items[lora_find<2>(items, n_items, tile)];
  const int n0 = (tile - it.first_db) * 32;
  const float* A = ad + it.a_off;
  const float* dW = grad + it.w_off;
  const int jrows = min(LORA_TN, (it.r + 31) & ~31);   // rows of A the tile's waves read
  for (int c0 = 0; c0 < it.K; c0 += LORA_KC) {
    if (c0) __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = t + LORA_THREADS * q, i = e >> 5, kk = e & 31;
      Ls[i * (LORA_KC + 1) + kk] = (n0 + i < it.N && c0 + kk < it.K) ? dW[(long long)(n0 + i) * it.K + c0 + kk] : 0.f;
    }
    for (int e = t; e < jrows * LORA_KC; e += LORA_THREADS) {
      const int j = e >> 5, kk = e & 31;
      Rs[j * (LORA_KC + 1) + kk] = (j < it.r && c0 + kk < it.K) ? A[(long long)j * it.K + c0 + kk] : 0.f;
    }
    __syncthreads();
    if (w * 32 < it.r) {   // wave-uniform: a wave whose 32 columns lie past r only helps staging
      const int qn = min(LORA_KC, (it.K - c0 + 1) & ~1);
      acc = lora_chunk(Ls, (lane & 31) * (LORA_KC + 1), 1, Rs, (w * 32 + (lane & 31)) * (LORA_KC + 1), 1, qn, acc);
    }
  }
  const int j = w * 32 + (lane & 31);
  if (j >= it.r) return;
  float* dB = adg + it.b_off;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int n = n0 + lora_row(g);
    if (n < it.N) dB[(long long)n * it.r + j] = it.scale * acc[g];
  }
}

extern "C" int da_lora_merge(const float* master, const float* adapters, const void* items, int n_items,
                             int total_tiles, void* shadow, float* vout, hipStream_t s) {
  DA_CLEAR_ERR();
  if (n_items <= 0 || total_tiles <= 0 || !master || !adapters || !items || !shadow) return DA_ERR_SHAPE;
  if ((((uintptr_t)master | (uintptr_t)adapters | (uintptr_t)vout) & 3) || ((uintptr_t)shadow & 1) || ((uintptr_t)items & 7))
    return DA_ERR_SHAPE;
  hipLaunchKernelGGL(lora_merge_kernel, dim3(total_tiles), dim3(LORA_THREADS), 0, s, master, adapters,
                     (const LoraItem*)items, n_items, (bf16*)shadow, vout);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

extern "C" int da_lora_project(const float* grad, const float* adapters, const void* items, int n_items, int tiles_da,
                               int tiles_db, float* adapter_grad, hipStream_t s) {
  DA_CLEAR_ERR();
  if (n_items <= 0 || tiles_da <= 0 || tiles_db <= 0 || !grad || !adapters || !items || !adapter_grad) return DA_ERR_SHAPE;
  if ((long long)tiles_da + tiles_db > 0x7fffffffLL) return DA_ERR_SHAPE;
  if ((((uintptr_t)grad | (uintptr_t)adapters | (uintptr_t)adapter_grad) & 3) || ((uintptr_t)items & 7)) return DA_ERR_SHAPE;
  if (adapter_grad == adapters) return DA_ERR_SHAPE;
  hipLaunchKernelGGL(lora_project_kernel, dim3(tiles_da + tiles_db), dim3(LORA_THREADS), 0, s, grad, adapters,
                     (const LoraItem*)items, n_items, tiles_da, adapter_grad);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
