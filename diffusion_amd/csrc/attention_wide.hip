// Flash-style forward attention for head_dim 512 on gfx950: the single mid-block head of the SD VAE (encoder and decoder).
// No N x N score matrix is written to HBM; forward only (the VAE is frozen).
//
// A 32-query x 512-column fp32 output tile is 256 accumulator registers per lane, so the head dimension is split over the
// four waves of a workgroup instead of the queries (attention.hip: one wave = 32 queries x all 64 columns):
//   workgroup = 64 queries, 32-key steps;  Q (64 x 512 bf16, 64 KB) stays in LDS for the whole sweep.
//   S^T = K.Q^T (32 keys x 64 queries, 512 deep): wave w multiplies query half (w & 1) over d half (w >> 1), 16 MFMAs, and
//     leaves its fp32 partial tile in LDS (lane-linear, 4 KB per wave).
//   softmax: EVERY wave adds the two d-half partials of both query halves (always lower half + upper half) and runs the same
//     online softmax on all 64 queries - identical arithmetic in identical order in the four waves, so the row statistics
//     need no exchange and P^T is, as in attention.hip, directly the B operand of the second product.
//   O^T += V^T.P^T: wave w owns output columns 128w .. 128w+127 (4 column blocks x 2 query halves x 16 = 128 accumulator
//     registers), V^T through the transposed LDS read of the swz_key image.
// K and V have ONE 32 KB stage each (Q 64 + K 32 + V 32 + partials 16 = 144 KB of the 160 KB): K is only read by the first
// product and V only by the second, so the next K tile is requested (LDS-DMA) once every wave is past the first product
// and lands under the second, and the next V tile is requested after the second product and lands under the first.
// Two barriers per step.  Every tile is 8 sub-images [rows][64 bf16] (attn_lds.hpp), one per 64 columns of d.
// Softmax in the exp2 domain on raw scores as in attention.hip: p = exp2(s*sc - m*sc), L2 = m*sc + log2(sum).
#include "attn_lds.hpp"
#include "common.hpp"
#include "diffusion_amd.h"

namespace {

struct WideParams {
  const bf16 *Q, *K, *V;
  bf16* Out;
  float* L2;
  long ldq, ldk, ldv, ldo;
  int H, Nq, Nk;
  float sc;  // softmax scale * log2(e)
};

constexpr int WD = 512;                // head_dim
constexpr int WQ = 64, WK = 32;        // queries per workgroup, keys per step
constexpr int Q_SUB = WQ * 128;        // one [64 queries][64 d] sub-image
constexpr int KV_SUB = WK * 128;       // one [32 keys][64 d] sub-image
constexpr int Q_IMG = 8 * Q_SUB, KV_IMG = 8 * KV_SUB;
constexpr int SX_WAVE = 16 * 64 * 4;   // one wave's fp32 partial S^T tile, [4 register quads][64 lanes][16 B]
constexpr int WIDE_SMEM = Q_IMG + 2 * KV_IMG + 4 * SX_WAVE;
static_assert(WIDE_SMEM <= 160 * 1024, "LDS of one CU");

__device__ __attribute__((aligned(256))) unsigned char g_attnw_zero[256];  // DMA source of rows past Nq / Nk

// ds_read_b128 through inline asm, for the same reason as lds_tr16_b64_asm (common.hpp): ordered with lds_wait_for<>
DEVINL u32x4 lds_b128_asm(unsigned lds_byte_offset) {
  u32x4 r;
  asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"(lds_byte_offset));
  return r;
}

__global__ __launch_bounds__(256) void attn_fwd_wide_kernel(WideParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const Qs = smem;
  char* const Ks = smem + Q_IMG;
  char* const Vs = Ks + KV_IMG;
  char* const Sx = Vs + KV_IMG;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, r = lane & 31;
  const int hd = blockIdx.y, b = blockIdx.z, q0 = blockIdx.x * WQ;
  const int qh = wave & 1, dh = wave >> 1;  // this wave's part of the first product

  // LDS-DMA geometry: one request fills 8 rows x 128 B of a sub-image; wave w takes rows 8w..8w+7 (and 32+8w.. of Q) of all
  // 8 sub-images.  The swizzle is applied on the source column.
  const int drow = wave * 8 + (lane >> 3);
  const int lc = ((lane & 7) ^ swz_key(drow)) * 8;
  const char* zero = reinterpret_cast<const char*>(g_attnw_zero);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = drow + 32 * i;  // swz_key(row) == swz_key(drow)
    const bool ok = q0 + row < p.Nq;
    const bf16* src = p.Q + ((long)b * p.Nq + q0 + row) * p.ldq + hd * WD + lc;
#pragma unroll
    for (int c = 0; c < 8; ++c) dma16(ok ? (const void*)(src + c * 64) : (const void*)zero, Qs + c * Q_SUB + i * 4096 + wave * 1024);
  }
  const bf16* kp = p.K + ((long)b * p.Nk + drow) * p.ldk + hd * WD + lc;
  const bf16* vp = p.V + ((long)b * p.Nk + drow) * p.ldv + hd * WD + lc;
  auto dma_tile = [&](const bf16* src, long ld, int t, char* img) {
    const bool ok = t * WK + drow < p.Nk;
    src += (long)t * WK * ld;
#pragma unroll
    for (int c = 0; c < 8; ++c) dma16(ok ? (const void*)(src + c * 64) : (const void*)zero, img + c * KV_SUB + wave * 1024);
  };
  auto sync = [&]() {  // my requests have landed and my LDS traffic is done; then everyone's
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  f32x16 o[2][4];  // [query half][32-column block of this wave's 128 columns]
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) o[a][j][i] = 0.f;
  float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};

  const int nt = (p.Nk + WK - 1) / WK;
  dma_tile(kp, p.ldk, 0, Ks);
  dma_tile(vp, p.ldv, 0, Vs);
  sync();

  const unsigned qa = lds_offset(Qs) + dh * 4 * Q_SUB, ka = lds_offset(Ks) + dh * 4 * KV_SUB;
  const unsigned va = lds_offset(Vs) + wave * 2 * KV_SUB;
  for (int t = 0; t < nt; ++t) {
    // ---- first product: this wave's 32 keys x 32 queries over 256 of the 512 columns.  8 batches of 2 k-steps (4 reads),
    //      the next batch in flight while the current one is multiplied.
    {
      f32x16 s;
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = 0.f;
      u32x4 kf[2][2], qf[2][2];
      auto issue = [&](int j, int bufi) {  // batch j: sub-image j >> 1 of this wave's four, k-steps 2*(j&1), 2*(j&1)+1
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int chunk = 2 * (2 * (j & 1) + e) + h;
          kf[bufi][e] = lds_b128_asm(ka + (j >> 1) * KV_SUB + swz128(r, chunk));
          qf[bufi][e] = lds_b128_asm(qa + (j >> 1) * Q_SUB + swz128(qh * 32 + r, chunk));
        }
      };
      issue(0, 0);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int cur = j & 1;
        if (j + 1 < 8) {
          issue(j + 1, cur ^ 1);
          lds_wait_for<4>(kf[cur][0], qf[cur][0], kf[cur][1], qf[cur][1]);
        } else {
          lds_wait_for<0>(kf[cur][0], qf[cur][0], kf[cur][1], qf[cur][1]);
        }
#pragma unroll
        for (int e = 0; e < 2; ++e)
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kf[cur][e]),
                                                      __builtin_bit_cast(bf16x8, qf[cur][e]), s, 0, 0, 0);
      }
#pragma unroll
      for (int i4 = 0; i4 < 4; ++i4)
        *reinterpret_cast<f32x4*>(Sx + wave * SX_WAVE + i4 * 1024 + lane * 16) =
            f32x4{s[4 * i4], s[4 * i4 + 1], s[4 * i4 + 2], s[4 * i4 + 3]};
    }
    sync();  // partial tiles visible; K stage released; V tile t has landed

    // ---- softmax of all 64 queries (the same in every wave): query = 32 * a + r on the lane, keys on the registers
    bf16x8 pk[2][2];
    const bool tail = (t + 1) * WK > p.Nk;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      f32x16 sv;
#pragma unroll
      for (int i4 = 0; i4 < 4; ++i4) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(Sx + a * SX_WAVE + i4 * 1024 + lane * 16);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(Sx + (a + 2) * SX_WAVE + i4 * 1024 + lane * 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) sv[4 * i4 + e] = lo[e] + hi[e];
      }
      if (tail) {  // keys >= Nk of the last block: -inf, not score 0
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (t * WK + acc_row(i, lane) >= p.Nk) sv[i] = -INFINITY;
      }
      float mx = sv[0];
#pragma unroll
      for (int i = 1; i < 16; ++i) mx = fmaxf(mx, sv[i]);
      mx = fmaxf(mx, xor32(mx));  // finite: key t * 32 is below Nk and belongs to the lower lane half
      if (__any(mx > m[a])) {
        const float mn = fmaxf(m[a], mx);
        const float alpha = __builtin_amdgcn_exp2f((m[a] - mn) * p.sc);
        l[a] *= alpha;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < 16; ++i) o[a][j][i] *= alpha;
        m[a] = mn;
      }
      const float msc = -m[a] * p.sc;
      float ls = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        sv[i] = __builtin_amdgcn_exp2f(fmaf(sv[i], p.sc, msc));
        ls += sv[i];
      }
      l[a] += ls;  // this lane's 16 of the 32 keys; the halves are joined once, after the sweep
      pk[a][0] = pack8(sv, 0);
      pk[a][1] = pack8(sv, 1);
    }
    if (t + 1 < nt) dma_tile(kp, p.ldk, t + 1, Ks);  // lands under the second product

    // ---- second product: O^T[128 columns of this wave][64 queries] += V^T . P^T
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      short4v tv[4][2];
#pragma unroll
      for (int j = 0; j < 4; ++j) tr_frag_issue(va + (j >> 1) * KV_SUB, 16 * ks, 32 * (j & 1), lane, tv[j][0], tv[j][1]);
      lds_wait_for<0>(tv[0][0], tv[0][1], tv[1][0], tv[1][1], tv[2][0], tv[2][1], tv[3][0], tv[3][1]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16x8 vt = tr_frag_join(tv[j][0], tv[j][1]);
        o[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vt, pk[0][ks], o[0][j], 0, 0, 0);
        o[1][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vt, pk[1][ks], o[1][j], 0, 0, 0);
      }
    }
    sync();  // V stage and partial tiles released; K tile t + 1 has landed
    if (t + 1 < nt) dma_tile(vp, p.ldv, t + 1, Vs);  // lands under the next first product
  }

#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int q = q0 + 32 * a + r;
    const float lt = l[a] + xor32(l[a]);
    const float inv = 1.0f / lt;
    if (q < p.Nq) {  // never store rows >= Nq
      bf16* op = p.Out + ((long)b * p.Nq + q) * p.ldo + hd * WD + wave * 128;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          bf16x4 x;
#pragma unroll
          for (int e = 0; e < 4; ++e) x[e] = f2bf(o[a][j][rg * 4 + e] * inv);
          *reinterpret_cast<bf16x4*>(op + 32 * j + 8 * rg + 4 * h) = x;
        }
      if (wave == 0 && h == 0) p.L2[((long)b * p.H + hd) * p.Nq + q] = m[a] * p.sc + log2f(lt);
    }
  }
}

int bad_ld(long ld, long cols) { return ((ld & 7) || ld < cols) ? 1 : 0; }

}  // namespace

extern "C" int da_attn_fwd_wide(const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, void* O,
                                long ldo, float* L2, int B, int H, int D, int Nq, int Nk, float scale,
                                hipStream_t stream) {
  DA_CLEAR_ERR();
  if (D != WD || B <= 0 || H <= 0 || Nq <= 0 || Nk <= 0) return DA_ERR_SHAPE;
  const long cols = (long)H * D;
  if (bad_ld(ldq, cols) || bad_ld(ldk, cols) || bad_ld(ldv, cols) || bad_ld(ldo, cols)) return DA_ERR_SHAPE;
  if (H > 65535 || B > 65535) return DA_ERR_SHAPE;  // grid y / z
  WideParams p = {};
  p.Q = (const bf16*)Q; p.K = (const bf16*)K; p.V = (const bf16*)V; p.Out = (bf16*)O; p.L2 = L2;
  p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
  p.H = H; p.Nq = Nq; p.Nk = Nk;
  p.sc = scale * 1.4426950408889634f;
  static unsigned long long attr_done = 0;
  if (da_ensure_dyn_smem((const void*)attn_fwd_wide_kernel, WIDE_SMEM, &attr_done) != DA_OK) return DA_ERR_LAUNCH;
  hipLaunchKernelGGL(attn_fwd_wide_kernel, dim3((Nq + WQ - 1) / WQ, H, B), dim3(256), WIDE_SMEM, stream, p);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
