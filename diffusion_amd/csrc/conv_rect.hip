// da_conv2d_relu_fwd: forward convolution with rectangular taps, fp32 bias and optional ReLU (the Inception-v3 tower of the
// FID metric: 1x7, 7x1, 1x3, 3x1, 5x5, 3x3 stride 2 without padding, and the plain 1x1 / 3x3 forms).
//
// Implicit GEMM, Y[M][Cout] = gather(X)[M][K] . W[Cout][K]^T with M = B Hout Wout and K = (tap, channel) flattened, i.e. the
// row-major order of W[n][kh][kw][Cin] itself.  K is walked in 16-byte vectors of 8 channels (Cin % 8 == 0, so a vector never
// straddles a tap): vector kv is tap kv / (Cin/8), channels 8 (kv % (Cin/8)).  A K step of 64 therefore spans several taps
// at Cin = 8, 32, 48, 80 and ends in a zero-filled tail when K % 64 != 0; out-of-image taps, rows >= M and weight rows >=
// Cout are zero vectors as well (the address of a zero vector is replaced by the operand's base, the load itself is
// unconditional, the value is selected afterwards).
//
// Tile: 128 rows x BN columns x 64 k, BN = 32 / 64 / 96 from a host-side table (Cout is 32..448 here); 4 waves, wave w owns
// rows 32 w .. 32 w + 31 and all BN columns: 2 x BN/16 accumulators of v_mfma_f32_16x16x32_bf16.  The product is issued
// transposed (weights as the A operand), so a lane ends with 4 consecutive output channels of one row and stores 8 bytes.
// Both operands are register-staged into two LDS buffers (one barrier per K step): rows of 128 bytes, the 16-byte slot of
// vector v in row r is v ^ (r & 7), which makes both the ds_write_b128 of the fill (8 lanes = one row) and the
// ds_read_b128 of the fragments (16 rows x 2 k groups per lane group) conflict-free.
#include "common.hpp"
#include "diffusion_amd.h"

namespace {

constexpr int CR_BM = 128, CR_BK = 64, CR_THREADS = 256;

struct ConvRectArgs {
  const bf16* X;
  const bf16* W;
  const float* bias;
  bf16* Y;
  long ldx, ldy;
  int Hin, Win, Hout, Wout, Cin, Cout, kw, stride, ph, pw, relu;
  int M, KV;          // rows of the product; 16-byte vectors per weight row (kh kw Cin / 8)
  FastDiv c8, kwd;    // / (Cin / 8), / kw
};

DEVINL int cr_slot(int row, int v) { return row * CR_BK + ((v ^ (row & 7)) << 3); }

template <int BN>
__global__ __launch_bounds__(CR_THREADS) void conv_rect_kernel(const ConvRectArgs a) {
  constexpr int NR = BN / 16;                 // 16-column fragments
  constexpr int BV = BN * 8 / CR_THREADS;     // weight vectors per thread and K step
  constexpr int BUF = (CR_BM + BN) * CR_BK;
  __shared__ __attribute__((aligned(16))) bf16 lds[2 * BUF];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int m0 = blockIdx.x * CR_BM, n0 = blockIdx.y * BN;
  const int vc = t & 7, vr = t >> 3;          // this thread's vector column; its rows are vr + 32 r
  const int HWo = a.Hout * a.Wout, C8 = a.Cin >> 3;

  int pix0[4], ih0[4], iw0[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + vr + 32 * r;
    if (m < a.M) {
      const int b = m / HWo, rem = m - b * HWo, oh = rem / a.Wout, ow = rem - oh * a.Wout;
      pix0[r] = b * a.Hin * a.Win;
      ih0[r] = oh * a.stride - a.ph;
      iw0[r] = ow * a.stride - a.pw;
    } else {
      pix0[r] = 0;
      ih0[r] = -(1 << 20);   // fails every bounds check
      iw0[r] = 0;
    }
  }
  long wrow[BV];
  bool wok[BV];
#pragma unroll
  for (int q = 0; q < BV; ++q) {
    const int n = n0 + vr + 32 * q;
    wok[q] = n < a.Cout;
    wrow[q] = wok[q] ? (long)n * a.KV * 8 : 0;
  }

  bf16x8 ra[4], rb[BV];
  auto fetch = [&](int step) {
    const int kv = step * 8 + vc;
    const bool kok = kv < a.KV;
    const int tap = (int)fdiv((unsigned)kv, a.c8), c = kv - tap * C8;
    const int i = (int)fdiv((unsigned)tap, a.kwd), j = tap - i * a.kw;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ih = ih0[r] + i, iw = iw0[r] + j;
      const bool ok = kok && (unsigned)ih < (unsigned)a.Hin && (unsigned)iw < (unsigned)a.Win;
      const long off = ok ? (long)(pix0[r] + ih * a.Win + iw) * a.ldx + c * 8 : 0;
      const bf16x8 v = ld8(a.X + off);
      ra[r] = ok ? v : zero8();
    }
#pragma unroll
    for (int q = 0; q < BV; ++q) {
      const bool ok = kok && wok[q];
      const bf16x8 v = ld8(a.W + (ok ? wrow[q] + (long)kv * 8 : 0));
      rb[q] = ok ? v : zero8();
    }
  };
  auto stage = [&](int buf) {
    bf16* p = lds + buf * BUF;
#pragma unroll
    for (int r = 0; r < 4; ++r) st8(p + cr_slot(vr + 32 * r, vc), ra[r]);
#pragma unroll
    for (int q = 0; q < BV; ++q) st8(p + cr_slot(CR_BM + vr + 32 * q, vc), rb[q]);
  };

  f32x4 acc[2][NR];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < NR; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int steps = (a.KV + 7) >> 3;
  const int fr = lane & 15, fq = lane >> 4;
  fetch(0);
  stage(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const bool more = s + 1 < steps;
    if (more) fetch(s + 1);
    const bf16* p = lds + (s & 1) * BUF;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 xf[2], wf[NR];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) xf[mi] = ld8(p + cr_slot(32 * w + 16 * mi + fr, kk * 4 + fq));
#pragma unroll
      for (int ni = 0; ni < NR; ++ni) wf[ni] = ld8(p + cr_slot(CR_BM + 16 * ni + fr, kk * 4 + fq));
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < NR; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ni], xf[mi], acc[mi][ni], 0, 0, 0);
    }
    if (more) stage((s + 1) & 1);
    __syncthreads();
  }

  // transposed product: register e of acc[mi][ni] is row fr of fragment mi, channel 4 fq + e of fragment ni
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int m = m0 + 32 * w + 16 * mi + fr;
#pragma unroll
    for (int ni = 0; ni < NR; ++ni) {
      const int n = n0 + 16 * ni + 4 * fq;
      if (m < a.M && n < a.Cout) {   // Cout % 8 == 0: a group of 4 channels is inside or outside as a whole
        f32x4 v = acc[mi][ni];
        if (a.bias) {
          const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias + n);
          v += bv;
        }
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = f2bf(a.relu ? fmaxf(v[e], 0.0f) : v[e]);
        *reinterpret_cast<bf16x4*>(a.Y + (long)m * a.ldy + n) = o;
      }
    }
  }
}

// padded columns of a BN-wide tiling, weighted by what a narrower tile costs per column (the activation tile is re-read
// per column block, and the MFMA-to-LDS-read ratio falls with BN)
int tile_for(int Cout) {
  const int bn[3] = {32, 64, 96};
  const double cost[3] = {1.25, 1.08, 1.0};
  int best = 96;
  double best_score = 1e30;
  for (int i = 0; i < 3; ++i) {
    const double s = (double)((Cout + bn[i] - 1) / bn[i] * bn[i]) * cost[i];
    if (s < best_score) {
      best_score = s;
      best = bn[i];
    }
  }
  return best;
}

}  // namespace

extern "C" int da_conv2d_tile_for(int Cout) { return Cout < 8 || Cout % 8 ? 0 : tile_for(Cout); }

extern "C" int da_conv2d_relu_fwd(const void* X, long ldx, const void* W, const float* bias, void* Y, long ldy, int B,
                                  int Hin, int Win, int Hout, int Wout, int Cin, int Cout, int kh, int kw, int stride,
                                  int ph, int pw, int relu, int tile_n, hipStream_t s) {
  DA_CLEAR_ERR();
  if (!X || !W || !Y || B < 1 || Hin < 1 || Win < 1 || Cin < 8 || Cout < 8 || Cin % 8 || Cout % 8) return DA_ERR_SHAPE;
  if (Cin > 65536 || Cout > 65536 || Hin > 65535 || Win > 65535) return DA_ERR_SHAPE;
  if (kh < 1 || kh > 7 || kw < 1 || kw > 7 || (stride != 1 && stride != 2) || ph < 0 || ph > 3 || pw < 0 || pw > 3)
    return DA_ERR_SHAPE;
  if (Hin + 2 * ph < kh || Win + 2 * pw < kw) return DA_ERR_SHAPE;
  if (Hout != (Hin + 2 * ph - kh) / stride + 1 || Wout != (Win + 2 * pw - kw) / stride + 1) return DA_ERR_SHAPE;
  if (ldx < Cin || ldy < Cout || ldx % 8 || ldy % 8) return DA_ERR_SHAPE;
  if (((uintptr_t)X | (uintptr_t)W | (uintptr_t)Y | (uintptr_t)bias) & 15) return DA_ERR_SHAPE;
  if (relu != 0 && relu != 1) return DA_ERR_SHAPE;
  if (tile_n != 0 && tile_n != 32 && tile_n != 64 && tile_n != 96) return DA_ERR_SHAPE;
  const long M = (long)B * Hout * Wout, pix = (long)B * Hin * Win;
  if (M > 0x7fffffffL - CR_BM || pix > 0x7fffffffL) return DA_ERR_SHAPE;
  ConvRectArgs a;
  a.X = static_cast<const bf16*>(X);
  a.W = static_cast<const bf16*>(W);
  a.bias = bias;
  a.Y = static_cast<bf16*>(Y);
  a.ldx = ldx;
  a.ldy = ldy;
  a.Hin = Hin, a.Win = Win, a.Hout = Hout, a.Wout = Wout, a.Cin = Cin, a.Cout = Cout, a.kw = kw, a.stride = stride;
  a.ph = ph, a.pw = pw, a.relu = relu;
  a.M = (int)M;
  a.KV = kh * kw * (Cin / 8);   // <= 49 * 8192: far inside FastDiv's exact range
  a.c8 = make_fastdiv((unsigned)(Cin / 8));
  a.kwd = make_fastdiv((unsigned)kw);
  const int bn = tile_n ? tile_n : tile_for(Cout);
  const dim3 grid((unsigned)((M + CR_BM - 1) / CR_BM), (unsigned)((Cout + bn - 1) / bn));
  if (bn == 32)
    hipLaunchKernelGGL(conv_rect_kernel<32>, grid, dim3(CR_THREADS), 0, s, a);
  else if (bn == 64)
    hipLaunchKernelGGL(conv_rect_kernel<64>, grid, dim3(CR_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(conv_rect_kernel<96>, grid, dim3(CR_THREADS), 0, s, a);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
