// Raw-image ingest: LargestCenterSquare(R) + ToTensor + Normalize(0.5, 0.5) of packed RGB uint8 images, i.e. PIL's
// antialiased bilinear resize of the shorter side to R followed by the centre crop, written straight into the layout the
// VAE encoder's conv_in reads (NHWC-8 bf16) or into the reference's fp32 NCHW `image` tensor.
//
// Arithmetic.  Along one axis (n_in source samples -> n_out resized samples, M = max(n_in, n_out)) output index i has its
// filter centre at c = (i + 0.5) n_in / n_out and the tap at source index x weighs 1 - |x - c + 0.5| / max(n_in/n_out, 1).
// With num = 2 n_out x + n_out - (2 i + 1) n_in that weight is (2M - |num|) / 2M: an INTEGER numerator W over a constant
// that the normalisation cancels.  So the weights are kept as exact integers, the tap window [lo, hi) comes from integer
// divisions (no float centre that loses bits at index 4000 of a 60000-pixel axis), the sums run in fp64 and are divided by
// the integer weight sum: a constant image comes out as exactly that constant (partition of unity holds at the borders,
// where the window is clipped), and every other value carries two fp32 roundings - the row cache and the output.
//
// Staging.  One 256-thread block owns a 16x16 tile of the cropped output of one image.  The source rows the tile needs are
// walked in chunks of 16: thread (r, x) filters source row v0 + r horizontally for output column x (3 channels, byte loads,
// nothing wider: an image may start at any byte address) into a 16x16x3 fp32 row cache in LDS; after a barrier thread
// (y, x) adds the rows of the chunk that fall into its vertical window.  Tap counts are loop bounds, not array sizes.
// The horizontal pass is shared by the 16 rows of the tile; vertically adjacent tiles repeat the rows their windows share
// ((16 + 2) / 16 of the minimum when downscaling).  Every read is at row lo..hi-1 < h, column lo..hi-1 < w of its own image.
//
// Rectangular targets.  The kernel takes the target as Rh rows x Rw columns and resizes to COVER it: the axis whose scale
// factor is the larger one lands exactly on its target extent (w Rh <= h Rw: nw = Rw, nh = floor(Rw h / w); else nh = Rh,
// nw = floor(Rh w / h)), so nw >= Rw and nh >= Rh and the centre crop lies inside the resized image.  At Rh == Rw the test
// is w <= h and the rule is LargestCenterSquare's: da_image_ingest is the same kernel with Rh = Rw = R.
//
// da_image_ingest_aug: the same cover-resize with the crop window and a horizontal flip chosen per image, aug[b] = (top,
// left, flip) in resized-image pixels: out[Y][X] = resized[top + Y][c] with c = left + X, or c = nw - 1 - (left + X) when
// flip = 1 (the crop at `left` of the mirrored image).  Only the index handed to axis_setup changes, so both passes are
// the ones above.  The kernel clamps top into [0, nh - Rh] and left into [0, nw - Rw]; no table can move a tap outside its
// image.  A flipped column has the mirrored taps with the same integer weights (num changes sign, |num| does not), and the
// horizontal sums are integers exact in fp64, so flip = 1 gives bit for bit what the mirrored source gives without it.
//
// da_image_resize: the same kernel with three independent switches (the COCO evaluation loader's transforms).
// geometry 1 stretches instead: nw = Rw, nh = Rh, crop origin 0, each axis resized on its own.  range 1 writes v / 255
// (ToTensor alone) instead of v / 127.5 - 1.  filter 1 is the two-tap bilinear of F.interpolate(align_corners=False,
// antialias=False): with num = max((2 i + 1) n_in - n_out, 0), i0 = num / (2 n_out) and r = num - 2 n_out i0 the taps are
// i0 and min(i0 + 1, n_in - 1) with the integer weights 2 n_out - r and r.  That is the window [i0, i0 + 2) clipped at n_in
// with W = 2 n_out - |num'|, num' starting at -r and stepping by 2 n_out: the antialiased filter's tap loop with M = n_out,
// so both passes and the normalisation by the integer weight sum are shared.
//
// Row walk with filter 1.  The two source rows of an output row are n_in / n_out apart from the next row's, so when
// reducing the windows of a tile's 16 rows are islands in [vlo, vhi) and not one contiguous run.  Before a chunk is staged
// every thread finds (from the row table in LDS, the same answer in all threads) the first output row whose window ends
// after the chunk's start; if that window begins past the chunk, the chunk start jumps forward by whole chunks to the one
// the window begins in.  A chunk no row falls into is neither read nor filtered, and at most 2 * 16 chunks are staged per
// tile whatever the reduction.  With filter 0 consecutive windows always touch, so nothing is ever skipped and the walk is
// the one above.
#include "common.hpp"
#include "diffusion_amd.h"

namespace {

constexpr int IMG_TILE = 16;       // output tile side; block = IMG_TILE^2 threads
constexpr int IMG_MAX_SIDE = 65535;  // sides above this are skipped (nothing written): keeps every numerator inside int32 / int64

// the taps of output index i (in the resized, uncropped axis): window [lo, hi), numerator of the first tap, 1 / sum of W
DEVINL void axis_setup(int n_in, int n_out, int i, int* lo_, int* hi_, int* num_, double* inv_) {
  const long long M2 = 2LL * (n_in > n_out ? n_in : n_out), ci = (2LL * i + 1) * n_in;
  const long long a_lo = ci - M2 + n_out, a_hi = ci + M2 + n_out;
  long long lo = a_lo > 0 ? a_lo / (2LL * n_out) : 0;   // int(c - fs + 0.5) clipped at 0
  long long hi = a_hi / (2LL * n_out);                  // int(c + fs + 0.5) clipped at n_in
  if (hi > n_in) hi = n_in;
  if (lo > hi) lo = hi;
  const int num0 = (int)(2LL * n_out * lo + n_out - ci);
  long long sum = 0;
  int num = num0;
  for (int x = (int)lo; x < (int)hi; ++x, num += 2 * n_out) {
    const int W = (int)M2 - abs(num);
    sum += W > 0 ? W : 0;
  }
  *lo_ = (int)lo;
  *hi_ = (int)hi;
  *num_ = num0;
  *inv_ = sum > 0 ? 1.0 / (double)sum : 0.0;
}

// the two taps of output index i for filter 1, in axis_setup's terms (see the header comment)
DEVINL void axis_setup_two_tap(int n_in, int n_out, int i, int* lo_, int* hi_, int* num_, double* inv_) {
  const long long d = 2LL * n_out;
  long long num = (2LL * i + 1) * n_in - n_out;
  if (num < 0) num = 0;
  const long long i0 = num / d;   // <= n_in - 1
  const int r = (int)(num - i0 * d);
  const bool two = i0 + 1 < n_in;   // at the last sample both taps are i0: one tap of weight 2 n_out - r, normalised to 1
  *lo_ = (int)i0;
  *hi_ = (int)i0 + (two ? 2 : 1);
  *num_ = -r;
  *inv_ = 1.0 / (double)(two ? d : d - r);
}

// One body for every entry.  AUG = false is the centre crop (da_image_ingest, da_image_ingest_rect, da_image_resize); AUG = true
// takes the crop origin and a horizontal flip per image from aug[b] = (top, left, flip), in resized-image pixels (see the
// header comment).  The switch is a template argument: the centre-crop kernel carries no trace of the other.
template <bool AUG>
DEVINL void image_ingest_body(const unsigned char* __restrict__ src, const long long* __restrict__ off,
                              const int* __restrict__ hw, const int* __restrict__ aug, int Rh, int Rw, int tiles_y,
                              int tiles_x, void* __restrict__ out, int kind, int geometry, int filter, int range) {
  __shared__ int s_lo[2][IMG_TILE], s_hi[2][IMG_TILE], s_num[2][IMG_TILE];
  __shared__ double s_inv[2][IMG_TILE];
  __shared__ float s_row[IMG_TILE][IMG_TILE][3];
  const int t = threadIdx.x;
  const int b = blockIdx.x / (tiles_y * tiles_x), tile = blockIdx.x - b * (tiles_y * tiles_x);
  const int ty0 = (tile / tiles_x) * IMG_TILE, tx0 = (tile % tiles_x) * IMG_TILE;
  const int h = hw[2 * b], w = hw[2 * b + 1];
  if (h < 1 || w < 1 || h > IMG_MAX_SIDE || w > IMG_MAX_SIDE) return;   // uniform over the block, before any barrier
  // geometry: resize to cover Rh x Rw (the tighter axis lands on its target, the other one is floored); crop origin rounded
  // half to even.  w * Rh, h * Rw <= 65535 * 4096 < 2^31.  geometry 1 (stretch): the target itself, no crop.
  const bool fit_w = w * Rh <= h * Rw;
  const int nw = geometry || fit_w ? Rw : (int)((long long)Rh * w / h);
  const int nh = geometry ? Rh : fit_w ? (int)((long long)Rw * h / w) : Rh;
  int top, left, flip = 0;
  if (AUG) {   // the caller's origins, clamped into [0, n - R]: whatever aug holds, every tap stays inside the image
    top = min(max(aug[3 * b], 0), nh - Rh);
    left = min(max(aug[3 * b + 1], 0), nw - Rw);
    flip = aug[3 * b + 2];
    if (flip & ~1) return;   // not 0 or 1: the image is skipped like an oversized one (uniform over the block, no barrier yet)
  } else {
    const int qy = (nh - Rh) >> 1, qx = (nw - Rw) >> 1;
    top = ((nh - Rh) & 1) ? qy + (qy & 1) : qy;
    left = ((nw - Rw) & 1) ? qx + (qx & 1) : qx;
  }
  if (t < 2 * IMG_TILE) {
    const int a = t >> 4, j = t & (IMG_TILE - 1);   // a = 0: columns, 1: rows; indices past the target repeat the last one
    int i = a ? min(ty0 + j, Rh - 1) + top : min(tx0 + j, Rw - 1) + left;
    if (AUG && !a && flip) i = nw - 1 - i;   // the crop at `left` of the mirrored image: resized column nw - 1 - (left + X)
    if (filter)
      axis_setup_two_tap(a ? h : w, a ? nh : nw, i, &s_lo[a][j], &s_hi[a][j], &s_num[a][j], &s_inv[a][j]);
    else
      axis_setup(a ? h : w, a ? nh : nw, i, &s_lo[a][j], &s_hi[a][j], &s_num[a][j], &s_inv[a][j]);
  }
  __syncthreads();
  const unsigned char* img = src + off[b];
  const int x = t & (IMG_TILE - 1), y = t >> 4;
  const int xlo = s_lo[0][x], xhi = s_hi[0][x], xnum = s_num[0][x];
  const int ylo = s_lo[1][y], yhi = s_hi[1][y], ynum = s_num[1][y];
  const double xinv = s_inv[0][x];
  const int M2x = 2 * (!filter && w > nw ? w : nw), M2y = 2 * (!filter && h > nh ? h : nh);
  const int vlo = s_lo[1][0], vhi = s_hi[1][IMG_TILE - 1];   // lo and hi do not decrease with the row
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
  for (int v0 = vlo; v0 < vhi; v0 += IMG_TILE) {
    if (filter) {   // two-tap windows are islands: jump to the chunk the next window begins in (uniform over the block)
      int j = 0;
      while (j < IMG_TILE && s_hi[1][j] <= v0) ++j;
      if (j == IMG_TILE) break;
      const int nlo = s_lo[1][j];
      if (nlo >= v0 + IMG_TILE) v0 += (nlo - v0) / IMG_TILE * IMG_TILE;
    }
    const int v = v0 + y;   // horizontal pass: this thread's source row of the chunk, output column x
    if (v < vhi) {
      const unsigned char* p = img + ((long)v * w + xlo) * 3;
      double h0 = 0.0, h1 = 0.0, h2 = 0.0;
      int num = xnum;
      for (int u = xlo; u < xhi; ++u, p += 3, num += 2 * nw) {
        const int W = M2x - abs(num);
        const double dw = (double)(W > 0 ? W : 0);
        h0 = fma(dw, (double)p[0], h0);
        h1 = fma(dw, (double)p[1], h1);
        h2 = fma(dw, (double)p[2], h2);
      }
      s_row[y][x][0] = (float)(h0 * xinv);
      s_row[y][x][1] = (float)(h1 * xinv);
      s_row[y][x][2] = (float)(h2 * xinv);
    }
    __syncthreads();
    const int r0 = max(ylo - v0, 0), r1 = min(yhi - v0, IMG_TILE);   // vertical pass over the rows of this chunk in [ylo, yhi)
    int num = ynum + (v0 + r0 - ylo) * (2 * nh);
    for (int r = r0; r < r1; ++r, num += 2 * nh) {
      const int W = M2y - abs(num);
      const double dw = (double)(W > 0 ? W : 0);
      acc0 = fma(dw, (double)s_row[r][x][0], acc0);
      acc1 = fma(dw, (double)s_row[r][x][1], acc1);
      acc2 = fma(dw, (double)s_row[r][x][2], acc2);
    }
    __syncthreads();
  }
  const int Y = ty0 + y, X = tx0 + x;
  if (Y >= Rh || X >= Rw) return;
  // range 0: ToTensor (/255) and Normalize(0.5, 0.5), v / 127.5 - 1; range 1: ToTensor alone, v / 255
  const double k = s_inv[1][y] * (range ? 1.0 / 255.0 : 1.0 / 127.5), sub = range ? 0.0 : 1.0;
  const float o0 = (float)(acc0 * k - sub), o1 = (float)(acc1 * k - sub), o2 = (float)(acc2 * k - sub);
  if (kind == 0) {
    bf16x8 o = zero8();
    o[0] = f2bf(o0);
    o[1] = f2bf(o1);
    o[2] = f2bf(o2);
    st8(static_cast<bf16*>(out) + (((long)b * Rh + Y) * Rw + X) * 8, o);
  } else {
    float* of = static_cast<float*>(out) + ((long)b * 3 * Rh + Y) * Rw + X;
    of[0] = o0;
    of[(long)Rh * Rw] = o1;
    of[2L * Rh * Rw] = o2;
  }
}

__global__ __launch_bounds__(IMG_TILE* IMG_TILE) void image_ingest_kernel(const unsigned char* __restrict__ src,
                                                                          const long long* __restrict__ off,
                                                                          const int* __restrict__ hw, int Rh, int Rw,
                                                                          int tiles_y, int tiles_x,
                                                                          void* __restrict__ out, int kind, int geometry,
                                                                          int filter, int range) {
  image_ingest_body<false>(src, off, hw, nullptr, Rh, Rw, tiles_y, tiles_x, out, kind, geometry, filter, range);
}

__global__ __launch_bounds__(IMG_TILE* IMG_TILE) void image_ingest_aug_kernel(const unsigned char* __restrict__ src,
                                                                              const long long* __restrict__ off,
                                                                              const int* __restrict__ hw,
                                                                              const int* __restrict__ aug, int Rh, int Rw,
                                                                              int tiles_y, int tiles_x,
                                                                              void* __restrict__ out, int kind) {
  image_ingest_body<true>(src, off, hw, aug, Rh, Rw, tiles_y, tiles_x, out, kind, 0, 0, 0);
}

// aug == nullptr: the centre-crop kernel; else the per-image crop / flip kernel (geometry, filter, range are then 0)
int launch_ingest(const unsigned char* src, const long long* off, const int* hw, const int* aug, int B, int Rh, int Rw,
                  void* out, int out_kind, int geometry, int filter, int range, hipStream_t s) {
  DA_CLEAR_ERR();
  if ((geometry | filter | range) & ~1) return DA_ERR_SHAPE;
  if (B < 1 || Rh < 1 || Rh > 4096 || Rw < 1 || Rw > 4096 || (out_kind != 0 && out_kind != 1) || !src || !off || !hw ||
      !out)
    return DA_ERR_SHAPE;
  if (out_kind == 0 && ((uintptr_t)out & 15)) return DA_ERR_SHAPE;
  if (out_kind == 1 && ((uintptr_t)out & 3)) return DA_ERR_SHAPE;
  const int tiles_y = (Rh + IMG_TILE - 1) / IMG_TILE, tiles_x = (Rw + IMG_TILE - 1) / IMG_TILE;
  const long blocks = (long)B * tiles_y * tiles_x;
  if (blocks > 0x7fffffffL) return DA_ERR_SHAPE;
  if (aug)
    hipLaunchKernelGGL(image_ingest_aug_kernel, dim3((unsigned)blocks), dim3(IMG_TILE * IMG_TILE), 0, s, src, off, hw, aug,
                       Rh, Rw, tiles_y, tiles_x, out, out_kind);
  else
    hipLaunchKernelGGL(image_ingest_kernel, dim3((unsigned)blocks), dim3(IMG_TILE * IMG_TILE), 0, s, src, off, hw, Rh, Rw,
                       tiles_y, tiles_x, out, out_kind, geometry, filter, range);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // namespace

extern "C" int da_image_ingest(const unsigned char* src, const long long* off, const int* hw, int B, int R, void* out,
                               int out_kind, hipStream_t s) {
  return launch_ingest(src, off, hw, nullptr, B, R, R, out, out_kind, 0, 0, 0, s);
}

extern "C" int da_image_ingest_rect(const unsigned char* src, const long long* off, const int* hw, int B, int Rh, int Rw,
                                    void* out, int out_kind, hipStream_t s) {
  return launch_ingest(src, off, hw, nullptr, B, Rh, Rw, out, out_kind, 0, 0, 0, s);
}

extern "C" int da_image_resize(const unsigned char* src, const long long* off, const int* hw, int B, int Rh, int Rw,
                               void* out, int out_kind, int geometry, int filter, int range, hipStream_t s) {
  return launch_ingest(src, off, hw, nullptr, B, Rh, Rw, out, out_kind, geometry, filter, range, s);
}

extern "C" int da_image_ingest_aug(const unsigned char* src, const long long* off, const int* hw, const int* aug, int B,
                                   int Rh, int Rw, void* out, int out_kind, hipStream_t s) {
  if (!aug) return DA_ERR_SHAPE;
  return launch_ingest(src, off, hw, aug, B, Rh, Rw, out, out_kind, 0, 0, 0, s);
}
