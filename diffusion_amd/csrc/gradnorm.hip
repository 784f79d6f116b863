// Segmented sum of squares of a flat fp32 buffer (the gradient buffer of FlatParams): one sum per storage, the total, and
// from the total the clip coefficient and the step guard that da_adamw_dev reads from device memory.  Stands where Composer's
// GradientClipping (torch.nn.utils.clip_grad_norm_), OptimizerMonitor's l2 norms and the GradScaler's inf/NaN check stand
// in the reference's trainer; none of them returns to the host here.
//
// Three launches, no atomics, no flags: a stage boundary is a launch boundary, and every sum has an order that depends only
// on the descriptor tables, never on the grid (norms.hip chan_reduce / chan_sum_finalize_kernel: the same two-stage shape).
//   stage 1  one workgroup per chunk (<= DA_SUMSQ_CHUNK floats of ONE segment), walking chunks c, c + grid, ... when there are
//            more chunks than the grid cap: a read-only HBM stream, 16 B per lane, 8 loads in flight per lane
//   stage 2  one wave per segment: its chunks' partials in fp64, stored as fp32
//   stage 3  one workgroup: the segments in fp64, the record {sumsq, norm, multiplier, finite} and the skipped-step counter
#include "common.hpp"
#include "diffusion_amd.h"

int da_usable_cus(int cus);  // gemm_nt_v2.hip: #CUs less da_set_option("reserve_cus")

namespace {

constexpr int SS_BLOCK = 256;
constexpr int SS_VEC_PER_LANE = DA_SUMSQ_CHUNK / 4 / SS_BLOCK;  // 8 x 16 B per lane for a full chunk
static_assert(DA_SUMSQ_CHUNK % 1024 == 0 && SS_VEC_PER_LANE * 4 * SS_BLOCK == DA_SUMSQ_CHUNK, "chunk size");

struct ChunkDesc {  // '<qii' on the host
  long off;         // floats from x
  int n;            // 1 .. DA_SUMSQ_CHUNK
  int seg;
};
struct SegDesc {  // '<ii'
  int first_chunk, n_chunks;
};

// Order inside a chunk (a function of (off & 3, n) only): lane t owns 16-byte vectors t, t + 256, ... of the aligned body,
// one accumulator per vector component; the <= 3 scalars before the body go to lanes 0..2 and the <= 3 after it to lanes
// 0..2 as well; then ((a0 + a1) + (a2 + a3)) + head + tail per lane, the xor butterfly over the wave, waves 0..3 in order.
__global__ __launch_bounds__(SS_BLOCK) void sumsq_chunk_kernel(const float* __restrict__ x, const ChunkDesc* __restrict__ cd,
                                                               int n_chunks, float* __restrict__ partial) {
  __shared__ float wsum[SS_BLOCK / 64];
  const int t = threadIdx.x;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const ChunkDesc d = cd[c];
    const float* p = x + d.off;
    int head = (int)((4 - (d.off & 3)) & 3);  // x is 16-byte aligned: scalars up to the next 16-byte boundary
    if (head > d.n) head = d.n;
    const int nvec = (d.n - head) >> 2;
    const int tail = d.n - head - 4 * nvec;
    const f32x4* pv = reinterpret_cast<const f32x4*>(p + head);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (nvec == SS_VEC_PER_LANE * SS_BLOCK) {  // a full aligned chunk: every load issued before the first use
      f32x4 v[SS_VEC_PER_LANE];
#pragma unroll
      for (int k = 0; k < SS_VEC_PER_LANE; ++k) v[k] = pv[t + k * SS_BLOCK];
#pragma unroll
      for (int k = 0; k < SS_VEC_PER_LANE; ++k) acc += v[k] * v[k];
    } else {
      for (int i = t; i < nvec; i += SS_BLOCK) {
        const f32x4 v = pv[i];
        acc += v * v;
      }
    }
    float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    if (t < head) s += p[t] * p[t];
    if (t < tail) {
      const float e = p[head + 4 * nvec + t];
      s += e * e;
    }
    s = wave_sum(s);
    if ((t & 63) == 0) wsum[t >> 6] = s;
    __syncthreads();
    if (t == 0) partial[c] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    __syncthreads();
  }
}

DEVINL double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one wave per segment: lane l takes partials l, l + 64, ... of the segment in chunk order, then the butterfly
__global__ __launch_bounds__(64) void sumsq_segment_kernel(const float* __restrict__ partial, const SegDesc* __restrict__ sd,
                                                           int n_segs, float* __restrict__ seg_sumsq) {
  for (int s = blockIdx.x; s < n_segs; s += gridDim.x) {
    const SegDesc d = sd[s];
    double a = 0.0;
    for (int i = threadIdx.x; i < d.n_chunks; i += 64) a += (double)partial[d.first_chunk + i];
    a = wave_sum_f64(a);
    if (threadIdx.x == 0) seg_sumsq[s] = (float)a;
  }
}

// one workgroup: segments s = t, t + 256, ... per lane in index order, butterfly, waves in order; lane 0 writes the record
__global__ __launch_bounds__(SS_BLOCK) void sumsq_stats_kernel(const float* __restrict__ seg_sumsq, int n_segs,
                                                               DaGradStats* __restrict__ st, float grad_scale,
                                                               float max_norm) {
  __shared__ double wsum[SS_BLOCK / 64];
  const int t = threadIdx.x;
  double a = 0.0;
  for (int i = t; i < n_segs; i += SS_BLOCK) a += (double)seg_sumsq[i];
  a = wave_sum_f64(a);
  if ((t & 63) == 0) wsum[t >> 6] = a;
  __syncthreads();
  if (t == 0) {
    const double tot = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    const float total = (float)tot;
    // one thread: the norm and the coefficient are worked out in fp64 and rounded once each
    const double norm64 = sqrt(tot) * (double)grad_scale;
    const float norm = (float)norm64;
    // torch.nn.utils.clip_grad_norm_: coef = min(1, max_norm / (norm + 1e-6)); exactly 1 when nothing is to be clipped, which
    // is decided on the fp32 norm the record reports.  A NaN norm leaves min(1, NaN) = 1: the multiplier stays finite and the
    // guard word below is what stops the step
    double coef = fmin(1.0, (double)max_norm / (norm64 + 1e-6));
    if (max_norm <= 0.0f || norm <= max_norm) coef = 1.0;
    const bool finite = isfinite(total);
    st->sumsq = total;
    st->norm = norm;
    st->grad_mult = (float)((double)grad_scale * coef);
    st->finite = finite ? 1.0f : 0.0f;
    if (!finite) st->skipped_steps = st->skipped_steps + 1;  // single thread, ordinary load and store
  }
}

}  // namespace

extern "C" long da_segment_sumsq_scratch_floats(int n_chunks) { return n_chunks > 0 ? (long)n_chunks : 0; }

extern "C" int da_segment_sumsq(const float* x, const void* chunk_desc, int n_chunks, const void* seg_desc, int n_segs,
                                float* chunk_partials, float* seg_sumsq, float* stats, float grad_scale, float max_norm,
                                hipStream_t s) {
  DA_CLEAR_ERR();
  if (n_chunks <= 0 || n_segs <= 0 || ((uintptr_t)x & 15)) return DA_ERR_SHAPE;
  if (!x || !chunk_desc || !seg_desc || !chunk_partials || !seg_sumsq || ((uintptr_t)stats & 3)) return DA_ERR_SHAPE;
  // one round of 8 workgroups per usable CU (the memory-bound grid idiom); the walk covers the rest.  The result does not
  // depend on this number
  const int cap = da_usable_cus(256) * 8;
  hipLaunchKernelGGL(sumsq_chunk_kernel, dim3(n_chunks < cap ? n_chunks : cap), dim3(SS_BLOCK), 0, s, x,
                     (const ChunkDesc*)chunk_desc, n_chunks, chunk_partials);
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(sumsq_segment_kernel, dim3(n_segs < cap ? n_segs : cap), dim3(64), 0, s, chunk_partials,
                     (const SegDesc*)seg_desc, n_segs, seg_sumsq);
  DA_CHECK_LAUNCH();
  if (stats) {
    hipLaunchKernelGGL(sumsq_stats_kernel, dim3(1), dim3(SS_BLOCK), 0, s, seg_sumsq, n_segs, (DaGradStats*)stats,
                       grad_scale, max_norm);
    DA_CHECK_LAUNCH();
  }
  return DA_OK;
}
