// Segment pooling of fp16 rows into fp32 embeddings (gfx950): score_mode "embed".
// flexible_llm_sharding_amd/embed.py holds the definition and the summation order.
//
// Launch 1, pool_rows_kernel: a grid over (segment, column slab).  Every thread owns 8 columns
// (VEC: one 16-byte load per row) or 1 column (scalar path) and adds the segment's rows to its
// fp32 accumulators in row order, then divides by the row count.  Columns are independent, so the
// row loop holds no barrier, and a column's value is the same on both paths.
// Launch 2 (normalise only), l2_normalize_kernel: one block per segment scales its D fp32 values
// by 1 / max(||e||, 1e-12); the sum of squares is taken in an order fixed by D alone.
// A segment's output depends on its own rows only: not on the grid, the other segments, or on
// whether its rows are gathered (row_idx) or contiguous.
#include "common.h"
#include "fls.h"

namespace {

constexpr int POOL_THREADS = 256;
constexpr int POOL_UNROLL = 8;      // row loads in flight per thread

// row j of the (gathered) row list -> its row in x, clamped into the buffer
__device__ __forceinline__ int pool_src_row(const int* __restrict__ row_idx, int j, int n_src) {
  int r = row_idx ? row_idx[j] : j;
  r = r < 0 ? 0 : r;
  return r >= n_src ? n_src - 1 : r;
}

template <bool VEC>   // 16-byte loads: ld % 8 == 0 and a 16-byte aligned base
__global__ __launch_bounds__(POOL_THREADS) void pool_rows_kernel(const half_t* __restrict__ x, int ld, int n_src,
                                                                 const int* __restrict__ row_idx, int n_list,
                                                                 const int* __restrict__ seg_start, int D,
                                                                 float* __restrict__ out) {
  const int seg = blockIdx.x;
  int j0 = seg_start[seg], j1 = seg_start[seg + 1];
  j0 = j0 < 0 ? 0 : j0;
  j1 = j1 > n_list ? n_list : j1;
  const int n = j1 > j0 ? j1 - j0 : 0;
  float* o = out + (size_t)seg * D;
  constexpr int W = VEC ? 8 : 1;
  const int c0 = (blockIdx.y * POOL_THREADS + threadIdx.x) * W;
  if (c0 >= D) return;
  const int nc = D - c0 < W ? D - c0 : W;        // columns this thread owns (a partial last vector)
  float acc[W];
#pragma unroll
  for (int k = 0; k < W; ++k) acc[k] = 0.f;
  if (n > 0 && VEC && nc == W) {
    // the first row starts the sum (a lone row keeps its bits, a signed zero included)
    const half8 f = *(const half8*)(x + (size_t)pool_src_row(row_idx, j0, n_src) * ld + c0);
#pragma unroll
    for (int k = 0; k < W; ++k) acc[k] = (float)f[k];
    int j = j0 + 1;
    for (; j + POOL_UNROLL <= j1; j += POOL_UNROLL) {
      half8 v[POOL_UNROLL];
#pragma unroll
      for (int u = 0; u < POOL_UNROLL; ++u)
        v[u] = *(const half8*)(x + (size_t)pool_src_row(row_idx, j + u, n_src) * ld + c0);
#pragma unroll
      for (int u = 0; u < POOL_UNROLL; ++u)
#pragma unroll
        for (int k = 0; k < W; ++k) acc[k] += (float)v[u][k];
    }
    for (; j < j1; ++j) {
      const half8 v = *(const half8*)(x + (size_t)pool_src_row(row_idx, j, n_src) * ld + c0);
#pragma unroll
      for (int k = 0; k < W; ++k) acc[k] += (float)v[k];
    }
  } else if (n > 0) {
    // scalar loads, the same additions in the same order; never reads a column >= D
    for (int j = j0; j < j1; ++j) {
      const half_t* xr = x + (size_t)pool_src_row(row_idx, j, n_src) * ld + c0;
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (k < nc) acc[k] = j == j0 ? (float)xr[k] : acc[k] + (float)xr[k];
    }
  }
  const float fn = (float)n;
#pragma unroll
  for (int k = 0; k < W; ++k)
    if (k < nc) o[c0 + k] = n > 0 ? acc[k] / fn : 0.f;     // an empty segment: zeros, no row read
}

// e <- e / max(||e||_2, 1e-12) per row of D fp32 values.  Thread t sums the squares of columns
// t, t + 256, ... in ascending order; the 64 lanes of a wave combine by the xor butterfly
// (offsets 32 .. 1), the 4 waves in wave order.
__global__ __launch_bounds__(POOL_THREADS) void l2_normalize_kernel(float* __restrict__ out, int D) {
  __shared__ float red[POOL_THREADS / WAVE];
  float* o = out + (size_t)blockIdx.x * D;
  float ss = 0.f;
  for (int c = threadIdx.x; c < D; c += POOL_THREADS) {
    const float v = o[c];
    ss += v * v;
  }
  ss = warp_sum(ss);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int i = 0; i < POOL_THREADS / WAVE; ++i) tot += red[i];
  const float nrm = fmaxf(sqrtf(tot), 1e-12f);
  for (int c = threadIdx.x; c < D; c += POOL_THREADS) o[c] = o[c] / nrm;
}

}  // namespace

extern "C" int fls_pool_rows(const void* x, int ld, int n_src, int H, const int* row_idx, int n_list,
                             const int* seg_start, int n_seg, int D, int normalize, float* out, fls_stream_t s) {
  if (n_seg <= 0) return 0;
  if (!x || !seg_start || !out || H <= 0 || ld < H || D < 1 || D > H || n_src < 0 || n_list < 0 ||
      (!row_idx && n_list > n_src) || (n_list > 0 && n_src == 0))
    return (int)hipErrorInvalidValue;
  auto st = (hipStream_t)s;
  const bool vec = ld % 8 == 0 && ((uintptr_t)x & 15) == 0;
  const int per_block = POOL_THREADS * (vec ? 8 : 1);
  const dim3 grid(n_seg, (D + per_block - 1) / per_block);
  if (vec)
    hipLaunchKernelGGL(pool_rows_kernel<true>, grid, dim3(POOL_THREADS), 0, st, (const half_t*)x, ld, n_src, row_idx,
                       n_list, seg_start, D, out);
  else
    hipLaunchKernelGGL(pool_rows_kernel<false>, grid, dim3(POOL_THREADS), 0, st, (const half_t*)x, ld, n_src, row_idx,
                       n_list, seg_start, D, out);
  FLS_CHECK_LAUNCH();
  if (normalize) {
    hipLaunchKernelGGL(l2_normalize_kernel, dim3(n_seg), dim3(POOL_THREADS), 0, st, out, D);
    FLS_CHECK_LAUNCH();
  }
  return 0;
}
