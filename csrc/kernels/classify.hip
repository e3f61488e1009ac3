// Linear classifier / reward head on fp16 rows (gfx950): score_mode "classify".
// flexible_llm_sharding_amd/classify.py holds the definition.
//
//   out[r, l] = act( sum_k float(x[row(r), k]) * float(w16[l, k]) + bias[l] ),  l < L <= 64, fp32
//
// "Many rows x very few columns": the labels are the N axis of v_mfma_f32_16x16x32_f16.  A block of
// 4 waves owns 16 rows; a wave's A fragment is those 16 rows x 32 columns of x, its B fragments are
// up to four tiles of 16 labels x the same 32 columns of w16 (NT = ceil(L / 16) accumulator tiles on
// one A fragment).  L is padded to 16 * NT in registers only, never in memory: D[row][label] depends on
// A's row and B's label alone, so a lane of an absent label (or row) re-reads the last real one and
// its accumulator entries are never stored; no load is predicated.
// No operand goes through LDS: an x element is used once per wave, so every lane loads its 8
// consecutive fp16 of its row straight into the A layout (through row_index when given); w16 is at
// most 1 MB and is re-read from L2.  Two batches of CLS_U K-steps are register-resident per wave:
// four K-steps of loads are in flight before the first of their MFMAs issues.
// The waves take K in four interleaved slabs fixed by H alone (wave j: K-steps j, j + 4, ...), write
// their 16 x 16 fp32 partials to LDS, and after one barrier every thread adds the four partials of
// its outputs in wave order 0..3, adds the bias, and applies the activation over the row's L values
// (the row's labels sit in 16 consecutive lanes: a 16-lane butterfly for the max and the sum).
// The scalar-load variant (VEC = false: H % 32 != 0, or x / w16 not 16-byte aligned) fills the same
// fragments with 2-byte loads, zeros beyond H: the arithmetic, and so every bit, is the same.
// A row's result depends on that row, w16, the bias and H only; rows at or beyond `rows` are not stored.
#include <math.h>

#include "common.h"
#include "fls.h"

namespace {

constexpr int CLS_THREADS = 256;
constexpr int CLS_WAVES = 4;
constexpr int CLS_ROWS = 16;       // rows per block (the MFMA's M)
constexpr int CLS_U = 2;           // K-steps per register batch; two batches are resident

enum { ACT_NONE = 0, ACT_SOFTMAX = 1, ACT_SIGMOID = 2 };

// 8 fp16 at p[k .. k + 8) as an MFMA operand: one 16-byte load, or 2-byte loads zero-filled from H on
template <bool VEC>
__device__ __forceinline__ half8 cls_load8(const half_t* __restrict__ p, int k, int H) {
  if (VEC) return *(const half8*)(p + k);
  half8 v = {};
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (k + e < H) v[e] = p[k + e];
  return v;
}

template <int NT>
struct ClsFrag {
  half8 a;
  half8 b[NT];
};

__device__ __forceinline__ float group16_max(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int NT, bool VEC>
__global__ __launch_bounds__(CLS_THREADS) void classify_rows_kernel(const half_t* __restrict__ x, size_t ldx,
                                                                    const int* __restrict__ row_index, int rows, int H,
                                                                    const half_t* __restrict__ w, int L,
                                                                    const float* __restrict__ bias, int activation,
                                                                    float* __restrict__ out) {
  __shared__ floatx4 part[CLS_WAVES * NT * WAVE];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, grp = lane >> 4;
  const size_t r0 = (size_t)blockIdx.x * CLS_ROWS;

  // A: row r0 + fr of the call (gathered through row_index); B tile t: label 16 t + fr.  D[row][label]
  // depends on A's row and B's label alone, so a lane of an absent row or label needs no zeros: it
  // re-reads the last real one (an address that is always valid, so no load is predicated) and its
  // accumulator entries are never stored.
  size_t arow = r0 + fr;
  arow = arow < (size_t)rows ? arow : (size_t)rows - 1;
  if (row_index) {
    const int ri = row_index[arow];
    arow = ri > 0 ? (size_t)ri : 0;
  }
  const half_t* xp = x + arow * ldx;
  const half_t* wp[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) wp[t] = w + (size_t)min(16 * t + fr, L - 1) * H;

  floatx4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};

  // this wave's K-steps: wave, wave + 4, ...: n_w of them (a function of H alone).  A batch index
  // past the end loads the last K-step again (never multiplied).
  const int nsteps = (H + 31) >> 5;
  const int n_w = nsteps > wave ? (nsteps - wave + CLS_WAVES - 1) / CLS_WAVES : 0;

  auto load = [&](ClsFrag<NT>(&f)[CLS_U], int i) {
#pragma unroll
    for (int u = 0; u < CLS_U; ++u) {
      const int k = (min(wave + (i + u) * CLS_WAVES, nsteps - 1) << 5) + grp * 8;
      f[u].a = cls_load8<VEC>(xp, k, H);
#pragma unroll
      for (int t = 0; t < NT; ++t) f[u].b[t] = cls_load8<VEC>(wp[t], k, H);
    }
  };
  auto mac = [&](const ClsFrag<NT>(&f)[CLS_U], int left) {      // the batch's first `left` steps
#pragma unroll
    for (int u = 0; u < CLS_U; ++u)
      if (u < left) {
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = mfma16x16x32(f[u].a, f[u].b[t], acc[t]);
      }
  };

  ClsFrag<NT> f0[CLS_U], f1[CLS_U];
  load(f0, 0);
  int i = 0;
  for (; i + 2 * CLS_U <= n_w; i += 2 * CLS_U) {                // two full batches, nothing predicated
    load(f1, i + CLS_U);
    mac(f0, CLS_U);
    load(f0, i + 2 * CLS_U);
    mac(f1, CLS_U);
  }
  load(f1, i + CLS_U);                                          // the last < 2 CLS_U steps
  mac(f0, n_w - i);
  mac(f1, n_w - i - CLS_U);

  // lane holds D[row = 4 grp + r][label = 16 t + fr], r = 0..3
#pragma unroll
  for (int t = 0; t < NT; ++t) part[(wave * NT + t) * WAVE + lane] = acc[t];
  __syncthreads();

  // thread (wave, lane) finishes row 4 grp + wave, labels 16 t + fr
  const float* pf = (const float*)part;
  float v[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    float s = pf[((0 * NT + t) * WAVE + lane) * 4 + wave];
#pragma unroll
    for (int j = 1; j < CLS_WAVES; ++j) s += pf[((j * NT + t) * WAVE + lane) * 4 + wave];
    const int l = 16 * t + fr;
    v[t] = (bias && l < L) ? s + bias[l] : s;
  }
  if (activation == ACT_SOFTMAX) {
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (16 * t + fr < L) m = fmaxf(m, v[t]);
    m = group16_max(m);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      v[t] = 16 * t + fr < L ? expf(v[t] - m) : 0.f;
      sum += v[t];
    }
    sum = group16_sum(sum);
#pragma unroll
    for (int t = 0; t < NT; ++t) v[t] = v[t] / sum;
  } else if (activation == ACT_SIGMOID) {
#pragma unroll
    for (int t = 0; t < NT; ++t) v[t] = 1.0f / (1.0f + expf(-v[t]));
  }
  const size_t orow = r0 + 4 * grp + wave;
  if (orow < (size_t)rows) {
    float* o = out + orow * L;
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (16 * t + fr < L) o[16 * t + fr] = v[t];
  }
}

template <int NT>
int cls_launch(bool vec, dim3 grid, hipStream_t st, const half_t* x, size_t ldx, const int* row_index, int rows, int H,
               const half_t* w, int L, const float* bias, int activation, float* out) {
  if (vec)
    hipLaunchKernelGGL((classify_rows_kernel<NT, true>), grid, dim3(CLS_THREADS), 0, st, x, ldx, row_index, rows, H, w,
                       L, bias, activation, out);
  else
    hipLaunchKernelGGL((classify_rows_kernel<NT, false>), grid, dim3(CLS_THREADS), 0, st, x, ldx, row_index, rows, H,
                       w, L, bias, activation, out);
  FLS_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int fls_classify_rows(const void* x, long long x_stride, const int* row_index, int rows, int H,
                                 const void* w16, int L, const float* bias, int activation, float* out,
                                 fls_stream_t s) {
  if (rows == 0) return 0;
  if (!x || !w16 || !out || rows < 0 || H <= 0 || x_stride < H || L < 1 || L > 64 || activation < ACT_NONE ||
      activation > ACT_SIGMOID)
    return (int)hipErrorInvalidValue;
  auto st = (hipStream_t)s;
  const bool vec = H % 32 == 0 && x_stride % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)w16 & 15) == 0;
  const dim3 grid((unsigned)(((size_t)rows + CLS_ROWS - 1) / CLS_ROWS));
  const half_t* xh = (const half_t*)x;
  const half_t* wh = (const half_t*)w16;
  switch ((L + 15) / 16) {
    case 1: return cls_launch<1>(vec, grid, st, xh, (size_t)x_stride, row_index, rows, H, wh, L, bias, activation, out);
    case 2: return cls_launch<2>(vec, grid, st, xh, (size_t)x_stride, row_index, rows, H, wh, L, bias, activation, out);
    case 3: return cls_launch<3>(vec, grid, st, xh, (size_t)x_stride, row_index, rows, H, wh, L, bias, activation, out);
    default: return cls_launch<4>(vec, grid, st, xh, (size_t)x_stride, row_index, rows, H, wh, L, bias, activation, out);
  }
}
