// Weight-only FP8 (OCP e4m3fn) expansion in place in the HBM weight slot (gfx950).
//
// A tensor of N weights owns a 2N-byte region of the layer image.  Its N checkpoint bytes land
// in the upper half [N, 2N) (runtime/stream.py); this file expands them to N fp16 values filling
// the whole region, with no memory beyond the region and the scales:
//
//   w16[i] = fp16_rne( fp32(e4m3fn(b[i])) * scale(i) )        (flexible_llm_sharding_amd/fp8.py)
//
// Element i is read at byte N + i and written at bytes [2i, 2i + 2).  A launch that expands
// elements [a, b) in parallel writes bytes [2a, 2b) and must not touch a source byte that is still
// unread, i.e. any byte >= N + a: it may run iff 2b <= N + a.  So each stream-ordered launch takes
// half of what is left (rounded down to the 16-element vector), and once at most kTail elements are
// left one block reads them all into registers, barriers, and writes them: about
// log2(N / kTail) + 1 launches per tensor (17 for 8192 x 28672).
//
// Each thread converts 16 weights: one 16-byte load, v_cvt_pk_f32_fp8 (gfx950 converts OCP
// e4m3fn), a plain fp32 multiply, v_cvt_f16_f32 (round to nearest even, overflow to +-inf), two
// 16-byte stores.  A region base that is not 16-byte aligned or an N that is no multiple of 16
// takes the same schedule with scalar loads and stores.
#include "common.h"
#include "fls.h"

namespace {

constexpr int kPerThread = 16;
constexpr int kThreads = 256;
constexpr int kTail = kPerThread * kThreads;   // elements the final single-block launch can hold

// scale kinds (flexible_llm_sharding_amd/fp8.py): 0 per tensor, 1 per row, 2 per 128 x 128 block
__device__ __forceinline__ float scale_at(const float* __restrict__ sc, int kind, uint64_t row, uint32_t col,
                                          uint32_t sb_cols) {
  if (kind == 1) return sc[row];
  if (kind == 2) return sc[(row >> 7) * sb_cols + (col >> 7)];
  return sc[0];
}

// fp16_rne of an fp32 product.  The product passes through an opaque register first: the compiler
// otherwise folds multiply + convert into one mixed-precision FMA with a +0 addend, which turns a
// -0 product into +0 (the definition is a plain fp32 multiply, then one rounding).
__device__ __forceinline__ half_t to_half(float p) {
  asm volatile("" : "+v"(p));
  return (half_t)p;
}

// region: the tensor's 2N-byte region; this launch expands elements [a, a + cnt).  TAIL: one block,
// cnt <= kTail, reads of every thread complete before any write (the ranges overlap).
// UNIFORM: the 16 elements of a thread share one scale (per tensor, or cols % 16 == 0).
template <bool VEC, bool TAIL, bool UNIFORM>
__global__ __launch_bounds__(kThreads) void dequant_fp8_kernel(uint8_t* region, uint64_t N, uint64_t a, uint64_t cnt,
                                                               const float* __restrict__ sc, int kind,
                                                               uint64_t cols, uint32_t sb_cols) {
  const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const uint64_t off = t * kPerThread;
  const bool active = off < cnt;
  if (!TAIL && !active) return;
  const uint64_t e0 = a + off;
  const int n = active ? (int)min((uint64_t)kPerThread, cnt - off) : 0;
  half_t o[kPerThread];
  if (active) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    const uint8_t* src = region + N + e0;
    if (VEC && n == kPerThread) {
      const uint4 v = *(const uint4*)src;
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
      for (int j = 0; j < n; ++j) w[j >> 2] |= (uint32_t)src[j] << (8 * (j & 3));
    }
    float f[kPerThread];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], false);
      const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], true);
      f[4 * j] = lo[0]; f[4 * j + 1] = lo[1]; f[4 * j + 2] = hi[0]; f[4 * j + 3] = hi[1];
      // e4m3fn's -0 (0x80) keeps its sign: the byte's sign bit is carried over explicitly (every
      // other negative pattern has it set already)
#pragma unroll
      for (int b = 0; b < 4; ++b)
        f[4 * j + b] = __uint_as_float(__float_as_uint(f[4 * j + b]) | ((w[j] << (24 - 8 * b)) & 0x80000000u));
    }
    if (UNIFORM) {
      uint64_t row = 0;
      uint32_t col = 0;
      if (kind != 0) {
        row = e0 / cols;
        col = (uint32_t)(e0 - row * cols);
      }
      const float s = scale_at(sc, kind, row, col, sb_cols);
#pragma unroll
      for (int j = 0; j < kPerThread; ++j) o[j] = to_half(f[j] * s);
    } else {
      uint64_t row = e0 / cols;
      uint32_t col = (uint32_t)(e0 - row * cols);
#pragma unroll
      for (int j = 0; j < kPerThread; ++j) {
        if (j < n) {
          o[j] = to_half(f[j] * scale_at(sc, kind, row, col, sb_cols));
          if (++col == (uint32_t)cols) { col = 0; ++row; }
        } else {
          o[j] = (half_t)0.f;
        }
      }
    }
  }
  if (TAIL) __syncthreads();
  if (!active) return;
  half_t* dst = (half_t*)region + e0;
  if (VEC && n == kPerThread) {
    half8 v0, v1;
#pragma unroll
    for (int j = 0; j < 8; ++j) { v0[j] = o[j]; v1[j] = o[8 + j]; }
    *(half8*)dst = v0;
    *(half8*)(dst + 8) = v1;
  } else {
    for (int j = 0; j < n; ++j) dst[j] = o[j];
  }
}

template <bool VEC, bool TAIL>
void launch(bool uniform, unsigned blocks, hipStream_t st, uint8_t* region, uint64_t N, uint64_t a, uint64_t cnt,
            const float* sc, int kind, uint64_t cols, uint32_t sb_cols) {
  if (uniform)
    hipLaunchKernelGGL((dequant_fp8_kernel<VEC, TAIL, true>), dim3(blocks), dim3(kThreads), 0, st, region, N, a, cnt, sc,
                       kind, cols, sb_cols);
  else
    hipLaunchKernelGGL((dequant_fp8_kernel<VEC, TAIL, false>), dim3(blocks), dim3(kThreads), 0, st, region, N, a, cnt,
                       sc, kind, cols, sb_cols);
}

// elements [a, b) of the next launch over what is left of N (b == N: the tail launch)
inline uint64_t next_end(uint64_t N, uint64_t a) {
  const uint64_t left = N - a;
  if (left <= (uint64_t)kTail) return N;
  return a + left / 2 / kPerThread * kPerThread;      // 2 (b - a) <= N - a
}

}  // namespace

extern "C" int fls_dequant_fp8_tail(void) { return kTail; }

// launches fls_dequant_fp8 enqueues for a tensor of n weights
extern "C" int fls_dequant_fp8_launches(uint64_t n) {
  int c = 0;
  for (uint64_t a = 0; a < n; a = next_end(n, a)) ++c;
  return c;
}

extern "C" int fls_dequant_fp8(void* region, uint64_t n, const float* scale, int kind, uint64_t cols, fls_stream_t s) {
  if (n == 0) return 0;
  if (!region || !scale || kind < 0 || kind > 2) return (int)hipErrorInvalidValue;
  if (((uintptr_t)region & 1) || ((uintptr_t)scale & 3)) return (int)hipErrorInvalidValue;
  if (kind != 0 && (cols == 0 || n % cols || cols > 0xFFFFFFFFull)) return (int)hipErrorInvalidValue;
  if (kind == 0) cols = n;
  const uint32_t sb_cols = (uint32_t)((cols + 127) / 128);
  const bool vec = (((uintptr_t)region & 15) == 0) && n % kPerThread == 0;
  const bool uniform = kind == 0 || cols % kPerThread == 0;
  auto st = (hipStream_t)s;
  auto* r = (uint8_t*)region;
  uint64_t a = 0;
  while (a < n) {
    const uint64_t b = next_end(n, a), cnt = b - a;
    const uint64_t blocks = ((cnt + kPerThread - 1) / kPerThread + kThreads - 1) / kThreads;
    if (blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    if (b == n) {      // cnt <= kTail: one block
      if (vec) launch<true, true>(uniform, 1u, st, r, n, a, cnt, scale, kind, cols, sb_cols);
      else launch<false, true>(uniform, 1u, st, r, n, a, cnt, scale, kind, cols, sb_cols);
    } else {
      if (vec) launch<true, false>(uniform, (unsigned)blocks, st, r, n, a, cnt, scale, kind, cols, sb_cols);
      else launch<false, false>(uniform, (unsigned)blocks, st, r, n, a, cnt, scale, kind, cols, sb_cols);
    }
    FLS_CHECK_LAUNCH();
    a = b;
  }
  return 0;
}
