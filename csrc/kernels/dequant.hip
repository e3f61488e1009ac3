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

// ---------------------------------------------------------------------------------------------
// Weight-only INT4 (W4A16, symmetric, group scales) expansion in place (flexible_llm_sharding_amd/int4.py
// holds the definition and, in region_layout(), the landing layout this file mirrors).
//
//   w16[i] = fp16_rne( fp32(nibble(i) - 8) * fp32(scale[i / g]) )
//
// The inputs of a tensor of N weights land in its own 2N-byte region segment by segment, one segment
// per launch, stacked downwards from the top of the region in reverse launch order:
//
//   [ ... free ... | scales_0 | packed_0 | scales_1 | packed_1 | ... | scales_tail | packed_tail ]
//
// Launch j expands elements [a_j, b_j) and writes bytes [2 a_j, 2 b_j); 2 b_j <= offset(scales_j), so
// it touches nothing unread.  scales_j holds the groups that END in [a_j, b_j); the group that
// straddles b_j is read from the next segment that holds scales, which lies above.  The tail (at
// most kTail4 weights) is one block that reads its nibbles and scales into registers, barriers, and
// writes.  Segments are sized from the top, each as large as the rule allows: the part that is left
// shrinks by 1 / (1/4 + es / 2g) per launch (10 launches for 8192 x 28672 at g = 32 with fp32 scales).
//
// Each thread expands 32 weights of one group (g % 32 == 0): one 16-byte load of nibbles, its one
// scale, nibble - 8 -> fp32, a plain fp32 multiply, v_cvt_f16_f32, four 16-byte stores.  A region
// base that is not 16-byte aligned takes the same schedule with scalar loads and stores.
namespace {

constexpr int kPer4 = 32;
constexpr int kTail4 = kPer4 * kThreads;

struct Seg4 {
  uint64_t a, b, p_off, s_off, k0, ng;
};

// scale k of a segment whose scales start at byte `off` of the region; dt 0 fp16, 1 bf16, 2 fp32.
// 2-byte loads only when the region base is not 16-byte aligned (an fp32 scale may then sit at an
// address that is no multiple of 4).
template <bool VEC>
__device__ __forceinline__ float load_scale(const uint8_t* region, uint64_t off, uint64_t idx, int dt) {
  if (dt == 2) {
    const uint8_t* p = region + off + idx * 4;
    if (VEC) return *(const float*)p;
    const uint32_t lo = *(const uint16_t*)p, hi = *(const uint16_t*)(p + 2);
    return __uint_as_float(lo | (hi << 16));
  }
  const uint16_t h = *(const uint16_t*)(region + off + idx * 2);
  if (dt == 1) return __uint_as_float((uint32_t)h << 16);
  return (float)__builtin_bit_cast(half_t, h);
}

// this launch expands elements [a, a + cnt), cnt % 32 == 0; their nibbles start at byte p_off.  Groups
// [k0, k_next) have their scales at s_off; group k_next (the one that straddles a + cnt) at s_next.
// TAIL: one block, cnt <= kTail4, every read completes before any write (the ranges overlap).
template <bool VEC, bool TAIL>
__global__ __launch_bounds__(kThreads) void dequant_int4_kernel(uint8_t* region, uint64_t a, uint64_t cnt,
                                                                uint64_t p_off, uint64_t s_off, uint64_t k0,
                                                                uint64_t k_next, uint64_t s_next, uint64_t g,
                                                                int dt) {
  const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const uint64_t off = t * kPer4;
  const bool active = off < cnt;
  if (!TAIL && !active) return;
  half_t o[kPer4];
  if (active) {
    uint32_t w[4];
    const uint8_t* src = region + p_off + off / 2;
    if (VEC) {
      const uint4 v = *(const uint4*)src;
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        w[j] = (uint32_t)src[4 * j] | ((uint32_t)src[4 * j + 1] << 8) | ((uint32_t)src[4 * j + 2] << 16) |
               ((uint32_t)src[4 * j + 3] << 24);
    }
    const uint64_t k = (a + off) / g;
    const float s = k < k_next ? load_scale<VEC>(region, s_off, k - k0, dt) : load_scale<VEC>(region, s_next, 0, dt);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const int q = (int)((w[j] >> (4 * b)) & 15u) - 8;
        o[8 * j + b] = to_half((float)q * s);
      }
  }
  if (TAIL) __syncthreads();
  if (!active) return;
  half_t* dst = (half_t*)region + a + off;
  if (VEC) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      half8 v;
#pragma unroll
      for (int b = 0; b < 8; ++b) v[b] = o[8 * j + b];
      *(half8*)(dst + 8 * j) = v;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kPer4; ++j) dst[j] = o[j];
  }
}

// int4.region_layout(): the segments from the top of the region down, i.e. in REVERSE launch order.
// Returns the count (0 for bad arguments: more than kMaxSeg4 cannot happen below 2^63 weights).
constexpr int kMaxSeg4 = 64;
inline int layout4(uint64_t n, uint64_t g, uint64_t es, Seg4* out) {
  int c = 0;
  uint64_t top = 2 * n, b = n, a = n <= (uint64_t)kTail4 ? 0 : n - kTail4;
  while (true) {
    if (c == kMaxSeg4) return 0;
    const uint64_t k0 = a / g, k1 = b / g;
    const uint64_t p_off = top - (b - a) / 2;
    const uint64_t s_off = (p_off - (k1 - k0) * es) & ~(uint64_t)15;
    out[c++] = Seg4{a, b, p_off, s_off, k0, k1 - k0};
    if (a == 0) break;
    top = s_off;
    b = a;
    // cnt / 2 nibble bytes, at most cnt / g + 1 scales and 15 bytes of alignment fit above the front 2b
    const uint64_t avail = top - 2 * b;
    if (avail <= es + 15) return 0;
    const uint64_t cnt = (avail - es - 15) * 2 * g / (g + 2 * es) / kPer4 * kPer4;
    if (cnt == 0) return 0;
    a = cnt >= b ? 0 : b - cnt;
  }
  return c;
}

inline bool args4_ok(uint64_t n, uint64_t group, int es) {
  return group != 0 && group % 32 == 0 && n % group == 0 && (es == 2 || es == 4) && n < (1ull << 60);
}

}  // namespace

extern "C" int fls_dequant_int4_tail(void) { return kTail4; }

// launches fls_dequant_int4 enqueues for a tensor of n weights in groups of `group` with scales of
// scale_es bytes (-1: bad arguments)
extern "C" int fls_dequant_int4_launches(uint64_t n, uint64_t group, int scale_es) {
  if (!args4_ok(n, group, scale_es)) return -1;
  if (n == 0) return 0;
  Seg4 segs[kMaxSeg4];
  const int c = layout4(n, group, (uint64_t)scale_es, segs);
  return c > 0 ? c : -1;
}

// launch j (0 .. launches - 1) of that chain, for tests of the mirror: out = {a, b, packed offset,
// scale offset, first group, groups}.  0, or -1 for bad arguments or j
extern "C" int fls_dequant_int4_segment(uint64_t n, uint64_t group, int scale_es, int j, uint64_t* out) {
  if (!out || n == 0 || !args4_ok(n, group, scale_es)) return -1;
  Seg4 segs[kMaxSeg4];
  const int c = layout4(n, group, (uint64_t)scale_es, segs);
  if (c <= 0 || j < 0 || j >= c) return -1;
  const Seg4& s = segs[c - 1 - j];
  out[0] = s.a; out[1] = s.b; out[2] = s.p_off; out[3] = s.s_off; out[4] = s.k0; out[5] = s.ng;
  return 0;
}

extern "C" int fls_dequant_int4(void* region, uint64_t n, uint64_t group, int scale_dtype, fls_stream_t s) {
  if (n == 0) return 0;
  if (!region || ((uintptr_t)region & 1)) return (int)hipErrorInvalidValue;
  if (scale_dtype < 0 || scale_dtype > 2) return (int)hipErrorInvalidValue;
  const int es = scale_dtype == 2 ? 4 : 2;
  if (!args4_ok(n, group, es)) return (int)hipErrorInvalidValue;
  Seg4 segs[kMaxSeg4];
  const int c = layout4(n, group, (uint64_t)es, segs);
  if (c <= 0) return (int)hipErrorInvalidValue;
  const bool vec = ((uintptr_t)region & 15) == 0;
  auto st = (hipStream_t)s;
  auto* r = (uint8_t*)region;
  for (int j = c - 1; j >= 0; --j) {      // launch order: from the bottom segment to the tail
    const Seg4& g4 = segs[j];
    // the straddling group g4.b / group: the first scale of the next segment (towards the tail) that has any
    uint64_t s_next = 0;
    for (int i = j - 1; i >= 0; --i)
      if (segs[i].ng) { s_next = segs[i].s_off; break; }
    const uint64_t cnt = g4.b - g4.a, k_next = g4.k0 + g4.ng;
    const uint64_t blocks = (cnt / kPer4 + kThreads - 1) / kThreads;
    if (blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    if (j == 0) {      // cnt <= kTail4: one block
      if (vec)
        hipLaunchKernelGGL((dequant_int4_kernel<true, true>), dim3(1), dim3(kThreads), 0, st, r, g4.a, cnt, g4.p_off,
                           g4.s_off, g4.k0, k_next, s_next, group, scale_dtype);
      else
        hipLaunchKernelGGL((dequant_int4_kernel<false, true>), dim3(1), dim3(kThreads), 0, st, r, g4.a, cnt, g4.p_off,
                           g4.s_off, g4.k0, k_next, s_next, group, scale_dtype);
    } else {
      if (vec)
        hipLaunchKernelGGL((dequant_int4_kernel<true, false>), dim3((unsigned)blocks), dim3(kThreads), 0, st, r, g4.a,
                           cnt, g4.p_off, g4.s_off, g4.k0, k_next, s_next, group, scale_dtype);
      else
        hipLaunchKernelGGL((dequant_int4_kernel<false, false>), dim3((unsigned)blocks), dim3(kThreads), 0, st, r, g4.a,
                           cnt, g4.p_off, g4.s_off, g4.k0, k_next, s_next, group, scale_dtype);
    }
    FLS_CHECK_LAUNCH();
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------
// bitsandbytes 4-bit (NF4 / FP4) expansion in place (flexible_llm_sharding_amd/nf4.py holds the
// definition; the landing layout is INT4's above with blocks for groups and raw absmax entries of 1
// (U8, double quantisation) or 4 (fp32) bytes for scales).
//
//   w16[i] = fp16_rne( code[nibble(i)] * s_k ),  k = i / block
//   s_k    = absmax[k]                                             (fp32 absmax)
//   s_k    = code2[absmax_u8[k]] * nested_absmax[k / B2] + offset    (U8 absmax; multiply, round, add, round)
//
// Byte j of the packed stream holds element 2j in its HIGH nibble.  Each thread expands 32 weights of
// one block (block % 32 == 0): one 16-byte load, its block's s_k once, 32 lookups in the 16-entry code
// book, 32 plain fp32 multiplies, v_cvt_f16_f32, four 16-byte stores.  The code book sits in LDS:
// its 16 dwords lie in 16 different banks and lanes that read the same entry are served by one
// broadcast, so a ds_read_b32 with any mix of nibbles is conflict-free.  code2 (1 KB), nested_absmax
// and the code book's source live in the table arena of the weight source and are only read.
namespace {

constexpr int kAbsmaxF32 = 0, kAbsmaxU8 = 1;

// fp32 multiply, then fp32 add, each rounded: the product passes through an opaque register so that
// -ffp-contract=fast cannot fuse the two into an FMA
__device__ __forceinline__ float mul_then_add(float x, float y, float z) {
  float p = x * y;
  asm volatile("" : "+v"(p));
  return p + z;
}

// s_k of block k whose raw absmax entry is entry idx of the entries at byte `off` of the region
template <bool VEC, int KIND>
__device__ __forceinline__ float block_scale(const uint8_t* region, uint64_t off, uint64_t idx, uint64_t k,
                                             const float* __restrict__ code2, const float* __restrict__ nested,
                                             uint64_t nested_block, float offset) {
  if (KIND == kAbsmaxF32) return load_scale<VEC>(region, off, idx, 2);
  const uint8_t q = region[off + idx];
  return mul_then_add(code2[q], nested[k / nested_block], offset);
}

// this launch expands elements [a, a + cnt), cnt % 32 == 0; their packed bytes start at byte p_off.
// Blocks [k0, k_next) have their absmax entries at s_off; block k_next (the one that straddles
// a + cnt) at s_next.  TAIL: one block, cnt <= kTail4, every read completes before any write.
template <bool VEC, bool TAIL, int KIND>
__global__ __launch_bounds__(kThreads) void dequant_nf4_kernel(uint8_t* region, uint64_t a, uint64_t cnt,
                                                               uint64_t p_off, uint64_t s_off, uint64_t k0,
                                                               uint64_t k_next, uint64_t s_next, uint64_t block,
                                                               const float* __restrict__ code,
                                                               const float* __restrict__ code2,
                                                               const float* __restrict__ nested,
                                                               uint64_t nested_block, float offset) {
  __shared__ float lut[16];
  if (threadIdx.x < 16) lut[threadIdx.x] = code[threadIdx.x];
  __syncthreads();
  const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const uint64_t off = t * kPer4;
  const bool active = off < cnt;
  if (!TAIL && !active) return;
  half_t o[kPer4];
  if (active) {
    uint32_t w[4];
    const uint8_t* src = region + p_off + off / 2;
    if (VEC) {
      const uint4 v = *(const uint4*)src;
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        w[j] = (uint32_t)src[4 * j] | ((uint32_t)src[4 * j + 1] << 8) | ((uint32_t)src[4 * j + 2] << 16) |
               ((uint32_t)src[4 * j + 3] << 24);
    }
    const uint64_t k = (a + off) / block;
    const float s = k < k_next ? block_scale<VEC, KIND>(region, s_off, k - k0, k, code2, nested, nested_block, offset)
                               : block_scale<VEC, KIND>(region, s_next, 0, k, code2, nested, nested_block, offset);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        // element b of word j: byte b / 2, an even b in the high nibble
        const uint32_t u = (w[j] >> (4 * (b ^ 1))) & 15u;
        o[8 * j + b] = to_half(lut[u] * s);
      }
  }
  if (TAIL) __syncthreads();
  if (!active) return;
  half_t* dst = (half_t*)region + a + off;
  if (VEC) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      half8 v;
#pragma unroll
      for (int b = 0; b < 8; ++b) v[b] = o[8 * j + b];
      *(half8*)(dst + 8 * j) = v;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kPer4; ++j) dst[j] = o[j];
  }
}

inline bool argsn4_ok(uint64_t n, uint64_t block, int es) {
  return block != 0 && block % 32 == 0 && n % block == 0 && (es == 1 || es == 4) && n < (1ull << 60);
}

template <bool VEC, bool TAIL>
void launch_nf4(int kind, unsigned blocks, hipStream_t st, uint8_t* r, const Seg4& g, uint64_t s_next, uint64_t block,
                const float* code, const float* code2, const float* nested, uint64_t nested_block, float offset) {
  const uint64_t cnt = g.b - g.a, k_next = g.k0 + g.ng;
  if (kind == kAbsmaxU8)
    hipLaunchKernelGGL((dequant_nf4_kernel<VEC, TAIL, kAbsmaxU8>), dim3(blocks), dim3(kThreads), 0, st, r, g.a, cnt,
                       g.p_off, g.s_off, g.k0, k_next, s_next, block, code, code2, nested, nested_block, offset);
  else
    hipLaunchKernelGGL((dequant_nf4_kernel<VEC, TAIL, kAbsmaxF32>), dim3(blocks), dim3(kThreads), 0, st, r, g.a, cnt,
                       g.p_off, g.s_off, g.k0, k_next, s_next, block, code, code2, nested, nested_block, offset);
}

}  // namespace

extern "C" int fls_dequant_nf4_tail(void) { return kTail4; }

// launches fls_dequant_nf4 enqueues for a tensor of n weights in blocks of `block` with absmax
// entries of absmax_es bytes (-1: bad arguments)
extern "C" int fls_dequant_nf4_launches(uint64_t n, uint64_t block, int absmax_es) {
  if (!argsn4_ok(n, block, absmax_es)) return -1;
  if (n == 0) return 0;
  Seg4 segs[kMaxSeg4];
  const int c = layout4(n, block, (uint64_t)absmax_es, segs);
  return c > 0 ? c : -1;
}

// launch j (0 .. launches - 1) of that chain, for tests of the mirror: out = {a, b, packed offset,
// absmax offset, first block, blocks}.  0, or -1 for bad arguments or j
extern "C" int fls_dequant_nf4_segment(uint64_t n, uint64_t block, int absmax_es, int j, uint64_t* out) {
  if (!out || n == 0 || !argsn4_ok(n, block, absmax_es)) return -1;
  Seg4 segs[kMaxSeg4];
  const int c = layout4(n, block, (uint64_t)absmax_es, segs);
  if (c <= 0 || j < 0 || j >= c) return -1;
  const Seg4& s = segs[c - 1 - j];
  out[0] = s.a; out[1] = s.b; out[2] = s.p_off; out[3] = s.s_off; out[4] = s.k0; out[5] = s.ng;
  return 0;
}

extern "C" int fls_dequant_nf4(void* region, uint64_t n, uint64_t block, int absmax_kind, const float* code,
                               const float* code2, const float* nested_absmax, uint64_t nested_block, float offset,
                               fls_stream_t s) {
  if (n == 0) return 0;
  if (!region || ((uintptr_t)region & 1) || !code || ((uintptr_t)code & 3)) return (int)hipErrorInvalidValue;
  if (absmax_kind != kAbsmaxF32 && absmax_kind != kAbsmaxU8) return (int)hipErrorInvalidValue;
  if (absmax_kind == kAbsmaxU8 && (!code2 || !nested_absmax || nested_block == 0 || ((uintptr_t)code2 & 3) ||
                                   ((uintptr_t)nested_absmax & 3)))
    return (int)hipErrorInvalidValue;
  const int es = absmax_kind == kAbsmaxU8 ? 1 : 4;
  if (!argsn4_ok(n, block, es)) return (int)hipErrorInvalidValue;
  Seg4 segs[kMaxSeg4];
  const int c = layout4(n, block, (uint64_t)es, segs);
  if (c <= 0) return (int)hipErrorInvalidValue;
  const bool vec = ((uintptr_t)region & 15) == 0;
  auto st = (hipStream_t)s;
  auto* r = (uint8_t*)region;
  for (int j = c - 1; j >= 0; --j) {      // launch order: from the bottom segment to the tail
    const Seg4& g4 = segs[j];
    // the straddling block g4.b / block: the first entry of the next segment (towards the tail) that has any
    uint64_t s_next = 0;
    for (int i = j - 1; i >= 0; --i)
      if (segs[i].ng) { s_next = segs[i].s_off; break; }
    const uint64_t blocks = ((g4.b - g4.a) / kPer4 + kThreads - 1) / kThreads;
    if (blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    if (j == 0) {      // at most kTail4 weights: one block
      if (vec) launch_nf4<true, true>(absmax_kind, 1u, st, r, g4, s_next, block, code, code2, nested_absmax, nested_block, offset);
      else launch_nf4<false, true>(absmax_kind, 1u, st, r, g4, s_next, block, code, code2, nested_absmax, nested_block, offset);
    } else {
      if (vec) launch_nf4<true, false>(absmax_kind, (unsigned)blocks, st, r, g4, s_next, block, code, code2, nested_absmax, nested_block, offset);
      else launch_nf4<false, false>(absmax_kind, (unsigned)blocks, st, r, g4, s_next, block, code, code2, nested_absmax, nested_block, offset);
    }
    FLS_CHECK_LAUNCH();
  }
  return 0;
}
