// GPTQ / AWQ 4-bit checkpoints: the transposing repack inside the HBM weight slot (gfx950).
// flexible_llm_sharding_amd/gptq.py holds the two file layouts, the value and input_layout().
//
// Both libraries store a projection weight W[out, in] "input-major":
//
//   GPTQ  qweight I32 [in / 8, out]   nibble i of word [r, o] is u[o, 8r + i]
//   AWQ   qweight I32 [in, out / 8]   nibble i of word [k, c] is u[8c + P[i], k],  P = 0 2 4 6 1 3 5 7
//   both  scales  F16 [in / g, out],  qzeros I32 [in / g, out / 8] (nibbles along `out`, AWQ's in P order)
//
// while the in-place expansion chain (dequant.hip, fls_dequant_w4z) wants what INT4 has: the nibbles
// row-major [out, in], element c of a row in bits 4 (c % 8) of word c / 8, and one entry per group in
// the order o * (in / g) + j, both cut into the segments of the landing layout (quant.segments with
// 4-byte entries) and stacked down from the top of the tensor's 2N-byte region.  The three file
// tensors land as they are at the BOTTOM of that region (qweight at 0, then scales, then qzeros;
// about 0.52 N bytes), the segments occupy about 0.53 .. 0.63 N bytes at the top, and the host checks
// that the two do not meet.  So one launch reads only the bottom and writes only the top: no block
// can overwrite what another has yet to read, and the kernel needs no memory beyond the region.
//
// Work split.  The output is two transposed matrices of 32-bit items:
//   words    Wt[o, r],  r < in / 8   (one word = 8 consecutive inputs of output row o)
//   entries  E[o, j],   j < in / g   (fp16 scale in the low half, the zero point 0..15 in the high half)
// A block of 256 threads owns one 64 x 64 tile of one of them; blockIdx.x counts the word tiles
// first, then the entry tiles, and within each the `out` axis runs fastest, so blocks that are
// resident together read neighbouring columns of the same input rows (AWQ and the entry tiles read
// 32-byte runs per row: their neighbours along `out` take the rest of the cache line from L2).
//
// Phase 1, global -> LDS, coalesced along `out`:
//   GPTQ words   lane (t / 16, t % 16) loads 16 bytes = words [r, o .. o + 3]: a wave reads four whole
//                256-byte tile rows per instruction, four passes cover the 64 rows; tile[r][o] = word.
//   AWQ words    lane (t / 8, t % 8) loads the eight words [8r .. 8r + 7, c] and transposes the 8 x 8
//                nibble matrix in registers by three rounds of masked exchanges between register
//                pairs (4-, 8- and 16-bit granularity: 12 exchanges, no per-nibble loop); word n then
//                holds inputs 8r .. 8r + 7 of output row 8c + P[n]:  tile[r][8c + P[n]] = word n.
//   entries      lane (t / 8, t % 8) loads 16 bytes of scales [j, o .. o + 7] and the one qzeros word
//                [j, o / 8], and writes tile[j][o + i] = scale_i | z_i << 16 with the zero point already
//                final: GPTQ's stored zs becomes (zs + 1) & 15, AWQ's comes from nibble Pinv[i].
// Phase 2, LDS -> global, coalesced along `in`: lane (t % 16, t / 16) reads tile[4q .. 4q + 3][c] down a
// column and stores them as 16 bytes (entries: four 4-byte stores, a row of entries has any length
// and its groups may end in different segments): 16 lanes write 256 consecutive bytes of one output
// row, four passes cover the 64 columns.
//
// LDS.  tile[64][65] dwords.  With the odd row stride, element (r, c) lies in bank (r + c) mod the
// bank count.  Every phase-1 store instruction and every phase-2 load instruction touches, over the
// 64 lanes of a wave, 64 addresses whose r + c takes 64 consecutive values (4 rows x 16 columns 4
// apart, 8 rows x 8 columns 8 apart, or 16 rows 4 apart x 4 columns): the lanes spread evenly over
// the banks, which is the least a 64-lane access can cost.
//
// Segments.  The landing layout has at most kMaxSeg segments for any tensor that fits a GPU (16
// segments hold 8192 * 3.2^15 weights); the table is a kernel argument.  Every segment boundary is a
// multiple of 32 elements and a lane's 4-word unit starts at element 8 (o in/8 + r) with r % 4 == 0 and
// in % 32 == 0, so a 16-byte store never straddles a segment.  Tiles at the edges are predicated
// with the same conditions in both phases (out % 8 == 0, in % 32 == 0), so no lane reads a tile
// element that was not written.
//
// A region base that is not 16-byte aligned (it is always 2-byte aligned) takes the same schedule
// with 2-byte loads and stores.  Plain C++ and vector memory instructions only.
#include "common.h"
#include "fls.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;
constexpr int kStride = kTile + 1;
constexpr int kMaxSeg = 16;
constexpr int kGptq = 0, kAwq = 1;

// the landing layout in launch order (ascending elements).  Element e of segment j has its packed
// byte at e / 2 + p_delta[j]; group k, whose entry segment j holds, has it at 4 k + s_delta[j].
struct SegTable {
  int n;
  uint64_t a[kMaxSeg];         // first element of the segment
  int64_t p_delta[kMaxSeg];    // packed offset - a / 2
  uint64_t k0[kMaxSeg];        // first group whose entry the segment holds
  int64_t s_delta[kMaxSeg];    // entry offset - 4 k0
};

template <bool VEC>
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) {
  if (VEC) return *(const uint32_t*)p;
  return (uint32_t)*(const uint16_t*)p | ((uint32_t)*(const uint16_t*)(p + 2) << 16);
}

template <bool VEC>
__device__ __forceinline__ uint4 ld128(const uint8_t* p) {
  if (VEC) return *(const uint4*)p;
  return make_uint4(ld32<false>(p), ld32<false>(p + 4), ld32<false>(p + 8), ld32<false>(p + 12));
}

template <bool VEC>
__device__ __forceinline__ void st32(uint8_t* p, uint32_t v) {
  if (VEC) {
    *(uint32_t*)p = v;
  } else {
    *(uint16_t*)p = (uint16_t)v;
    *(uint16_t*)(p + 2) = (uint16_t)(v >> 16);
  }
}

template <bool VEC>
__device__ __forceinline__ void st128(uint8_t* p, const uint32_t (&v)[4]) {
  if (VEC) {
    *(uint4*)p = make_uint4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) st32<false>(p + 4 * i, v[i]);
  }
}

// AWQ's nibble order: nibble i of a word holds column 8c + awq_col(i); column 8c + m sits in nibble
// awq_nibble(m)
__device__ __forceinline__ constexpr int awq_col(int i) { return i < 4 ? 2 * i : 2 * (i - 4) + 1; }
__device__ __forceinline__ constexpr int awq_nibble(int m) { return (m & 1) * 4 + (m >> 1); }

// exchange the bits `mask << shift` of x with the bits `mask` of y
__device__ __forceinline__ void exchange(uint32_t& x, uint32_t& y, int shift, uint32_t mask) {
  const uint32_t d = ((x >> shift) ^ y) & mask;
  y ^= d;
  x ^= d << shift;
}

// w[i] nibble n  <->  w[n] nibble i: 2 x 2 blocks of nibbles, then of bytes, then of half words
__device__ __forceinline__ void transpose_nibbles(uint32_t (&w)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i += 2) exchange(w[i], w[i + 1], 4, 0x0F0F0F0Fu);
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if ((i & 2) == 0) exchange(w[i], w[i + 2], 8, 0x00FF00FFu);
#pragma unroll
  for (int i = 0; i < 4; ++i) exchange(w[i], w[i + 4], 16, 0x0000FFFFu);
}

// region: the tensor's 2 * out * 8R-byte region with qweight at 0, scales at sc_off, qzeros at z_off.
// R = in / 8 word rows, G = in / g groups per row.  Blocks [0, word_blocks) own word tiles, the rest
// entry tiles; tile index = tile_row * tiles_o + tile_o.
template <bool VEC, int LAYOUT>
__global__ __launch_bounds__(kThreads) void repack_w4_kernel(uint8_t* region, uint32_t out, uint32_t R, uint32_t G,
                                                             uint64_t sc_off, uint64_t z_off, uint32_t tiles_o,
                                                             uint32_t word_blocks, SegTable tab) {
  __shared__ uint32_t tile[kTile * kStride];
  const uint32_t t = threadIdx.x;
  const bool words = blockIdx.x < word_blocks;                 // (uniform over the block)
  const uint32_t bid = words ? blockIdx.x : blockIdx.x - word_blocks;
  const uint32_t o0 = (bid % tiles_o) * kTile, r0 = (bid / tiles_o) * kTile;
  const uint32_t rows = words ? R : G;
  const uint32_t out8 = out >> 3;

  // ---- phase 1: global -> tile[row][column]
  if (words && LAYOUT == kGptq) {
    const uint32_t lc = (t & 15u) * 4u, o = o0 + lc;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const uint32_t lr = (t >> 4) + 16u * p, r = r0 + lr;
      if (r < R && o < out) {                                   // (out % 4 == 0: o + 3 < out)
        const uint4 v = ld128<VEC>(region + ((uint64_t)r * out + o) * 4);
        uint32_t* d = tile + lr * kStride + lc;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
      }
    }
  } else {
    const uint32_t c = t & 7u, o = o0 + 8u * c;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const uint32_t lr = (t >> 3) + 32u * p, r = r0 + lr;
      if (r < rows && o < out) {                                // (out % 8 == 0: o + 7 < out)
        uint32_t* d = tile + lr * kStride + 8u * c;
        if (words) {
          uint32_t w[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) w[i] = ld32<VEC>(region + (((uint64_t)8 * r + i) * out8 + (o >> 3)) * 4);
          transpose_nibbles(w);
#pragma unroll
          for (int i = 0; i < 8; ++i) d[awq_col(i)] = w[i];
        } else {
          const uint4 s = ld128<VEC>(region + sc_off + ((uint64_t)r * out + o) * 2);
          const uint32_t zw = ld32<VEC>(region + z_off + ((uint64_t)r * out8 + (o >> 3)) * 4);
          const uint32_t sw[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const uint32_t sbits = (sw[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
            uint32_t z = (zw >> (4 * (LAYOUT == kAwq ? awq_nibble(i) : i))) & 15u;
            if (LAYOUT == kGptq) z = (z + 1u) & 15u;
            d[i] = sbits | (z << 16);
          }
        }
      }
    }
  }
  __syncthreads();

  // ---- phase 2: tile[4q .. 4q + 3][column] -> four consecutive items of output row o
  const uint32_t lq = (t & 15u) * 4u, r = r0 + lq;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const uint32_t lc = (t >> 4) + 16u * p, o = o0 + lc;
    if (o >= out || r >= rows) continue;
    uint32_t v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = tile[(lq + i) * kStride + lc];
    if (words) {                                                // (R % 4 == 0: r + 3 < R)
      const uint64_t e = 8 * ((uint64_t)o * R + r);
      int64_t delta = tab.p_delta[0];
      for (int j = 1; j < tab.n; ++j)
        if (e >= tab.a[j]) delta = tab.p_delta[j];
      st128<VEC>(region + (int64_t)(e >> 1) + delta, v);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (r + i >= G) break;
        const uint64_t k = (uint64_t)o * G + r + i;
        int64_t delta = tab.s_delta[0];
        for (int j = 1; j < tab.n; ++j)
          if (k >= tab.k0[j]) delta = tab.s_delta[j];
        st32<VEC>(region + (int64_t)(4 * k) + delta, v[i]);
      }
    }
  }
}

inline bool repack_args_ok(uint64_t out, uint64_t in, uint64_t group, int layout) {
  return (layout == kGptq || layout == kAwq) && out % 8 == 0 && in % 32 == 0 && group != 0 && group % 32 == 0 &&
         in % group == 0 && out <= 0x7FFFFFFFull && in <= 0x7FFFFFFFull;
}

}  // namespace

// where the three file tensors of an [out, in] weight in groups of `group` land in its region (gptq.py,
// input_layout): o[4] = {qweight offset, scales offset, qzeros offset, end}.  0, or -1 for bad arguments
extern "C" int fls_repack_w4_input(uint64_t out, uint64_t in, uint64_t group, uint64_t* o) {
  if (!o || !repack_args_ok(out, in, group, kGptq)) return -1;
  const uint64_t n = out * in, G = in / group;
  o[0] = 0;
  o[1] = (n / 2 + 15) & ~(uint64_t)15;
  o[2] = (o[1] + G * out * 2 + 15) & ~(uint64_t)15;
  o[3] = o[2] + G * (out / 8) * 4;
  return 0;
}

extern "C" int fls_repack_w4(void* region, uint64_t out, uint64_t in, uint64_t group, int layout, fls_stream_t s) {
  if (out == 0 || in == 0) return 0;
  if (!region || ((uintptr_t)region & 1) || !repack_args_ok(out, in, group, layout)) return (int)hipErrorInvalidValue;
  const uint64_t n = out * in, R = in / 8, G = in / group;
  uint64_t land[4];
  if (fls_repack_w4_input(out, in, group, land) != 0) return (int)hipErrorInvalidValue;
  const int c = fls_dequant_w4z_launches(n, group);
  if (c <= 0 || c > kMaxSeg) return (int)hipErrorInvalidValue;
  SegTable tab;
  tab.n = c;
  for (int j = 0; j < kMaxSeg; ++j) {
    uint64_t sg[6] = {0, 0, 0, 0, 0, 0};
    if (j < c && fls_dequant_w4z_segment(n, group, j, sg) != 0) return (int)hipErrorInvalidValue;
    tab.a[j] = sg[0];
    tab.p_delta[j] = (int64_t)sg[2] - (int64_t)(sg[0] / 2);
    tab.k0[j] = sg[4];
    tab.s_delta[j] = (int64_t)sg[3] - (int64_t)(4 * sg[4]);
    if (j == 0 && land[3] > sg[3]) return (int)hipErrorInvalidValue;      // the input must end below the output
  }
  const uint64_t tiles_o = (out + kTile - 1) / kTile;
  const uint64_t word_blocks = tiles_o * ((R + kTile - 1) / kTile);
  const uint64_t blocks = word_blocks + tiles_o * ((G + kTile - 1) / kTile);
  if (blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
  const bool vec = ((uintptr_t)region & 15) == 0;
  auto st = (hipStream_t)s;
  auto* r = (uint8_t*)region;
#define FLS_REPACK_LAUNCH(VEC, LAYOUT)                                                                              \
  hipLaunchKernelGGL((repack_w4_kernel<VEC, LAYOUT>), dim3((unsigned)blocks), dim3(kThreads), 0, st, r, (uint32_t)out, \
                     (uint32_t)R, (uint32_t)G, land[1], land[2], (uint32_t)tiles_o, (uint32_t)word_blocks, tab)
  if (layout == kGptq) {
    if (vec) FLS_REPACK_LAUNCH(true, kGptq);
    else FLS_REPACK_LAUNCH(false, kGptq);
  } else {
    if (vec) FLS_REPACK_LAUNCH(true, kAwq);
    else FLS_REPACK_LAUNCH(false, kAwq);
  }
#undef FLS_REPACK_LAUNCH
  FLS_CHECK_LAUNCH();
  return 0;
}
