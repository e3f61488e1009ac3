// Sampled next token of each row of fp16 probabilities: temperature, top-k and top-p, integer-exact
// (flexible_llm_sharding_amd/sampling.py holds the definition and the host sampler that returns the
// same token for every input).
//
// A probability is an fp16 bit pattern b in 1..0x3C00 (0 < p <= 1); table[b] is its uint32 weight
// (round(2^30 p^(1/T)), non-decreasing in b).  Tokens are ranked by (b descending, index
// ascending); bit patterns outside 1..0x3C00 (zero, negative, NaN, > 1) are never chosen.
//   S_k = weight sum of the first top_k ranked tokens (top_k = 0: all)
//   tau = max(1, ceil(S_k P / 65536)); S = weight sum of the shortest ranked prefix reaching tau
//   u   = (draw * S) >> 64; the token is the first ranked one whose inclusive weight sum exceeds u
// One 256-thread block per row:
//   pass 1  histogram of the row's bit patterns in LDS (15,361 uint32 bins; same-address LDS
//           atomics serialise, which is why zeros are skipped: most of a real row is zero)
//   scan    thread t owns the 61 bins from 0x3C00 - 61 t downwards; a block prefix over the
//           threads' (count, weight sum) gives every thread its rank and weight offsets, and the
//           one thread whose bins hold a threshold walks them: S_k, then S, then the bin of u and
//           the rank r = (u - offset) / W of the token inside that bin
//   pass 2  the r-th occurrence of that bit pattern in index order: each wave counts the matches of
//           its contiguous quarter of the row; the wave whose quarter holds the r-th walks it again,
//           64 lanes at a time, with a lane prefix over the match counts
// No floating-point value is compared or summed: every decision is an integer one.
#include "common.h"
#include "fls.h"

namespace {

constexpr int SAMPLE_BINS = 0x3C01;   // bit patterns 0 .. 0x3C00 (1.0)
constexpr int SAMPLE_CHUNK = 61;      // bins per thread (256 x 61 >= 0x3C00; odd: no LDS bank conflicts)

typedef unsigned short ushort8 __attribute__((ext_vector_type(8)));

template <bool VEC>   // 16-byte loads: V % 8 == 0, ld % 8 == 0 and a 16-byte aligned base
__global__ __launch_bounds__(256) void sample_rows_kernel(const half_t* __restrict__ probs, int ld, int V,
                                                        const uint32_t* __restrict__ table,
                                                        const uint64_t* __restrict__ draws, int top_k, uint32_t P,
                                                        int* __restrict__ out) {
  __shared__ uint32_t hist[SAMPLE_BINS];
  __shared__ uint32_t wave_c[4];
  __shared__ uint64_t wave_s[4];
  __shared__ uint64_t found_s[2];     // S_k, S
  __shared__ uint32_t found_bin[2];   // the chosen bit pattern, the token's rank among its occurrences
  __shared__ uint32_t wave_hits[4];
  const unsigned short* row = (const unsigned short*)(probs + (size_t)blockIdx.x * ld);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < SAMPLE_BINS; i += 256) hist[i] = 0;
  __syncthreads();

  // a unit is what one lane loads at a time (8 columns, or 1); wave w owns units [u0, u1)
  const int units = VEC ? V / 8 : V;
  const int per_wave = (units + 3) / 4;
  const int u0 = min(units, wave * per_wave), u1 = min(units, u0 + per_wave);
  for (int u = u0 + lane; u < u1; u += 64) {
    if (VEC) {
      const ushort8 v = *(const ushort8*)(row + (size_t)u * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t b = v[j];
        if (b - 1u < 0x3C00u) atomicAdd(&hist[b], 1u);
      }
    } else {
      const uint32_t b = row[u];
      if (b - 1u < 0x3C00u) atomicAdd(&hist[b], 1u);
    }
  }
  __syncthreads();

  // this thread's bins, from the top: (count, weight sum), then the exclusive block prefix
  const int top_bin = 0x3C00 - tid * SAMPLE_CHUNK;
  uint32_t c = 0;
  uint64_t s = 0;
  for (int i = 0; i < SAMPLE_CHUNK; ++i) {
    const int b = top_bin - i;
    if (b < 1) break;
    const uint32_t n = hist[b];
    if (n) {
      c += n;
      s += (uint64_t)n * table[b];
    }
  }
  uint32_t ci = c;
  uint64_t si = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t tc = __shfl_up(ci, o, 64);
    const uint64_t ts = __shfl_up((unsigned long long)si, o, 64);
    if (lane >= o) {
      ci += tc;
      si += ts;
    }
  }
  if (lane == 63) {
    wave_c[wave] = ci;
    wave_s[wave] = si;
  }
  __syncthreads();
  uint32_t c_ex = ci - c, n_total = 0;
  uint64_t s_ex = si - s, s_total = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) {
      c_ex += wave_c[w];
      s_ex += wave_s[w];
    }
    n_total += wave_c[w];
    s_total += wave_s[w];
  }

  // top-k: S_k, the weight of the first k ranked tokens
  uint64_t s_k = s_total;
  if (top_k > 0 && (uint32_t)top_k < n_total) {
    const uint32_t k = (uint32_t)top_k;
    if (c_ex < k && k <= c_ex + c) {
      uint32_t rc = c_ex;
      uint64_t rs = s_ex;
      for (int i = 0; i < SAMPLE_CHUNK; ++i) {
        const int b = top_bin - i;
        if (b < 1) break;
        const uint32_t n = hist[b];
        if (!n) continue;
        const uint64_t w = table[b];
        if (rc + n >= k) {
          rs += (uint64_t)(k - rc) * w;
          break;
        }
        rc += n;
        rs += (uint64_t)n * w;
      }
      found_s[0] = rs;
    }
    __syncthreads();
    s_k = found_s[0];
  }
  if (s_k == 0) {   // an all-zero row (or nothing with a weight): token 0, as argmax_rows_kernel
    if (tid == 0) out[blockIdx.x] = 0;
    return;
  }

  // top-p: S, the weight of the shortest ranked prefix whose weight reaches tau (V < 2^18 and
  // W <= 2^30, so S_k P < 2^64)
  uint64_t s_keep = s_k;
  if (P < 65536u) {
    uint64_t tau = (s_k * P + 65535u) >> 16;
    tau = tau ? tau : 1;
    if (s_ex < tau && tau <= s_ex + s) {
      uint64_t rs = s_ex;
      for (int i = 0; i < SAMPLE_CHUNK; ++i) {
        const int b = top_bin - i;
        if (b < 1) break;
        const uint32_t n = hist[b];
        if (!n) continue;
        const uint64_t w = table[b];
        if (!w) continue;
        if (rs + (uint64_t)n * w >= tau) {
          rs += (tau - rs + w - 1) / w * w;
          break;
        }
        rs += (uint64_t)n * w;
      }
      found_s[1] = rs;
    }
    __syncthreads();
    s_keep = found_s[1];
  }

  // the draw: u in [0, S) -> its bin and the rank inside it
  const uint64_t u = __umul64hi(draws[blockIdx.x], s_keep);
  if (s_ex <= u && u < s_ex + s) {
    uint64_t rs = s_ex;
    for (int i = 0; i < SAMPLE_CHUNK; ++i) {
      const int b = top_bin - i;
      if (b < 1) break;
      const uint32_t n = hist[b];
      if (!n) continue;
      const uint64_t w = table[b];
      if (u < rs + (uint64_t)n * w) {
        found_bin[0] = (uint32_t)b;
        found_bin[1] = (uint32_t)((u - rs) / w);
        break;
      }
      rs += (uint64_t)n * w;
    }
  }
  __syncthreads();
  const uint32_t tb = found_bin[0], tr = found_bin[1];

  // pass 2: matches of tb per wave, in index order
  uint32_t hits = 0;
  for (int x = u0 + lane; x < u1; x += 64) {
    if (VEC) {
      const ushort8 v = *(const ushort8*)(row + (size_t)x * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) hits += v[j] == tb;
    } else {
      hits += row[x] == tb;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o, 64);
  if (lane == 0) wave_hits[wave] = hits;
  __syncthreads();
  uint32_t run = 0;
  for (int w = 0; w < wave; ++w) run += wave_hits[w];
  if (tr < run || tr >= run + hits) return;   // (wave-uniform) the r-th occurrence is another wave's
  for (int xb = u0; xb < u1; xb += 64) {
    const int x = xb + lane;
    ushort8 v = {0, 0, 0, 0, 0, 0, 0, 0};       // (0 never equals tb >= 1)
    if (x < u1) {
      if (VEC) {
        v = *(const ushort8*)(row + (size_t)x * 8);
      } else {
        v[0] = row[x];
      }
    }
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) m += v[j] == tb;
    if (__ballot(m != 0) == 0) continue;
    uint32_t incl = m;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    const uint32_t tot = __shfl(incl, 63, 64);
    if (run + tot > tr) {
      const uint32_t ex = run + incl - m;
      if (ex <= tr && tr < ex + m) {
        const uint32_t left = tr - ex;          // the left-th match among the lane's columns
        uint32_t seen = 0;
        int col = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool hit = v[j] == tb;
          if (hit && seen == left) col = j;
          seen += hit;
        }
        out[blockIdx.x] = VEC ? x * 8 + col : x;
      }
      return;
    }
    run += tot;
  }
}

}  // namespace

extern "C" int fls_sample_rows(const void* probs, int ld, int rows, int V, const uint32_t* table,
                               const uint64_t* draws, int top_k, int P, int* out, fls_stream_t s) {
  if (rows <= 0) return 0;
  if (V <= 0 || V >= (1 << 18) || ld < V || top_k < 0 || P < 1 || P > 65536) return (int)hipErrorInvalidValue;
  const bool vec = V % 8 == 0 && ld % 8 == 0 && ((uintptr_t)probs & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(sample_rows_kernel<true>, dim3(rows), dim3(256), 0, (hipStream_t)s, (const half_t*)probs, ld,
                       V, table, draws, top_k, (uint32_t)P, out);
  else
    hipLaunchKernelGGL(sample_rows_kernel<false>, dim3(rows), dim3(256), 0, (hipStream_t)s, (const half_t*)probs,
                       ld, V, table, draws, top_k, (uint32_t)P, out);
  FLS_CHECK_LAUNCH();
  return 0;
}
