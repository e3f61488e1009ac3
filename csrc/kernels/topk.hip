// The K best next-token scores of each row of fp16 probabilities, selected on the device, integer-exact
// (flexible_llm_sharding_amd/topk.py holds the definition and the host implementation that returns the
// same entries for every input).
//
// The key of an entry is its fp16 bit pattern b if b <= 0x3C00 (0 <= p <= 1), else 0: negative, NaN
// and > 1 patterns rank with the zeros, as in the sampler.  Entries are ranked by (key descending,
// index ascending); ids[r, 0..K) and vals[r, 0..K) are the first K ranked entries of row r (vals: the
// key itself), and picked_vals[r] is the key of entry picked[r] (0 for an id outside [0, V)).
// One 256-thread block per row:
//   pass 1  histogram of the row's non-zero keys in LDS (15,361 uint32 bins, zeros skipped: most of a
//           real row is zero and same-address LDS atomics serialise), as sample_rows_kernel
//   scan    thread t owns the 61 bins from 0x3C00 - 61 t downwards; a block prefix over the threads'
//           counts finds the threshold bin tb (the first bin, from the top, where the running count
//           reaches K) and c_above < K, the entries in the bins above it.  Fewer than K non-zero
//           keys: tb = 0 and c_above is their count
//   pass 2  every entry with key > tb is a candidate (an LDS slot counter: their order does not
//           matter, all are kept); of the entries with key == tb the first K - c_above in index
//           order are: each wave counts the matches of its contiguous quarter of the row, then walks
//           it again, 64 lanes at a time with a lane prefix over the match counts, until the last
//           needed occurrence is placed (a wave whose quarter starts past it walks nothing)
//   sort    bitonic sort, descending, of the K candidates (key << 32 | 0xFFFFFFFF - index) in LDS
// No floating-point value is compared: every decision is an integer one.
#include "common.h"
#include "fls.h"

namespace {

constexpr int TOPK_BINS = 0x3C01;   // bit patterns 0 .. 0x3C00 (1.0)
constexpr int TOPK_CHUNK = 61;      // bins per thread (256 x 61 >= 0x3C00; odd: no LDS bank conflicts)
constexpr int TOPK_MAX = 1024;      // the largest K: 8 KB of candidates next to the 61.5 KB histogram

typedef unsigned short ushort8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ uint32_t topk_key(uint32_t b) { return b <= 0x3C00u ? b : 0u; }

__device__ __forceinline__ uint64_t topk_composite(uint32_t key, int index) {
  return ((uint64_t)key << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)index);
}

template <bool VEC>   // 16-byte loads: V % 8 == 0, ld % 8 == 0 and a 16-byte aligned base
__global__ __launch_bounds__(256) void topk_rows_kernel(const half_t* __restrict__ probs, int ld, int V, int K,
                                                      int* __restrict__ ids, unsigned short* __restrict__ vals,
                                                      const int* __restrict__ picked,
                                                      unsigned short* __restrict__ picked_vals) {
  __shared__ uint32_t hist[TOPK_BINS];
  __shared__ uint64_t cand[TOPK_MAX];
  __shared__ uint32_t wave_c[4];
  __shared__ uint32_t wave_hits[4];
  __shared__ uint32_t found[2];       // tb, c_above
  __shared__ uint32_t slot;           // candidates with key > tb placed so far
  constexpr int NV = VEC ? 8 : 1;     // columns a lane loads at a time
  const unsigned short* row = (const unsigned short*)(probs + (size_t)blockIdx.x * ld);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < TOPK_BINS; i += 256) hist[i] = 0;
  if (tid == 0) {
    found[0] = 0;
    found[1] = 0;
    slot = 0;
  }
  __syncthreads();

  // the token the engine chose for this row: its key, the same clamp (an id outside the row reads nothing)
  if (tid == 0 && picked != nullptr) {
    const int p = picked[blockIdx.x];
    picked_vals[blockIdx.x] = (uint32_t)p < (uint32_t)V ? (unsigned short)topk_key(row[p]) : (unsigned short)0;
  }

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

  // this thread's bins, from the top: their count, then the exclusive block prefix
  const int top_bin = 0x3C00 - tid * TOPK_CHUNK;
  uint32_t c = 0;
  for (int i = 0; i < TOPK_CHUNK; ++i) {
    const int b = top_bin - i;
    if (b < 1) break;
    c += hist[b];
  }
  uint32_t ci = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t tc = __shfl_up(ci, o, 64);
    if (lane >= o) ci += tc;
  }
  if (lane == 63) wave_c[wave] = ci;
  __syncthreads();
  uint32_t c_ex = ci - c, n_total = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) c_ex += wave_c[w];
    n_total += wave_c[w];
  }
  const uint32_t k = (uint32_t)K;
  if (n_total >= k) {                 // (block-uniform) exactly one thread's bins hold the K-th ranked entry
    if (c_ex < k && k <= c_ex + c) {
      uint32_t rc = c_ex;
      for (int i = 0; i < TOPK_CHUNK; ++i) {
        const int b = top_bin - i;
        if (b < 1) break;
        const uint32_t n = hist[b];
        if (rc + n >= k) {
          found[0] = (uint32_t)b;
          found[1] = rc;
          break;
        }
        rc += n;
      }
    }
    __syncthreads();
  }
  const uint32_t tb = n_total >= k ? found[0] : 0u;
  const uint32_t c_above = n_total >= k ? found[1] : n_total;
  const uint32_t need = k - c_above;  // entries of key tb to keep, in index order (>= 1)

  // pass 2a: every key > tb is a candidate; count this wave's matches of tb
  uint32_t hits = 0;
  for (int x = u0 + lane; x < u1; x += 64) {
    ushort8 v;
    if (VEC) {
      v = *(const ushort8*)(row + (size_t)x * 8);
    } else {
      v[0] = row[x];
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const uint32_t key = topk_key(v[j]);
      hits += key == tb;
      if (key > tb) {
        const uint32_t at = atomicAdd(&slot, 1u);
        if (at < (uint32_t)TOPK_MAX) cand[at] = topk_composite(key, x * NV + j);   // (at < c_above by the histogram)
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o, 64);
  if (lane == 0) wave_hits[wave] = hits;
  __syncthreads();

  // pass 2b: the first `need` matches of tb in index order, behind the c_above candidates
  uint32_t run = 0;                   // (wave-uniform) matches in front of the 64 units being looked at
  for (int w = 0; w < wave; ++w) run += wave_hits[w];
  for (int xb = u0; xb < u1 && run < need; xb += 64) {
    const int x = xb + lane;
    const bool in = x < u1;
    ushort8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (in) {
      if (VEC) {
        v = *(const ushort8*)(row + (size_t)x * 8);
      } else {
        v[0] = row[x];
      }
    }
    uint32_t m = 0;
    if (in) {
#pragma unroll
      for (int j = 0; j < NV; ++j) m += topk_key(v[j]) == tb;
    }
    if (__ballot(m != 0) == 0) continue;
    uint32_t incl = m;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    const uint32_t tot = __shfl(incl, 63, 64);
    uint32_t pos = run + incl - m;    // the rank of this lane's first match
    if (m != 0 && pos < need) {
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        if (topk_key(v[j]) == tb) {
          if (pos < need) cand[c_above + pos] = topk_composite(tb, x * NV + j);   // c_above + pos < K
          ++pos;
        }
      }
    }
    run += tot;
  }

  // sort: K candidates, padded with zeros (below every candidate: an index is < 2^31) to a power of two
  int n = 1;
  while (n < K) n <<= 1;
  for (int i = K + tid; i < n; i += 256) cand[i] = 0;
  __syncthreads();
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < n; i += 256) {
        const int l = i ^ stride;
        if (l > i) {
          const uint64_t a = cand[i], b = cand[l];
          const bool down = (i & size) == 0;          // this pair's larger value goes first
          if (down ? a < b : a > b) {
            cand[i] = b;
            cand[l] = a;
          }
        }
      }
      __syncthreads();
    }
  }
  int* out_ids = ids + (size_t)blockIdx.x * K;
  unsigned short* out_vals = vals + (size_t)blockIdx.x * K;
  for (int i = tid; i < K; i += 256) {
    const uint64_t e = cand[i];
    out_ids[i] = (int)(0xFFFFFFFFu - (uint32_t)e);
    out_vals[i] = (unsigned short)(e >> 32);
  }
}

}  // namespace

extern "C" int fls_topk_rows(const void* probs, int ld, int rows, int V, int K, int* ids, void* vals,
                             const int* picked, void* picked_vals, fls_stream_t s) {
  if (rows <= 0) return 0;
  if (V <= 0 || ld < V || K < 1 || K > V || K > TOPK_MAX) return (int)hipErrorInvalidValue;
  if (probs == nullptr || ids == nullptr || vals == nullptr || (picked == nullptr) != (picked_vals == nullptr))
    return (int)hipErrorInvalidValue;
  const bool vec = V % 8 == 0 && ld % 8 == 0 && ((uintptr_t)probs & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(topk_rows_kernel<true>, dim3(rows), dim3(256), 0, (hipStream_t)s, (const half_t*)probs, ld, V,
                       K, ids, (unsigned short*)vals, picked, (unsigned short*)picked_vals);
  else
    hipLaunchKernelGGL(topk_rows_kernel<false>, dim3(rows), dim3(256), 0, (hipStream_t)s, (const half_t*)probs, ld, V,
                       K, ids, (unsigned short*)vals, picked, (unsigned short*)picked_vals);
  FLS_CHECK_LAUNCH();
  return 0;
}
