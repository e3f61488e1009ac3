// Verification of prompt-lookup drafts (flexible_llm_sharding_amd/lookup.py holds the definition and
// the host implementation that returns the same entries for every input).
//
// A call with drafts scores, per suffix, its last token and every draft token: suffix i owns rows
// row_start[i] .. row_start[i + 1] - 1 of the fp16 probabilities, and draft[r] is the draft token
// scored next to row r (-1 on a suffix's last row).
//   launch 1  verify_argmax_kernel, one 256-thread block per row: tok[r] = the row's greedy id, by
//             argmax_rows_kernel's rule (largest bit pattern, first index on ties; an all-zero row
//             gives 0).  16-byte loads where V, the row stride and the base allow, scalar otherwise
//   launch 2  verify_accept_kernel, one 256-thread block, behind launch 1 on the same stream:
//             accept[i] = the number of leading rows j of suffix i with tok[j] == draft[j], then a
//             block prefix sum of accept + 1 over the suffixes (256 at a time, with a carry) places
//             the kept rows - rows 0 .. accept[i] of every suffix, in suffix order - in keep, and
//             their count in n_kept
// No workgroup waits for another: the second launch is ordered by the stream.  Every decision is an
// integer one.
#include "common.h"
#include "fls.h"

namespace {

typedef unsigned short ushort8 __attribute__((ext_vector_type(8)));

template <bool VEC>   // 16-byte loads: V % 8 == 0, ld % 8 == 0 and a 16-byte aligned base
__global__ __launch_bounds__(256) void verify_argmax_kernel(const half_t* __restrict__ probs, int ld, int V,
                                                          int* __restrict__ tok) {
  __shared__ unsigned sb[256];
  __shared__ int si[256];
  const unsigned short* r = (const unsigned short*)(probs + (size_t)blockIdx.x * ld);
  unsigned best = 0;
  int bi = 0x7fffffff;
  if (VEC) {
    for (int u = threadIdx.x; u < V / 8; u += 256) {
      const ushort8 v = *(const ushort8*)(r + (size_t)u * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned b = v[j];
        const int c = u * 8 + j;
        if (b > best || (b == best && c < bi)) {
          best = b;
          bi = c;
        }
      }
    }
  } else {
    for (int c = threadIdx.x; c < V; c += 256) {
      const unsigned b = r[c];
      if (b > best || (b == best && c < bi)) {
        best = b;
        bi = c;
      }
    }
  }
  sb[threadIdx.x] = best;
  si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      const unsigned b = sb[threadIdx.x + s];
      const int i = si[threadIdx.x + s];
      if (b > sb[threadIdx.x] || (b == sb[threadIdx.x] && i < si[threadIdx.x])) {
        sb[threadIdx.x] = b;
        si[threadIdx.x] = i;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) tok[blockIdx.x] = si[0] == 0x7fffffff ? 0 : si[0];
}

__global__ __launch_bounds__(256) void verify_accept_kernel(const int* __restrict__ tok,
                                                          const int* __restrict__ row_start,
                                                          const int* __restrict__ draft, int n_sfx,
                                                          int n_rows, int* __restrict__ accept, int* __restrict__ keep,
                                                          int* __restrict__ n_kept) {
  __shared__ int scan[256];
  __shared__ int carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n_sfx; base += 256) {
    const int i = base + tid;
    int r0 = 0, cnt = 0;
    if (i < n_sfx) {
      // (a row range outside [0, n_rows] is cut to it: nothing outside tok / draft / keep is touched)
      r0 = min(max(row_start[i], 0), n_rows);
      const int rows = min(max(row_start[i + 1], r0), n_rows) - r0;
      int a = 0;
      while (a < rows - 1 && tok[r0 + a] == draft[r0 + a]) ++a;
      accept[i] = a;
      cnt = rows > 0 ? a + 1 : 0;
    }
    // inclusive prefix sum of cnt over the 256 suffixes of this round
    scan[tid] = cnt;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int v = tid >= o ? scan[tid - o] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    const int off = carry + scan[tid] - cnt;
    for (int j = 0; j < cnt && off + j < n_rows; ++j) keep[off + j] = r0 + j;
    __syncthreads();                    // every thread has read carry
    if (tid == 255) carry += scan[255];
    __syncthreads();
  }
  if (tid == 0) n_kept[0] = min(carry, n_rows);
}

}  // namespace

extern "C" int fls_verify_rows(const void* probs, int ld, int rows, int V, const int* row_start, int n_sfx,
                               const int* draft, int* tok, int* accept, int* keep, int* n_kept, fls_stream_t s) {
  if (rows < 0 || n_sfx < 0 || V <= 0 || ld < V) return (int)hipErrorInvalidValue;
  if (row_start == nullptr || accept == nullptr || keep == nullptr || n_kept == nullptr)
    return (int)hipErrorInvalidValue;
  if (rows > 0 && (probs == nullptr || draft == nullptr || tok == nullptr)) return (int)hipErrorInvalidValue;
  if (rows > 0) {
    const bool vec = V % 8 == 0 && ld % 8 == 0 && ((uintptr_t)probs & 15) == 0;
    if (vec)
      hipLaunchKernelGGL(verify_argmax_kernel<true>, dim3(rows), dim3(256), 0, (hipStream_t)s, (const half_t*)probs,
                         ld, V, tok);
    else
      hipLaunchKernelGGL(verify_argmax_kernel<false>, dim3(rows), dim3(256), 0, (hipStream_t)s, (const half_t*)probs,
                         ld, V, tok);
    FLS_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(verify_accept_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, tok, row_start, draft, n_sfx, rows,
                     accept, keep, n_kept);
  FLS_CHECK_LAUNCH();
  return 0;
}
