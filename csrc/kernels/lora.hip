// LoRA merge in place in the HBM weight slot (flexible_llm_sharding_amd/lora.py is the definition):
//
//   acc_0 = fp32(W[o, i]);  acc_{k+1} = fmaf(Bs[o, k], A[k, i], acc_k), k = 0 .. R-1 ascending;
//   W[o, i] = fp16_rne(acc_R)
//
// with R = r rounded up to a multiple of 4 (the host pads A and Bs with +0).  The chain runs on the
// f32-input MFMA (v_mfma_f32_16x16x4_f32), whose result is a k-ordered fmaf chain with one rounding
// per product: the data path holds loads, fp16 <-> fp32 conversions and MFMAs only, no VALU
// arithmetic a compiler could contract or reorder.
//
// A wave owns a (16 RG)-row x 64-column tile of W as RG x 4 accumulator tiles of 16 x 16 (4 RG
// independent MFMA chains; RG = 2 for r < 32, RG = 4 above, where twice the rows reuse every A
// operand).  The MFMA computes the TRANSPOSED tile -- its A operand is the adapter's A (index m = a
// column of W), its B operand is Bs (index n = a row of W) -- so a lane's four accumulator
// registers are four consecutive columns of one row of W: lane (n = lane & 15, g = lane >> 4) holds
// row n, columns 8g .. 8g+7 and 32+8g .. 32+8g+7 of the tile, and W moves with two 16-byte loads
// and two 16-byte stores per lane and 16-row group.  Accumulator tile t, register j of lane group g
// is column 32 (t >> 1) + 8 g + 4 (t & 1) + j.  A and Bs are read straight from L2 (a layer's are
// a few MB), one dword per lane and operand, the next k-step's while this one's MFMAs run.
#include "common.h"
#include "fls.h"

namespace {

constexpr int LORA_COLS = 64, LORA_WAVES = 4;

// VEC: cols % 8 == 0 and W 16-byte aligned (16-byte accesses of W); else 2-byte accesses.
// Waves take the tiles in row-major order (consecutive waves walk along a row of tiles).
template <bool VEC, int RG>
__global__ __launch_bounds__(LORA_WAVES * 64) void lora_merge_kernel(half_t* __restrict__ W, int rows, int cols,
                                                                    const float* __restrict__ A,
                                                                    const float* __restrict__ Bs, int R,
                                                                    unsigned ctiles, long long tiles) {
  const int lane = threadIdx.x & 63;
  const long long wid = (long long)blockIdx.x * LORA_WAVES + (threadIdx.x >> 6);
  if (wid >= tiles) return;                              // (wave-uniform)
  long long rt;
  if (tiles <= 0xffffffffLL) rt = (unsigned)wid / ctiles;  // (a 32-bit division where it serves)
  else rt = wid / ctiles;
  const long long row0 = rt * (16 * RG), col0 = (wid - rt * ctiles) * LORA_COLS;
  const int n = lane & 15, g = lane >> 4;

  // this lane's W elements: rows row0 + 16 rg + n, column runs cbase[h] .. cbase[h] + 7
  long long cbase[2];
  cbase[0] = col0 + 8 * g;
  cbase[1] = col0 + 32 + 8 * g;
  floatx4 acc[RG][4];
#pragma unroll
  for (int rg = 0; rg < RG; ++rg) {
    const long long row = row0 + 16 * rg + n;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      half8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (half_t)0.f;
      if (row < rows) {
        half_t* p = W + row * (long long)cols + cbase[h];
        if (VEC) {
          if (cbase[h] < cols) v = *(const half8*)p;     // (cols % 8 == 0: the run is whole or absent)
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (cbase[h] + j < cols) v[j] = p[j];
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[rg][2 * h + (j >> 2)][j & 3] = (float)v[j];
    }
  }

  // operand addresses.  A operand of tile t: lane (m = lane & 15, k = g) holds A[k0 + g][column of m];
  // B operand of row group rg: lane (n, k = g) holds Bs[row][k0 + g].  Rows and columns past the end
  // read nothing (0): they only feed results that are not written.
  long long acol[4];
  bool aok[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    acol[t] = col0 + 32 * (t >> 1) + 8 * (n >> 2) + 4 * (t & 1) + (n & 3);
    aok[t] = acol[t] < cols;
  }
  const float* bp[RG];
  bool bok[RG];
#pragma unroll
  for (int rg = 0; rg < RG; ++rg) {
    const long long row = row0 + 16 * rg + n;
    bok[rg] = row < rows;
    bp[rg] = Bs + (bok[rg] ? row : 0) * (long long)R + g;
  }
  const float* ap = A + (long long)g * cols;
  const long long astep = 4LL * cols;

  float a[4], b[RG];
#pragma unroll
  for (int t = 0; t < 4; ++t) a[t] = aok[t] ? ap[acol[t]] : 0.f;
#pragma unroll
  for (int rg = 0; rg < RG; ++rg) b[rg] = bok[rg] ? bp[rg][0] : 0.f;
  if (RG == 2) {
    // short chains (r < 32): the plain loop; the other waves of the SIMD cover the operand loads
    for (int k0 = 0; k0 < R; k0 += 4) {
      if (k0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) a[t] = aok[t] ? ap[acol[t]] : 0.f;
#pragma unroll
        for (int rg = 0; rg < RG; ++rg) b[rg] = bok[rg] ? bp[rg][k0] : 0.f;
      }
      ap += astep;
#pragma unroll
      for (int rg = 0; rg < RG; ++rg)
#pragma unroll
        for (int t = 0; t < 4; ++t)
          acc[rg][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[rg], acc[rg][t], 0, 0, 0);
    }
  } else
  for (int k0 = 0; k0 < R; k0 += 4) {
    float an[4], bn[RG];
    ap += astep;
    const bool more = k0 + 4 < R;                        // (the next k-step's operands: A has R rows)
#pragma unroll
    for (int t = 0; t < 4; ++t) an[t] = (more && aok[t]) ? ap[acol[t]] : 0.f;
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) bn[rg] = (more && bok[rg]) ? bp[rg][k0 + 4] : 0.f;
#pragma unroll
    for (int rg = 0; rg < RG; ++rg)
#pragma unroll
      for (int t = 0; t < 4; ++t)
        acc[rg][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[rg], acc[rg][t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t) a[t] = an[t];
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) b[rg] = bn[rg];
  }

#pragma unroll
  for (int rg = 0; rg < RG; ++rg) {
    const long long row = row0 + 16 * rg + n;
    if (row >= rows) continue;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      half8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (half_t)acc[rg][2 * h + (j >> 2)][j & 3];
      half_t* p = W + row * (long long)cols + cbase[h];
      if (VEC) {
        if (cbase[h] < cols) *(half8*)p = v;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (cbase[h] + j < cols) p[j] = v[j];
      }
    }
  }
}

template <bool VEC, int RG>
void lora_launch(half_t* W, long long rows, long long cols, const float* A, const float* Bs, int R, hipStream_t s) {
  const long long rtiles = (rows + 16 * RG - 1) / (16 * RG), ctiles = (cols + LORA_COLS - 1) / LORA_COLS;
  const long long tiles = rtiles * ctiles, blocks = (tiles + LORA_WAVES - 1) / LORA_WAVES;
  hipLaunchKernelGGL((lora_merge_kernel<VEC, RG>), dim3((unsigned)blocks), dim3(LORA_WAVES * 64), 0, s, W, (int)rows,
                     (int)cols, A, Bs, R, (unsigned)ctiles, tiles);
}

}  // namespace

extern "C" int fls_lora_merge(void* W, long long rows, long long cols, const void* A, const void* Bs, int r,
                              fls_stream_t s) {
  if (!W || !A || !Bs || rows <= 0 || cols <= 0 || r < 1 || r > 256) return (int)hipErrorInvalidValue;
  if (rows > 0x7fffffffLL || cols > 0x7fffffffLL || ((uintptr_t)W & 1) || (((uintptr_t)A | (uintptr_t)Bs) & 3))
    return (int)hipErrorInvalidValue;
  const int R = (r + 3) & ~3;
  // one block per four tiles of 32 x 64 at the least: the grid holds 2^31 - 1 blocks
  if (((rows + 31) / 32) * ((cols + LORA_COLS - 1) / LORA_COLS) / LORA_WAVES >= 0x7fffffffLL)
    return (int)hipErrorInvalidValue;
  const bool vec = cols % 8 == 0 && ((uintptr_t)W & 15) == 0;
  half_t* w = (half_t*)W;
  const float *a = (const float*)A, *b = (const float*)Bs;
  if (R >= 32) {
    if (vec) lora_launch<true, 4>(w, rows, cols, a, b, R, (hipStream_t)s);
    else lora_launch<false, 4>(w, rows, cols, a, b, R, (hipStream_t)s);
  } else {
    if (vec) lora_launch<true, 2>(w, rows, cols, a, b, R, (hipStream_t)s);
    else lora_launch<false, 2>(w, rows, cols, a, b, R, (hipStream_t)s);
  }
  FLS_CHECK_LAUNCH();
  return 0;
}
