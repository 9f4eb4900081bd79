// Cosine positive mask of SupCon pre-training from caption sentence embeddings that are resident on the device
// (models/SupConLoss/supcon_utils.py:140-168: bert_embedd writes it out, sentence_trans calls util.cos_sim).  The
// encoder that makes the embeddings is not run here: the table [table_rows][CM_TEXTS][D] fp32 is computed once,
// offline, uploaded once and normalised in place by normalize_rows (x / max(|x|, eps), :152-157), so that per batch
//   mask[i][j] = 1                                              i == j   (positions in the batch, fill_diagonal_(1))
//              = sum_k table[rowsA[i]][colsA[i]][k] * table[rowsB[j]][colsB[j]][k]
// One workgroup per anchor i: its row is staged in LDS once, wave w takes the columns j = w, w + 4, ...; the lanes
// stride over D (16-byte loads when D % 4 == 0 and the table is 16-byte aligned, scalar loads otherwise) with one fmaf
// chain per lane, the 64 partial sums are added in a fixed butterfly and lane 0 stores the entry.  No atomics and no
// order that depends on timing: the same inputs give the same bits on every launch and in every process, which the
// data-parallel path needs (every rank builds the global mask itself).  A (row, column) outside the table gives NaN in
// its row / column of the mask rather than a read outside the table.
#include "common.h"
#include "kernels.h"

#include <cstdint>

#define CM_TEXTS 4      // texts per table row: the caption and its three back-translations
#define CM_MAX_D 4096   // the anchor's row in LDS: 16 KB

__device__ __forceinline__ bool cm_text(int row, int col, int table_rows) {
  return row >= 0 && row < table_rows && col >= 0 && col < CM_TEXTS;
}

__device__ __forceinline__ float cm_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one wave per row, rows strided over the grid: two passes over a row that the first pass has just brought in
__global__ void __launch_bounds__(256) normalize_rows_kernel(float* __restrict__ x, long long rows, int D, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long r = (long long)blockIdx.x * 4 + wave; r < rows; r += (long long)gridDim.x * 4) {
    float* p = x + (size_t)r * D;
    float ss = 0.0f;
    for (int k = lane; k < D; k += 64) ss = fmaf(p[k], p[k], ss);
    const float d = fmaxf(sqrtf(cm_wave_sum(ss)), eps);
    for (int k = lane; k < D; k += 64) p[k] = p[k] / d;
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) cosine_mask_kernel(const float* __restrict__ table, const int* __restrict__ rowsA,
                                                          const int* __restrict__ colsA, const int* __restrict__ rowsB,
                                                          const int* __restrict__ colsB, float* __restrict__ mask, int n,
                                                          int D, int table_rows) {
  __shared__ __attribute__((aligned(16))) float sa[CM_MAX_D];
  const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ra = rowsA[i], ca = colsA[i];
  const bool okA = cm_text(ra, ca, table_rows);
  if (okA) {
    const float* a = table + ((size_t)ra * CM_TEXTS + ca) * D;
    if constexpr (VEC) {
      for (int k = threadIdx.x * 4; k < D; k += 1024) *(float4*)(sa + k) = *(const float4*)(a + k);
    } else {
      for (int k = threadIdx.x; k < D; k += 256) sa[k] = a[k];
    }
  }
  __syncthreads();
  for (int j = wave; j < n; j += 4) {             // j, okB and the branch below are uniform over the wave
    const int rb = rowsB[j], cb = colsB[j];
    const bool okB = cm_text(rb, cb, table_rows);
    float acc = 0.0f;
    if (i != j && okA && okB) {
      const float* b = table + ((size_t)rb * CM_TEXTS + cb) * D;
      if constexpr (VEC) {
#pragma unroll 4
        for (int k = lane * 4; k < D; k += 256) {
          const float4 u = *(const float4*)(sa + k), v = *(const float4*)(b + k);
          acc = fmaf(u.x, v.x, acc);
          acc = fmaf(u.y, v.y, acc);
          acc = fmaf(u.z, v.z, acc);
          acc = fmaf(u.w, v.w, acc);
        }
      } else {
#pragma unroll 4
        for (int k = lane; k < D; k += 64) acc = fmaf(sa[k], b[k], acc);
      }
    }
    acc = cm_wave_sum(acc);
    if (lane == 0) {
      float q;
      if (!okA || !okB) q = __int_as_float(0x7fc00000);
      else if (i == j) q = 1.0f;
      else q = acc;
      mask[(size_t)i * n + j] = q;
    }
  }
}

extern "C" int mmvqa_normalize_rows(mmvqa_stream_t s, float* x, long long rows, int D, float eps) {
  hipStream_t st = (hipStream_t)s;
  if (rows < 1 || D < 1 || D > CM_MAX_D)
    return mmvqa_set_error(MMVQA_ERR_ARG, "normalize_rows: rows=%lld D=%d (rows >= 1, 1 <= D <= %d)", rows, D, CM_MAX_D);
  if (!x) return mmvqa_set_error(MMVQA_ERR_ARG, "normalize_rows: null operand");
  const long long blocks = (rows + 3) / 4;
  hipLaunchKernelGGL(normalize_rows_kernel, dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(256), 0, st, x,
                     rows, D, eps);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

extern "C" int mmvqa_cosine_mask(mmvqa_stream_t s, const float* table, const int* rowsA, const int* colsA,
                                 const int* rowsB, const int* colsB, float* mask, int n, int D, int table_rows) {
  hipStream_t st = (hipStream_t)s;
  if (n < 1 || table_rows < 1 || D < 1 || D > CM_MAX_D)
    return mmvqa_set_error(MMVQA_ERR_ARG, "cosine_mask: n=%d table_rows=%d D=%d (n, table_rows >= 1, 1 <= D <= %d)", n,
                           table_rows, D, CM_MAX_D);
  if (!table || !rowsA || !colsA || !rowsB || !colsB || !mask)
    return mmvqa_set_error(MMVQA_ERR_ARG, "cosine_mask: null operand");
  // every text starts at a multiple of D floats: 16-byte loads need D % 4 == 0 and a 16-byte aligned table
  if (D % 4 == 0 && ((uintptr_t)table & 15) == 0)
    hipLaunchKernelGGL(cosine_mask_kernel<true>, dim3(n), dim3(256), 0, st, table, rowsA, colsA, rowsB, colsB, mask, n, D,
                       table_rows);
  else
    hipLaunchKernelGGL(cosine_mask_kernel<false>, dim3(n), dim3(256), 0, st, table, rowsA, colsA, rowsB, colsB, mask, n, D,
                       table_rows);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}
