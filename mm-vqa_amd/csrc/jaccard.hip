// Jaccard positive mask of SupCon pre-training (models/SupConLoss/supcon_utils.py:110-138) from word-id sets that
// are resident on the device.  The table's texts are held as one CSR: text t = row * JC_TEXTS + column owns the sorted,
// unique word ids ids[offsets[t] .. offsets[t + 1]) (mmvqa_amd.data.WordSets builds it on the host, once).
//   mask[i][j] = 1                                   i == j   (positions in the batch, :114-117)
//              = |A_i & B_j| / |A_i | B_j|           A_i = text (rowsA[i], colsA[i]), B_j = text (rowsB[j], colsB[j])
//              = 0                                   both sets empty (:134-138)
// One workgroup per anchor i: A_i is staged in LDS once, wave w takes the columns j = w, w + 4, ...; its lanes walk
// B_j and binary-search each id in A_i, the hit count is wave-reduced, |union| = |A| + |B| - hits.  The quotient is
// formed in double and rounded once to fp32, which is what the reference's Python float division stored into a float
// tensor gives, so the result is bit-equal to it.  A set longer than JC_LDS ids is searched in global memory instead
// (same code, flat pointer): no length is truncated.  A (row, column) outside the table gives NaN in its row / column
// of the mask rather than a read outside the CSR.
#include "common.h"
#include "kernels.h"

#define JC_TEXTS 4      // texts per table row: the caption and its three back-translations
#define JC_LDS 512      // ids of the anchor's set kept in LDS

__device__ __forceinline__ bool jc_text(int row, int col, int table_rows, const int* __restrict__ offsets, int& lo,
                                        int& len) {
  lo = 0; len = 0;
  if (row < 0 || row >= table_rows || col < 0 || col >= JC_TEXTS) return false;
  const int t = row * JC_TEXTS + col;
  lo = offsets[t];
  len = offsets[t + 1] - lo;
  return len >= 0;
}

__global__ void __launch_bounds__(256) jaccard_mask_kernel(const int* __restrict__ offsets, const int* __restrict__ ids,
                                                           const int* __restrict__ rowsA, const int* __restrict__ colsA,
                                                           const int* __restrict__ rowsB, const int* __restrict__ colsB,
                                                           float* __restrict__ mask, int n, int table_rows) {
  __shared__ int sa[JC_LDS];
  const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int loA, lenA;
  const bool okA = jc_text(rowsA[i], colsA[i], table_rows, offsets, loA, lenA);
  const bool in_lds = lenA <= JC_LDS;
  if (in_lds)
    for (int k = threadIdx.x; k < lenA; k += blockDim.x) sa[k] = ids[loA + k];
  __syncthreads();
  const int* A = in_lds ? sa : ids + loA;
  for (int j = wave; j < n; j += 4) {
    int loB, lenB;
    const bool okB = jc_text(rowsB[j], colsB[j], table_rows, offsets, loB, lenB);
    int hits = 0;
    if (i != j && okA && okB) {
      for (int k = lane; k < lenB; k += 64) {
        const int v = ids[loB + k];
        int lo = 0, hi = lenA;                       // first index with A[idx] >= v
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (A[mid] < v) lo = mid + 1; else hi = mid;
        }
        hits += (lo < lenA && A[lo] == v) ? 1 : 0;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o, 64);
    if (lane == 0) {
      float q;
      if (!okA || !okB) q = __int_as_float(0x7fc00000);
      else if (i == j) q = 1.0f;
      else {
        const int uni = lenA + lenB - hits;
        q = uni != 0 ? (float)((double)hits / (double)uni) : 0.0f;
      }
      mask[(size_t)i * n + j] = q;
    }
  }
}

extern "C" int mmvqa_jaccard_mask(mmvqa_stream_t s, const int* offsets, const int* ids, const int* rowsA,
                                  const int* colsA, const int* rowsB, const int* colsB, float* mask, int n,
                                  int table_rows) {
  hipStream_t st = (hipStream_t)s;
  if (n < 1 || table_rows < 1) return mmvqa_set_error(MMVQA_ERR_ARG, "jaccard_mask: n=%d table_rows=%d (both >= 1)", n, table_rows);
  if (!offsets || !ids || !rowsA || !colsA || !rowsB || !colsB || !mask)
    return mmvqa_set_error(MMVQA_ERR_ARG, "jaccard_mask: null operand");
  hipLaunchKernelGGL(jaccard_mask_kernel, dim3(n), dim3(256), 0, st, offsets, ids, rowsA, colsA, rowsB, colsB, mask, n,
                     table_rows);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}
