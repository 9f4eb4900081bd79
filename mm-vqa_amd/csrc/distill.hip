// Distillation loss of pre-training (pretrain/roco_train.py:94-95 nn.MSELoss; roco_utils.py:230-238 loss = MSE(h, target))
// with the target gathered from the teacher's per-token states, which are resident on the device (roco_utils.py:112-132
// computes them per caption; here they are computed once, offline).  The dense target of encode_text's distillation
// branch (roco_utils.py:162-199) is never stored: for row r = b T + t of h [B T][ld]
//   target(r) = table[start[b] + t - first]     first <= t < first + n_b,  n_b = min(count[b], T - first - 1)  (:175-176)
//             = 0                               every other row: CLS, the visual rows, both SEPs, the padding (:196-197)
//   row_sq[r] = sum_j (h[r][j] - target(r)[j])^2
//   dh[r][j]  = (h[r][j] - target(r)[j]) * gscale          one subtraction, one multiplication
//   *loss     = (sum_r row_sq[r]) / (B T H)                the mean over ALL elements, as nn.MSELoss takes it
// One wave per row, four rows per 256-thread workgroup.  Vector form (H % 4 == 0, ld and dld multiples of 4, h, dh and
// the table aligned to a whole access): 16-byte loads and stores of h / dh, 16-byte loads of an fp32 table row and 8-byte
// loads of four halves of an fp16 one; otherwise one element at a time.  Each lane squares and adds its differences in
// one fmaf chain, the 64 partial sums are added in a fixed butterfly and lane 0 stores the row's sum; a second launch of
// one workgroup adds the rows in a fixed order.  No atomics and no order that depends on timing: the loss is bit-equal
// from run to run.
// Longest chain of additions a summand passes through (every summand is non-negative, so the relative error of the sum
// is at most that many roundings):
//   L = 4 ceil(H / 256)  (lane chain; the scalar form's ceil(H / 64) is never longer)  +  6  (butterfly)
//       + ceil(B T / 256) + 6 + 2  (finishing launch: thread chain, butterfly, the four waves)
// A sample with start < 0, count < 0 or start + n_b > table_rows gets NaN in all its row_sq and dh rows and reads
// nothing from the table.
#include "common.h"
#include "kernels.h"

#include <cstdint>
#include <hip/hip_fp16.h>

template <bool F16>
__device__ __forceinline__ f32x4 dm_load4(const void* __restrict__ row, int k) {
  if constexpr (F16) {
    const uint2 q = *reinterpret_cast<const uint2*>(static_cast<const __half*>(row) + k);   // four halves
    const __half2 a = *reinterpret_cast<const __half2*>(&q.x), b = *reinterpret_cast<const __half2*>(&q.y);
    return f32x4{__low2float(a), __high2float(a), __low2float(b), __high2float(b)};
  } else {
    return *reinterpret_cast<const f32x4*>(static_cast<const float*>(row) + k);
  }
}

template <bool F16>
__device__ __forceinline__ float dm_load1(const void* __restrict__ row, int k) {
  if constexpr (F16) return __half2float(static_cast<const __half*>(row)[k]);
  else return static_cast<const float*>(row)[k];
}

template <bool VEC, bool F16>
__global__ void __launch_bounds__(256) distill_mse_kernel(const float* __restrict__ h, int ld, const void* __restrict__ table,
                                                          long long table_rows, const long long* __restrict__ start,
                                                          const int* __restrict__ count, int first, int M, int T, int H,
                                                          float* __restrict__ row_sq, float* __restrict__ dh, int dld,
                                                          float gscale) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= M) return;                                  // (whole waves leave; nothing below synchronises the workgroup)
  const int b = r / T, t = r - b * T;
  const long long st = start[b];
  const int cnt = count[b];
  const int n = min(cnt, T - first - 1);               // roco_utils.py:175-176
  const bool bad = st < 0 || cnt < 0 || st > table_rows - n;   // start + n_b > table_rows, without the overflow
  const bool has = !bad && t >= first && t < first + n;   // uniform over the wave
  const void* trow = nullptr;
  if (has) {
    const size_t off = (size_t)(st + (t - first)) * (size_t)H;
    trow = F16 ? (const void*)(static_cast<const __half*>(table) + off) : (const void*)(static_cast<const float*>(table) + off);
  }
  const float nan = __int_as_float(0x7fc00000);
  const float* x = h + (size_t)r * ld;
  float* d = dh ? dh + (size_t)r * dld : nullptr;
  float acc = 0.0f;
  if constexpr (VEC) {
#pragma unroll 2
    for (int k = lane * 4; k < H; k += 256) {
      const f32x4 u = *reinterpret_cast<const f32x4*>(x + k);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (has) v = dm_load4<F16>(trow, k);
      f32x4 e = u - v;
      if (bad) e = f32x4{nan, nan, nan, nan};
      acc = fmaf(e[0], e[0], acc);
      acc = fmaf(e[1], e[1], acc);
      acc = fmaf(e[2], e[2], acc);
      acc = fmaf(e[3], e[3], acc);
      if (d) *reinterpret_cast<f32x4*>(d + k) = e * gscale;
    }
  } else {
#pragma unroll 4
    for (int k = lane; k < H; k += 64) {
      float e = x[k] - (has ? dm_load1<F16>(trow, k) : 0.f);
      if (bad) e = nan;
      acc = fmaf(e, e, acc);
      if (d) d[k] = e * gscale;
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) row_sq[r] = bad ? nan : acc;
}

// loss = (sum of row_sq) / count: one workgroup, a fixed order of additions
__global__ void __launch_bounds__(256) distill_mean_kernel(const float* __restrict__ row_sq, float* __restrict__ loss, int rows,
                                                           double count) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < rows; i += 256) s += row_sq[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *loss = (float)((double)((red[0] + red[1]) + (red[2] + red[3])) / count);
}

extern "C" int mmvqa_distill_mse(mmvqa_stream_t s, const float* h, int ld, const void* table, int table_f16,
                                 long long table_rows, const long long* start, const int* count, int first, int B,
                                 int T, int H, float* row_sq, float* loss, float* dh, int dld, float gscale) {
  hipStream_t st = (hipStream_t)s;
  const char* who = "mmvqa_distill_mse";
  if (!h || !table || !start || !count || !row_sq || !loss)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: null operand (h, table, start, count, row_sq and loss are required)", who);
  if (B < 1 || T < 1 || H < 1 || table_rows < 1)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: B=%d T=%d H=%d table_rows=%lld (all >= 1)", who, B, T, H, table_rows);
  if (first < 0 || first >= T) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: first=%d outside [0, T=%d)", who, first, T);
  if (ld < H) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: ld=%d < H=%d", who, ld, H);
  if (dh && dld < H) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: dld=%d < H=%d", who, dld, H);
  if ((long long)B * T > 0x7fffffffLL / 4)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: B*T=%lld rows are more than one launch takes", who, (long long)B * T);
  const int M = B * T;
  const bool f16 = table_f16 != 0;
  // every table row starts at a multiple of H elements: a whole access needs H % 4 == 0 and an aligned base
  const bool vec = H % 4 == 0 && (ld & 3) == 0 && ((uintptr_t)h & 15) == 0 &&
                   (!dh || ((dld & 3) == 0 && ((uintptr_t)dh & 15) == 0)) && ((uintptr_t)table & (f16 ? 7 : 15)) == 0;
  auto kernel = vec ? (f16 ? distill_mse_kernel<true, true> : distill_mse_kernel<true, false>)
                    : (f16 ? distill_mse_kernel<false, true> : distill_mse_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, h, ld, table, table_rows, start, count, first,
                     M, T, H, row_sq, dh, dld, gscale);
  KERNEL_CHECK_RET();
  hipLaunchKernelGGL(distill_mean_kernel, dim3(1), dim3(256), 0, st, row_sq, loss, M, (double)M * (double)H);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}
