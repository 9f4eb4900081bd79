// SupCon / SimCLR loss (models/SupConLoss/loss.py:21-98, contrast_mode 'all', two views), forward and gradient,
// without a mask (the other view is the only positive) and with a positive mask (loss.py:45-55,76-96).
// features f [R=2N, D] ordered view-major (cat(unbind(features,1)), loss.py:57): positive of r is (r+N) mod 2N.
// Tiled over row blocks so that the all-gathered view set of a data-parallel job (R = 2N*world, SURVEY 8(e)
// collective 2) runs at any size: a workgroup owns SC_ROWS anchor rows and walks the contrast rows in tiles of
// 64 staged in LDS (lane = contrast row, so a score never leaves its register); nothing of size R*R exists.
//   pass 1 (supcon_rows_kernel): z = f f^T / T (loss.py:70-72), row max over ALL columns incl. the diagonal
//     (:74-75), log sum of exp over the columns != row (:88-89) -> lse[r], row_loss[r] = -(z[r,pos] - lse[r]) (:92-95)
//   pass 2 (supcon_grad_kernel): dL/dz[a][b] = c (p_a[b] - [b = pos a]) with p_a = softmax over b != a; z and the
//     positive map are symmetric, so df[a] = c/T * sum_b (p_a[b] + p_b[a] - 2 [b = pos a]) f[b]: scores recomputed.
//   pass 3 (supcon_reduce_kernel): loss = (T/T_base) * mean_r row_loss[r] (:95-96), fixed summation order.
// With a mask (MASKED) the caller's m [N][N] (fp32, any weights, may be asymmetric) is read tiled 2x2 with the diagonal
// of the tiling zeroed (loss.py:77-85): mt[a][b] = m[a mod N][b mod N] for b != a, 0 on b == a.  The mask is the only
// R*R-shaped thing read and nothing of that shape is written.
//   pass 1: lse[a] as above; M[a] = sum_b mt[a][b]; S[a] = sum_b mt[a][b] (z[a][b] - z[a][a]) (the anchor's own score
//     is the shift: it is the row maximum of unit-norm features, and it keeps the weighted sum small next to lse);
//     row_loss[a] = -(S[a] / M[a] + z[a][a] - lse[a]) (:92-95).  M[a] == 0 divides 0 by 0: NaN, as the reference's
//     (mask * log_prob).sum(1) / mask.sum(1).
//   pass 2: dL/dz[a][b] = c (p_a[b] - mt[a][b] / M[a]); the mask is not symmetric, so the weight of f[b] in df[a] is
//     p_a[b] + p_b[a] - mt[a][b] / M[a] - mt[b][a] / M[b]: M of every row comes from pass 1.
//   pass 3: the same reduce.
// Both forms are one template each; only the lines that differ sit under `if constexpr (MASKED)`, and every
// floating-point expression keeps the operands and the order it had when the two forms were separate kernels.
// The score loop stands in both kernels and not in a helper they share: behind a helper the compiler issues the
// loop's five LDS reads in two groups instead of one, and forward + gradient measured 6-7 % slower.
#include "common.h"
#include "kernels.h"

#define SC_ROWS 16
#define SC_COLS 64
#define SC_MAXD 256

__device__ __forceinline__ void sc_stage(float* dst, int dst_ld, const float* __restrict__ f, int row0, int nrows,
                                         int R, int D) {
  for (int i = threadIdx.x; i < nrows * D; i += blockDim.x) {
    const int r = i / D, k = i - r * D;
    dst[r * dst_ld + k] = (row0 + r < R) ? f[(size_t)(row0 + r) * D + k] : 0.f;
  }
}
__device__ __forceinline__ float sc_mask_at(const float* __restrict__ mk, int N, int a, int b) {
  return a == b ? 0.f : mk[(size_t)(a >= N ? a - N : a) * N + (b >= N ? b - N : b)];
}

// mk and msum are read / written only when MASKED
template <bool MASKED>
__global__ void __launch_bounds__(256) supcon_rows_kernel(const float* __restrict__ f, const float* __restrict__ mk,
                                                          float* __restrict__ lse, float* __restrict__ row_loss,
                                                          float* __restrict__ msum, int N, int D, float temp) {
  extern __shared__ float sm[];
  const int R = 2 * N, ldb = D + 1;
  float* fa = sm;                      // [SC_ROWS][D]   anchors of this workgroup
  float* fb = sm + SC_ROWS * D;        // [SC_COLS][D+1] contrast tile (odd stride: lane = row reads conflict-free)
  const int a0 = blockIdx.x * SC_ROWS, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  sc_stage(fa, D, f, a0, SC_ROWS, R, D);
  float m[4], s[4];
  float zp[4];                         // unmasked: score of the positive
  float ms[4], mz[4], zd[4];           // masked: sum of weights, weighted sum of z - z[a][a], z[a][a]
  if constexpr (MASKED) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float q = 0.f;
      for (int k = lane; k < D; k += 64) { const float v = fa[(wave * 4 + r) * D + k]; q += v * v; }
      zd[r] = wave_sum(q) / temp;
      m[r] = -INFINITY; s[r] = 0.f; ms[r] = 0.f; mz[r] = 0.f;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; s[r] = 0.f; zp[r] = 0.f; }
  }
  for (int b0 = 0; b0 < R; b0 += SC_COLS) {
    __syncthreads();
    sc_stage(fb, ldb, f, b0, SC_COLS, R, D);
    __syncthreads();
    const int b = b0 + lane;
    float dot[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < D; ++k) {
      const float vb = fb[lane * ldb + k];
#pragma unroll
      for (int r = 0; r < 4; ++r) dot[r] += fa[(wave * 4 + r) * D + k] * vb;
    }
    if (b < R) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int a = a0 + wave * 4 + r;
        const float z = dot[r] / temp;
        const float mn = fmaxf(m[r], z);                 // the diagonal takes part in the max, not in the sum
        s[r] = s[r] * __expf(m[r] - mn) + (b != a ? __expf(z - mn) : 0.f);
        m[r] = mn;
        if constexpr (MASKED) {
          if (a < R) {
            const float w = sc_mask_at(mk, N, a, b);
            ms[r] += w;
            mz[r] += w * (z - zd[r]);
          }
        } else {
          if (b == (a + N) % R) zp[r] = z;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int a = a0 + wave * 4 + r;
    const float M = wave_max(m[r]);
    const float S = wave_sum(m[r] == -INFINITY ? 0.f : s[r] * __expf(m[r] - M));
    if constexpr (MASKED) {
      const float W = wave_sum(ms[r]), WZ = wave_sum(mz[r]);
      if (lane == 0 && a < R) {
        const float l = M + logf(S);
        lse[a] = l;
        msum[a] = W;
        row_loss[a] = -(WZ / W + (zd[r] - l));
      }
    } else {
      const float Z = wave_sum(zp[r]);
      if (lane == 0 && a < R) {
        const float l = M + logf(S);
        lse[a] = l;
        row_loss[a] = -(Z - l);
      }
    }
  }
}

// mk and msum are read only when MASKED
template <bool MASKED>
__global__ void __launch_bounds__(256) supcon_grad_kernel(const float* __restrict__ f, const float* __restrict__ mk,
                                                          const float* __restrict__ lse,
                                                          const float* __restrict__ msum, float* __restrict__ df,
                                                          int N, int D, float temp, float cscale) {
  extern __shared__ float sm[];
  const int R = 2 * N, ldb = D + 1;
  float* fa = sm;                               // [SC_ROWS][D]
  float* fb = fa + SC_ROWS * D;                 // [SC_COLS][D+1]
  float* w = fb + SC_COLS * ldb;                // [SC_ROWS][SC_COLS] gradient weights of the current tile
  const int a0 = blockIdx.x * SC_ROWS, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  sc_stage(fa, D, f, a0, SC_ROWS, R, D);
  float lse_a[4], M_a[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int a = a0 + wave * 4 + r;
    lse_a[r] = a < R ? lse[a] : 0.f;
    if constexpr (MASKED) M_a[r] = a < R ? msum[a] : 1.f;
  }
  float acc[SC_ROWS * SC_MAXD / 256];
#pragma unroll
  for (int j = 0; j < SC_ROWS * SC_MAXD / 256; ++j) acc[j] = 0.f;
  for (int b0 = 0; b0 < R; b0 += SC_COLS) {
    __syncthreads();
    sc_stage(fb, ldb, f, b0, SC_COLS, R, D);
    __syncthreads();
    const int b = b0 + lane;
    float dot[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < D; ++k) {
      const float vb = fb[lane * ldb + k];
#pragma unroll
      for (int r = 0; r < 4; ++r) dot[r] += fa[(wave * 4 + r) * D + k] * vb;
    }
    const float lse_b = b < R ? lse[b] : 0.f;
    float M_b = 1.f;
    if constexpr (MASKED) M_b = b < R ? msum[b] : 1.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = a0 + wave * 4 + r;
      float g = 0.f;
      if (b < R && a < R && b != a) {
        const float z = dot[r] / temp;
        if constexpr (MASKED)
          g = __expf(z - lse_a[r]) + __expf(z - lse_b) - sc_mask_at(mk, N, a, b) / M_a[r] - sc_mask_at(mk, N, b, a) / M_b;
        else
          g = __expf(z - lse_a[r]) + __expf(z - lse_b) - (b == (a + N) % R ? 2.f : 0.f);
      }
      w[(wave * 4 + r) * SC_COLS + lane] = g;
    }
    __syncthreads();
    // The masked form unrolls the inner product by 8, not by 64: fully unrolled, the 64 row offsets c * ldb of the
    // tile are loop invariants that each take a scalar register and push the kernel's scalar file over its limit.
    // The unmasked form keeps the full unroll it has always had (it parks those values in VGPR lanes instead).
    constexpr int unroll_c = MASKED ? 8 : SC_COLS;
#pragma unroll
    for (int j = 0; j < SC_ROWS * SC_MAXD / 256; ++j) {
      const int i = threadIdx.x + j * 256;
      if (i < SC_ROWS * D) {
        const int r = i / D, k = i - r * D;
        float t = 0.f;
#pragma unroll unroll_c
        for (int c = 0; c < SC_COLS; ++c) t += w[r * SC_COLS + c] * fb[c * ldb + k];
        acc[j] += t;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < SC_ROWS * SC_MAXD / 256; ++j) {
    const int i = threadIdx.x + j * 256;
    if (i < SC_ROWS * D) {
      const int r = i / D, k = i - r * D;
      if (a0 + r < R) df[(size_t)(a0 + r) * D + k] = acc[j] * cscale;
    }
  }
}

__global__ void supcon_reduce_kernel(const float* __restrict__ row_loss, float* __restrict__ loss_out, int R,
                                     float coef) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < R; i += blockDim.x) s += row_loss[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *loss_out = coef * (red[0] + red[1] + red[2] + red[3]) / (float)R;
}

// mask == nullptr: the unmasked kernels, ws = 4*N floats (lse, row losses); otherwise the masked ones, ws = 6*N floats
// (2*N more: the mask row sums).  Every argument is checked before the first HIP call.
static int supcon(hipStream_t st, const float* f, const float* mask, float* loss, float* df, float* ws, int N, int D,
                  float temp, float base_temp, float gscale) {
  const char* who = mask ? "supcon_masked" : "supcon";
  if (!f) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: f is null", who);
  if (!loss) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: loss is null", who);
  if (!ws)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: ws is null (workspace of %d*N floats required: lse, row losses%s)", who,
                           mask ? 6 : 4, mask ? ", mask row sums" : "");
  if (N < 1) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: N=%d (N >= 1)", who, N);
  if (D < 1 || D > SC_MAXD) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: D=%d (1 <= D <= %d)", who, D, SC_MAXD);
  const int R = 2 * N;
  float* lse = ws;
  float* row_loss = ws + R;
  float* msum = mask ? ws + 2 * R : nullptr;
  auto rows_kernel = mask ? supcon_rows_kernel<true> : supcon_rows_kernel<false>;
  auto grad_kernel = mask ? supcon_grad_kernel<true> : supcon_grad_kernel<false>;
  const int blocks = (R + SC_ROWS - 1) / SC_ROWS;
  const size_t sm1 = ((size_t)SC_ROWS * D + (size_t)SC_COLS * (D + 1)) * sizeof(float);
  const size_t sm2 = sm1 + (size_t)SC_ROWS * SC_COLS * sizeof(float);
  if (sm2 > 48 * 1024) {
    HIP_CHECK_RET(hipFuncSetAttribute((const void*)rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm1));
    HIP_CHECK_RET(hipFuncSetAttribute((const void*)grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm2));
  }
  hipLaunchKernelGGL(rows_kernel, dim3(blocks), dim3(256), sm1, st, f, mask, lse, row_loss, msum, N, D, temp);
  KERNEL_CHECK_RET();
  const float coef = temp / base_temp;
  if (df) {
    hipLaunchKernelGGL(grad_kernel, dim3(blocks), dim3(256), sm2, st, f, mask, lse, (const float*)msum, df, N, D, temp,
                       coef / (float)R / temp * gscale);
    KERNEL_CHECK_RET();
  }
  hipLaunchKernelGGL(supcon_reduce_kernel, dim3(1), dim3(256), 0, st, row_loss, loss, R, coef);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

extern "C" int mmvqa_supcon_loss(mmvqa_stream_t s, const float* f, float* loss, float* df, float* ws, int N, int D, float temp,
                                 float base_temp, float gscale) {
  return supcon((hipStream_t)s, f, nullptr, loss, df, ws, N, D, temp, base_temp, gscale);
}
extern "C" int mmvqa_supcon_loss_masked(mmvqa_stream_t s, const float* f, const float* mask, float* loss, float* df, float* ws,
                                        int N, int D, float temp, float base_temp, float gscale) {
  // a null mask is refused here: to the launcher it would mean the unmasked loss
  if (!mask) return mmvqa_set_error(MMVQA_ERR_ARG, "supcon_masked: mask is null (mmvqa_supcon_loss is the loss without one)");
  return supcon((hipStream_t)s, f, mask, loss, df, ws, N, D, temp, base_temp, gscale);
}
