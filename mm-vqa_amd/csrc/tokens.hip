// The visual-token cache: one fp32 device array cache[N][K][num_vis][H] (N images, K views of each).
//   mmvqa_tokens_gather  out[t][b][:]                = cache[idx[b]][view[b]][t][:]   (the engine's [num_vis][B][H] layout)
//   mmvqa_tokens_scatter cache[idx[b]][view][t][:]   = vis[t][b][:]                   (its inverse; one view, distinct idx)
// Pure copies of a few hundred KB: one wave per (t, b) row, 16-byte accesses along H, no LDS, no atomics.  Neither kernel
// range-checks idx or view: the caller validates them on the host before they are uploaded.
#include "common.h"

namespace {

constexpr int TOKEN_WAVES = 4;   // waves (rows) per workgroup

// element offset, in 16-byte units, of cache[i][v][t][0]
__device__ __forceinline__ size_t cache_row(int i, int v, int t, int K, int num_vis, int H4) {
  return (((size_t)i * K + v) * num_vis + t) * H4;
}

__global__ __launch_bounds__(64 * TOKEN_WAVES) void tokens_gather_kernel(const float* __restrict__ cache,
                                                                         const int* __restrict__ idx,
                                                                         const int* __restrict__ view,
                                                                         float* __restrict__ out, int K, int B, int H4,
                                                                         int num_vis, int rows) {
  const int row = blockIdx.x * TOKEN_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int t = row / B, b = row - t * B;
  const f32x4* src = reinterpret_cast<const f32x4*>(cache) + cache_row(idx[b], view[b], t, K, num_vis, H4);
  f32x4* dst = reinterpret_cast<f32x4*>(out) + (size_t)row * H4;
  for (int v = lane; v < H4; v += 64) dst[v] = src[v];
}

__global__ __launch_bounds__(64 * TOKEN_WAVES) void tokens_scatter_kernel(const float* __restrict__ vis,
                                                                          const int* __restrict__ idx, int view,
                                                                          float* __restrict__ cache, int K, int B, int H4,
                                                                          int num_vis, int rows) {
  const int row = blockIdx.x * TOKEN_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int t = row / B, b = row - t * B;
  const f32x4* src = reinterpret_cast<const f32x4*>(vis) + (size_t)row * H4;
  f32x4* dst = reinterpret_cast<f32x4*>(cache) + cache_row(idx[b], view, t, K, num_vis, H4);
  for (int v = lane; v < H4; v += 64) dst[v] = src[v];
}

int check_args(const char* who, const void* cache, const void* idx, const void* rows_buf, int N, int K, int B, int H,
               int num_vis) {
  if (!cache || !idx || !rows_buf) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: null pointer", who);
  if (H < 8 || H % 8 != 0 || H > 1024)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: hidden=%d must be a multiple of 8, at most 1024", who, H);
  if (B < 1 || N < 1 || K < 1 || num_vis < 1)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: B=%d N=%d K=%d num_vis=%d must all be at least 1", who, B, N, K, num_vis);
  if ((long long)num_vis * B > 0x7fffffffLL / TOKEN_WAVES)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: num_vis=%d x B=%d rows are more than one launch takes", who, num_vis, B);
  if (((uintptr_t)cache | (uintptr_t)rows_buf) & 15)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: cache and token rows must be 16-byte aligned", who);
  return MMVQA_OK;
}

}  // namespace

extern "C" int mmvqa_tokens_gather(mmvqa_stream_t s, const float* cache, int N, int K, const int* idx, const int* view,
                                   float* out, int B, int hidden, int num_vis) {
  TRY(check_args("tokens_gather", cache, idx, out, N, K, B, hidden, num_vis));
  if (!view) return mmvqa_set_error(MMVQA_ERR_ARG, "tokens_gather: null pointer");
  const int rows = num_vis * B;
  hipLaunchKernelGGL(tokens_gather_kernel, dim3((rows + TOKEN_WAVES - 1) / TOKEN_WAVES), dim3(64 * TOKEN_WAVES), 0,
                     (hipStream_t)s, cache, idx, view, out, K, B, hidden / 4, num_vis, rows);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

extern "C" int mmvqa_tokens_scatter(mmvqa_stream_t s, const float* vis, const int* idx, int view, float* cache, int N,
                                    int K, int B, int hidden, int num_vis) {
  TRY(check_args("tokens_scatter", cache, idx, vis, N, K, B, hidden, num_vis));
  if (view < 0 || view >= K) return mmvqa_set_error(MMVQA_ERR_ARG, "tokens_scatter: view=%d is outside 0 .. K-1 = %d", view, K - 1);
  const int rows = num_vis * B;
  hipLaunchKernelGGL(tokens_scatter_kernel, dim3((rows + TOKEN_WAVES - 1) / TOKEN_WAVES), dim3(64 * TOKEN_WAVES), 0,
                     (hipStream_t)s, vis, idx, view, cache, K, B, hidden / 4, num_vis, rows);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}
