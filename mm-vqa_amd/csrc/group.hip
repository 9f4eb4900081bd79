// Grouped batches: NI images feed B >= NI questions, group[b] names the image of question b.
//   mmvqa_vis_expand     vis_q[t][b][:]  = vis_i[t][group[b]][:]                          (forward, before the embedding)
//   mmvqa_dvis_group_sum dvis_i[t][i][:] = sum of dvis_q[t][b][:] over offsets[i] <= b < offsets[i+1]   (backward, after it)
// Both are bandwidth kernels over a few hundred KB: one wave per row, 16-byte accesses along H, no LDS, no atomics.
#include "common.h"

namespace {

constexpr int GROUP_WAVES = 4;   // waves (rows) per workgroup

// one wave per (t, b)
__global__ __launch_bounds__(64 * GROUP_WAVES) void vis_expand_kernel(const float* __restrict__ vis_i,
                                                                      const int* __restrict__ group,
                                                                      float* __restrict__ vis_q, int NI, int B, int H4,
                                                                      int rows) {
  const int row = blockIdx.x * GROUP_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int t = row / B, b = row - t * B;
  const f32x4* src = reinterpret_cast<const f32x4*>(vis_i) + ((size_t)t * NI + group[b]) * H4;
  f32x4* dst = reinterpret_cast<f32x4*>(vis_q) + (size_t)row * H4;
  for (int v = lane; v < H4; v += 64) dst[v] = src[v];
}

// one wave per (t, i): the rows of image i are adjacent, added in ascending b starting FROM the first row -- the order
// and the operations of a sequential fp32 host loop, so the result is that loop's bit for bit
__global__ __launch_bounds__(64 * GROUP_WAVES) void dvis_group_sum_kernel(const float* __restrict__ dvis_q,
                                                                          const int* __restrict__ offsets,
                                                                          float* __restrict__ dvis_i, int NI, int B, int H4,
                                                                          int rows) {
  const int row = blockIdx.x * GROUP_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int t = row / NI, i = row - t * NI;
  const int b0 = offsets[i], b1 = offsets[i + 1];
  const f32x4* src = reinterpret_cast<const f32x4*>(dvis_q) + (size_t)t * B * H4;
  f32x4* dst = reinterpret_cast<f32x4*>(dvis_i) + (size_t)row * H4;
  for (int v = lane; v < H4; v += 64) {
    f32x4 acc = src[(size_t)b0 * H4 + v];
#pragma unroll 4
    for (int b = b0 + 1; b < b1; ++b) acc += src[(size_t)b * H4 + v];
    dst[v] = acc;
  }
}

int check_args(const char* who, const void* a, const void* idx, const void* c, int NI, int B, int H, int num_vis) {
  if (!a || !idx || !c) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: null pointer", who);
  if (NI < 1 || B < NI) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: NI=%d B=%d (1 <= NI <= B)", who, NI, B);
  if (H < 4 || H % 4 != 0) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: H=%d must be a positive multiple of 4", who, H);
  if (num_vis < 1) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: num_vis=%d", who, num_vis);
  if ((long long)num_vis * B > 0x7fffffffLL / GROUP_WAVES)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: num_vis=%d x B=%d rows are more than one launch takes", who, num_vis, B);
  return MMVQA_OK;
}

}  // namespace

extern "C" int mmvqa_vis_expand(mmvqa_stream_t s, const float* vis_i, const int* group, float* vis_q, int NI, int B, int H,
                                int num_vis) {
  TRY(check_args("vis_expand", vis_i, group, vis_q, NI, B, H, num_vis));
  const int rows = num_vis * B;
  hipLaunchKernelGGL(vis_expand_kernel, dim3((rows + GROUP_WAVES - 1) / GROUP_WAVES), dim3(64 * GROUP_WAVES), 0,
                     (hipStream_t)s, vis_i, group, vis_q, NI, B, H / 4, rows);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

extern "C" int mmvqa_dvis_group_sum(mmvqa_stream_t s, const float* dvis_q, const int* offsets, float* dvis_i, int NI, int B,
                                    int H, int num_vis) {
  TRY(check_args("dvis_group_sum", dvis_q, offsets, dvis_i, NI, B, H, num_vis));
  const int rows = num_vis * NI;
  hipLaunchKernelGGL(dvis_group_sum_kernel, dim3((rows + GROUP_WAVES - 1) / GROUP_WAVES), dim3(64 * GROUP_WAVES), 0,
                     (hipStream_t)s, dvis_q, offsets, dvis_i, NI, B, H / 4, rows);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}
