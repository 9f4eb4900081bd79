// Loss scaling of mixed-precision training (mmvqa_amd.amp.GradScaler): the non-finite check of the flat gradient buffer
// with the optional in-place unscale, and the scale / growth-tracker update.  Same arithmetic as torch's
// _amp_foreach_non_finite_check_and_unscale_ and _amp_update_scale_ (CUDA kernels), so that a run with this scaler makes
// the same skip decisions and carries the same scale as one with torch.amp.GradScaler.
#include "kernels.h"

// found_inf = 1 if any g[i] is inf / nan (the flag is stored by the vector lane that saw it); g *= inv_scale when mul
__global__ __launch_bounds__(256) void amp_unscale_kernel(float* __restrict__ g, long n, const float* __restrict__ inv_scale,
                                                          float* __restrict__ found_inf, int mul) {
  const float s = mul ? *inv_scale : 1.f;
  bool bad = false;
  const long stride = (long)gridDim.x * 256 * 4;
  const bool vec = ((uintptr_t)g & 15) == 0;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride) {
    if (vec && i + 3 < n) {
      f32x4 v = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) bad |= !__builtin_isfinite(v[j]);
      if (mul) *reinterpret_cast<f32x4*>(g + i) = v * s;
    } else {
      for (long j = i; j < n && j < i + 4; ++j) {
        const float v = g[j];
        bad |= !__builtin_isfinite(v);
        if (mul) g[j] = v * s;
      }
    }
  }
  if (bad) *found_inf = 1.f;
}

__global__ void amp_update_scale_kernel(float* scale, int* growth_tracker, const float* found_inf, double growth_factor,
                                        double backoff_factor, int growth_interval) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (*found_inf) {
    *scale = (float)((double)*scale * backoff_factor);
    *growth_tracker = 0;
  } else {
    const int successful = *growth_tracker + 1;
    if (successful == growth_interval) {
      const float grown = (float)((double)*scale * growth_factor);
      if (__builtin_isfinite(grown)) *scale = grown;   // never grow past the fp32 range
      *growth_tracker = 0;
    } else {
      *growth_tracker = successful;
    }
  }
}

extern "C" int mmvqa_amp_unscale(mmvqa_stream_t s, float* g, long n, const float* inv_scale, float* found_inf,
                                 int mul) {
  hipStream_t st = (hipStream_t)s;
  if (!g || !found_inf || (mul && !inv_scale)) return mmvqa_set_error(MMVQA_ERR_ARG, "amp_unscale: null pointer");
  if (n <= 0) return MMVQA_OK;
  long blocks = (n + 1023) / 1024;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(amp_unscale_kernel, dim3((unsigned)blocks), dim3(256), 0, st, g, n, inv_scale, found_inf, mul);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

extern "C" int mmvqa_amp_update_scale(mmvqa_stream_t s, float* scale, int* growth_tracker, const float* found_inf,
                                      double growth_factor, double backoff_factor, int growth_interval) {
  hipStream_t st = (hipStream_t)s;
  if (!scale || !growth_tracker || !found_inf) return mmvqa_set_error(MMVQA_ERR_ARG, "amp_update_scale: null pointer");
  if (growth_interval <= 0) return mmvqa_set_error(MMVQA_ERR_ARG, "amp_update_scale: growth_interval=%d", growth_interval);
  hipLaunchKernelGGL(amp_update_scale_kernel, dim3(1), dim3(64), 0, st, scale, growth_tracker, found_inf, growth_factor,
                     backoff_factor, growth_interval);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}
