// Grad-CAM of the deepest backbone feature map (vqamed2019/grad_cam2.py:139-176, batched).
// Per sample b, with A and dA = d(sum dlogits*logits)/dA both NHWC [B][H*W][C] fp32:
//   w[c]   = mean_p dA[b][p][c]                    cam[p] = mean_c w[c] * A[b][p][c]
//   cam    = max(cam, 0) / max_p cam               (all zeros and valid[b] = 0 when max_p cam <= 0)
//   up     = bilinear resize of cam to [IH][IW]    (half-pixel centres, edge clamp)
//   q      = (uint8)(255 * up)                     overlay = clip(alpha * JET[q] + image_u8, 0, 255)   (the plain image where valid[b] = 0)
// cam_kernel: one 1024-thread workgroup per sample.  A and dA are read once, 16 bytes per lane along C; only w[C], the
// partial sums that produce it and cam[H*W] live in LDS (A of a ResNet sample is 401 KB: it never would fit).
// render: the resize + colour + blend stage, 4 consecutive pixels per thread, either as a second launch over
// (pixel groups, B) or as the tail of cam_kernel's workgroup (MMVQA_GRADCAM_FUSED=1, A/B switch).
#include "common.h"

#include <cstdlib>

namespace {

constexpr int GC_THREADS = 1024;
constexpr int GC_MAX_HW = 256;
constexpr int GC_MAX_C = 4096;

struct RenderArgs {
  float* up;                     // [B][IH*IW] or null
  const unsigned char* image;    // [B][IH*IW][3] or null
  const unsigned char* jet;      // [256][3]
  unsigned char* overlay;        // [B][IH*IW][3] or null
  int H, W, IH, IW;
  float alpha;
};

__device__ __forceinline__ void src_coord(int o, float scale, int n, int& i0, int& i1, float& f) {
  float s = ((float)o + 0.5f) * scale - 0.5f;
  if (s < 0.f) s = 0.f;
  int i = (int)s;            // s >= 0: truncation is floor
  f = s - (float)i;
  if (i >= n - 1) { i = n - 1; f = 0.f; }
  i0 = i;
  i1 = i + 1 < n ? i + 1 : n - 1;
}

__device__ __forceinline__ float bilinear(const float* cam, const RenderArgs& r, int pix) {
  const int y = pix / r.IW, x = pix - y * r.IW;
  int x0, x1, y0, y1;
  float fx, fy;
  src_coord(x, (float)r.W / (float)r.IW, r.W, x0, x1, fx);
  src_coord(y, (float)r.H / (float)r.IH, r.H, y0, y1, fy);
  const float top = (1.f - fx) * cam[y0 * r.W + x0] + fx * cam[y0 * r.W + x1];
  const float bot = (1.f - fx) * cam[y1 * r.W + x0] + fx * cam[y1 * r.W + x1];
  return (1.f - fy) * top + fy * bot;
}

__device__ __forceinline__ unsigned blend(const RenderArgs& r, float u, unsigned img, int ch, bool valid) {
  if (!valid) return img;     // no positive evidence: the plain image
  int q = (int)(255.f * u);   // u in [0, 1]: truncation, as np.uint8 does
  q = q < 0 ? 0 : (q > 255 ? 255 : q);
  // separately rounded multiply and add (no FMA contraction): the byte must equal the host formula's
  float v = __fadd_rn(__fmul_rn(r.alpha, (float)r.jet[q * 3 + ch]), (float)img);
  v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
  return (unsigned)v;
}

// pixels [4 * g, 4 * g + 4) of sample b for the groups g = g0, g0 + gstride, ... (cam: the sample's normalised map in LDS)
__device__ __forceinline__ void render(const float* cam, const RenderArgs& r, int b, int g0, int gstride, bool valid) {
  const int total = r.IH * r.IW;
  const int ngroups = (total + 3) >> 2;
  const bool vec = (total & 3) == 0;   // every sample's rows then start 16-byte (up) / 4-byte (overlay) aligned
  for (int g = g0; g < ngroups; g += gstride) {
    const int p0 = g * 4;
    float u[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = p0 + k < total ? bilinear(cam, r, p0 + k) : 0.f;
    const size_t base = (size_t)b * total + p0;
    if (r.up) {
      if (vec) *reinterpret_cast<f32x4*>(r.up + base) = f32x4{u[0], u[1], u[2], u[3]};
      else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (p0 + k < total) r.up[base + k] = u[k];
      }
    }
    if (r.overlay) {
      if (vec) {
        const uint3 in = *reinterpret_cast<const uint3*>(r.image + base * 3);
        const unsigned iw[3] = {in.x, in.y, in.z};
        unsigned ow[3] = {0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 12; ++j) {   // byte j of the 12: pixel j / 3, channel j % 3
          const unsigned byte = (iw[j >> 2] >> ((j & 3) * 8)) & 255u;
          ow[j >> 2] |= blend(r, u[j / 3], byte, j % 3, valid) << ((j & 3) * 8);
        }
        *reinterpret_cast<uint3*>(r.overlay + base * 3) = uint3{ow[0], ow[1], ow[2]};
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (p0 + k < total)
            for (int ch = 0; ch < 3; ++ch)
              r.overlay[(base + k) * 3 + ch] = (unsigned char)blend(r, u[k], r.image[(base + k) * 3 + ch], ch, valid);
      }
    }
  }
}

template <bool FUSED>
__global__ __launch_bounds__(GC_THREADS) void gradcam_cam_kernel(const float* __restrict__ A, const float* __restrict__ dA,
                                                                 float* __restrict__ cam_out, int* __restrict__ valid,
                                                                 int HW, int C, RenderArgs r) {
  __shared__ __attribute__((aligned(16))) float part[GC_THREADS * 4];   // [position group][C] partial sums of dA (16 KB whatever C is)
  __shared__ __attribute__((aligned(16))) float w[GC_MAX_C];
  __shared__ float cam[GC_MAX_HW];
  __shared__ float red[1];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nq = C >> 2;                   // channel quads, <= 1024
  const int npg = GC_THREADS / nq;         // position groups that share the workgroup
  const float* dAb = dA + (size_t)b * HW * C;
  const float* Ab = A + (size_t)b * HW * C;
  {  // w[c] = mean over positions of dA
    const int q = tid % nq, pg = tid / nq;
    if (pg < npg) {
      f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int p = pg; p < HW; p += npg) s += reinterpret_cast<const f32x4*>(dAb + (size_t)p * C)[q];
      reinterpret_cast<f32x4*>(part + (size_t)pg * C)[q] = s;
    }
    __syncthreads();
    const float inv = 1.f / (float)HW;
    for (int c = tid; c < C; c += GC_THREADS) {
      float s = 0.f;
      for (int g = 0; g < npg; ++g) s += part[g * C + c];
      w[c] = s * inv;
    }
    __syncthreads();
  }
  // cam[p] = mean over channels of w[c] * A[p][c]: one wave per position, a wave reduction over the channels
  for (int p = wave; p < HW; p += GC_THREADS / 64) {
    float s = 0.f;
    for (int q = lane; q < nq; q += 64) {
      const f32x4 a = reinterpret_cast<const f32x4*>(Ab + (size_t)p * C)[q];
      const f32x4 ww = reinterpret_cast<const f32x4*>(w)[q];
      s += a[0] * ww[0] + a[1] * ww[1] + a[2] * ww[2] + a[3] * ww[3];
    }
    s = wave_sum(s);
    if (lane == 0) cam[p] = s / (float)C;
  }
  __syncthreads();
  if (wave == 0) {   // max over the (<= 256) positions
    float m = -3.0e38f;
    for (int p = lane; p < HW; p += 64) m = fmaxf(m, cam[p]);
    m = wave_max(m);
    if (lane == 0) { red[0] = m; valid[b] = m > 0.f ? 1 : 0; }
  }
  __syncthreads();
  const float m = red[0];
  for (int p = tid; p < HW; p += GC_THREADS) {
    const float v = m > 0.f ? fmaxf(cam[p], 0.f) / m : 0.f;   // (a division: the maximum becomes exactly 1)
    cam[p] = v;
    cam_out[(size_t)b * HW + p] = v;
  }
  if (FUSED) {
    __syncthreads();
    render(cam, r, b, tid, GC_THREADS, m > 0.f);
  }
}

__global__ __launch_bounds__(256) void gradcam_render_kernel(const float* __restrict__ cam_in, const int* __restrict__ valid,
                                                             int HW, RenderArgs r) {
  __shared__ float cam[GC_MAX_HW];
  const int b = blockIdx.y;
  for (int p = threadIdx.x; p < HW; p += 256) cam[p] = cam_in[(size_t)b * HW + p];
  __syncthreads();
  render(cam, r, b, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256, valid[b] != 0);
}

}  // namespace

extern "C" int mmvqa_gradcam(mmvqa_stream_t s, const float* A, const float* dA, int B, int H, int W, int C, float* cam,
                             int* valid, float* up, int IH, int IW, const unsigned char* image_u8,
                             const unsigned char* jet, float alpha, unsigned char* overlay) {
  if (!A || !dA || !cam || !valid) return mmvqa_set_error(MMVQA_ERR_ARG, "gradcam: null A / dA / cam / valid");
  if (B <= 0 || H <= 0 || W <= 0 || (long)H * W > GC_MAX_HW)
    return mmvqa_set_error(MMVQA_ERR_ARG, "gradcam: B=%d, map %dx%d (at most %d positions)", B, H, W, GC_MAX_HW);
  if (C <= 0 || (C & 3) || C > GC_MAX_C)
    return mmvqa_set_error(MMVQA_ERR_ARG, "gradcam: C=%d must be a multiple of 4, at most %d", C, GC_MAX_C);
  if ((((uintptr_t)A | (uintptr_t)dA) & 15) != 0) return mmvqa_set_error(MMVQA_ERR_ARG, "gradcam: A / dA must be 16-byte aligned");
  const bool want_render = up != nullptr || overlay != nullptr;
  if (want_render && (IH <= 0 || IW <= 0 || (long)IH * IW > (1L << 26)))
    return mmvqa_set_error(MMVQA_ERR_ARG, "gradcam: output size %dx%d", IH, IW);
  if (overlay && (!image_u8 || !jet)) return mmvqa_set_error(MMVQA_ERR_ARG, "gradcam: overlay needs image_u8 and the colour table");
  if (up && ((uintptr_t)up & 15)) return mmvqa_set_error(MMVQA_ERR_ARG, "gradcam: up must be 16-byte aligned");
  if (overlay && (((uintptr_t)overlay | (uintptr_t)image_u8) & 3))
    return mmvqa_set_error(MMVQA_ERR_ARG, "gradcam: image_u8 / overlay must be 4-byte aligned");
  hipStream_t st = (hipStream_t)s;
  RenderArgs r{up, image_u8, jet, overlay, H, W, IH, IW, alpha};
  // default: the render stage as a launch of its own (B workgroups cannot fill the chip with 50 176 pixels each)
  static const bool fused = getenv("MMVQA_GRADCAM_FUSED") != nullptr;   // A/B switch
  const int HW = H * W;
  if (want_render && fused) {
    hipLaunchKernelGGL(gradcam_cam_kernel<true>, dim3(B), dim3(GC_THREADS), 0, st, A, dA, cam, valid, HW, C, r);
    KERNEL_CHECK_RET();
    return MMVQA_OK;
  }
  hipLaunchKernelGGL(gradcam_cam_kernel<false>, dim3(B), dim3(GC_THREADS), 0, st, A, dA, cam, valid, HW, C, r);
  KERNEL_CHECK_RET();
  if (want_render) {
    const int ngroups = (IH * IW + 3) / 4;
    int gx = (ngroups + 255) / 256;
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(gradcam_render_kernel, dim3(gx, B), dim3(256), 0, st, cam, valid, HW, r);
    KERNEL_CHECK_RET();
  }
  return MMVQA_OK;
}
