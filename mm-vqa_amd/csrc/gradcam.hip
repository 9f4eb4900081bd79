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
// Other attribution methods (vqamed2019/grad_cam.py:65-72) share everything after the channel
// weights: cam_kernel takes w[B][C] (or, for Eigen-CAM, the raw map [B][H*W]) from memory instead of the mean of dA.
//   cam_weights_kernel   w of gradcam / gradcam++ / xgradcam, one workgroup per sample, the column sums of cam_kernel
//   eigencam_kernel      first left singular vector of the column-centred A[b] by power iteration on its Gram matrix
//   ablated_tokens       the visual token of the deepest tap with one channel of A zeroed, a chunk of channels per launch
//   ablation_weights     w = (s - s_c) / s
#include "common.h"
#include "kernels.h"

#include <cstdlib>
#include <cstring>

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

enum { CAM_SRC_MEAN_DA = 0, CAM_SRC_W = 1, CAM_SRC_RAW = 2 };   // where cam_kernel's channel weights (or raw map) come from
enum { CAM_GRADCAM = 0, CAM_GRADCAMPP = 1, CAM_XGRADCAM = 2 };    // mmvqa_cam_weights' methods
constexpr int EIG_ITERS = 64;

// out[c] = scale * sum_p term(p, channel quad of c) for the whole workgroup (GC_THREADS threads): the positions are split
// over the position groups that share the workgroup, each quad is read 16 bytes per lane, and the groups' partial sums are
// added in group order.  part: GC_THREADS * 4 floats of LDS.  Ends with a barrier.
template <class F>
__device__ __forceinline__ void column_sums(float* part, float* out, int HW, int C, float scale, F term) {
  const int tid = threadIdx.x;
  const int nq = C >> 2;                   // channel quads, <= 1024
  const int npg = GC_THREADS / nq;         // position groups that share the workgroup
  const int q = tid % nq, pg = tid / nq;
  if (pg < npg) {
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int p = pg; p < HW; p += npg) s += term(p, q);
    reinterpret_cast<f32x4*>(part + (size_t)pg * C)[q] = s;
  }
  __syncthreads();
  for (int c = tid; c < C; c += GC_THREADS) {
    float s = 0.f;
    for (int g = 0; g < npg; ++g) s += part[g * C + c];
    out[c] = s * scale;
  }
  __syncthreads();
}

// src: dA [B][HW][C] (CAM_SRC_MEAN_DA), w [B][C] (CAM_SRC_W) or the raw map [B][HW] (CAM_SRC_RAW, A unused)
template <int SRC, bool FUSED>
__global__ __launch_bounds__(GC_THREADS) void gradcam_cam_kernel(const float* __restrict__ A, const float* __restrict__ src,
                                                                 float* __restrict__ cam_out, int* __restrict__ valid,
                                                                 int HW, int C, RenderArgs r) {
  __shared__ __attribute__((aligned(16))) float part[GC_THREADS * 4];   // [position group][C] partial sums of dA (16 KB whatever C is)
  __shared__ __attribute__((aligned(16))) float w[GC_MAX_C];
  __shared__ float cam[GC_MAX_HW];
  __shared__ float red[1];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nq = C >> 2;                   // channel quads, <= 1024
  const float* Ab = A + (size_t)b * HW * C;
  if (SRC == CAM_SRC_MEAN_DA) {  // w[c] = mean over positions of dA
    const float* dAb = src + (size_t)b * HW * C;
    column_sums(part, w, HW, C, 1.f / (float)HW,
                [&](int p, int q) { return reinterpret_cast<const f32x4*>(dAb + (size_t)p * C)[q]; });
  } else if (SRC == CAM_SRC_W) {
    for (int c = tid; c < C; c += GC_THREADS) w[c] = src[(size_t)b * C + c];
    __syncthreads();
  }
  // cam[p] = mean over channels of w[c] * A[p][c]: one wave per position, a wave reduction over the channels
  for (int p = wave; p < HW; p += GC_THREADS / 64) {
    if (SRC == CAM_SRC_RAW) {
      if (lane == 0) cam[p] = src[(size_t)b * HW + p];
      continue;
    }
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

// w[b][c] of one method, with S_c = sum_p A[b][p][c]:
//   gradcam    mean_p dA                        (the arithmetic and order of cam_kernel's own mean: bit-equal)
//   gradcam++  sum_p max(g, 0) * g^2 / (2 g^2 + S_c g^3 + 1e-7)   (0 where g == 0)
//   xgradcam   sum_p g * a / (S_c + 1e-7)
template <int METHOD>
__global__ __launch_bounds__(GC_THREADS) void cam_weights_kernel(const float* __restrict__ A, const float* __restrict__ dA,
                                                                 float* __restrict__ wout, int HW, int C) {
  __shared__ __attribute__((aligned(16))) float part[GC_THREADS * 4];
  __shared__ __attribute__((aligned(16))) float S[GC_MAX_C];
  __shared__ __attribute__((aligned(16))) float w[GC_MAX_C];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* dAb = dA + (size_t)b * HW * C;
  const float* Ab = A + (size_t)b * HW * C;
  if (METHOD == CAM_GRADCAM) {
    column_sums(part, w, HW, C, 1.f / (float)HW,
                [&](int p, int q) { return reinterpret_cast<const f32x4*>(dAb + (size_t)p * C)[q]; });
  } else {
    column_sums(part, S, HW, C, 1.f, [&](int p, int q) { return reinterpret_cast<const f32x4*>(Ab + (size_t)p * C)[q]; });
    column_sums(part, w, HW, C, 1.f, [&](int p, int q) {
      const f32x4 g = reinterpret_cast<const f32x4*>(dAb + (size_t)p * C)[q];
      f32x4 t;
      if (METHOD == CAM_GRADCAMPP) {
        const f32x4 sc = reinterpret_cast<const f32x4*>(S)[q];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float g2 = g[k] * g[k];
          const float alpha = g[k] != 0.f ? g2 / (2.f * g2 + sc[k] * g2 * g[k] + 1e-7f) : 0.f;
          t[k] = fmaxf(g[k], 0.f) * alpha;
        }
      } else {
        t = g * reinterpret_cast<const f32x4*>(Ab + (size_t)p * C)[q];
      }
      return t;
    });
  }
  for (int c = tid; c < C; c += GC_THREADS)
    wout[(size_t)b * C + c] = METHOD == CAM_XGRADCAM ? w[c] / (S[c] + 1e-7f) : w[c];
}

// Eigen-CAM's raw map: X = A[b] as [HW][C] with every column centred over the positions, raw = X v1 = sigma1 * u1 with
// u1 the first eigenvector of the Gram matrix G = X X^T [HW][HW].  G (up to 256 KB) lives in the caller's scratch, where the
// workgroup that wrote it re-reads it from L2 in each of the EIG_ITERS power iterations; only the vectors are in LDS.
// Start: the column of G with the largest diagonal entry (G 1 = 0: the centred columns rule out the vector of ones).
// Sign: the entry of largest magnitude is positive (ties: lowest position).  resid = |G u - lambda u| / lambda.
// X all zero, H*W = 1 or lambda <= 0: raw = 0 (cam_kernel then reports valid = 0) and resid = 0.
__global__ __launch_bounds__(GC_THREADS) void eigencam_kernel(const float* __restrict__ A, float* gram,
                                                              float* __restrict__ raw_out, float* __restrict__ resid_out,
                                                              int HW, int C) {
  __shared__ __attribute__((aligned(16))) float part[GC_THREADS * 4];
  __shared__ __attribute__((aligned(16))) float mean[GC_MAX_C];
  __shared__ float u[GC_MAX_HW];
  __shared__ float y[GC_MAX_HW];
  __shared__ float red[2];
  __shared__ int redi[1];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = GC_THREADS / 64;
  const int nq = C >> 2;
  const float* Ab = A + (size_t)b * HW * C;
  float* G = gram + (size_t)b * HW * HW;
  column_sums(part, mean, HW, C, 1.f / (float)HW,
              [&](int p, int q) { return reinterpret_cast<const f32x4*>(Ab + (size_t)p * C)[q]; });
  for (int i = wave; i < HW * HW; i += NW) {   // one wave per entry of the upper triangle, mirrored: G is exactly symmetric
    const int p = i / HW, q = i - p * HW;
    if (q < p) continue;
    float s = 0.f;
    for (int k = lane; k < nq; k += 64) {
      const f32x4 m = reinterpret_cast<const f32x4*>(mean)[k];
      const f32x4 xp = reinterpret_cast<const f32x4*>(Ab + (size_t)p * C)[k] - m;
      const f32x4 xq = reinterpret_cast<const f32x4*>(Ab + (size_t)q * C)[k] - m;
      s += xp[0] * xq[0] + xp[1] * xq[1] + xp[2] * xq[2] + xp[3] * xq[3];
    }
    s = wave_sum(s);
    if (lane == 0) { G[(size_t)p * HW + q] = s; G[(size_t)q * HW + p] = s; }
  }
  __syncthreads();
  if (wave == 0) {   // the largest diagonal entry, lowest position on ties
    float m = -1.f; int j = 0;
    for (int p = lane; p < HW; p += 64) { const float d = G[(size_t)p * HW + p]; if (d > m) { m = d; j = p; } }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float m2 = __shfl_xor(m, o, 64); const int j2 = __shfl_xor(j, o, 64);
      if (m2 > m || (m2 == m && j2 < j)) { m = m2; j = j2; }
    }
    if (lane == 0) { red[0] = m; redi[0] = j; }
  }
  __syncthreads();
  bool ok = HW > 1 && red[0] > 0.f;
  float lambda = 0.f, resid = 0.f;
  if (ok) {
    const int j = redi[0];
    for (int p = tid; p < HW; p += GC_THREADS) y[p] = G[(size_t)p * HW + j];
    __syncthreads();
    for (int it = 0; it <= EIG_ITERS && ok; ++it) {
      if (wave == 0) {   // u = y / |y|
        float n2 = 0.f;
        for (int p = lane; p < HW; p += 64) n2 += y[p] * y[p];
        n2 = wave_sum(n2);
        if (lane == 0) red[0] = sqrtf(n2);
      }
      __syncthreads();
      const float nrm = red[0];
      ok = nrm > 0.f;
      if (!ok) break;
      for (int p = tid; p < HW; p += GC_THREADS) u[p] = y[p] / nrm;
      __syncthreads();
      for (int p = wave; p < HW; p += NW) {   // y = G u: one wave per row (the last pass serves lambda and resid)
        float sacc = 0.f;
        for (int q = lane; q < HW; q += 64) sacc += G[(size_t)p * HW + q] * u[q];
        sacc = wave_sum(sacc);
        if (lane == 0) y[p] = sacc;
      }
      __syncthreads();
    }
  }
  if (ok) {
    if (wave == 0) {
      float l = 0.f;
      for (int p = lane; p < HW; p += 64) l += u[p] * y[p];
      l = wave_sum(l);
      float r2 = 0.f;
      for (int p = lane; p < HW; p += 64) { const float d = y[p] - l * u[p]; r2 += d * d; }
      r2 = wave_sum(r2);
      float m = -1.f; int j = 0;   // the entry of largest magnitude, lowest position on ties
      for (int p = lane; p < HW; p += 64) { const float d = fabsf(u[p]); if (d > m) { m = d; j = p; } }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64); const int j2 = __shfl_xor(j, o, 64);
        if (m2 > m || (m2 == m && j2 < j)) { m = m2; j = j2; }
      }
      if (lane == 0) { red[0] = l; red[1] = sqrtf(r2); redi[0] = j; }
    }
    __syncthreads();
    lambda = red[0];
    ok = lambda > 0.f;
    if (ok) resid = red[1] / lambda;
  }
  const float scale = ok ? (u[redi[0]] < 0.f ? -sqrtf(lambda) : sqrtf(lambda)) : 0.f;
  for (int p = tid; p < HW; p += GC_THREADS) raw_out[(size_t)b * HW + p] = ok ? scale * u[p] : 0.f;
  if (tid == 0) resid_out[b] = resid;
}

// tokens[b][j][n] = mean_p act(u[b][p][n] - W[n][c0 + j] * A[b][p][c0 + j]): the deepest tap's visual token with channel
// c0 + j of A zeroed (u = A W^T, the tap's 1x1 convolution without bias).  One workgroup per (channel, sample).
template <int ACT>
__global__ __launch_bounds__(256) void ablated_tokens_kernel(const float* __restrict__ A, const float* __restrict__ Wt,
                                                             const float* __restrict__ u, float* __restrict__ tokens,
                                                             int HW, int C, int hidden, int c0) {
  __shared__ float a[GC_MAX_HW];
  const int j = blockIdx.x, nc = gridDim.x, b = blockIdx.y, c = c0 + j;
  for (int p = threadIdx.x; p < HW; p += 256) a[p] = A[((size_t)b * HW + p) * C + c];
  __syncthreads();
  const float* ub = u + (size_t)b * HW * hidden;
  const float inv = 1.f / (float)HW;
  for (int n = threadIdx.x; n < hidden; n += 256) {
    const float wn = Wt[(size_t)n * C + c];
    float s = 0.f;
    for (int p = 0; p < HW; ++p) s += act_fwd(ACT, fmaf(-wn, a[p], ub[(size_t)p * hidden + n]));
    tokens[((size_t)b * nc + j) * hidden + n] = s * inv;
  }
}

// w[b][c] = (s[b] - s_c[b][c]) / s[b], zeros where s[b] == 0 (cam_kernel then reports valid = 0)
__global__ __launch_bounds__(256) void ablation_weights_kernel(const float* __restrict__ s, const float* __restrict__ sc,
                                                               float* __restrict__ w, int C) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float s0 = s[b];
  w[(size_t)b * C + c] = s0 != 0.f ? (s0 - sc[(size_t)b * C + c]) / s0 : 0.f;
}

// the argument checks that every entry point on a map [B][H][W][C] shares (what: the entry point's name)
int check_map(const char* what, int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || (long)H * W > GC_MAX_HW)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: B=%d, map %dx%d (at most %d positions)", what, B, H, W, GC_MAX_HW);
  if (C <= 0 || (C & 3) || C > GC_MAX_C)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: C=%d must be a multiple of 4, at most %d", what, C, GC_MAX_C);
  return MMVQA_OK;
}

int check_render(const char* what, float* up, int IH, int IW, const unsigned char* image_u8, const unsigned char* jet,
                 unsigned char* overlay) {
  const bool want_render = up != nullptr || overlay != nullptr;
  if (want_render && (IH <= 0 || IW <= 0 || (long)IH * IW > (1L << 26)))
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: output size %dx%d", what, IH, IW);
  if (overlay && (!image_u8 || !jet)) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: overlay needs image_u8 and the colour table", what);
  if (up && ((uintptr_t)up & 15)) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: up must be 16-byte aligned", what);
  if (overlay && (((uintptr_t)overlay | (uintptr_t)image_u8) & 3))
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: image_u8 / overlay must be 4-byte aligned", what);
  return MMVQA_OK;
}

// cam_kernel with its weights from SRC, then the render stage: a launch of its own by default (B workgroups cannot fill
// the chip with 50 176 pixels each), the tail of cam_kernel's workgroup under MMVQA_GRADCAM_FUSED=1 (A/B switch)
template <int SRC>
int launch_cam(hipStream_t st, const float* A, const float* src, int B, int HW, int C, float* cam, int* valid,
               const RenderArgs& r) {
  static const bool fused = getenv("MMVQA_GRADCAM_FUSED") != nullptr;
  const bool want_render = r.up != nullptr || r.overlay != nullptr;
  if (want_render && fused) {
    hipLaunchKernelGGL((gradcam_cam_kernel<SRC, true>), dim3(B), dim3(GC_THREADS), 0, st, A, src, cam, valid, HW, C, r);
    KERNEL_CHECK_RET();
    return MMVQA_OK;
  }
  hipLaunchKernelGGL((gradcam_cam_kernel<SRC, false>), dim3(B), dim3(GC_THREADS), 0, st, A, src, cam, valid, HW, C, r);
  KERNEL_CHECK_RET();
  if (want_render) {
    const int ngroups = (r.IH * r.IW + 3) / 4;
    int gx = (ngroups + 255) / 256;
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(gradcam_render_kernel, dim3(gx, B), dim3(256), 0, st, cam, valid, HW, r);
    KERNEL_CHECK_RET();
  }
  return MMVQA_OK;
}

}  // namespace

extern "C" int mmvqa_cam_weights(mmvqa_stream_t s, int method, const float* A, const float* dA, int B, int H, int W, int C,
                                 float* w) {
  if (method < CAM_GRADCAM || method > CAM_XGRADCAM)
    return mmvqa_set_error(MMVQA_ERR_ARG, "cam_weights: method=%d (0 = gradcam, 1 = gradcam++, 2 = xgradcam)", method);
  if (!A || !dA || !w) return mmvqa_set_error(MMVQA_ERR_ARG, "cam_weights: null A / dA / w");
  TRY(check_map("cam_weights", B, H, W, C));
  if ((((uintptr_t)A | (uintptr_t)dA) & 15) != 0) return mmvqa_set_error(MMVQA_ERR_ARG, "cam_weights: A / dA must be 16-byte aligned");
  hipStream_t st = (hipStream_t)s;
  const int HW = H * W;
  if (method == CAM_GRADCAM)
    hipLaunchKernelGGL(cam_weights_kernel<CAM_GRADCAM>, dim3(B), dim3(GC_THREADS), 0, st, A, dA, w, HW, C);
  else if (method == CAM_GRADCAMPP)
    hipLaunchKernelGGL(cam_weights_kernel<CAM_GRADCAMPP>, dim3(B), dim3(GC_THREADS), 0, st, A, dA, w, HW, C);
  else
    hipLaunchKernelGGL(cam_weights_kernel<CAM_XGRADCAM>, dim3(B), dim3(GC_THREADS), 0, st, A, dA, w, HW, C);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

extern "C" int mmvqa_cam_from_weights(mmvqa_stream_t s, const float* A, const float* w, const float* raw, int B, int H,
                                      int W, int C, float* cam, int* valid, float* up, int IH, int IW,
                                      const unsigned char* image_u8, const unsigned char* jet, float alpha,
                                      unsigned char* overlay) {
  if (!cam || !valid) return mmvqa_set_error(MMVQA_ERR_ARG, "cam_from_weights: null cam / valid");
  if ((w != nullptr) == (raw != nullptr))
    return mmvqa_set_error(MMVQA_ERR_ARG, "cam_from_weights: exactly one of w and raw must be given");
  if (w && !A) return mmvqa_set_error(MMVQA_ERR_ARG, "cam_from_weights: w needs A");
  TRY(check_map("cam_from_weights", B, H, W, C));
  if (w && ((uintptr_t)A & 15)) return mmvqa_set_error(MMVQA_ERR_ARG, "cam_from_weights: A must be 16-byte aligned");
  TRY(check_render("cam_from_weights", up, IH, IW, image_u8, jet, overlay));
  RenderArgs r{up, image_u8, jet, overlay, H, W, IH, IW, alpha};
  if (w) return launch_cam<CAM_SRC_W>((hipStream_t)s, A, w, B, H * W, C, cam, valid, r);
  return launch_cam<CAM_SRC_RAW>((hipStream_t)s, A, raw, B, H * W, C, cam, valid, r);
}

extern "C" int mmvqa_eigencam_raw(mmvqa_stream_t s, const float* A, int B, int H, int W, int C, float* gram, float* raw,
                                  float* resid) {
  if (!A || !gram || !raw || !resid) return mmvqa_set_error(MMVQA_ERR_ARG, "eigencam_raw: null A / gram / raw / resid");
  TRY(check_map("eigencam_raw", B, H, W, C));
  if ((uintptr_t)A & 15) return mmvqa_set_error(MMVQA_ERR_ARG, "eigencam_raw: A must be 16-byte aligned");
  hipLaunchKernelGGL(eigencam_kernel, dim3(B), dim3(GC_THREADS), 0, (hipStream_t)s, A, gram, raw, resid, H * W, C);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

extern "C" int mmvqa_ablated_tokens(mmvqa_stream_t s, const float* A, const float* Wt, float* u, int B, int HW, int C,
                                    int hidden, int act, int c0, int nc, int compute_u, float* tokens) {
  if (!A || !Wt || !u || !tokens) return mmvqa_set_error(MMVQA_ERR_ARG, "ablated_tokens: null A / W / u / tokens");
  TRY(check_map("ablated_tokens", B, HW, 1, C));
  if (B > 65535) return mmvqa_set_error(MMVQA_ERR_ARG, "ablated_tokens: B=%d (at most 65535)", B);
  if (hidden <= 0 || (hidden & 3)) return mmvqa_set_error(MMVQA_ERR_ARG, "ablated_tokens: hidden=%d must be a positive multiple of 4", hidden);
  if (act != ACT_RELU && act != ACT_SERF) return mmvqa_set_error(MMVQA_ERR_ARG, "ablated_tokens: act=%d (1 = ReLU, 3 = SERF)", act);
  if (c0 < 0 || nc < 1 || (long)c0 + nc > C)
    return mmvqa_set_error(MMVQA_ERR_ARG, "ablated_tokens: channels [%d, %d + %d) outside [0, %d)", c0, c0, nc, C);
  if ((((uintptr_t)A | (uintptr_t)Wt | (uintptr_t)u) & 15) != 0)
    return mmvqa_set_error(MMVQA_ERR_ARG, "ablated_tokens: A / W / u must be 16-byte aligned");
  hipStream_t st = (hipStream_t)s;
  if (compute_u) {   // u [B * HW][hidden] = A W^T, once per pass: the tap's 1x1 convolution as a plain product
    GemmParams g;
    memset(&g, 0, sizeof(g));
    g.g_SH = g.g_SW = g.g_OH = g.g_OW = 1;
    g.g_KH = g.g_KW = 1; g.g_stride = 1; g.g_pad = 0;
    g.M = B * HW; g.N = hidden; g.K = C;
    g.A = A; g.a_ld = C; g.g_Cs = C;
    g.B = Wt; g.b_ld = C;
    g.C = u; g.c_ld = hidden;
    TRY(mmvqa_launch_igemm(g, KIND_FWD, 0, 0, st));
  }
  if (act == ACT_RELU)
    hipLaunchKernelGGL(ablated_tokens_kernel<ACT_RELU>, dim3(nc, B), dim3(256), 0, st, A, Wt, u, tokens, HW, C, hidden, c0);
  else
    hipLaunchKernelGGL(ablated_tokens_kernel<ACT_SERF>, dim3(nc, B), dim3(256), 0, st, A, Wt, u, tokens, HW, C, hidden, c0);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

extern "C" int mmvqa_ablation_weights(mmvqa_stream_t s, const float* score, const float* score_abl, int B, int C, float* w) {
  if (!score || !score_abl || !w) return mmvqa_set_error(MMVQA_ERR_ARG, "ablation_weights: null score / score_abl / w");
  if (B <= 0 || B > 65535 || C <= 0) return mmvqa_set_error(MMVQA_ERR_ARG, "ablation_weights: B=%d C=%d", B, C);
  hipLaunchKernelGGL(ablation_weights_kernel, dim3((C + 255) / 256, B), dim3(256), 0, (hipStream_t)s, score, score_abl, w, C);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

extern "C" int mmvqa_gradcam(mmvqa_stream_t s, const float* A, const float* dA, int B, int H, int W, int C, float* cam,
                             int* valid, float* up, int IH, int IW, const unsigned char* image_u8,
                             const unsigned char* jet, float alpha, unsigned char* overlay) {
  if (!A || !dA || !cam || !valid) return mmvqa_set_error(MMVQA_ERR_ARG, "gradcam: null A / dA / cam / valid");
  TRY(check_map("gradcam", B, H, W, C));
  if ((((uintptr_t)A | (uintptr_t)dA) & 15) != 0) return mmvqa_set_error(MMVQA_ERR_ARG, "gradcam: A / dA must be 16-byte aligned");
  TRY(check_render("gradcam", up, IH, IW, image_u8, jet, overlay));
  RenderArgs r{up, image_u8, jet, overlay, H, W, IH, IW, alpha};
  return launch_cam<CAM_SRC_MEAN_DA>((hipStream_t)s, A, dA, B, H * W, C, cam, valid, r);
}
