// Device input pipeline: the image transforms of the reference's data layer
//   pretrain/roco_train.py:98-112, vqamed2019/train.py:179-200
//     Resize(224) -> CenterCrop(224) -> RandomResizedCrop -> RandomRotation -> ColorJitter -> ToTensor -> Normalize
// on decoded uint8 RGB images resident in HBM.  The reference runs them per sample on the host through
// torchvision's PIL backend, i.e. the pixel arithmetic is Pillow's C code; these kernels restate that arithmetic
// bit for bit (byte / integer work: the bar is bit-exact, tests/test_augment.py compares with Pillow itself):
//   resample   ImagingResample (src/libImaging/Resample.c): separable convolution with the bilinear (triangle)
//              filter whose support grows with the down-scale factor (anti-aliasing), coefficients normalised
//              and quantised to 22 fractional bits, 32-bit integer accumulation, horizontal pass then vertical
//   rotate     Image.rotate(..., NEAREST) -> ImagingTransformAffine -> affine_fixed (src/libImaging/Geometry.c):
//              16.16 fixed-point inverse mapping, black fill
//   colour     ImageEnhance.{Brightness, Contrast, Color} = ImagingBlend with a degenerate image (Blend.c: fp32
//              interpolate, truncate / clip), L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 (Convert.c),
//              hue = RGB -> HSV -> H += shift (uint8 wrap) -> RGB (Convert.c rgb2hsv_row / hsv2rgb, double maths)
//   to_tensor  ToTensor (x / 255) + Normalize ((x - mean) / std) into fp32 NCHW
// All of it is HBM-bound byte work: one thread per output pixel (3 channels), rows contiguous across lanes.
// This file is compiled with -ffp-contract=off: Pillow's results depend on separately rounded multiplies and adds.
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "common.h"

typedef unsigned char u8;

// --------------------------------------------------------------------------- coefficients (host, Resample.c precompute_coeffs)
// Bilinear filter, support 1.  bounds[2*i] = first source index, bounds[2*i+1] = tap count of output i;
// kk[i*ksize + k] = round(w_k * 2^22).  Returns ksize (taps allocated per output), or a negative error.
extern "C" int mmvqa_resample_coeffs(int in_size, double in0, double in1, int out_size, int* bounds, int* kk,
                                     int ksize_cap) {
  if (in_size <= 0 || out_size <= 0 || !(in1 > in0)) return mmvqa_set_error(MMVQA_ERR_ARG, "resample_coeffs: bad sizes");
  const double scale = (in1 - in0) / out_size;
  double filterscale = scale;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = 1.0 * filterscale;
  const int ksize = (int)ceil(support) * 2 + 1;
  if (!bounds || !kk) return ksize;                       // size query
  if (ksize > ksize_cap) return mmvqa_set_error(MMVQA_ERR_ARG, "resample_coeffs: ksize %d > cap %d", ksize, ksize_cap);
  const double ss = 1.0 / filterscale;
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = in0 + (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double w[64];
    if (ksize > 64) return mmvqa_set_error(MMVQA_ERR_ARG, "resample_coeffs: down-scale factor too large (ksize %d)", ksize);
    int x = 0;
    for (; x < xmax; ++x) {
      double a = (x + xmin - center + 0.5) * ss;
      if (a < 0.0) a = -a;
      const double v = a < 1.0 ? 1.0 - a : 0.0;
      w[x] = v;
      ww += v;
    }
    for (x = 0; x < xmax; ++x)
      if (ww != 0.0) w[x] /= ww;
    for (; x < ksize; ++x) w[x] = 0.0;
    for (x = 0; x < ksize; ++x)
      kk[xx * ksize + x] = w[x] < 0 ? (int)(-0.5 + w[x] * (1 << 22)) : (int)(0.5 + w[x] * (1 << 22));
    bounds[xx * 2] = xmin;
    bounds[xx * 2 + 1] = xmax;
  }
  return ksize;
}

// --------------------------------------------------------------------------- resample
__device__ __forceinline__ u8 clip8_22(int v) {
  v >>= 22;
  return (u8)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// horizontal pass of job blockIdx.z: tmp[y - ty0][x][c] for y in [ty0, ty0 + tyn), x in [0, out_w)
__global__ __launch_bounds__(256) void resample_h_kernel(const mmvqa_resample_job* __restrict__ jobs, int out_w) {
  const mmvqa_resample_job j = jobs[blockIdx.z];
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), yl = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= out_w || yl >= j.tyn) return;
  const int xo = j.ox + x;                           // column of the resized image
  const int xmin = j.hb[xo * 2], xn = j.hb[xo * 2 + 1];
  const int* k = j.hk + (size_t)xo * j.hks;
  const u8* row = j.src + (size_t)(j.by + j.ty0 + yl) * j.spitch + (size_t)(j.bx + xmin) * 3;
  int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
  for (int t = 0; t < xn; ++t) {
    const int c = k[t];
    s0 += (int)row[t * 3] * c; s1 += (int)row[t * 3 + 1] * c; s2 += (int)row[t * 3 + 2] * c;
  }
  u8* o = j.tmp + ((size_t)yl * out_w + x) * 3;
  o[0] = clip8_22(s0); o[1] = clip8_22(s1); o[2] = clip8_22(s2);
}

// vertical pass: dst[y][x][c] for y in [0, out_h), x in [0, out_w)
__global__ __launch_bounds__(256) void resample_v_kernel(const mmvqa_resample_job* __restrict__ jobs, int out_h,
                                                         int out_w) {
  const mmvqa_resample_job j = jobs[blockIdx.z];
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= out_w || y >= out_h) return;
  const int yo = j.oy + y;
  const int ymin = j.vb[yo * 2], yn = j.vb[yo * 2 + 1];
  const int* k = j.vk + (size_t)yo * j.vks;
  const u8* col = j.tmp + ((size_t)(ymin - j.ty0) * out_w + x) * 3;
  int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
  for (int t = 0; t < yn; ++t) {
    const int c = k[t];
    const u8* p = col + (size_t)t * out_w * 3;
    s0 += (int)p[0] * c; s1 += (int)p[1] * c; s2 += (int)p[2] * c;
  }
  u8* o = j.dst + (size_t)y * j.dpitch + (size_t)x * 3;
  o[0] = clip8_22(s0); o[1] = clip8_22(s1); o[2] = clip8_22(s2);
}

// --------------------------------------------------------------------------- rotate (affine_fixed, nearest)
// fix[b][6] = {a0, a1, a2, a3, a4, a5} in 16.16 fixed point (host: FIX(v) = floor-or-truncate(v * 65536 + 0.5))
__global__ __launch_bounds__(256) void rotate_nearest_kernel(const u8* __restrict__ src, u8* __restrict__ dst,
                                                             const int* __restrict__ fix, int H, int W) {
  const int b = blockIdx.z;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const int* a = fix + b * 6;
  const int xx = a[2] + a[1] * y + a[0] * x, yy = a[5] + a[4] * y + a[3] * x;   // (wraps like the C int arithmetic)
  const int xin = xx >> 16, yin = yy >> 16;
  const size_t img = (size_t)b * H * W * 3;
  u8* o = dst + img + ((size_t)y * W + x) * 3;
  if (xin >= 0 && xin < W && yin >= 0 && yin < H) {
    const u8* p = src + img + ((size_t)yin * W + xin) * 3;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
  } else {
    o[0] = 0; o[1] = 0; o[2] = 0;
  }
}

// --------------------------------------------------------------------------- colour jitter
__device__ __forceinline__ int lum(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// sums[b] += sum of L over the pixels of image b (exact integer), for ImageStat.Stat(convert("L")).mean
__global__ __launch_bounds__(256) void lsum_kernel(const u8* __restrict__ img, unsigned long long* __restrict__ sums,
                                                   int npix) {
  const int b = blockIdx.y;
  const u8* p = img + (size_t)b * npix * 3;
  unsigned int s = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) s += (unsigned)lum(p[i * 3], p[i * 3 + 1], p[i * 3 + 2]);
  __shared__ unsigned int red[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&sums[b], (unsigned long long)(red[0] + red[1] + red[2] + red[3]));
}

// ImagingBlend(degenerate, image, alpha) for one byte
__device__ __forceinline__ u8 blend1(int deg, int v, float alpha, bool inside) {
  const float t = (float)deg + alpha * (float)(v - deg);     // separately rounded (no contraction in this file)
  if (inside) return (u8)(int)t;
  if (t <= 0.0f) return 0;
  if (t >= 255.0f) return 255;
  return (u8)(int)t;
}

__device__ __forceinline__ void rgb2hsv(int r, int g, int b, int& uh, int& us, int& uv) {
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  uv = maxc;
  if (minc == maxc) { uh = 0; us = 0; return; }
  const float cr = (float)(maxc - minc);
  const float s = cr / (float)maxc;
  const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
  float h;
  if (r == maxc) h = bc - gc;
  else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
  else h = (float)(4.0 + (double)gc - (double)rc);
  h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
  int ih = (int)((double)h * 255.0), is = (int)((double)s * 255.0);
  uh = ih < 0 ? 0 : (ih > 255 ? 255 : ih);
  us = is < 0 ? 0 : (is > 255 ? 255 : is);
}
__device__ __forceinline__ int round_half_away(double x) { return (int)(x >= 0.0 ? floor(x + 0.5) : ceil(x - 0.5)); }
__device__ __forceinline__ void hsv2rgb(int h, int s, int v, int& r, int& g, int& b) {
  if (s == 0) { r = g = b = v; return; }
  const double hf = (double)h * 6.0 / 255.0;
  const int i = (int)floor(hf);
  const float f = (float)(hf - (double)i);
  const float fs = (float)((double)s / 255.0);
  int p = round_half_away((double)v * (1.0 - (double)fs));
  int q = round_half_away((double)v * (1.0 - (double)fs * (double)f));
  int t = round_half_away((double)v * (1.0 - (double)fs * (1.0 - (double)f)));
  p = p < 0 ? 0 : (p > 255 ? 255 : p); q = q < 0 ? 0 : (q > 255 ? 255 : q); t = t < 0 ? 0 : (t > 255 ? 255 : t);
  switch (i % 6) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

// One round of ColorJitter: image b applies op[b] (0 brightness, 1 contrast, 2 saturation, 3 hue, <0 nothing) with
// factor[b]; contrast uses mean[b] = int(Lsum / npix + 0.5) of the image as it stands (lsum_kernel just before).
__global__ __launch_bounds__(256) void jitter_kernel(u8* __restrict__ img, const int* __restrict__ op,
                                                     const float* __restrict__ factor,
                                                     const unsigned long long* __restrict__ lsums, int npix) {
  const int b = blockIdx.y, o = op[b];
  if (o < 0) return;
  const float f = factor[b];
  const bool inside = f >= 0.0f && f <= 1.0f;
  u8* p = img + (size_t)b * npix * 3;
  int mean = 0, shift = 0;
  if (o == 1) mean = (int)((double)lsums[b] / (double)npix + 0.5);
  if (o == 3) shift = ((int)f) & 0xFF;                  // the host passes np.uint8(hue_factor * 255) itself (integer-valued)
  for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
    int r = p[i * 3], g = p[i * 3 + 1], bb = p[i * 3 + 2];
    if (o == 0) {
      r = blend1(0, r, f, inside); g = blend1(0, g, f, inside); bb = blend1(0, bb, f, inside);
    } else if (o == 1) {
      r = blend1(mean, r, f, inside); g = blend1(mean, g, f, inside); bb = blend1(mean, bb, f, inside);
    } else if (o == 2) {
      const int L = lum(r, g, bb);
      r = blend1(L, r, f, inside); g = blend1(L, g, f, inside); bb = blend1(L, bb, f, inside);
    } else {
      int h, s, v;
      rgb2hsv(r, g, bb, h, s, v);
      h = (h + shift) & 0xFF;
      hsv2rgb(h, s, v, r, g, bb);
    }
    p[i * 3] = (u8)r; p[i * 3 + 1] = (u8)g; p[i * 3 + 2] = (u8)bb;
  }
}

// --------------------------------------------------------------------------- ToTensor + Normalize -> fp32 NCHW
__global__ __launch_bounds__(256) void to_tensor_kernel(const u8* __restrict__ img, float* __restrict__ out, int npix,
                                                        float m0, float m1, float m2, float s0, float s1, float s2) {
  const int b = blockIdx.y;
  const u8* p = img + (size_t)b * npix * 3;
  float* o = out + (size_t)b * npix * 3;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
    o[i] = ((float)p[i * 3] / 255.0f - m0) / s0;
    o[npix + i] = ((float)p[i * 3 + 1] / 255.0f - m1) / s1;
    o[2 * npix + i] = ((float)p[i * 3 + 2] / 255.0f - m2) / s2;
  }
}

// --------------------------------------------------------------------------- the whole train chain in one launch
// One workgroup per image, the working image in LDS ([S][S][3] bytes, 147 KiB at S = 224).  Row blockIdx.x of img is
// the workgroup's scratch: the two passes that read LDS while producing the next LDS contents write their pixels
// there first (thread tid owns pixels tid, tid + 1024, ...), then copy them back after a barrier.  Holding the ~49
// pixels per thread in registers instead took the kernel past 128 VGPRs (spills) at 1024 threads.
//   RandomResizedCrop  horizontal pass source -> LDS tmp [tyn][S][3]; vertical pass LDS -> img -> LDS
//   RandomRotation     gather LDS -> img -> LDS
//   ColorJitter        four rounds in LDS; contrast takes the exact integer L sum of the workgroup
//   ToTensor+Normalize LDS -> out (fp32 NCHW); the final bytes also go back to img (the last byte stage)
// Same arithmetic as resample_h/v, rotate_nearest, lsum + jitter and to_tensor above, so the result is bit-identical.
// VIEWS = false (mmvqa_aug_train_fused): the source is the row's own slot of img, read by the horizontal pass before
//   anything is written there (in place; vsrc is unused).
// VIEWS = true (mmvqa_aug_train_fused_views): row blockIdx.x = v * nsrc + n is view v of image n; the source is image
//   n of vsrc, which is only read and does not overlap img (the host checks it), so both pointers are __restrict__.
#define AUG_FUSED_THREADS 1024

template <bool VIEWS>
__global__ __launch_bounds__(AUG_FUSED_THREADS) void aug_train_fused_kernel(u8* __restrict__ img, float* __restrict__ out,
                                                                            const mmvqa_aug_record* __restrict__ recs,
                                                                            const int* __restrict__ tabs, int S, float m0,
                                                                            float m1, float m2, float s0, float s1,
                                                                            float s2, const u8* __restrict__ vsrc,
                                                                            int nsrc) {
  extern __shared__ u8 lds[];                   // [S][S][3]
  __shared__ unsigned red[AUG_FUSED_THREADS / 64];
  const int tid = threadIdx.x, npix = S * S;
  const mmvqa_aug_record r = recs[blockIdx.x];
  u8* slot = img + (size_t)blockIdx.x * npix * 3;
  const u8* src = VIEWS ? vsrc + (size_t)(blockIdx.x % nsrc) * npix * 3 : slot;
  // a record whose box leaves the image would make the passes below index outside LDS: that image's outputs are left
  // unwritten (documented in mmvqa.h; the host side validates every box before it packs the records)
  if (r.bx < 0 || r.by < 0 || r.bw <= 0 || r.bh <= 0 || r.bx + r.bw > S || r.by + r.bh > S || r.ty0 < 0 || r.tyn <= 0 ||
      r.ty0 + r.tyn > r.bh)
    return;
  // RandomResizedCrop, horizontal pass: box rows [ty0, ty0 + tyn) -> lds[yl][x]
  {
    const int* hb = tabs + r.hb;
    const int* hk = tabs + r.hk;
    for (int q = tid; q < r.tyn * S; q += AUG_FUSED_THREADS) {
      const int yl = q / S, x = q - yl * S;
      const int xmin = hb[x * 2], xn = hb[x * 2 + 1];
      const int* k = hk + (size_t)x * r.hks;
      const u8* row = src + (size_t)(r.by + r.ty0 + yl) * S * 3 + (size_t)(r.bx + xmin) * 3;
      int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
      for (int t = 0; t < xn; ++t) {
        const int c = k[t];
        a0 += (int)row[t * 3] * c; a1 += (int)row[t * 3 + 1] * c; a2 += (int)row[t * 3 + 2] * c;
      }
      lds[q * 3] = clip8_22(a0); lds[q * 3 + 1] = clip8_22(a1); lds[q * 3 + 2] = clip8_22(a2);
    }
  }
  __syncthreads();
  // vertical pass: lds tmp -> img (in place, its own bytes were read above): from here on the slot is this
  // workgroup's scratch, L2-hot
  {
    const int* vb = tabs + r.vb;
    const int* vk = tabs + r.vk;
    for (int p = tid; p < npix; p += AUG_FUSED_THREADS) {
      const int y = p / S, x = p - y * S;
      const int ymin = vb[y * 2], yn = vb[y * 2 + 1];
      const int* kk = vk + (size_t)y * r.vks;
      const u8* col = lds + ((ymin - r.ty0) * S + x) * 3;
      int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
      for (int t = 0; t < yn; ++t) {
        const int c = kk[t];
        const u8* q = col + t * S * 3;
        a0 += (int)q[0] * c; a1 += (int)q[1] * c; a2 += (int)q[2] * c;
      }
      slot[p * 3] = clip8_22(a0); slot[p * 3 + 1] = clip8_22(a1); slot[p * 3 + 2] = clip8_22(a2);
    }
  }
  __syncthreads();                              // every read of tmp is done
  // (each thread reads back only the bytes it wrote itself: program order, no fence needed)
  for (int p = tid; p < npix; p += AUG_FUSED_THREADS) {
    lds[p * 3] = slot[p * 3]; lds[p * 3 + 1] = slot[p * 3 + 1]; lds[p * 3 + 2] = slot[p * 3 + 2];
  }
  __syncthreads();
  // RandomRotation (affine_fixed, nearest, black fill): gather lds -> img, then back to lds
  for (int p = tid; p < npix; p += AUG_FUSED_THREADS) {
    const int y = p / S, x = p - y * S;
    const int xx = r.fix[2] + r.fix[1] * y + r.fix[0] * x, yy = r.fix[5] + r.fix[4] * y + r.fix[3] * x;
    const int xin = xx >> 16, yin = yy >> 16;
    u8 c0 = 0, c1 = 0, c2 = 0;
    if (xin >= 0 && xin < S && yin >= 0 && yin < S) {
      const u8* q = lds + (yin * S + xin) * 3;
      c0 = q[0]; c1 = q[1]; c2 = q[2];
    }
    slot[p * 3] = c0; slot[p * 3 + 1] = c1; slot[p * 3 + 2] = c2;
  }
  __syncthreads();                              // every gather is done
  for (int p = tid; p < npix; p += AUG_FUSED_THREADS) {
    lds[p * 3] = slot[p * 3]; lds[p * 3 + 1] = slot[p * 3 + 1]; lds[p * 3 + 2] = slot[p * 3 + 2];
  }
  // ColorJitter in LDS: round rnd applies op[rnd] (the image's own permutation).  Each thread keeps to the pixels it
  // wrote just above, so only contrast's mean (a sum over the whole image) needs the workgroup.
  for (int rnd = 0; rnd < 4; ++rnd) {
    const int o = recs[blockIdx.x].op[rnd];       // (from memory: a dynamic index into r would put r in scratch)
    if (o < 0) continue;
    const float f = recs[blockIdx.x].factor[rnd];
    const bool inside = f >= 0.0f && f <= 1.0f;
    int mean = 0, shift = 0;
    if (o == 1) {                               // exact integer sum of L: S * S * 255 < 2^32 for any S whose image fits LDS
      unsigned s = 0;
      for (int p = tid; p < npix; p += AUG_FUSED_THREADS) s += (unsigned)lum(lds[p * 3], lds[p * 3 + 1], lds[p * 3 + 2]);
#pragma unroll
      for (int w = 32; w > 0; w >>= 1) s += __shfl_xor(s, w, 64);
      if ((tid & 63) == 0) red[tid >> 6] = s;
      __syncthreads();
      unsigned tot = 0;
#pragma unroll
      for (int w = 0; w < AUG_FUSED_THREADS / 64; ++w) tot += red[w];
      __syncthreads();                          // red is free for the next contrast round
      mean = (int)((double)tot / (double)npix + 0.5);
    }
    if (o == 3) shift = ((int)f) & 0xFF;
    for (int p = tid; p < npix; p += AUG_FUSED_THREADS) {
      int cr = lds[p * 3], cg = lds[p * 3 + 1], cb = lds[p * 3 + 2];
      if (o == 0) {
        cr = blend1(0, cr, f, inside); cg = blend1(0, cg, f, inside); cb = blend1(0, cb, f, inside);
      } else if (o == 1) {
        cr = blend1(mean, cr, f, inside); cg = blend1(mean, cg, f, inside); cb = blend1(mean, cb, f, inside);
      } else if (o == 2) {
        const int L = lum(cr, cg, cb);
        cr = blend1(L, cr, f, inside); cg = blend1(L, cg, f, inside); cb = blend1(L, cb, f, inside);
      } else {
        int h, sat, val;
        rgb2hsv(cr, cg, cb, h, sat, val);
        h = (h + shift) & 0xFF;
        hsv2rgb(h, sat, val, cr, cg, cb);
      }
      lds[p * 3] = (u8)cr; lds[p * 3 + 1] = (u8)cg; lds[p * 3 + 2] = (u8)cb;
    }
  }
  // ToTensor + Normalize (coalesced fp32 planes) and the final bytes back to img
  float* o = out + (size_t)blockIdx.x * npix * 3;
  for (int p = tid; p < npix; p += AUG_FUSED_THREADS) {
    const int cr = lds[p * 3], cg = lds[p * 3 + 1], cb = lds[p * 3 + 2];
    o[p] = ((float)cr / 255.0f - m0) / s0;
    o[npix + p] = ((float)cg / 255.0f - m1) / s1;
    o[2 * npix + p] = ((float)cb / 255.0f - m2) / s2;
    slot[p * 3] = (u8)cr; slot[p * 3 + 1] = (u8)cg; slot[p * 3 + 2] = (u8)cb;
  }
}

// --------------------------------------------------------------------------- C ABI
extern "C" {

size_t mmvqa_sizeof_resample_job(void) { return sizeof(mmvqa_resample_job); }

int mmvqa_aug_resample(mmvqa_stream_t s, const mmvqa_resample_job* jobs_dev, int njobs, int max_tmp_rows, int out_h,
                       int out_w) {
  if (!jobs_dev || njobs <= 0 || out_h <= 0 || out_w <= 0 || max_tmp_rows <= 0)
    return mmvqa_set_error(MMVQA_ERR_ARG, "aug_resample: bad arguments");
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(resample_h_kernel, dim3((out_w + 63) / 64, (max_tmp_rows + 3) / 4, njobs), dim3(256), 0, st, jobs_dev, out_w);
  KERNEL_CHECK_RET();
  hipLaunchKernelGGL(resample_v_kernel, dim3((out_w + 63) / 64, (out_h + 3) / 4, njobs), dim3(256), 0, st, jobs_dev, out_h, out_w);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

int mmvqa_aug_rotate(mmvqa_stream_t s, const unsigned char* src, unsigned char* dst, const int* fix_dev, int B, int H,
                     int W) {
  if (!src || !dst || src == dst || !fix_dev || B <= 0 || H <= 0 || W <= 0)
    return mmvqa_set_error(MMVQA_ERR_ARG, "aug_rotate: bad arguments (src and dst must differ)");
  hipLaunchKernelGGL(rotate_nearest_kernel, dim3((W + 63) / 64, (H + 3) / 4, B), dim3(256), 0, (hipStream_t)s, src, dst, fix_dev, H, W);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

int mmvqa_aug_jitter_round(mmvqa_stream_t s, unsigned char* img, const int* op_dev, const float* factor_dev,
                           unsigned long long* lsum_dev, int B, int npix) {
  if (!img || !op_dev || !factor_dev || !lsum_dev || B <= 0 || npix <= 0)
    return mmvqa_set_error(MMVQA_ERR_ARG, "aug_jitter_round: bad arguments");
  hipStream_t st = (hipStream_t)s;
  HIP_CHECK_RET(hipMemsetAsync(lsum_dev, 0, sizeof(unsigned long long) * (size_t)B, st));
  const int gx = (npix + 256 * 8 - 1) / (256 * 8);
  hipLaunchKernelGGL(lsum_kernel, dim3(gx, B), dim3(256), 0, st, img, lsum_dev, npix);
  KERNEL_CHECK_RET();
  hipLaunchKernelGGL(jitter_kernel, dim3(gx, B), dim3(256), 0, st, img, op_dev, factor_dev, lsum_dev, npix);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

int mmvqa_aug_to_tensor(mmvqa_stream_t s, const unsigned char* img, float* out, int B, int npix, const float* mean3,
                        const float* std3) {
  if (!img || !out || !mean3 || !std3 || B <= 0 || npix <= 0) return mmvqa_set_error(MMVQA_ERR_ARG, "aug_to_tensor: bad arguments");
  const int gx = (npix + 256 * 4 - 1) / (256 * 4);
  hipLaunchKernelGGL(to_tensor_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)s, img, out, npix, mean3[0], mean3[1],
                     mean3[2], std3[0], std3[1], std3[2]);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

size_t mmvqa_sizeof_aug_record(void) { return sizeof(mmvqa_aug_record); }

// dynamic LDS the fused kernel may use on the current device (its attribute raised to that once per device)
static int fused_lds_cap(int* cap_out) {
  static int lds_cap[32] = {0};
  int dev = 0;
  HIP_CHECK_RET(hipGetDevice(&dev));
  if (dev < 0 || dev >= 32) return mmvqa_set_error(MMVQA_ERR_ARG, "aug_train_fused: device %d out of range", dev);
  if (!lds_cap[dev]) {
    int a = 0, b = 0;
    HIP_CHECK_RET(hipDeviceGetAttribute(&a, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    HIP_CHECK_RET(hipDeviceGetAttribute(&b, hipDeviceAttributeSharedMemPerBlockOptin, dev));
    const int cap = (a > b ? a : b) - (int)(sizeof(unsigned) * (AUG_FUSED_THREADS / 64));   // less the static LDS
    HIP_CHECK_RET(hipFuncSetAttribute((const void*)aug_train_fused_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, cap));
    HIP_CHECK_RET(hipFuncSetAttribute((const void*)aug_train_fused_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, cap));
    lds_cap[dev] = cap;
  }
  *cap_out = lds_cap[dev];
  return MMVQA_OK;
}

int mmvqa_aug_train_fused_fits(int S) {
  if (S <= 0) return mmvqa_set_error(MMVQA_ERR_ARG, "aug_train_fused_fits: S = %d", S);
  int cap = 0;
  const int rc = fused_lds_cap(&cap);
  if (rc != MMVQA_OK) return rc;
  return (size_t)S * S * 3 <= (size_t)cap ? 1 : 0;
}

int mmvqa_aug_train_fused(mmvqa_stream_t s, unsigned char* src_u8, float* out_f32, const mmvqa_aug_record* records_dev,
                          const int* tables_dev, int B, int S, const float* mean3, const float* std3) {
  if (!src_u8 || !out_f32 || !records_dev || !tables_dev || !mean3 || !std3 || B <= 0 || S <= 0)
    return mmvqa_set_error(MMVQA_ERR_ARG, "aug_train_fused: bad arguments");
  int cap = 0;
  const int rc = fused_lds_cap(&cap);
  if (rc != MMVQA_OK) return rc;
  const size_t lds = (size_t)S * S * 3;
  if (lds > (size_t)cap)
    return mmvqa_set_error(MMVQA_ERR_ARG, "aug_train_fused: S = %d needs %zu B of LDS, the device gives %d", S, lds, cap);
  hipLaunchKernelGGL(aug_train_fused_kernel<false>, dim3(B), dim3(AUG_FUSED_THREADS), lds, (hipStream_t)s, src_u8, out_f32,
                     records_dev, tables_dev, S, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2],
                     (const u8*)nullptr, B);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

int mmvqa_aug_train_fused_views(mmvqa_stream_t s, const unsigned char* src_u8, unsigned char* scratch_u8, float* out_f32,
                                const mmvqa_aug_record* records_dev, const int* tables_dev, int B, int V, int S,
                                const float* mean3, const float* std3) {
  if (!src_u8 || !scratch_u8 || !out_f32 || !records_dev || !tables_dev || !mean3 || !std3 || B <= 0 || V <= 0 || S <= 0)
    return mmvqa_set_error(MMVQA_ERR_ARG, "aug_train_fused_views: bad arguments");
  const size_t img = (size_t)S * S * 3;
  if ((size_t)V * B > (size_t)INT_MAX)
    return mmvqa_set_error(MMVQA_ERR_ARG, "aug_train_fused_views: %d x %d views are too many for one launch", V, B);
  const uintptr_t s0 = (uintptr_t)src_u8, s1 = s0 + img * B, d0 = (uintptr_t)scratch_u8, d1 = d0 + img * V * B;
  if (s0 < d1 && d0 < s1)
    return mmvqa_set_error(MMVQA_ERR_ARG, "aug_train_fused_views: src_u8 and scratch_u8 overlap");
  int cap = 0;
  const int rc = fused_lds_cap(&cap);
  if (rc != MMVQA_OK) return rc;
  if (img > (size_t)cap)
    return mmvqa_set_error(MMVQA_ERR_ARG, "aug_train_fused_views: S = %d needs %zu B of LDS, the device gives %d", S, img, cap);
  hipLaunchKernelGGL(aug_train_fused_kernel<true>, dim3(V * B), dim3(AUG_FUSED_THREADS), img, (hipStream_t)s, scratch_u8,
                     out_f32, records_dev, tables_dev, S, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], src_u8, B);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

// --------------------------------------------------------------------------- low-priority stream (input pipeline)
int mmvqa_low_priority_stream(mmvqa_stream_t* out, int* priority) {
  if (!out) return mmvqa_set_error(MMVQA_ERR_ARG, "low_priority_stream: null output");
  static hipStream_t streams[32] = {nullptr};
  int dev = 0;
  HIP_CHECK_RET(hipGetDevice(&dev));
  if (dev < 0 || dev >= 32) return mmvqa_set_error(MMVQA_ERR_ARG, "low_priority_stream: device %d out of range", dev);
  if (!streams[dev]) {
    int least = 0, greatest = 0;
    HIP_CHECK_RET(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIP_CHECK_RET(hipStreamCreateWithPriority(&streams[dev], hipStreamNonBlocking, least));
  }
  *out = (mmvqa_stream_t)streams[dev];
  if (priority) HIP_CHECK_RET(hipStreamGetPriority(streams[dev], priority));
  return MMVQA_OK;
}

int mmvqa_stream_priority(mmvqa_stream_t s, int* priority) {
  if (!priority) return mmvqa_set_error(MMVQA_ERR_ARG, "stream_priority: null output");
  HIP_CHECK_RET(hipStreamGetPriority((hipStream_t)s, priority));
  return MMVQA_OK;
}

}  // extern "C"
