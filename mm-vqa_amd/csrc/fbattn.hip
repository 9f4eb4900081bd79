// Feedback-Transformer pieces that exist nowhere else in the hot path (models/feedback_transformer_pytorch.py):
//   * attention of one window (1 or 2 queries per sample and head) against the growing memory plus its own keys,
//     forward and backward (Attention.forward :160-193 with RelativePositionBias :71-79)
//   * the layer-weighted aggregation of a window's hiddens into the memory input (:272-299), forward and backward
//   * GEGLU with dropout (:114-133), forward and backward
//   * the [B,T,H] <-> window-major row permutation of the engine's schedule
// All of them are small and latency-bound: every load of a pass is issued before its first use, the per-key rows travel
// as 16-byte accesses, and nothing here uses LDS beyond a few hundred floats.  8 heads of width 64 are the reference's
// constants (mmbert.py:118-119), not parameters.
#include "kernels.h"

namespace {

constexpr int FB_HEADS = 8, FB_DH = 64, FB_MAXKEYS = 256, FB_MAXHID = MMVQA_FB_MAX_HIDDENS;

typedef mmvqa_fb_attn_desc FbAttnParams;

// row of key / value j of sample b: memory entry j (window j/2, token j&1) below n_mem, the window's own row above
__device__ __forceinline__ const float* fb_row(const float* mem, const float* self, const FbAttnParams& p, int b, int h, int j) {
  if (j < p.n_mem) return mem + (size_t)(j >> 1) * p.mem_win + (size_t)(b * 2 + (j & 1)) * p.mem_ld + h * FB_DH;
  return self + (size_t)(b * 2 + (j - p.n_mem)) * p.self_ld + h * FB_DH;
}
__device__ __forceinline__ float* fb_row_w(float* mem, float* self, int self_ld, const FbAttnParams& p, int b, int h, int j) {
  if (j < p.n_mem) return mem + (size_t)(j >> 1) * p.mem_win + (size_t)(b * 2 + (j & 1)) * p.mem_ld + h * FB_DH;
  return self + (size_t)(b * 2 + (j - p.n_mem)) * self_ld + h * FB_DH;
}

// two block-wide reductions at once (one value per query); every thread of the block calls it
template <bool MAX>
__device__ __forceinline__ void fb_block_reduce2(float& a, float& b, float (*red)[4]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  a = MAX ? wave_max(a) : wave_sum(a);
  b = MAX ? wave_max(b) : wave_sum(b);
  __syncthreads();   // the previous use of `red` has been read
  if (lane == 0) { red[0][wv] = a; red[1][wv] = b; }
  __syncthreads();
  a = red[0][0]; b = red[1][0];
  for (int w = 1; w < nw; ++w) {
    a = MAX ? fmaxf(a, red[0][w]) : a + red[0][w];
    b = MAX ? fmaxf(b, red[1][w]) : b + red[1][w];
  }
}

// probs[i][j] * rows[j][d] summed over the keys: wave w takes keys w, w + nw, ..., lane = d; partial sums meet in LDS
__device__ __forceinline__ void fb_weighted_rows(const float* mem, const float* self, const FbAttnParams& p, int b, int h, int J,
                                                 const float (*w)[FB_MAXKEYS], float (*part)[2][FB_DH], float& o0, float& o1) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  float a0 = 0.f, a1 = 0.f;
#pragma unroll 4
  for (int j = wv; j < J; j += nw) {
    const float x = fb_row(mem, self, p, b, h, j)[lane];
    a0 += w[0][j] * x;
    a1 += w[1][j] * x;
  }
  part[wv][0][lane] = a0; part[wv][1][lane] = a1;
  __syncthreads();
  o0 = 0.f; o1 = 0.f;
  if (threadIdx.x < FB_DH)   // the first wave finishes both queries (a block may be one wave)
    for (int k = 0; k < nw; ++k) { o0 += part[k][0][lane]; o1 += part[k][1][lane]; }
}

// grid: B * 8 (sample, head); block: 64 * ceil(keys / 64) threads, thread j owns key j
__global__ __launch_bounds__(256) void fb_attn_fwd_kernel(FbAttnParams p) {
  __shared__ float s_w[2][FB_MAXKEYS];
  __shared__ float s_red[2][4];
  __shared__ float s_part[4][2][FB_DH];
  const int b = blockIdx.x >> 3, h = blockIdx.x & 7, t = threadIdx.x;
  const int n = p.n, J = p.n_mem + (n == 2 ? 2 : 0);
  const bool valid = t < J;
  const float* q0 = p.q + (size_t)(b * n) * p.q_ld + h * FB_DH;
  const float* q1 = n == 2 ? q0 + p.q_ld : q0;
  f32x4 k[FB_DH / 4];
  {
    const f32x4* kp = reinterpret_cast<const f32x4*>(fb_row(p.mem_k, p.self_k, p, b, h, valid ? t : 0));
#pragma unroll
    for (int c = 0; c < FB_DH / 4; ++c) k[c] = kp[c];
  }
  const float b0 = p.bias[h], b1 = p.bias[FB_HEADS + h];
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int c = 0; c < FB_DH / 4; ++c) {
    const f32x4 a = reinterpret_cast<const f32x4*>(q0)[c], d = reinterpret_cast<const f32x4*>(q1)[c];
#pragma unroll
    for (int e = 0; e < 4; ++e) { s0 += a[e] * k[c][e]; s1 += d[e] * k[c][e]; }
  }
  // bias row max(i - j, 0): row 1 for (query 1, key 0), row 0 elsewhere; query 0 does not see the window's second key
  s0 = s0 * p.scale + b0;
  s1 = s1 * p.scale + ((n == 2 && t == 0) ? b1 : b0);
  const bool on0 = valid && !(n == 2 && t == J - 1), on1 = valid && n == 2;
  float m0 = on0 ? s0 : -INFINITY, m1 = on1 ? s1 : -INFINITY;
  fb_block_reduce2<true>(m0, m1, s_red);
  const float e0 = on0 ? expf(s0 - m0) : 0.f, e1 = on1 ? expf(s1 - m1) : 0.f;
  float z0 = e0, z1 = e1;
  fb_block_reduce2<false>(z0, z1, s_red);
  float p0 = e0 / z0, p1 = on1 ? e1 / z1 : 0.f;
  if (valid) {
    float* pr = p.probs + (size_t)((b * FB_HEADS + h) * n) * p.p_ld + t;
    pr[0] = p0;
    if (n == 2) pr[p.p_ld] = p1;
  }
  if (p.drop_p > 0.f) {
    const float ks = 1.0f / (1.0f - p.drop_p);
    const uint32_t r0 = (uint32_t)((b * FB_HEADS + h) * p.T + p.n_mem) * (uint32_t)p.T + (uint32_t)t;
    p0 = rng_uniform(p.seed, r0) >= p.drop_p ? p0 * ks : 0.f;
    p1 = rng_uniform(p.seed, r0 + (uint32_t)p.T) >= p.drop_p ? p1 * ks : 0.f;
  }
  s_w[0][t] = p0; s_w[1][t] = p1;
  __syncthreads();
  float o0, o1;
  fb_weighted_rows(p.mem_v, p.self_v, p, b, h, J, s_w, s_part, o0, o1);
  if (t < FB_DH) {
    float* o = p.out + (size_t)(b * n) * p.out_ld + h * FB_DH + t;
    o[0] = o0;
    if (n == 2) o[p.out_ld] = o1;
  }
}

// same grid.  Thread j owns row j of dk / dv (memory rows are added to: one owner per element within a launch, stream
// order between launches); dq meets over the keys in LDS; the bias-table gradient is reduced over the block first.
__global__ __launch_bounds__(256) void fb_attn_bwd_kernel(FbAttnParams p) {
  __shared__ float s_w[2][FB_MAXKEYS];
  __shared__ float s_red[2][4];
  __shared__ float s_part[4][2][FB_DH];
  const int b = blockIdx.x >> 3, h = blockIdx.x & 7, t = threadIdx.x;
  const int n = p.n, J = p.n_mem + (n == 2 ? 2 : 0);
  const bool valid = t < J;
  const bool is_mem = t < p.n_mem;
  const f32x4* g0 = reinterpret_cast<const f32x4*>(p.dout + (size_t)(b * n) * p.dout_ld + h * FB_DH);
  const f32x4* g1 = n == 2 ? reinterpret_cast<const f32x4*>(p.dout + (size_t)(b * n + 1) * p.dout_ld + h * FB_DH) : g0;
  const f32x4* q0 = reinterpret_cast<const f32x4*>(p.q + (size_t)(b * n) * p.q_ld + h * FB_DH);
  const f32x4* q1 = n == 2 ? reinterpret_cast<const f32x4*>(p.q + (size_t)(b * n + 1) * p.q_ld + h * FB_DH) : q0;
  f32x4 v[FB_DH / 4];
  {
    const f32x4* vp = reinterpret_cast<const f32x4*>(fb_row(p.mem_v, p.self_v, p, b, h, valid ? t : 0));
#pragma unroll
    for (int c = 0; c < FB_DH / 4; ++c) v[c] = vp[c];
  }
  float pr0 = 0.f, pr1 = 0.f;
  if (valid) {
    const float* pr = p.probs + (size_t)((b * FB_HEADS + h) * n) * p.p_ld + t;
    pr0 = pr[0];
    if (n == 2) pr1 = pr[p.p_ld];
  }
  float dp0 = 0.f, dp1 = 0.f;
#pragma unroll
  for (int c = 0; c < FB_DH / 4; ++c) {
    const f32x4 a = g0[c], d = g1[c];
#pragma unroll
    for (int e = 0; e < 4; ++e) { dp0 += a[e] * v[c][e]; dp1 += d[e] * v[c][e]; }
  }
  float pd0 = pr0, pd1 = pr1;   // the probabilities the forward multiplied the values with
  if (p.drop_p > 0.f) {
    const float ks = 1.0f / (1.0f - p.drop_p);
    const uint32_t r0 = (uint32_t)((b * FB_HEADS + h) * p.T + p.n_mem) * (uint32_t)p.T + (uint32_t)t;
    const bool k0 = rng_uniform(p.seed, r0) >= p.drop_p, k1 = rng_uniform(p.seed, r0 + (uint32_t)p.T) >= p.drop_p;
    pd0 = k0 ? pr0 * ks : 0.f; dp0 = k0 ? dp0 * ks : 0.f;
    pd1 = k1 ? pr1 * ks : 0.f; dp1 = k1 ? dp1 * ks : 0.f;
  }
  float c0 = pr0 * dp0, c1 = pr1 * dp1;
  fb_block_reduce2<false>(c0, c1, s_red);
  const float ds0 = pr0 * (dp0 - c0), ds1 = pr1 * (dp1 - c1);
  if (valid) {
    // dv_j = sum_i pd_i dout_i ; dk_j = scale * sum_i ds_i q_i
    f32x4* dvp = reinterpret_cast<f32x4*>(fb_row_w(p.dmem_v, p.dself_v, p.dself_ld, p, b, h, t));
    f32x4* dkp = reinterpret_cast<f32x4*>(fb_row_w(p.dmem_k, p.dself_k, p.dself_ld, p, b, h, t));
    f32x4 ov[FB_DH / 4], ok[FB_DH / 4];
#pragma unroll
    for (int c = 0; c < FB_DH / 4; ++c) {
      ov[c] = f32x4{0.f, 0.f, 0.f, 0.f}; ok[c] = ov[c];
      if (is_mem) { ov[c] = dvp[c]; ok[c] = dkp[c]; }
    }
    const float a0 = ds0 * p.scale, a1 = ds1 * p.scale;
#pragma unroll
    for (int c = 0; c < FB_DH / 4; ++c) {
      ov[c] += pd0 * g0[c] + pd1 * g1[c];
      ok[c] += a0 * q0[c] + a1 * q1[c];
      dvp[c] = ov[c]; dkp[c] = ok[c];
    }
  }
  s_w[0][t] = ds0; s_w[1][t] = ds1;
  if (p.dbias) {
    // row 1 collects (query 1, key 0), row 0 every other pair
    float r0 = ds0 + ((n == 2 && t == 0) ? 0.f : ds1), unused = 0.f;
    fb_block_reduce2<false>(r0, unused, s_red);
    if (t == 0) {
      atomicAdd(p.dbias + h, r0);
      if (n == 2) atomicAdd(p.dbias + FB_HEADS + h, ds1);
    }
  }
  __syncthreads();
  float o0, o1;
  fb_weighted_rows(p.mem_k, p.self_k, p, b, h, J, s_w, s_part, o0, o1);
  if (t < FB_DH) {
    float* o = p.dq + (size_t)(b * n) * p.dq_ld + h * FB_DH + t;
    o[0] = o0 * p.scale;
    if (n == 2) o[p.dq_ld] = o1 * p.scale;
  }
}

// softmax(layer_weight) into LDS; all threads call it; ends with a barrier
__device__ __forceinline__ void fb_layer_softmax(const float* __restrict__ lw, int nh, float* s_w) {
  if (threadIdx.x == 0) {
    float m = -INFINITY, z = 0.f;
    for (int l = 0; l < nh; ++l) m = fmaxf(m, lw[l]);
    for (int l = 0; l < nh; ++l) { s_w[l] = expf(lw[l] - m); z += s_w[l]; }
    for (int l = 0; l < nh; ++l) s_w[l] /= z;
  }
  __syncthreads();
}

// agg = sum_l softmax(lw)_l * hid_l ; one float4 per thread
__global__ __launch_bounds__(256) void fb_agg_fwd_kernel(const float* __restrict__ hid, long long hstride, int nh,
                                                         const float* __restrict__ lw, float* __restrict__ agg, long n4) {
  __shared__ float s_w[FB_MAXHID];
  fb_layer_softmax(lw, nh, s_w);
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  f32x4 x[FB_MAXHID];
#pragma unroll
  for (int l = 0; l < FB_MAXHID; ++l) {
    x[l] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (l < nh) x[l] = reinterpret_cast<const f32x4*>(hid + (size_t)l * hstride)[i];
  }
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int l = 0; l < FB_MAXHID; ++l)
    if (l < nh) a += s_w[l] * x[l];
  reinterpret_cast<f32x4*>(agg)[i] = a;
}

// dh_l = softmax(lw)_l * dagg (the top hidden's share is ADDED to dtop when given), and
// dlw_l += sw_l * (<dagg, hid_l> - sum_m sw_m <dagg, hid_m>): linear in the dot products, so every block applies it to its
// own partial dot products and adds nh floats
__global__ __launch_bounds__(256) void fb_agg_bwd_kernel(const float* __restrict__ dagg, const float* __restrict__ hid,
                                                         long long hstride, int nh, const float* __restrict__ lw,
                                                         float* __restrict__ dh, long long dstride, float* __restrict__ dtop,
                                                         float* __restrict__ dlw, long n4) {
  __shared__ float s_w[FB_MAXHID];
  __shared__ float s_dot[4][FB_MAXHID];
  fb_layer_softmax(lw, nh, s_w);
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool on = i < n4;
  f32x4 g = {0.f, 0.f, 0.f, 0.f}, top = g;
  f32x4 x[FB_MAXHID];
  if (on) {
    g = reinterpret_cast<const f32x4*>(dagg)[i];
    if (dtop) top = reinterpret_cast<const f32x4*>(dtop)[i];
  }
#pragma unroll
  for (int l = 0; l < FB_MAXHID; ++l) {
    x[l] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (on && dlw && l < nh) x[l] = reinterpret_cast<const f32x4*>(hid + (size_t)l * hstride)[i];
  }
  if (on) {
#pragma unroll
    for (int l = 0; l < FB_MAXHID; ++l) {
      if (l >= nh) continue;
      if (dtop && l == nh - 1) reinterpret_cast<f32x4*>(dtop)[i] = top + s_w[l] * g;
      else reinterpret_cast<f32x4*>(dh + (size_t)l * dstride)[i] = s_w[l] * g;
    }
  }
  if (!dlw) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int l = 0; l < FB_MAXHID; ++l) {
    if (l >= nh) continue;
    const float d = wave_sum(g[0] * x[l][0] + g[1] * x[l][1] + g[2] * x[l][2] + g[3] * x[l][3]);
    if (lane == 0) s_dot[wv][l] = d;
  }
  __syncthreads();
  if (threadIdx.x < nh) {
    float mine = 0.f, all = 0.f;
    for (int l = 0; l < nh; ++l) {
      const float d = s_dot[0][l] + s_dot[1][l] + s_dot[2][l] + s_dot[3][l];
      all += s_w[l] * d;
      if (l == (int)threadIdx.x) mine = d;
    }
    atomicAdd(dlw + threadIdx.x, s_w[threadIdx.x] * (mine - all));
  }
}

// (u | gate) [M][2F] -> dropout(gelu(gate) * u) [M][F]; the dropout index of element (r, c) is idx0 + r * F + c
__global__ __launch_bounds__(256) void fb_geglu_fwd_kernel(const float* __restrict__ pre, float* __restrict__ y, long M, int F,
                                                           float drop_p, uint32_t seed, uint32_t idx0) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int f4 = F >> 2;
  if (i >= M * f4) return;
  const long r = i / f4;
  const int c = (int)(i - r * f4) * 4;
  const f32x4 u = *reinterpret_cast<const f32x4*>(pre + r * 2 * F + c);
  const f32x4 g = *reinterpret_cast<const f32x4*>(pre + r * 2 * F + F + c);
  const float ks = 1.0f / (1.0f - drop_p);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    o[e] = act_fwd(ACT_GELU, g[e]) * u[e];
    if (drop_p > 0.f) o[e] = rng_uniform(seed, idx0 + (uint32_t)r * (uint32_t)F + (uint32_t)(c + e)) >= drop_p ? o[e] * ks : 0.f;
  }
  *reinterpret_cast<f32x4*>(y + r * F + c) = o;
}

// d(u | gate) from dy, the saved pre-activation and the forward's mask
__global__ __launch_bounds__(256) void fb_geglu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ pre,
                                                           float* __restrict__ dpre, long M, int F, float drop_p, uint32_t seed,
                                                           uint32_t idx0) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int f4 = F >> 2;
  if (i >= M * f4) return;
  const long r = i / f4;
  const int c = (int)(i - r * f4) * 4;
  f32x4 d = *reinterpret_cast<const f32x4*>(dy + r * F + c);
  const f32x4 u = *reinterpret_cast<const f32x4*>(pre + r * 2 * F + c);
  const f32x4 g = *reinterpret_cast<const f32x4*>(pre + r * 2 * F + F + c);
  const float ks = 1.0f / (1.0f - drop_p);
  f32x4 du, dg;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (drop_p > 0.f) d[e] = rng_uniform(seed, idx0 + (uint32_t)r * (uint32_t)F + (uint32_t)(c + e)) >= drop_p ? d[e] * ks : 0.f;
    du[e] = d[e] * act_fwd(ACT_GELU, g[e]);
    dg[e] = d[e] * u[e] * act_bwd(ACT_GELU, g[e]);
  }
  *reinterpret_cast<f32x4*>(dpre + r * 2 * F + c) = du;
  *reinterpret_cast<f32x4*>(dpre + r * 2 * F + F + c) = dg;
}

// row (b, t) of [B][T][H] <-> window-major row (t / 2) * 2B + b * n + (t & 1), n = tokens of that window (the last
// window of an odd T has one)
__global__ __launch_bounds__(256) void fb_reorder_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int T,
                                                         int H4, int to_window) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * T * H4) return;
  const long row = i / H4;
  const int c = (int)(i - row * H4);
  const int b = (int)(row / T), t = (int)(row - (long)b * T);
  const int w = t >> 1, n = (2 * w + 1 < T) ? 2 : 1;
  const long wrow = (long)w * 2 * B + (long)b * n + (t & 1);
  const long s = (to_window ? row : wrow) * H4 + c, d = (to_window ? wrow : row) * H4 + c;
  reinterpret_cast<f32x4*>(dst)[d] = reinterpret_cast<const f32x4*>(src)[s];
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int mmvqa_fb_attention(const mmvqa_fb_attn_desc* d, int bwd, mmvqa_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  if (!d) return mmvqa_set_error(MMVQA_ERR_ARG, "fb_attention: null descriptor");
  const mmvqa_fb_attn_desc& p = *d;
  const int J = p.n_mem + (p.n == 2 ? 2 : 0);
  if (p.B <= 0 || (p.n != 1 && p.n != 2) || p.n_mem < 0 || (p.n_mem & 1) || J < 1 || J > FB_MAXKEYS)
    return mmvqa_set_error(MMVQA_ERR_ARG, "fb_attention: B=%d n=%d n_mem=%d (n in {1,2}, n_mem even, 1 <= keys <= %d)", p.B, p.n,
                           p.n_mem, FB_MAXKEYS);
  if (!p.q || !p.bias || !p.probs || (p.n_mem > 0 && (!p.mem_k || !p.mem_v)) || (p.n == 2 && (!p.self_k || !p.self_v)))
    return mmvqa_set_error(MMVQA_ERR_ARG, "fb_attention: null operand");
  if (p.drop_p < 0.f || p.drop_p >= 1.f || (p.drop_p > 0.f && p.T < p.n_mem + p.n))
    return mmvqa_set_error(MMVQA_ERR_ARG, "fb_attention: drop_p=%g T=%d", (double)p.drop_p, p.T);
  if (p.p_ld < J || (p.q_ld & 3) || (p.mem_ld & 3) || (p.mem_win & 3) || (p.n == 2 && (p.self_ld & 3)) || !al16(p.q) ||
      !al16(p.mem_k) || !al16(p.mem_v) || !al16(p.self_k) || !al16(p.self_v))
    return mmvqa_set_error(MMVQA_ERR_ARG, "fb_attention: p_ld=%d < keys=%d, or a row stride / pointer that is not 16-byte aligned",
                           p.p_ld, J);
  const int threads = 64 * ((J + 63) / 64);
  if (!bwd) {
    if (!p.out || p.out_ld < FB_HEADS * FB_DH) return mmvqa_set_error(MMVQA_ERR_ARG, "fb_attention: out / out_ld=%d", p.out_ld);
    hipLaunchKernelGGL(fb_attn_fwd_kernel, dim3(p.B * FB_HEADS), dim3(threads), 0, st, p);
  } else {
    if (!p.dout || !p.dq || (p.n_mem > 0 && (!p.dmem_k || !p.dmem_v)) || (p.n == 2 && (!p.dself_k || !p.dself_v)))
      return mmvqa_set_error(MMVQA_ERR_ARG, "fb_attention backward: null gradient pointer");
    if ((p.dout_ld & 3) || (p.n == 2 && (p.dself_ld & 3)) || !al16(p.dout) || !al16(p.dmem_k) || !al16(p.dmem_v) ||
        !al16(p.dself_k) || !al16(p.dself_v) || p.dq_ld < FB_HEADS * FB_DH)
      return mmvqa_set_error(MMVQA_ERR_ARG, "fb_attention backward: gradient row stride / pointer not 16-byte aligned");
    hipLaunchKernelGGL(fb_attn_bwd_kernel, dim3(p.B * FB_HEADS), dim3(threads), 0, st, p);
  }
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

static int fb_agg_check(const char* who, const float* a, const float* hid, long long hstride, int nh, const float* lw, long rows,
                        int H) {
  if (!a || !hid || !lw) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: null operand", who);
  if (nh < 1 || nh > FB_MAXHID || rows <= 0 || H <= 0 || (H & 3) || (hstride & 3) || !al16(a) || !al16(hid))
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: hiddens=%d (1..%d) rows=%ld H=%d (H and the stride multiples of 4, 16-byte pointers)",
                           who, nh, FB_MAXHID, rows, H);
  return MMVQA_OK;
}

extern "C" int mmvqa_fb_aggregate_fwd(mmvqa_stream_t s, const float* hid, long long hstride, int nh, const float* lw,
                                      float* agg, long rows, int H) {
  hipStream_t st = (hipStream_t)s;
  int r = fb_agg_check("fb_aggregate_fwd", agg, hid, hstride, nh, lw, rows, H);
  if (r != MMVQA_OK) return r;
  const long n4 = rows * (H / 4);
  hipLaunchKernelGGL(fb_agg_fwd_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, hid, hstride, nh, lw, agg, n4);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

extern "C" int mmvqa_fb_aggregate_bwd(mmvqa_stream_t s, const float* dagg, const float* hid, long long hstride, int nh,
                                      const float* lw, float* dh, long long dstride, float* dtop, float* dlw, long rows,
                                      int H) {
  hipStream_t st = (hipStream_t)s;
  int r = fb_agg_check("fb_aggregate_bwd", dagg, hid, hstride, nh, lw, rows, H);
  if (r != MMVQA_OK) return r;
  if (!dh || (dstride & 3) || !al16(dh) || !al16(dtop))
    return mmvqa_set_error(MMVQA_ERR_ARG, "fb_aggregate_bwd: dh is null, or a gradient stride / pointer is not 16-byte aligned");
  const long n4 = rows * (H / 4);
  hipLaunchKernelGGL(fb_agg_bwd_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, dagg, hid, hstride, nh, lw, dh,
                     dstride, dtop, dlw, n4);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

static int fb_geglu_check(const char* who, const void* a, const void* b, const void* c, long M, int F, float drop_p,
                          unsigned long long idx0) {
  if (!a || !b || !c) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: null operand", who);
  if (M <= 0 || F <= 0 || (F & 3) || !al16(a) || !al16(b) || !al16(c) || drop_p < 0.f || drop_p >= 1.f)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: M=%ld F=%d drop_p=%g (F a multiple of 4, 16-byte pointers, 0 <= p < 1)", who, M, F,
                           (double)drop_p);
  if (idx0 + (unsigned long long)M * F > 0xFFFFFFFFull)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: dropout index %llu + %ld x %d exceeds 32 bits", who, idx0, M, F);
  return MMVQA_OK;
}

extern "C" int mmvqa_geglu_fwd(mmvqa_stream_t s, const float* pre, float* y, long M, int F, float drop_p, uint32_t seed,
                               uint32_t idx0) {
  hipStream_t st = (hipStream_t)s;
  int r = fb_geglu_check("geglu_fwd", pre, y, y, M, F, drop_p, idx0);
  if (r != MMVQA_OK) return r;
  const long n4 = M * (F / 4);
  hipLaunchKernelGGL(fb_geglu_fwd_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, pre, y, M, F, drop_p, seed, idx0);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

extern "C" int mmvqa_geglu_bwd(mmvqa_stream_t s, const float* dy, const float* pre, float* dpre, long M, int F,
                               float drop_p, uint32_t seed, uint32_t idx0) {
  hipStream_t st = (hipStream_t)s;
  int r = fb_geglu_check("geglu_bwd", dy, pre, dpre, M, F, drop_p, idx0);
  if (r != MMVQA_OK) return r;
  const long n4 = M * (F / 4);
  hipLaunchKernelGGL(fb_geglu_bwd_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, dy, pre, dpre, M, F, drop_p, seed,
                     idx0);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

int k_fb_reorder(hipStream_t st, const float* src, float* dst, int B, int T, int H, int to_window) {
  if (!src || !dst || B <= 0 || T <= 0 || H <= 0 || (H & 3) || !al16(src) || !al16(dst))
    return mmvqa_set_error(MMVQA_ERR_ARG, "fb_reorder: B=%d T=%d H=%d", B, T, H);
  const long n4 = (long)B * T * (H / 4);
  hipLaunchKernelGGL(fb_reorder_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, src, dst, B, T, H / 4, to_window);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}
