// Forward-only self-attention with per-sample key lengths for the BERT teacher (head dimension 64, T <= 512):
//   out[b][i][h][:] = softmax_j( q_i . k_j * scale ; j < len[b] ) . v_j          1 <= len[b] <= T
// No dropout, nothing saved for a backward pass, no score tensor in HBM, no LDS, no atomics.
//
// One wave owns (batch b, head, 32-query tile), as attention.hip's forward does, and the scores are produced
// TRANSPOSED (the wave-tile idiom of wave_tile.h: keys on accumulator registers, queries on lanes) so that the
// probability tile is directly the A operand of the P.V product on v_mfma_f32_32x32x2_f32.  The key axis is a RUN-TIME
// loop over ceil(len[b] / 32) tiles with an online softmax: running maximum m, running sum l and the two 32 x 32
// output accumulators rescaled by exp(m_old - m_new) per tile.  Each tile's order of operations is fixed, so the result
// is bit-equal from launch to launch, and what a query computes does not depend on the lane or tile it sits in.
//
// Lengths: keys j >= len[b] are SELECTED out (probability exactly 0, the v row replaced by 0), never read, and tiles
// that lie wholly past len[b] are not visited; an additive -10000 is not used.  Query rows i >= len[b] (i < T) are
// computed like any other row, over the valid keys.  A len[b] outside [1, T] makes every output row of that sample NaN
// and reads nothing (the convention of distill.hip).
#include "common.h"
#include "kernels.h"
#include "wave_tile.h"

#include <cstdint>

#define BA_D 64          // head dimension
#define BA_D2 32         // what one lane half carries of a q / k row
#define BA_MAX_T 512

struct BertAttnParams {
  const float* q;
  const float* k;
  const float* v;
  float* out;
  const int* len;
  int row_stride, head_stride, out_row_stride, out_head_stride;
  int B, T, heads;
  float scale;
};

template <int VW>
__global__ __launch_bounds__(64) void attn_len_fwd_kernel(const BertAttnParams p) {
  const int lane = threadIdx.x, li = lane & 31, lh = lane >> 5;
  const int it = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
  const int T = p.T;
  const int n = p.len[b];
  const size_t ors = (size_t)p.out_row_stride;
  float* __restrict__ ob = p.out + (size_t)b * T * ors + (size_t)head * p.out_head_stride;

  if (n < 1 || n > T) {   // uniform over the wave: nothing of q / k / v is read
    const float nan = __int_as_float(0x7fc00000);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int i = it * 32 + tile_row(e, lh);
      if (i < T) { ob[(size_t)i * ors + li] = nan; ob[(size_t)i * ors + 32 + li] = nan; }
    }
    return;
  }

  const size_t rs = (size_t)p.row_stride;
  const size_t base = (size_t)b * T * rs + (size_t)head * p.head_stride;
  const float* __restrict__ qb = p.q + base;
  const float* __restrict__ kb = p.k + base;
  const float* __restrict__ vb = p.v + base;

  const int qi = it * 32 + li;
  float qf[BA_D2];
  load_half_row<BA_D2, VW>(qb + (size_t)qi * rs + lh * BA_D2, qi < T, qf);

  // O[query tile_row(e, lh)][d = li] and [d = 32 + li], not yet divided by the row sum
  f32x16 o0 = tile_zero(), o1 = tile_zero();
  float m = -INFINITY, l = 0.f;   // running maximum / sum of query qi (the same value in both lane halves)

  const int nt = (n + 31) >> 5;
  for (int jt = 0; jt < nt; ++jt) {
    // every tile visited holds at least one valid key (jt * 32 < n), so its maximum is finite
    const int kj = jt * 32 + li;
    float kf[BA_D2];
    load_half_row<BA_D2, VW>(kb + (size_t)kj * rs + lh * BA_D2, kj < n, kf);
    // the tile's v rows, issued ahead of the score product: key tile_row(e, lh) on the registers, d on the lanes
    float v0[16], v1[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int j = jt * 32 + tile_row(e, lh);
      v0[e] = 0.f; v1[e] = 0.f;
      if (j < n) {
        const float* __restrict__ vr = vb + (size_t)j * rs + li;
        v0[e] = vr[0]; v1[e] = vr[32];
      }
    }

    f32x16 a = tile_product<BA_D2>(kf, qf);

    float mt = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int j = jt * 32 + tile_row(e, lh);
      const float s = (j < n) ? a[e] * p.scale : -INFINITY;
      a[e] = s;
      mt = fmaxf(mt, s);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float mn = fmaxf(m, mt);
    const float alpha = expf(m - mn);          // first tile: exp(-inf) = 0 against zero accumulators
    float ps = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float pr = (a[e] == -INFINITY) ? 0.f : expf(a[e] - mn);
      a[e] = pr;
      ps += pr;
    }
    ps += __shfl_xor(ps, 32, 64);
    l = l * alpha + ps;
    m = mn;

    // the accumulators carry queries on their registers: the factor of query tile_row(e, lh) lives in lane tile_row(e, lh)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float ar = __shfl(alpha, tile_row(e, lh), 64);
      o0[e] *= ar; o1[e] *= ar;
    }
    // O += P V: A = the probability tile as it stands (row = query on lanes, k = key on registers / half), B = v rows
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], v0[e], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], v1[e], o1, 0, 0, 0);
    }
  }

  const float inv = 1.0f / l;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int i = it * 32 + tile_row(e, lh);
    const float r = __shfl(inv, tile_row(e, lh), 64);
    if (i < T) {
      ob[(size_t)i * ors + li] = o0[e] * r;
      ob[(size_t)i * ors + 32 + li] = o1[e] * r;
    }
  }
}

extern "C" int mmvqa_attention_len_fwd(mmvqa_stream_t s, const float* q, const float* k, const float* v, int row_stride,
                                       int head_stride, float* out, int out_row_stride, int out_head_stride,
                                       const int* len, int B, int T, int heads, float scale) {
  hipStream_t st = (hipStream_t)s;
  const char* who = "attention_len_fwd";
  if (!q || !k || !v || !out || !len)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: null operand (q, k, v, out and len are required)", who);
  if (B < 1 || T < 1 || heads < 1) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: B=%d T=%d heads=%d (all >= 1)", who, B, T, heads);
  if (T > BA_MAX_T) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: T=%d > %d unsupported", who, T, BA_MAX_T);
  if (B > 65535 || heads > 65535)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: B=%d heads=%d are more than one launch takes (65535)", who, B, heads);
  if (row_stride < BA_D || out_row_stride < BA_D || head_stride < 0 || out_head_stride < 0)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: row strides %d / %d below the head dimension %d, or a negative head stride", who,
                           row_stride, out_row_stride, BA_D);
  if ((row_stride & 3) || (head_stride & 3) || (out_row_stride & 3) || (out_head_stride & 3))
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: strides must be multiples of 4 (row %d head %d out row %d out head %d)", who,
                           row_stride, head_stride, out_row_stride, out_head_stride);
  BertAttnParams p;
  p.q = q; p.k = k; p.v = v; p.out = out; p.len = len;
  p.row_stride = row_stride; p.head_stride = head_stride;
  p.out_row_stride = out_row_stride; p.out_head_stride = out_head_stride;
  p.B = B; p.T = T; p.heads = heads; p.scale = scale;
  // 16-byte loads of the q / k half rows need aligned bases (the strides are multiples of 4); element loads otherwise
  const bool vec = ((((uintptr_t)q) | ((uintptr_t)k)) & 15) == 0;
  const dim3 grid((unsigned)((T + 31) / 32), (unsigned)heads, (unsigned)B);
  if (vec) hipLaunchKernelGGL(attn_len_fwd_kernel<4>, grid, dim3(64), 0, st, p);
  else hipLaunchKernelGGL(attn_len_fwd_kernel<1>, grid, dim3(64), 0, st, p);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}
