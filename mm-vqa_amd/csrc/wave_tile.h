// The wave-level 32 x 32 tile idiom of the attention kernels (attention.hip, qkvattn.hip, bertattn.hip, bertscore.hip),
// device code only.
//
// A tile is the f32x16 accumulator of v_mfma_f32_32x32x2_f32: lane l = (lh = l >> 5, li = l & 31) holds, in register e,
// the element [row tile_row(e, lh)][column li].  Scores are produced TRANSPOSED (S^T[j][i] = K_j . Q_i: keys on the
// registers, queries on the lanes), so that
//  * a reduction over the keys is an in-register reduction plus one exchange between the two lane halves, and
//  * the probability tile is directly the A operand of the P.V MFMA (its k index = key sits on the registers / lane
//    half exactly as the instruction wants it; see cdna_hip_programming.md "An accumulator tile as the next MFMA's
//    operand").
// The attention-dropout stream lives here too: the forward kernels draw the mask and attn_bwd_kernel regenerates it in
// another launch, so there is one definition of the decision.
#pragma once
#include "common.h"

// row of accumulator register e in lane half lh of a 32 x 32 MFMA result
__device__ __forceinline__ int tile_row(int e, int lh) { return (e & 3) + 8 * (e >> 2) + 4 * lh; }

// N consecutive floats of a row (what one lane half carries of it): 16-byte loads when VW == 4 (p 16-byte aligned),
// element loads otherwise
template <int N, int VW>
__device__ __forceinline__ void load_half_row(const float* p, float (&r)[N]) {
  if constexpr (VW == 4) {
#pragma unroll
    for (int s = 0; s < N; s += 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(p + s);
      r[s] = t[0]; r[s + 1] = t[1]; r[s + 2] = t[2]; r[s + 3] = t[3];
    }
  } else {
#pragma unroll
    for (int s = 0; s < N; ++s) r[s] = p[s];
  }
}
template <int N>
__device__ __forceinline__ void zero_row(float (&r)[N]) {
#pragma unroll
  for (int s = 0; s < N; ++s) r[s] = 0.f;
}
// the same for a row that may not exist: zeros, and nothing read, when !ok
template <int N, int VW>
__device__ __forceinline__ void load_half_row(const float* p, bool ok, float (&r)[N]) {
  if (ok) load_half_row<N, VW>(p, r);
  else zero_row(r);
}

__device__ __forceinline__ f32x16 tile_zero() {
  f32x16 t;
#pragma unroll
  for (int e = 0; e < 16; ++e) t[e] = 0.f;
  return t;
}

// acc[row of a][row of b] += sum_s a[s] * b[s] over both lane halves: a chain of N MFMAs in the order s = 0 .. N-1
template <int N>
__device__ __forceinline__ f32x16 tile_mac(const float (&a)[N], const float (&b)[N], f32x16 acc) {
#pragma unroll
  for (int s = 0; s < N; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
  return acc;
}
template <int N>
__device__ __forceinline__ f32x16 tile_product(const float (&a)[N], const float (&b)[N]) {
  return tile_mac<N>(a, b, tile_zero());
}

// Softmax over the keys of NJ transposed score tiles, given this lane's maximum mx over its own registers: sc becomes
// exp(s - max) (-inf -> 0) and the return value is what turns it into probabilities, 1 / sum (0 for a query that does
// not exist)
template <int NJ>
__device__ __forceinline__ float tile_softmax(f32x16 (&sc)[NJ], float mx, bool qvalid) {
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float ex = (sc[jt][e] == -INFINITY) ? 0.f : expf(sc[jt][e] - mx);
      sc[jt][e] = ex;
      sum += ex;
    }
  }
  sum += __shfl_xor(sum, 32, 64);
  return qvalid ? 1.0f / sum : 0.f;
}

// Attention dropout: probability (b, head, query, key) is kept iff its counter-based uniform is >= p, and kept values
// are scaled by ks.  bh = b * heads + head.
struct AttnDrop {
  uint32_t seed;
  float p, ks;
  __device__ __forceinline__ AttnDrop(uint32_t seed_, float p_) : seed(seed_), p(p_), ks(p_ > 0.f ? 1.0f / (1.0f - p_) : 1.f) {}
  __device__ __forceinline__ bool keep(int bh, int T, int query, int key) const {
    return rng_uniform(seed, (uint32_t)((bh * T + query) * T + key)) >= p;
  }
};
