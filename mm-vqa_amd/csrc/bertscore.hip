// BERTScore F1 positive mask of SupCon pre-training (models/SupConLoss/supcon_utils.py:170-182: mask[i][j] = F1 of
// caption i against the translation sample j drew, unit diagonal), from token states that are resident on the device.
// The library (bert_score) is restated, not pinned: its greedy_cos_idf with idf = False, one candidate against one
// reference, so no padding ever enters a score.  For texts with unit-length states c[0..la) and r[0..lb), position 0
// [CLS] and the last position [SEP]:
//   S[t][u] = <c_t, r_u>  over ALL positions (the specials are match targets)
//   P = mean over t in 1..la-2 of max_u S[t][u]          R = mean over u in 1..lb-2 of max_t S[t][u]
//   F = 2 P R / (P + R), NaN -> 0; an empty text (len == 2) gives P = R = F = 0; F <- (F - b) / (1 - b) with a baseline b
//
// One workgroup of four waves per pair (i, j); j is the fast grid axis, so the workgroups in flight share candidate i's
// states in L2.  S is produced in 32 x 32 tiles on v_mfma_f32_32x32x2_f32 (wave_tile.h: candidates on the accumulator
// registers, references on the lanes), the K loop runs over D in chunks of 64 floats that a lane half loads as 16-byte pieces of its
// own row, the next chunk's loads issued ahead of this chunk's 32 products.  Wave w owns the row tiles ti = w, w + 4, ...
// and walks all column tiles: the running row maxima stay in registers (one value per accumulator element, folded over
// the lanes once per row tile), the column maxima of a tile go to the wave's own [T] strip in LDS.  One barrier, then a
// fixed-order fold of the strips and fixed-order sums.  No [n][n][T][T] tensor exists anywhere.
//
// No atomics, no order that depends on timing: the MFMA is a k-ordered fmaf chain, maxima do not depend on order and the
// two sums run in one fixed order, so the same inputs give the same bits on every launch and in every process (under
// data parallelism every rank builds the global mask itself).  Positions >= len are SELECTED out, never read: a lane
// whose row lies past the length feeds zeros and its products enter no maximum; tiles wholly past a length are not
// visited.  A len outside [2, T] gives NaN in the row (lenA) or column (lenB) it touches and reads nothing (the
// convention of distill.hip and bertattn.hip); the diagonal is 1 whatever the lengths are.
#include "common.h"
#include "kernels.h"
#include "wave_tile.h"

#include <cstdint>

#define BS_MAX_T 512
#define BS_MAX_D 1024
#define BS_WAVES 4
#define BS_KC 64         // floats of a row per K chunk
#define BS_KH 32         // of which one lane half carries

__global__ __launch_bounds__(64 * BS_WAVES) void bertscore_kernel(const float* __restrict__ xa, const int* __restrict__ lenA,
                                                                 const float* __restrict__ xb, const int* __restrict__ lenB,
                                                                 float* __restrict__ mask, float* __restrict__ prec,
                                                                 float* __restrict__ rec, int n, int T, int D,
                                                                 float baseline) {
  __shared__ float s_row[BS_MAX_T];               // max_u S[t][u]: row t is written by the one wave that owns its tile
  __shared__ float s_col[BS_WAVES][BS_MAX_T];     // max over wave w's rows of S[t][u]
  __shared__ float s_red[2][BS_WAVES];
  const int j = blockIdx.x, i = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const size_t o = (size_t)i * n + j;
  // every early return below is uniform over the workgroup and precedes the first barrier
  if (i == j) {
    if (tid == 0) { mask[o] = 1.0f; if (prec) { prec[o] = 1.0f; rec[o] = 1.0f; } }
    return;
  }
  const int la = lenA[i], lb = lenB[j];
  if (la < 2 || la > T || lb < 2 || lb > T) {   // nothing of xa / xb is read
    const float nan = __int_as_float(0x7fc00000);
    if (tid == 0) { mask[o] = nan; if (prec) { prec[o] = nan; rec[o] = nan; } }
    return;
  }
  const float inv_b = 1.0f - baseline;
  if (la == 2 || lb == 2) {                     // an empty text: the library scores it 0
    if (tid == 0) { mask[o] = baseline != 0.0f ? (0.0f - baseline) / inv_b : 0.0f; if (prec) { prec[o] = 0.0f; rec[o] = 0.0f; } }
    return;
  }

  const float* __restrict__ A = xa + (size_t)i * T * D;
  const float* __restrict__ B = xb + (size_t)j * T * D;
  const int nta = (la + 31) >> 5, ntb = (lb + 31) >> 5;
  // the strip element (wave, u) is only ever touched by lane (u & 31, half 0) of that wave
  if (lh == 0)
    for (int tj = 0; tj < ntb; ++tj) s_col[wave][tj * 32 + li] = -INFINITY;

  for (int ti = wave; ti < nta; ti += BS_WAVES) {
    const int t = ti * 32 + li;                 // this lane's candidate row (the A operand's row)
    const bool okA = t < la;
    const float* __restrict__ ap = A + (size_t)t * D + lh * BS_KH;
    float rm[16];                               // max over the columns u = li (mod 32) seen so far of S[row of e][u]
#pragma unroll
    for (int e = 0; e < 16; ++e) rm[e] = -INFINITY;

    for (int tj = 0; tj < ntb; ++tj) {
      const int u = tj * 32 + li;               // this lane's reference row (the B operand's column)
      const bool okB = u < lb;
      const float* __restrict__ bp = B + (size_t)u * D + lh * BS_KH;
      f32x16 acc = tile_zero();
      float af[BS_KH], bf[BS_KH], an[BS_KH], bn[BS_KH];
      load_half_row<BS_KH, 4>(ap, okA, af);
      load_half_row<BS_KH, 4>(bp, okB, bf);
      for (int k = 0; k < D; k += BS_KC) {
        const bool more = k + BS_KC < D;        // uniform
        if (more) {
          load_half_row<BS_KH, 4>(ap + k + BS_KC, okA, an);
          load_half_row<BS_KH, 4>(bp + k + BS_KC, okB, bn);
        }
        acc = tile_mac<BS_KH>(af, bf, acc);
        if (more) {
#pragma unroll
          for (int s = 0; s < BS_KH; ++s) { af[s] = an[s]; bf[s] = bn[s]; }
        }
      }
      // acc[e] = S[ti * 32 + tile_row(e, lh)][u]
      float cm = -INFINITY;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float sv = acc[e];
        if (okB) rm[e] = fmaxf(rm[e], sv);
        if (ti * 32 + tile_row(e, lh) < la) cm = fmaxf(cm, sv);
      }
      cm = fmaxf(cm, __shfl_xor(cm, 32, 64));
      if (lh == 0 && okB) s_col[wave][u] = fmaxf(s_col[wave][u], cm);
    }
    // the row maxima over the 32 lanes of a half; lane li == e of half lh then stores row tile_row(e, lh)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      float v = rm[e];
#pragma unroll
      for (int sh = 16; sh > 0; sh >>= 1) v = fmaxf(v, __shfl_xor(v, sh, 64));
      const int te = ti * 32 + tile_row(e, lh);
      if (li == e && te < la) s_row[te] = v;
    }
  }
  __syncthreads();

  // weight 1 for the word pieces 1 .. len-2, weight 0 for [CLS] and [SEP]; thread tid takes positions tid, tid + 256
  float ps = 0.f, rs = 0.f;
  for (int t = tid; t < T; t += 64 * BS_WAVES) {
    if (t >= 1 && t < la - 1) ps += s_row[t];
    if (t >= 1 && t < lb - 1) {
      float c = s_col[0][t];
#pragma unroll
      for (int w = 1; w < BS_WAVES; ++w) c = fmaxf(c, s_col[w][t]);
      rs += c;
    }
  }
  ps = wave_sum(ps);
  rs = wave_sum(rs);
  if (lane == 0) { s_red[0][wave] = ps; s_red[1][wave] = rs; }
  __syncthreads();
  if (tid == 0) {
    const float P = ((s_red[0][0] + s_red[0][1]) + (s_red[0][2] + s_red[0][3])) / (float)(la - 2);
    const float R = ((s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3])) / (float)(lb - 2);
    float F = 2.0f * P * R / (P + R);
    if (F != F) F = 0.0f;
    if (baseline != 0.0f) F = (F - baseline) / inv_b;
    mask[o] = F;
    if (prec) { prec[o] = P; rec[o] = R; }
  }
}

extern "C" int mmvqa_bertscore_mask(mmvqa_stream_t s, const float* xa, const int* lenA, const float* xb,
                                    const int* lenB, float* mask, float* prec, float* rec, int n, int T, int D,
                                    float baseline) {
  hipStream_t st = (hipStream_t)s;
  const char* who = "bertscore_mask";
  if (!xa || !xb || !lenA || !lenB || !mask)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: null operand (xa, lenA, xb, lenB and mask are required)", who);
  if ((prec == nullptr) != (rec == nullptr))
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: prec and rec go together (both or neither)", who);
  if (n < 1 || n > 65535) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: n=%d (1..65535: one launch, a grid axis per text)", who, n);
  if (T < 2 || T > BS_MAX_T) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: T=%d (2..%d)", who, T, BS_MAX_T);
  if (D < BS_KC || D % BS_KC != 0 || D > BS_MAX_D)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: D=%d (a multiple of %d in %d..%d, the teacher's widths)", who, D, BS_KC, BS_KC,
                           BS_MAX_D);
  if ((((uintptr_t)xa) | ((uintptr_t)xb)) & 15)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: xa and xb must be 16-byte aligned (16-byte loads of the rows)", who);
  if (baseline == 1.0f || baseline != baseline)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: baseline=%g (a rescaling by 1 - baseline needs baseline != 1)", who, (double)baseline);
  hipLaunchKernelGGL(bertscore_kernel, dim3((unsigned)n, (unsigned)n), dim3(64 * BS_WAVES), 0, st, xa, lenA, xb, lenB, mask,
                     prec, rec, n, T, D, baseline);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}
