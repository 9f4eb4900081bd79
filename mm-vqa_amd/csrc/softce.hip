// Soft-target cross entropy of the VQA-Med fine-tuning loop, forward and backward in one launch:
//   mode 0  hard target                              nn.CrossEntropyLoss (vqamed2019/utils.py:1261-1264)
//   mode 1  uniform smoothing, LabelSmoothing        vqamed2019/utils.py:178-200
//   mode 2  smoothing by question category,          vqamed2019/utils.py:1247-1260, 1296-1300
//           LabelSmoothByCategory
// Per row:  soft_j = base_j, with soft_t OVERWRITTEN by `confidence` in mode 2 (:1254) and `confidence` ADDED at t in
// modes 0 / 1;  base_j = 0 | smoothing / C | table[category][j].
//   row_loss = sum_j soft_j (lse - x_j)          every term >= 0: nothing cancels
//   dlogits_j = (S p_j - soft_j) gscale          S = sum_j soft_j (< 1 in mode 2 when t is in its category's set),
//                                                p_j = exp(x_j - lse)
// One 256-thread workgroup per row.  Up to SCE_COLS columns a thread holds its 8 logits and 8 soft targets in registers:
// the row is read from memory once.  Longer rows take the streaming form of the same code, which walks the row in pieces
// of SCE_COLS columns twice (max / sum / S, then loss / gradient).  16-byte loads and stores where the leading dimension
// is a multiple of 4 and the base is 16-byte aligned, whole vectors only; the last C % 4 columns, and everything
// otherwise, go one float at a time.  A target outside [0, C) or a category outside [0, n_cat) makes the row's loss and
// gradient NaN and reads nothing from the table.  The mean over the rows is a second launch of one workgroup that adds
// the row losses in a fixed order: the loss is bit-equal from run to run.
#include "common.h"
#include "kernels.h"

#define SCE_COLS 2048                         // columns held in registers: 256 threads x 2 x float4
#define SCE_PER (SCE_COLS / 256)

// columns c0 + 4 (threadIdx.x + 256 u) + e, u = 0..1, e = 0..3, of one row; columns >= C read as `fill`
__device__ __forceinline__ void sce_load(const float* __restrict__ r, bool vec, int c0, int C, float fill,
                                         float (&v)[SCE_PER]) {
#pragma unroll
  for (int u = 0; u < SCE_PER / 4; ++u) {
    const int base = c0 + 4 * ((int)threadIdx.x + 256 * u);
    if (vec && base + 3 < C) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(r + base);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * u + e] = q[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * u + e] = base + e < C ? r[base + e] : fill;
    }
  }
}

// (max, sum of exp(x - max)) of two disjoint parts of a row
__device__ __forceinline__ void sce_combine(float& m, float& s, float om, float os) {
  const float M = fmaxf(m, om);
  const float sa = m == -INFINITY ? 0.f : s * expf(m - M);
  const float sb = om == -INFINITY ? 0.f : os * expf(om - M);
  m = M; s = sa + sb;
}

template <bool STREAM>
__global__ void __launch_bounds__(256) soft_ce_kernel(const float* __restrict__ logits, int ld,
                                                      const long long* __restrict__ target,
                                                      const long long* __restrict__ category,
                                                      const float* __restrict__ table, int table_ld, int n_cat, int mode,
                                                      float confidence, float uniform, float* __restrict__ row_loss,
                                                      float* __restrict__ dlogits, int dld, int C, float gscale,
                                                      int vec_x, int vec_t, int vec_d) {
  __shared__ float red[3][4];
  const int row = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* x = logits + (size_t)row * ld;
  const long long tg64 = target[row];
  bool bad = tg64 < 0 || tg64 >= C;
  const float* trow = nullptr;
  if (mode == 2) {
    const long long cat = category[row];
    if (cat < 0 || cat >= n_cat) bad = true;
    else trow = table + (size_t)cat * table_ld;
  }
  const int tg = bad ? -1 : (int)tg64;

  // soft targets of the columns sce_load hands this thread from c0 (0 in the pad columns)
  auto soft = [&](int c0, float (&sv)[SCE_PER]) {
    if (trow) sce_load(trow, vec_t != 0, c0, C, 0.f, sv);
#pragma unroll
    for (int k = 0; k < SCE_PER; ++k) {
      const int col = c0 + 4 * ((int)threadIdx.x + 256 * (k >> 2)) + (k & 3);
      if (!trow) sv[k] = col < C ? uniform : 0.f;
      if (col == tg) sv[k] = mode == 2 ? confidence : sv[k] + confidence;
    }
  };

  float xv[SCE_PER], sv[SCE_PER];
  float m = -INFINITY, s = 0.f, S = 0.f;
  const int c_end = STREAM ? C : 1;
  for (int c0 = 0; c0 < c_end; c0 += SCE_COLS) {
    sce_load(x, vec_x != 0, c0, C, -INFINITY, xv);
    soft(c0, sv);
    float cm = m;
#pragma unroll
    for (int k = 0; k < SCE_PER; ++k) { cm = fmaxf(cm, xv[k]); S += sv[k]; }
    if (cm > -INFINITY) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < SCE_PER; ++k) acc += expf(xv[k] - cm);      // exp(-inf) = 0 in the pad columns
      s = (m == -INFINITY ? 0.f : s * expf(m - cm)) + acc;
      m = cm;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
    sce_combine(m, s, om, os);
  }
  S = wave_sum(S);
  if (lane == 0) { red[0][wave] = m; red[1][wave] = s; red[2][wave] = S; }
  __syncthreads();
  m = red[0][0]; s = red[1][0];
#pragma unroll
  for (int w = 1; w < 4; ++w) sce_combine(m, s, red[0][w], red[1][w]);
  S = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
  if (bad) S = __int_as_float(0x7fc00000);
  const float lse = m + logf(s);
  __syncthreads();

  float loss = 0.f;
  float* d = dlogits ? dlogits + (size_t)row * dld : nullptr;
  for (int c0 = 0; c0 < c_end; c0 += SCE_COLS) {
    if (STREAM) {
      sce_load(x, vec_x != 0, c0, C, -INFINITY, xv);
      soft(c0, sv);
    }
#pragma unroll
    for (int u = 0; u < SCE_PER / 4; ++u) {
      const int base = c0 + 4 * ((int)threadIdx.x + 256 * u);
      f32x4 g;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = 4 * u + e;
        const bool in = base + e < C;
        if (in) loss += sv[k] * (lse - xv[k]);
        g[e] = in ? (S * expf(xv[k] - lse) - sv[k]) * gscale : 0.f;
      }
      if (d && base < C) {
        if (vec_d) *reinterpret_cast<f32x4*>(d + base) = g;        // dld >= round_up(C, 4): the pad columns get 0
        else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (base + e < C) d[base + e] = g[e];
        }
      }
    }
  }
  loss = wave_sum(loss);
  if (lane == 0) red[0][wave] = loss;
  __syncthreads();
  if (threadIdx.x == 0)
    row_loss[row] = bad ? __int_as_float(0x7fc00000) : (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
}

// loss = mean(row_loss): one workgroup, a fixed order of additions
__global__ void __launch_bounds__(256) soft_ce_mean_kernel(const float* __restrict__ row_loss, float* __restrict__ loss,
                                                           int rows) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < rows; i += 256) s += row_loss[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *loss = ((red[0] + red[1]) + (red[2] + red[3])) / (float)rows;
}

static bool sce_vec_ok(const void* p, int ld) { return p && (ld & 3) == 0 && ((uintptr_t)p & 15) == 0; }

extern "C" int mmvqa_soft_ce_loss(mmvqa_stream_t s, const float* logits, int ld, const long long* target,
                                  const long long* category, const float* table, int table_ld, int n_cat, int mode,
                                  double smoothing, float* row_loss, float* loss, float* dlogits, int dld, int rows,
                                  int C, float gscale) {
  hipStream_t st = (hipStream_t)s;
  if (mode < 0 || mode > 2) return mmvqa_set_error(MMVQA_ERR_ARG, "soft_ce_loss: mode=%d (0 hard, 1 uniform, 2 category table)", mode);
  if (rows <= 0 || C <= 0) return mmvqa_set_error(MMVQA_ERR_ARG, "soft_ce_loss: rows=%d C=%d (both >= 1)", rows, C);
  if (!logits || !target || !row_loss || !loss) return mmvqa_set_error(MMVQA_ERR_ARG, "soft_ce_loss: null operand");
  if (ld < C) return mmvqa_set_error(MMVQA_ERR_ARG, "soft_ce_loss: ld=%d < C=%d", ld, C);
  if (dlogits && dld < C) return mmvqa_set_error(MMVQA_ERR_ARG, "soft_ce_loss: dld=%d < C=%d", dld, C);
  if (mode == 2) {
    if (!table || !category) return mmvqa_set_error(MMVQA_ERR_ARG, "soft_ce_loss: mode 2 needs the category table and the category ids");
    if (table_ld < C) return mmvqa_set_error(MMVQA_ERR_ARG, "soft_ce_loss: table_ld=%d < C=%d", table_ld, C);
    if (n_cat < 1) return mmvqa_set_error(MMVQA_ERR_ARG, "soft_ce_loss: n_cat=%d (>= 1)", n_cat);
  }
  if (!(smoothing >= 0.0 && smoothing <= 1.0)) return mmvqa_set_error(MMVQA_ERR_ARG, "soft_ce_loss: smoothing=%g outside [0, 1]", smoothing);
  // the reference keeps both as Python doubles and rounds once, on the store into the fp32 target (utils.py:1237,1254)
  const float confidence = mode == 0 ? 1.0f : (float)(1.0 - smoothing);
  const float uniform = mode == 1 ? (float)(smoothing / (double)C) : 0.0f;
  const int vx = sce_vec_ok(logits, ld), vt = mode == 2 && sce_vec_ok(table, table_ld), vd = sce_vec_ok(dlogits, dld);
  if (C <= SCE_COLS)
    hipLaunchKernelGGL(soft_ce_kernel<false>, dim3(rows), dim3(256), 0, st, logits, ld, target, category, table, table_ld,
                       n_cat, mode, confidence, uniform, row_loss, dlogits, dld, C, gscale, vx, vt, vd);
  else
    hipLaunchKernelGGL(soft_ce_kernel<true>, dim3(rows), dim3(256), 0, st, logits, ld, target, category, table, table_ld,
                       n_cat, mode, confidence, uniform, row_loss, dlogits, dld, C, gscale, vx, vt, vd);
  KERNEL_CHECK_RET();
  hipLaunchKernelGGL(soft_ce_mean_kernel, dim3(1), dim3(256), 0, st, row_loss, loss, rows);
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}
