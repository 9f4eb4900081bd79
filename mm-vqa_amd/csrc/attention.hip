// Fused self-attention for T <= 128 on the gfx950 fp32-input MFMA; no LDS, no score tensor in HBM
// other than the probabilities kept for backward.
//
// One wave owns (batch b, head, 32-query tile).  Scores are produced TRANSPOSED (S^T[j][i] = K_j . Q_i: keys on
// accumulator registers, queries on lanes): the wave-tile idiom of wave_tile.h, which also defines the dropout stream.
//
// Covers both encoders of the reference:
//   BertLayer  (models/transformer.py:19-30): S/sqrt(d) - 10000(1-mask[key]); softmax; dropout; .V
//   RealFormer (models/realformer.py:30-45) : S/sqrt(d) + prev - 10000(1-mask[QUERY]); prev<-S; softmax; .V
// fp32 op order follows the reference: (q.k)/sqrt(d), then +prev, then -10000*(1-m).
// A QUERY mask shifts a whole row by one constant, which the softmax cancels: prev_out gets the shifted score as the
// reference writes it, but the softmax of such a row takes the unshifted one.  Subtracting 10000 in fp32 first would
// round the row's scores to a grid of 2^-10 and leave its probabilities (and through dK / dV every gradient) ~2e-4 off
// the exact result.
#include "wave_tile.h"

// Global operands of the forward kernel that its one-tile form (HOIST) prefetches and its other forms load at the point
// of use: the address is written once, here, and both places call it.
__device__ __forceinline__ float key_mask(const long long* mask, int b, int T, int j) { return (float)mask[b * T + j]; }
// [b][query][key][head] of prev_in / prev_out
__device__ __forceinline__ size_t prev_at(int b, int T, int query, int key, int heads, int head) {
  return ((size_t)(b * T + query) * T + key) * heads + head;
}
// element dd of row r of sample b of a [B*T][stride] operand (this head's columns from hoff); 0 outside
template <int D>
__device__ __forceinline__ float ld_elem(const float* x, int b, int T, int r, int dd, int stride, size_t hoff) {
  return (r < T && dd < D) ? x[(size_t)(b * T + r) * stride + hoff + dd] : 0.f;
}

// --------------------------------------------------------------------------- forward
template <int D, int NJ>
__global__ __launch_bounds__(64) void attn_fwd_kernel(const AttnParams p) {
  constexpr int D2 = D / 2, VW = (D2 % 4 == 0) ? 4 : 1, ND = (D + 31) / 32;
  const int lane = threadIdx.x, li = lane & 31, lh = lane >> 5;
  const int it = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
  const int T = p.T;
  const int qi = it * 32 + li;
  const bool qvalid = qi < T;
  const size_t hb = (size_t)head * p.head_stride;

  float qf[D2];
  if (qvalid) load_half_row<D2, VW>(p.q + (size_t)(b * T + qi) * p.row_stride + hb + lh * D2, qf);
  else zero_row(qf);
  const float qmask = (qvalid && p.mask_on_query) ? (float)p.mask[b * T + qi] : 1.f;

  // One 32-key tile (T <= 32, the bench's shape): every global load of the kernel is issued here, before the first
  // store.  The stores below (prev_out, probs, out) may alias the inputs as far as the compiler knows, so loads placed
  // after them each waited for a full memory round trip: 20 us for 64 MFMAs of work (round-2 profile).
  constexpr bool HOIST = (NJ == 1);
  float h_mk[HOIST ? 16 : 1], h_pv[HOIST ? 16 : 1], h_v[HOIST ? ND * 16 : 1];
  if constexpr (HOIST) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int j = tile_row(e, lh);
      const bool ok = j < T && qvalid;
      h_mk[e] = (ok && !p.mask_on_query) ? key_mask(p.mask, b, T, j) : 1.f;
      h_pv[e] = (ok && p.prev_in) ? p.prev_in[prev_at(b, T, qi, j, p.heads, head)] : 0.f;
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) h_v[dt * 16 + e] = ld_elem<D>(p.v, b, T, j, dt * 32 + li, p.row_stride, hb);
    }
  }

  f32x16 sc[NJ];
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt) {
    float kf[D2];
    const int kj = jt * 32 + li;
    if (kj < T) load_half_row<D2, VW>(p.k + (size_t)(b * T + kj) * p.row_stride + hb + lh * D2, kf);
    else zero_row(kf);
    sc[jt] = tile_product<D2>(kf, qf);
  }

  // scale, residual, mask; row max
  float mx = -INFINITY;
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int j = jt * 32 + tile_row(e, lh);
      float s = -INFINITY;
      if (j < T && qvalid) {
        s = sc[jt][e] / p.sqrt_d;
        const size_t po = prev_at(b, T, qi, j, p.heads, head);
        if (p.prev_in) s = s + (HOIST ? h_pv[e] : p.prev_in[po]);
        const float mval = p.mask_on_query ? qmask : (HOIST ? h_mk[e] : key_mask(p.mask, b, T, j));
        const float sm = s - 10000.0f * (1.0f - mval);
        if (p.prev_out) p.prev_out[po] = sm;
        if (!p.mask_on_query) s = sm;
      }
      sc[jt][e] = s;
      mx = fmaxf(mx, s);
    }
  }
  const float inv = tile_softmax<NJ>(sc, mx, qvalid);
  const AttnDrop drop(p.seed, p.drop_p);
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int j = jt * 32 + tile_row(e, lh);
      float pr = sc[jt][e] * inv;
      if (p.probs && j < T && qvalid) p.probs[((size_t)(b * p.heads + head) * T + j) * T + qi] = pr;
      if (drop.p > 0.f) pr = drop.keep(b * p.heads + head, T, qi, j) ? pr * drop.ks : 0.f;
      sc[jt][e] = pr;
    }
  }

  // O[i][d] = sum_j P[i][j] V[j][d]: A = P^T accumulator (k = key on registers/half), B = V rows
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) {
    f32x16 o = tile_zero();
    const int dd = dt * 32 + li;
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int j = jt * 32 + tile_row(e, lh);
        const float vv = HOIST ? h_v[dt * 16 + e] : ld_elem<D>(p.v, b, T, j, dd, p.row_stride, hb);
        o = __builtin_amdgcn_mfma_f32_32x32x2f32(sc[jt][e], vv, o, 0, 0, 0);
      }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int i = it * 32 + tile_row(e, lh);
      if (i < T && dd < D)
        p.out[(size_t)(b * T + i) * p.out_row_stride + (size_t)head * p.out_head_stride + dd] = o[e];
    }
  }
}

// --------------------------------------------------------------------------- backward
// One wave per (b, head).  Pass A (queries on lanes): dP^T, delta_i = sum_j dP.P, dS^T -> dQ.
// Pass B (keys on lanes): dP, dS -> dK, dV.  Both passes recompute their tiles from q/k/v/dout,
// so nothing but P (and the dropout seed) is carried from forward.
template <int D, int NJ>
__global__ __launch_bounds__(64) void attn_bwd_kernel(const AttnParams p) {
  constexpr int D2 = D / 2, VW = (D2 % 4 == 0) ? 4 : 1, ND = (D + 31) / 32;
  const int lane = threadIdx.x, li = lane & 31, lh = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const int T = p.T;
  const size_t hb = (size_t)head * p.head_stride;
  const size_t ohb = (size_t)head * p.out_head_stride;
  const AttnDrop drop(p.seed, p.drop_p);
  const int bh = b * p.heads + head;
  const size_t pbase = (size_t)bh * T * T;

  float delta[NJ];  // delta[it] for query it*32+li
  // One 32 x 32 tile (T <= 32): every global load of both passes is issued here, before the first store (see the
  // forward kernel: the dq / dprev stores would otherwise fence the loads of pass B behind them, one round trip each)
  constexpr bool HOIST = (NJ == 1);
  float h_pa[HOIST ? 16 : 1], h_pb[HOIST ? 16 : 1], h_da[HOIST ? 16 : 1], h_db[HOIST ? 16 : 1];
  float h_k[HOIST ? ND * 16 : 1], h_q[HOIST ? ND * 16 : 1], h_do[HOIST ? ND * 16 : 1];
  if constexpr (HOIST) {
    const bool lv = li < T;   // this lane's query (pass A) / key (pass B) exists
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int r = tile_row(e, lh);   // the key of pass A, the query of pass B
      const bool ok = r < T && lv;
      h_pa[e] = ok ? p.probs[pbase + (size_t)r * T + li] : 0.f;
      h_pb[e] = ok ? p.probs[pbase + (size_t)li * T + r] : 0.f;
      h_da[e] = (ok && p.dprev_in) ? p.dprev_in[((size_t)(b * T + li) * T + r) * p.heads + head] : 0.f;
      h_db[e] = (ok && p.dprev_in) ? p.dprev_in[((size_t)(b * T + r) * T + li) * p.heads + head] : 0.f;
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) {
        const int dd = dt * 32 + li;
        const bool okd = r < T && dd < D;
        h_k[dt * 16 + e] = okd ? p.k[(size_t)(b * T + r) * p.row_stride + hb + dd] : 0.f;
        h_q[dt * 16 + e] = okd ? p.q[(size_t)(b * T + r) * p.row_stride + hb + dd] : 0.f;
        h_do[dt * 16 + e] = okd ? p.dout[(size_t)(b * T + r) * p.out_row_stride + ohb + dd] : 0.f;
      }
    }
  }
  // ------------------------------ pass A
#pragma unroll
  for (int it = 0; it < NJ; ++it) {
    const int qi = it * 32 + li;
    const bool qvalid = qi < T;
    float dof[D2];
    if (qvalid) load_half_row<D2, VW>(p.dout + (size_t)(b * T + qi) * p.out_row_stride + ohb + lh * D2, dof);
    else zero_row(dof);
    f32x16 ds[NJ];
    float dl = 0.f;
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt) {
      float vf[D2];
      const int kj = jt * 32 + li;
      if (kj < T) load_half_row<D2, VW>(p.v + (size_t)(b * T + kj) * p.row_stride + hb + lh * D2, vf);
      else {   // written out, not zero_row(vf): with it attn_bwd_kernel<96, 2> compiled to other register counts
#pragma unroll
        for (int s = 0; s < D2; ++s) vf[s] = 0.f;
      }
      const f32x16 a = tile_product<D2>(vf, dof);   // a[e] = dP'[i=qi][j(e)]  (grad wrt post-dropout probabilities)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int j = jt * 32 + tile_row(e, lh);
        float pr = 0.f, dp = 0.f;
        if (j < T && qvalid) {
          if constexpr (HOIST) pr = h_pa[e];
          else pr = p.probs[pbase + (size_t)j * T + qi];
          dp = a[e];
          if (drop.p > 0.f) dp = drop.keep(bh, T, qi, j) ? dp * drop.ks : 0.f;
        }
        dl += dp * pr;
        ds[jt][e] = pr * dp;  // dS = P*dP - P*delta once delta is known (P is re-read: tiny, cache-resident)
      }
    }
    dl += __shfl_xor(dl, 32, 64);
    delta[it] = dl;
    // dS^T[j][i] = P*dP - P*delta (+ dprev) ; then dQ += dS . K / sqrt(d)
    f32x16 dq[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) dq[dt] = tile_zero();
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int j = jt * 32 + tile_row(e, lh);
        float g = 0.f;
        if (j < T && qvalid) {
          float pr;
          if constexpr (HOIST) pr = h_pa[e];
          else pr = p.probs[pbase + (size_t)j * T + qi];
          g = ds[jt][e] - pr * dl;
          const size_t po = ((size_t)(b * T + qi) * T + j) * p.heads + head;
          if constexpr (HOIST) { if (p.dprev_in) g += h_da[e]; }
          else { if (p.dprev_in) g += p.dprev_in[po]; }
          if (p.dprev_out) p.dprev_out[po] = g;
          g = g / p.sqrt_d;
        }
        ds[jt][e] = g;
      }
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) {
        const int dd = dt * 32 + li;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int j = jt * 32 + tile_row(e, lh);
          float kv;
          if constexpr (HOIST) kv = h_k[dt * 16 + e];
          else kv = (j < T && dd < D) ? p.k[(size_t)(b * T + j) * p.row_stride + hb + dd] : 0.f;
          dq[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ds[jt][e], kv, dq[dt], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
      const int dd = dt * 32 + li;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = it * 32 + tile_row(e, lh);
        if (i < T && dd < D) p.dq[(size_t)(b * T + i) * p.row_stride + hb + dd] = dq[dt][e];
      }
    }
  }

  // ------------------------------ pass B (keys on lanes)
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt) {
    const int kj = jt * 32 + li;
    const bool kvalid = kj < T;
    float vf[D2];
    if (kvalid) load_half_row<D2, VW>(p.v + (size_t)(b * T + kj) * p.row_stride + hb + lh * D2, vf);
    else zero_row(vf);
    f32x16 dk[ND], dv[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) { dk[dt] = tile_zero(); dv[dt] = tile_zero(); }
#pragma unroll
    for (int it = 0; it < NJ; ++it) {
      float dof[D2];
      const int qi_l = it * 32 + li;
      if (qi_l < T) load_half_row<D2, VW>(p.dout + (size_t)(b * T + qi_l) * p.out_row_stride + ohb + lh * D2, dof);
      else zero_row(dof);
      // a[e] = dP'[i(e)][j=kj] = dO_i . V_j   (A = dO rows -> registers carry i, B = V rows -> lanes carry j)
      const f32x16 a = tile_product<D2>(dof, vf);
      f32x16 pd, sd;  // P' (post-dropout) and dS, element e <-> query i(e), lane <-> key kj
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = it * 32 + tile_row(e, lh);
        const float dli = __shfl(delta[it], tile_row(e, lh), 64);  // delta of query i lives in lane (i & 31)
        float pr = 0.f, prd = 0.f, g = 0.f;
        if (i < T && kvalid) {
          if constexpr (HOIST) pr = h_pb[e];
          else pr = p.probs[pbase + (size_t)kj * T + i];
          float dp = a[e];
          prd = pr;
          if (drop.p > 0.f) {
            const bool keep = drop.keep(bh, T, i, kj);
            dp = keep ? dp * drop.ks : 0.f;
            prd = keep ? pr * drop.ks : 0.f;
          }
          g = pr * (dp - dli);
          if constexpr (HOIST) { if (p.dprev_in) g += h_db[e]; }
          else { if (p.dprev_in) g += p.dprev_in[((size_t)(b * T + i) * T + kj) * p.heads + head]; }
          g = g / p.sqrt_d;
        }
        pd[e] = prd; sd[e] = g;
      }
      // dK[j][d] += sum_i dS[i][j] Q[i][d] ; dV[j][d] += sum_i P'[i][j] dO[i][d]
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) {
        const int dd = dt * 32 + li;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = it * 32 + tile_row(e, lh);
          const bool ok = (i < T && dd < D);
          float qv, dov;
          if constexpr (HOIST) { qv = h_q[dt * 16 + e]; dov = h_do[dt * 16 + e]; }
          else {
            qv = ok ? p.q[(size_t)(b * T + i) * p.row_stride + hb + dd] : 0.f;
            dov = ok ? p.dout[(size_t)(b * T + i) * p.out_row_stride + ohb + dd] : 0.f;
          }
          // A operand must carry k = i on registers/half with the OUTPUT row (key) on lanes:
          // sd/pd have lane <-> key, register <-> query, i.e. A^T; the MFMA wants A[row=key][k=query].
          // v_mfma A operand: lane l supplies A[row = l&31][k = l>>5]  -> row = key (lane) OK, k = query half.
          dk[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(sd[e], qv, dk[dt], 0, 0, 0);
          dv[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(pd[e], dov, dv[dt], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
      const int dd = dt * 32 + li;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int j = jt * 32 + tile_row(e, lh);
        if (j < T && dd < D) {
          p.dk[(size_t)(b * T + j) * p.row_stride + hb + dd] = dk[dt][e];
          p.dv[(size_t)(b * T + j) * p.row_stride + hb + dd] = dv[dt][e];
        }
      }
    }
  }
}

// --------------------------------------------------------------------------- host
template <int D>
static int attn_dispatch(const AttnParams& p, int bwd, hipStream_t st) {
  const int nj = (p.T + 31) / 32;
  dim3 gf(nj, p.heads, p.B), gb(1, p.heads, p.B);
#define L(NJ_)                                                                               \
  do {                                                                                       \
    if (bwd) hipLaunchKernelGGL((attn_bwd_kernel<D, NJ_>), gb, dim3(64), 0, st, p);          \
    else hipLaunchKernelGGL((attn_fwd_kernel<D, NJ_>), gf, dim3(64), 0, st, p);              \
  } while (0)
  switch (nj) {
    case 1: L(1); break;
    case 2: L(2); break;
    case 3: L(3); break;
    case 4: L(4); break;
    default: return mmvqa_set_error(MMVQA_ERR_ARG, "attention: T=%d > 128 unsupported", p.T);
  }
#undef L
  KERNEL_CHECK_RET();
  return MMVQA_OK;
}

int mmvqa_launch_attention(const AttnParams& p, int head_dim, int bwd, hipStream_t st) {
  if (p.B <= 0 || p.T <= 0 || p.heads <= 0 || !(p.drop_p >= 0.f && p.drop_p < 1.f))
    return mmvqa_set_error(MMVQA_ERR_ARG, "attention: B=%d T=%d heads=%d drop_p=%g", p.B, p.T, p.heads, (double)p.drop_p);
  if (!p.q || !p.k || !p.v || !p.mask || !p.probs) return mmvqa_set_error(MMVQA_ERR_ARG, "attention: null operand");
  if ((p.row_stride & 3) || (p.head_stride & 3) || (p.out_row_stride & 3) || (p.out_head_stride & 3))
    return mmvqa_set_error(MMVQA_ERR_ARG, "attention: strides must be multiples of 4");
  if (bwd && (!p.dout || !p.dq || !p.dk || !p.dv))
    return mmvqa_set_error(MMVQA_ERR_ARG, "attention backward: null gradient pointer");
  if (!bwd && !p.out) return mmvqa_set_error(MMVQA_ERR_ARG, "attention: null output");
  switch (head_dim) {
    case 8: return attn_dispatch<8>(p, bwd, st);
    case 12: return attn_dispatch<12>(p, bwd, st);
    case 64: return attn_dispatch<64>(p, bwd, st);
    case 96: return attn_dispatch<96>(p, bwd, st);
    default: return mmvqa_set_error(MMVQA_ERR_ARG, "attention: head_dim=%d unsupported (8,12,64,96)", head_dim);
  }
}

extern "C" int mmvqa_attention(const mmvqa_attn_desc* d, int head_dim, int backward, mmvqa_stream_t s) {
  if (!d) return mmvqa_set_error(MMVQA_ERR_ARG, "attention: null operand");
  return mmvqa_launch_attention(*d, head_dim, backward, (hipStream_t)s);
}
