// Per-tensor statistics of a flat fp32 buffer (mmvqa_amd.watch.TensorStats): counts of finite / nan / +-inf / zero values,
// exact min and max, fp64 sum and sum of squares and a 64-bin histogram between min and max, for every segment of a
// table in a constant number of launches.
//
//   launch 1  ts_moments_kernel   one workgroup per CHUNK of a segment -> one partial per chunk in the workspace
//   launch 2  ts_combine_kernel   one workgroup per segment: its partials in a fixed order -> the record (histogram zeroed)
//   launch 3  ts_hist_kernel      one workgroup per chunk again, with the segment's final min / max from its record
//
// A workgroup finds its segment by a binary search of blockIdx in the table's chunk0 column (the running chunk count,
// filled on the host by mmvqa_tensor_stats_workspace): the grid is the total number of chunks whatever the number of
// segments, the 23 M word-embedding table gets thousands of workgroups and a bias of 4 floats one.  Only [offset,
// offset + numel) of a segment is read, never the padding behind it.  Results are bit-identical from call to call:
// every element has a fixed thread, every reduction a fixed tree, the chunk partials are combined in chunk order per
// thread and the only atomics are integer adds of histogram counts.  No workgroup waits for another inside a launch.
#include "kernels.h"

namespace {

constexpr int CHUNK = MMVQA_TENSOR_STATS_CHUNK;
constexpr int BINS = MMVQA_TENSOR_HIST_BINS;
constexpr int THREADS = 256;
static_assert(BINS == 64, "one histogram bin per lane of a wave");
static_assert(CHUNK % (THREADS * 4) == 0, "a chunk is a whole number of float4 rounds of the workgroup");
constexpr int ROUNDS = CHUNK / (THREADS * 4);

struct Partial {
  double sum, sumsq;
  float mn, mx;
  unsigned n_finite, n_nan, n_posinf, n_neginf, n_zero, pad;
};
static_assert(sizeof(Partial) == 48, "workspace layout");

struct Acc {
  double sum, sumsq;
  float mn, mx;
  unsigned n_finite, n_nan, n_posinf, n_neginf, n_zero;
  __device__ __forceinline__ void clear() {
    sum = sumsq = 0.0;
    mn = __builtin_inff(); mx = -__builtin_inff();
    n_finite = n_nan = n_posinf = n_neginf = n_zero = 0;
  }
  __device__ __forceinline__ void take(float x) {
    if (__builtin_isfinite(x)) {
      const double d = (double)x;
      sum += d;
      sumsq += d * d;          // exact: 48 significant bits
      mn = fminf(mn, x);
      mx = fmaxf(mx, x);
      n_finite += 1;
      n_zero += x == 0.f;
    } else if (x != x) {
      n_nan += 1;
    } else if (x > 0.f) {
      n_posinf += 1;
    } else {
      n_neginf += 1;
    }
  }
  __device__ __forceinline__ void merge(const Acc& o) {
    sum += o.sum; sumsq += o.sumsq;
    mn = fminf(mn, o.mn); mx = fmaxf(mx, o.mx);
    n_finite += o.n_finite; n_nan += o.n_nan; n_posinf += o.n_posinf; n_neginf += o.n_neginf; n_zero += o.n_zero;
  }
};

// the segment of workgroup `b`: the last entry whose chunk0 <= b (chunk0 is strictly ascending: every segment, an empty
// one too, owns at least one chunk)
__device__ __forceinline__ int seg_of_chunk(const mmvqa_stat_seg* __restrict__ segs, int nseg, long long b) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].chunk0 <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// calls f(x) for every element of chunk `c` of the segment at `p` (numel floats); float4 loads when p is 16-byte
// aligned.  The element -> thread assignment depends on nothing but (numel, c).
template <class F>
__device__ __forceinline__ void for_chunk(const float* __restrict__ p, long long numel, long long c, F&& f) {
  const long long lo = c * CHUNK;
  const int n = (int)(numel - lo < CHUNK ? numel - lo : CHUNK);
  const float* __restrict__ q = p + lo;
  if (((uintptr_t)q & 15) == 0 && n == CHUNK) {
    // a whole chunk, which is nearly all of a large tensor: every load of the thread is issued before the first use
    // (same elements per thread, in the same order, as the loop below)
    f32x4 v[ROUNDS];
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) v[k] = reinterpret_cast<const f32x4*>(q)[threadIdx.x + k * THREADS];
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) { f(v[k][0]); f(v[k][1]); f(v[k][2]); f(v[k][3]); }
  } else if (((uintptr_t)q & 15) == 0) {
    const int n4 = n >> 2;
    for (int i = threadIdx.x; i < n4; i += THREADS) {
      const f32x4 v = reinterpret_cast<const f32x4*>(q)[i];
      f(v[0]); f(v[1]); f(v[2]); f(v[3]);
    }
    const int t = (n4 << 2) + threadIdx.x;
    if (t < n) f(q[t]);
  } else {
    for (int i = threadIdx.x; i < n; i += THREADS) f(q[i]);
  }
}

__device__ __forceinline__ double shfl_down_f64(double v, int d) {
  const long long b = __double_as_longlong(v);
  const int lo = __shfl_down((int)(b & 0xffffffffll), d, 64), hi = __shfl_down((int)(b >> 32), d, 64);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// the workgroup's accumulators -> thread 0, by a fixed tree: lanes of a wave, then the waves in order
__device__ __forceinline__ Acc block_reduce(Acc a) {
  __shared__ Acc part[THREADS / 64];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    Acc o;
    o.sum = shfl_down_f64(a.sum, d); o.sumsq = shfl_down_f64(a.sumsq, d);
    o.mn = __shfl_down(a.mn, d, 64); o.mx = __shfl_down(a.mx, d, 64);
    o.n_finite = __shfl_down(a.n_finite, d, 64); o.n_nan = __shfl_down(a.n_nan, d, 64);
    o.n_posinf = __shfl_down(a.n_posinf, d, 64); o.n_neginf = __shfl_down(a.n_neginf, d, 64);
    o.n_zero = __shfl_down(a.n_zero, d, 64);
    a.merge(o);     // (lanes whose partner is past the wave merge their own copy: only lane 0's value is used)
  }
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < THREADS / 64; ++w) a.merge(part[w]);
  return a;
}

__global__ __launch_bounds__(THREADS) void ts_moments_kernel(const float* __restrict__ base,
                                                             const mmvqa_stat_seg* __restrict__ segs, int nseg,
                                                             Partial* __restrict__ ws) {
  const long long b = blockIdx.x;
  const int s = seg_of_chunk(segs, nseg, b);
  Acc a;
  a.clear();
  for_chunk(base + segs[s].offset, segs[s].numel, b - segs[s].chunk0, [&](float x) { a.take(x); });
  a = block_reduce(a);
  if (threadIdx.x == 0) {
    Partial p;
    p.sum = a.sum; p.sumsq = a.sumsq; p.mn = a.mn; p.mx = a.mx;
    p.n_finite = a.n_finite; p.n_nan = a.n_nan; p.n_posinf = a.n_posinf; p.n_neginf = a.n_neginf; p.n_zero = a.n_zero;
    p.pad = 0;
    ws[b] = p;
  }
}

// 64-bit counts of a segment: a chunk's fit 32 bits, a segment's need not
struct Counts { long long n_finite, n_nan, n_posinf, n_neginf, n_zero; };

__global__ __launch_bounds__(THREADS) void ts_combine_kernel(const mmvqa_stat_seg* __restrict__ segs, int nseg,
                                                             long long nchunks, const Partial* __restrict__ ws,
                                                             mmvqa_tensor_stat* __restrict__ out, int with_hist) {
  const int s = blockIdx.x;
  const long long c0 = segs[s].chunk0, c1 = s + 1 < nseg ? segs[s + 1].chunk0 : nchunks;
  // thread t takes chunks t, t + 256, ... in ascending order; then the fixed tree of block_reduce
  Acc a;
  a.clear();
  Counts n = {0, 0, 0, 0, 0};
  for (long long c = c0 + threadIdx.x; c < c1; c += THREADS) {
    const Partial p = ws[c];
    a.sum += p.sum; a.sumsq += p.sumsq;
    a.mn = fminf(a.mn, p.mn); a.mx = fmaxf(a.mx, p.mx);
    n.n_finite += p.n_finite; n.n_nan += p.n_nan; n.n_posinf += p.n_posinf; n.n_neginf += p.n_neginf; n.n_zero += p.n_zero;
  }
  __shared__ Counts cnt[THREADS];
  cnt[threadIdx.x] = n;
  a = block_reduce(a);          // (its barrier also publishes cnt)
  if (threadIdx.x == 0) {
    Counts t = {0, 0, 0, 0, 0};
    for (int i = 0; i < THREADS; ++i) {
      t.n_finite += cnt[i].n_finite; t.n_nan += cnt[i].n_nan; t.n_posinf += cnt[i].n_posinf;
      t.n_neginf += cnt[i].n_neginf; t.n_zero += cnt[i].n_zero;
    }
    mmvqa_tensor_stat* r = out + s;
    r->sum = a.sum; r->sumsq = a.sumsq;
    r->n_finite = t.n_finite; r->n_nan = t.n_nan; r->n_posinf = t.n_posinf; r->n_neginf = t.n_neginf; r->n_zero = t.n_zero;
    r->min = a.mn; r->max = a.mx;
  }
  if (with_hist && threadIdx.x < BINS) out[s].hist[threadIdx.x] = 0;
}

// Histogram of one chunk.  Gradients put nearly everything into a handful of bins, so one LDS atomic per element would
// queue the 64 lanes of a wave on one address.  Instead each wave owns a sub-histogram and counts by ballot: the bin of
// the first lane still waiting is broadcast, the lanes holding the same bin are counted with one popcount and retire
// together, at most PEEL times; whatever is still waiting after that (spread-out data: few lanes per bin, so little
// queueing) takes an LDS atomic each.  The sub-histograms are summed per bin and non-zero sums go to the record with
// one integer atomic each.  PEEL_N = 0 is the form without the ballots, an LDS atomic per element into the wave's
// sub-histogram: kept for the comparison of DESIGN.md section 23 (MMVQA_TENSOR_STATS_PEEL=0), same counts.
constexpr int PEEL = 4;

template <int PEEL_N>
__device__ __forceinline__ void wave_count(unsigned* __restrict__ h, int bin, bool valid) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < PEEL_N; ++it) {
    const unsigned long long waiting = __ballot(valid);
    if (waiting == 0) return;
    const int leader = __ffsll((long long)waiting) - 1;
    const int b = __builtin_amdgcn_readlane(bin, leader);   // (leader comes from a ballot: wave-uniform)
    const bool same = valid && bin == b;
    const unsigned long long m = __ballot(same);
    if (lane == leader) h[b] += (unsigned)__popcll(m);   // the wave's own sub-histogram: no other wave touches it
    valid = valid && !same;
  }
  if (valid) atomicAdd(&h[bin], 1u);
}

template <int PEEL_N>
__global__ __launch_bounds__(THREADS) void ts_hist_kernel(const float* __restrict__ base,
                                                          const mmvqa_stat_seg* __restrict__ segs, int nseg,
                                                          mmvqa_tensor_stat* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ unsigned hist[THREADS / 64][BINS];
  const long long b = blockIdx.x;
  const int s = seg_of_chunk(segs, nseg, b);
  hist[threadIdx.x >> 6][threadIdx.x & 63] = 0;
  __syncthreads();
  const float mn = out[s].min, mx = out[s].max;
  // the rule of include/mmvqa.h, every operation rounded on its own: scale = 64 / (max - min) and
  // pos = (x - min) * scale in fp64; max == min (and a segment without a finite value, where nothing is counted): bin 0
  const double dmn = (double)mn;
  const bool flat = !(mx > mn);
  const double scale = flat ? 0.0 : __ddiv_rn((double)BINS, __dsub_rn((double)mx, dmn));
  unsigned* h = hist[threadIdx.x >> 6];
  // every lane of a wave must reach wave_count together: the loop bounds of for_chunk are not wave-uniform at a ragged
  // end, so the element loop is restated here with a uniform trip count and a `valid` flag per lane
  const long long numel = segs[s].numel, lo = (b - segs[s].chunk0) * CHUNK;
  const int n = (int)(numel - lo < CHUNK ? numel - lo : CHUNK);
  const float* __restrict__ q = base + segs[s].offset + lo;
  auto count = [&](float x, bool in) {
    const bool valid = in && __builtin_isfinite(x);
    int bin = 0;
    if (valid && !flat) {
      const int t = (int)__dmul_rn(__dsub_rn((double)x, dmn), scale);
      bin = t < BINS - 1 ? (t > 0 ? t : 0) : BINS - 1;   // (t >= 0 by the rule: x >= min; the lower clamp keeps the LDS index safe)
    }
    wave_count<PEEL_N>(h, bin, valid);
  };
  if (((uintptr_t)q & 15) == 0 && n == CHUNK) {      // as in for_chunk: the loads first
    f32x4 v[ROUNDS];
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) v[k] = reinterpret_cast<const f32x4*>(q)[threadIdx.x + k * THREADS];
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) { count(v[k][0], true); count(v[k][1], true); count(v[k][2], true); count(v[k][3], true); }
  } else if (((uintptr_t)q & 15) == 0) {
    const int n4 = n >> 2;
    for (int i0 = 0; i0 < n4; i0 += THREADS) {
      const int i = i0 + threadIdx.x;
      const bool in = i < n4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (in) v = reinterpret_cast<const f32x4*>(q)[i];
      count(v[0], in); count(v[1], in); count(v[2], in); count(v[3], in);
    }
    if ((n & 3) != 0) {          // block-uniform
      const int t = (n4 << 2) + threadIdx.x;
      const bool in = t < n;
      count(in ? q[t] : 0.f, in);
    }
  } else {
    for (int i0 = 0; i0 < n; i0 += THREADS) {
      const int i = i0 + threadIdx.x;
      const bool in = i < n;
      count(in ? q[i] : 0.f, in);
    }
  }
  __syncthreads();
  if (threadIdx.x < BINS) {
    unsigned t = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) t += hist[w][threadIdx.x];
    if (t) atomicAdd(&out[s].hist[threadIdx.x], t);
  }
}

// checks the table and gives every entry its chunk0; -> the number of chunks, or -1 with the error set
long long plan_table(const char* who, mmvqa_stat_seg* segs, int nseg, bool fill) {
  if (!segs) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: null pointer", who);
  if (nseg <= 0) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: nseg=%d", who, nseg);
  long long pos = 0, chunks = 0;
  for (int i = 0; i < nseg; ++i) {
    mmvqa_stat_seg& sg = segs[i];
    if (sg.offset < 0 || sg.numel < 0)
      return mmvqa_set_error(MMVQA_ERR_ARG, "%s: segment %d has negative offset=%lld or numel=%lld", who, i, sg.offset, sg.numel);
    if (sg.offset > (1ll << 62))
      return mmvqa_set_error(MMVQA_ERR_ARG, "%s: segment %d has offset=%lld", who, i, sg.offset);
    if (sg.numel > 0xffffffffll)
      return mmvqa_set_error(MMVQA_ERR_ARG, "%s: segment %d has numel=%lld, more than a 32-bit histogram count holds", who, i, sg.numel);
    if (sg.offset < pos)
      return mmvqa_set_error(MMVQA_ERR_ARG, "%s: segment %d at offset=%lld starts before the end %lld of the one before it "
                             "(segments are ascending and disjoint)", who, i, sg.offset, pos);
    if (fill) sg.chunk0 = chunks;
    else if (sg.chunk0 != chunks)
      return mmvqa_set_error(MMVQA_ERR_ARG, "%s: segment %d has chunk0=%lld, expected %lld (mmvqa_tensor_stats_workspace "
                             "fills it)", who, i, sg.chunk0, chunks);
    const long long c = (sg.numel + CHUNK - 1) / CHUNK;
    chunks += c > 0 ? c : 1;
    pos = sg.offset + sg.numel;
  }
  if (chunks > 0x7fffffffll) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: %lld chunks, more than one grid holds", who, chunks);
  return chunks;
}

}  // namespace

extern "C" size_t mmvqa_sizeof_tensor_stat(void) { return sizeof(mmvqa_tensor_stat); }
extern "C" size_t mmvqa_sizeof_stat_seg(void) { return sizeof(mmvqa_stat_seg); }

extern "C" size_t mmvqa_tensor_stats_workspace(mmvqa_stat_seg* segs, int nseg) {
  const long long chunks = plan_table("tensor_stats_workspace", segs, nseg, true);
  return chunks < 0 ? 0 : (size_t)chunks * sizeof(Partial);
}

extern "C" int mmvqa_tensor_stats(mmvqa_stream_t s, const float* base, long long n, const mmvqa_stat_seg* segs,
                                  const mmvqa_stat_seg* segs_dev, int nseg, mmvqa_tensor_stat* out, void* ws,
                                  size_t ws_bytes, int flags) {
  hipStream_t st = (hipStream_t)s;
  // everything the kernels' addressing relies on is checked here, on the host copy of the table, before any HIP call
  if (!base || !segs || !segs_dev || !out || !ws) return mmvqa_set_error(MMVQA_ERR_ARG, "tensor_stats: null pointer");
  if (flags & ~MMVQA_TENSOR_STATS_MOMENTS_ONLY) return mmvqa_set_error(MMVQA_ERR_ARG, "tensor_stats: unknown flags=%d", flags);
  const long long chunks = plan_table("tensor_stats", const_cast<mmvqa_stat_seg*>(segs), nseg, false);
  if (chunks < 0) return MMVQA_ERR_ARG;
  const mmvqa_stat_seg& last = segs[nseg - 1];
  if (n < 0 || last.offset + last.numel > n)
    return mmvqa_set_error(MMVQA_ERR_ARG, "tensor_stats: segment %d [%lld, %lld) reaches beyond the buffer's %lld floats",
                           nseg - 1, last.offset, last.offset + last.numel, n);
  if (ws_bytes < (size_t)chunks * sizeof(Partial))
    return mmvqa_set_error(MMVQA_ERR_ARG, "tensor_stats: workspace of %zu bytes, %zu needed", ws_bytes,
                           (size_t)chunks * sizeof(Partial));
  const int with_hist = (flags & MMVQA_TENSOR_STATS_MOMENTS_ONLY) ? 0 : 1;
  Partial* part = (Partial*)ws;
  hipLaunchKernelGGL(ts_moments_kernel, dim3((unsigned)chunks), dim3(THREADS), 0, st, base, segs_dev, nseg, part);
  KERNEL_CHECK_RET();
  hipLaunchKernelGGL(ts_combine_kernel, dim3((unsigned)nseg), dim3(THREADS), 0, st, segs_dev, nseg, chunks, part, out,
                     with_hist);
  KERNEL_CHECK_RET();
  if (with_hist) {
    const char* peel_s = getenv("MMVQA_TENSOR_STATS_PEEL");
    if (peel_s && atoi(peel_s) == 0)
      hipLaunchKernelGGL(ts_hist_kernel<0>, dim3((unsigned)chunks), dim3(THREADS), 0, st, base, segs_dev, nseg, out);
    else
      hipLaunchKernelGGL(ts_hist_kernel<PEEL>, dim3((unsigned)chunks), dim3(THREADS), 0, st, base, segs_dev, nseg, out);
    KERNEL_CHECK_RET();
  }
  return MMVQA_OK;
}
