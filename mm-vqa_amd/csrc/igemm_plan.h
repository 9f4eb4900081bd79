// Launch plan of the implicit-GEMM family: everything the host decides before igemm_kernel is enqueued (instance,
// split-K, loader family, BatchNorm fold placement, compact class order, ticket or finishing launch, XCD mode, grid and
// LDS bytes) as ONE pure function of the descriptor, igemm_plan.  No HIP here: the plain host compiler builds this
// header, and tests/test_igemm_plan_cpu.py runs the rules under the address / undefined-behaviour sanitizers.  A wrong
// plan is a memory-safety bug -- the uniform-tap loaders let the range check of a 2 GB buffer window stand in for
// per-element bounds tests -- so the rules are written once, here, and igemm.hip only carries a plan out (igemm_run).
//
// Nothing below makes a HIP call, reads the environment, keeps static state or dereferences a pointer of the
// descriptor: pointers are tested for null and copied.
#pragma once
#include <stddef.h>
#include <vector>

#include "host_defs.h"

struct FastDiv {  // q = n / d for 0 <= n < 2^31 (host-computed magic; CUTLASS FastDivmod scheme)
  uint32_t mul, shr, d;
};
struct GemmAux {
  FastDiv ohw, ow;
  int fast;   // 0: general loaders | 1: uniform-tap loaders | 2: uniform-tap loaders with a halo mask (host-decided)
  int stagger;   // 8-wave variant: the second wave group runs its VALU/LDS-write block first (0 = off, for A/B timing)
  float* part;   // split-K over workgroups with a finishing launch: partial tiles [split][M][N] go here, no epilogue
  int ldsc;      // the A-prologue coefficients are folded from raw BatchNorm sums into an LDS table in the setup phase
                 // (mmvqa_bn_fold) and the K loop reads them there
  // ticketed split-K (split over the grid's z WITHOUT a finishing launch): the sk_slots (= splits) workgroups of a tile
  // publish their partial tiles to sk_part and draw a ticket each; the tile is completed by whichever of them arrives
  // LAST (nobody waits): it sums the partial tiles and runs the epilogue.
  int pad0;            // unused: keeps the kernel-argument offsets of the fields behind it (with sk_part 8 bytes lower the
                       // compiler groups the argument loads differently and every kernel's register assignment shifts)
  int sk_gx, sk_gy;    // tile grid
  int sk_slots;        // partial tiles a tile receives (= splits)
  float* sk_part;      // [tile][sk_slots][BM*BN]
  unsigned* sk_cnt;    // [tile] arrival tickets, zero before and after every launch
  int tick;            // 1: this launch is a ticketed split | 0: one workgroup per tile, or a split with a finishing launch (part)
  int xcd;       // workgroup ids are dealt round-robin to the 8 XCDs: renumber so that an XCD gets a CONTIGUOUS run of
                 // tiles (1: the N-tiles of an M-panel, 2: the M-tiles of an N-panel share that XCD's L2 instead of
                 // pulling the panel into up to 8 of them)
  // compact stride-2 data gradient (S2C instantiations only; appended so that every offset above stays where it was):
  // the output pixels are split by parity (y&1, x&1) into four classes of s2_M = images * OH/2 * OW/2 rows; grid.y holds
  // s2_tiles row tiles per class, class slot c = by / s2_tiles has parity bits (s2_ord >> 2c) & 3 = py*2 + px
  FastDiv s2_hw, s2_w;   // row of a class -> (image, i, j): divisors OH/2 * OW/2 and OW/2
  int s2_M, s2_tiles, s2_ord;
};

#define MAX_TAPS 32
#define SK_PART_MAX 8    // most splits of one tile in the ticketed split-K (host-checked)
constexpr int FOLD_MAX_FLOATS = 3072;   // largest LDS table of folded BatchNorm coefficients (12 KB: 1024 channels x P, Q, R)
constexpr int SK_MAX = 8;   // most workgroups one output tile's K range is split over (finishing-launch form)

// LDS geometry of the operand tiles, in floats per buffer.  fp32: [row][k] rows of BK+4 floats, [k][row] rows of
// R+4 floats.  f16: [row][k] rows of BK+8 halves (16-byte rows for ds_read_b128); [k][row] rows of R halves, +32
// when R/2 is a multiple of 32 dwords, so that the four k-rows of one ds_read_b64_tr_b16 block fall on distinct
// banks (row pitch = 16 or 48 dwords mod 64).
constexpr int km_ld_h(int R) { return R + (((R / 2) % 64 == 16 || (R / 2) % 64 == 48) ? 0 : 32); }
constexpr int tile_rowk(int prec, int R, int BK) { return prec == MMVQA_PREC_F16 ? R * (BK + 8) / 2 : R * (BK + 4); }
constexpr int tile_km(int prec, int R, int BK) { return prec == MMVQA_PREC_F16 ? BK * km_ld_h(R) / 2 : BK * (R + 4); }

inline FastDiv make_fastdiv(int d) {
  FastDiv f;
  f.d = (uint32_t)d;
  if (d <= 1) { f.mul = 0; f.shr = 0; f.d = 1; return f; }
  int lg = 31;
  while (lg > 0 && !((uint32_t)d >> lg)) --lg;   // floor(log2 d)
  if (d & (d - 1)) ++lg;                         // ceil(log2 d)
  const int pw = 31 + lg;
  const uint64_t m = ((1ull << pw) + (uint64_t)d - 1) / (uint64_t)d;
  f.mul = (uint32_t)m;
  f.shr = (uint32_t)(pw - 32);
  return f;
}

struct IgemmChoice { int tile, splitk; };   // a per-shape choice of the tuner, a candidate it times
struct IgemmShape { int bm, bn, bk, ks, kind, nchw, prec, s2c; };   // the template arguments of one igemm_kernel instance
// the process's A/B switches (MMVQA_IGEMM_GENERAL, _NOSTAGGER, MMVQA_SK_FINISH, MMVQA_IGEMM_NOXCD, MMVQA_DGRAD_S2_DENSE,
// MMVQA_IGEMM_LOG, MMVQA_SK_GAIN, MMVQA_TUNE_REPS), read once by igemm.hip
struct IgemmSwitches { bool general, no_stagger, sk_finish, no_xcd, s2_dense, log; float sk_gain; int tune_reps; };
struct IgemmPlan {
  IgemmShape shape;        // selects the instance
  GemmParams p;            // the descriptor as the kernel receives it (splitk, ktiles_per_split, c_atomic, default
                           // geometry; a_c0..2 set and a_fold.stat cleared when a coefficient launch goes in front)
  GemmAux x;
  unsigned grid[3]; int threads; size_t smem;
  int coef_launch;         // 0 none | 1 forward coefficients in front | 2 backward coefficients in front
  const double* coef_stat; // the raw sums that launch reads (p.a_fold.stat before it was cleared)
  bool finish;             // splitk_finish_kernel after the main launch (on x.part, p.splitk partial tiles)
};

// dynamic LDS bytes of an instance whose setup folds `fold_floats` BatchNorm coefficients
constexpr size_t igemm_smem_bytes(const IgemmShape& s, size_t fold_floats) {
  const int a_tile = s.kind != KIND_WGRAD ? tile_rowk(s.prec, s.bm, s.bk) : tile_km(s.prec, s.bm, s.bk);
  const int b_tile = s.kind == KIND_FWD ? tile_rowk(s.prec, s.bn, s.bk) : tile_km(s.prec, s.bn, s.bk);
  const size_t tile_floats = (size_t)(2 * a_tile + 2 * b_tile + MAX_TAPS) + fold_floats;
  const size_t epi_floats = (size_t)s.bm * (s.bn + 4) + 8 * s.bn;   // staged output tile + tap accumulators
  return (tile_floats > epi_floats ? tile_floats : epi_floats) * sizeof(float);
}

// tile id of the ABI -> workgroup tile, K-tile depth and wave groups.  5: 8 waves (the K-tile split in 2); 6: 37 KB of
// LDS, four workgroups per CU for short contractions with many tiles.  0 = auto; any other id runs as 3.
struct IgemmTile { int bm, bn, bk, ks; };
constexpr IgemmTile IGEMM_TILES[7] = {{0, 0, 0, 0},    {128, 128, 32, 1}, {128, 64, 32, 1}, {64, 64, 64, 1},
                                      {64, 128, 32, 1}, {64, 64, 64, 2},   {64, 64, 32, 1}};

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// split-K of a forward / data-gradient product over workgroups (partial tiles, ticketed or with a finishing launch):
// the caller gave a scratch, the epilogue is the general one, nothing accumulates into C
inline bool sk_eligible(const GemmParams& p, int kind) {
  return kind != KIND_WGRAD && p.sk_ws && p.sk_ws_floats > 0 && p.epi_mode == EPI_PLAIN && !p.c_atomic;
}

// Loader family of an NHWC product on a bm x bn tile with K-tiles of bk.  The uniform-tap loaders (1, and 2 with a halo
// mask) need: a K-tile never straddles a filter tap, nothing ragged, 31-bit byte offsets.  0: the general loaders.
inline int igemm_loader_family(const GemmParams& p, int kind, int bm, int bn, int bk) {
  if (!(p.K % bk == 0 || (kind == KIND_WGRAD && p.pixmask)) || p.gate) return 0;
  const int taps = p.g_KH * p.g_KW;
  const double lim = 2147483648.0 - 16777216.0;
  if (kind != KIND_WGRAD) {
    const bool pro_ok = (kind == KIND_FWD) ? (p.a_pro == PRO_NONE || p.a_pro == PRO_AFFINE_RELU)
                                           : (p.a_pro == PRO_NONE || p.a_pro == PRO_DZ);
    const double a_bytes = (kind == KIND_FWD) ? (double)p.M * p.g_stride * p.g_stride * p.a_ld * 4.0 + (double)(p.g_SW + 2) * p.g_KH * p.a_ld * 4.0
                                              : (double)p.M * p.a_ld * 4.0;
    const double b_bytes = (kind == KIND_FWD) ? (double)p.N * p.b_ld * 4.0 : (double)p.g_Cs * p.b_ld * 4.0;
    if (pro_ok && p.b_pro == PRO_NONE && p.g_Cs % bk == 0 && p.g_stride <= 2 && a_bytes < lim && b_bytes < lim &&
        (kind == KIND_FWD || p.N % 4 == 0))
      return (taps > 1 || (kind == KIND_DGRAD && p.g_stride > 1)) ? 2 : 1;
    return 0;
  }
  const bool pro_ok = (p.a_pro == PRO_NONE || p.a_pro == PRO_DZ) && (p.b_pro == PRO_NONE || p.b_pro == PRO_AFFINE_RELU);
  if (pro_ok && taps == 1 && p.K % bk == 0 && p.g_stride == 1 && p.g_pad == 0 && p.M % 4 == 0 && p.N % 4 == 0 &&
      (double)p.K * p.a_ld * 4.0 < lim && (double)p.K * p.b_ld * 4.0 < lim)
    return 1;
  // 3x3-like "same" convolution, stride 1, with the caller's tap-validity table; pixels past K are masked by
  // the table's range check, so K need not be a multiple of the K-tile here
  if (pro_ok && taps > 1 && taps <= 32 && p.pixmask && p.g_stride == 1 && p.g_OH == p.g_SH && p.g_OW == p.g_SW &&
      2 * p.g_pad == p.g_KH - 1 && p.g_KH == p.g_KW && bm == 64 && bn == 64 && p.g_Cs % bn == 0 && p.M % 4 == 0 &&
      (double)p.K * p.a_ld * 4.0 < lim && (double)(p.K + (double)p.g_SW * p.g_KH) * p.b_ld * 4.0 < lim)
    return 2;
  return 0;
}

// Compact form of a stride-2 data gradient (igemm_kernel, S2C): the halo family of the uniform-tap loaders at both K-tile
// depths, an output grid with even sides, a plain epilogue, fp32 operands.  Everything else -- and everything under the
// s2_dense or general switch -- takes the dense walk over all KH*KW taps.
inline bool s2c_eligible(const GemmParams& p, int kind, int nchw, const IgemmSwitches& sw) {
  if (sw.s2_dense || sw.general || kind != KIND_DGRAD || nchw || p.g_KH <= 0 || p.g_KW <= 0 || p.g_stride != 2) return false;
  if (p.reserved0 != MMVQA_PREC_F32 || p.epi_mode != EPI_PLAIN || p.c_atomic) return false;
  if ((p.g_OH & 1) || (p.g_OW & 1) || p.M != (p.M / (p.g_OH * p.g_OW)) * p.g_OH * p.g_OW) return false;
  if (((p.g_KH + 1) / 2) * ((p.g_KW + 1) / 2) > MAX_TAPS) return false;   // validity bits of one class
  return p.K == p.g_KH * p.g_KW * p.g_Cs && igemm_loader_family(p, kind, 64, 64, 32) == 2 &&
         igemm_loader_family(p, kind, 64, 64, 64) == 2;
}

// --------------------------------------------------------------------------- descriptor checks
// Host-side consistency check of a descriptor.  The loaders address the operands from (M, N, K, geometry, leading
// dimensions) alone -- the uniform-tap path even lets the hardware range check of a 2 GB buffer window stand in for
// per-element bounds tests -- so a descriptor whose dimensions disagree with each other (or a prologue / epilogue
// option without its tensors) would read outside the caller's buffers.  Such a descriptor is refused here.
#define BAD(...) return mmvqa_set_error(MMVQA_ERR_ARG, "igemm: " __VA_ARGS__)
// the part that does not depend on the product's size: mmvqa_igemm refuses these even for an empty product
inline int validate_operands(const GemmParams& p, int kind, int nchw) {
  if (kind < KIND_FWD || kind > KIND_WGRAD) BAD("kind=%d", kind);
  if (!p.A || !p.B || (!p.C && p.epi_mode != EPI_TAP_FWD)) BAD("null operand");
  if (!nchw) {   // NHWC operands: rows of A and B, and every tap's channel run, start 16-byte aligned
    if ((p.a_ld & 3) || (p.b_ld & 3) || (p.g_KH * p.g_KW > 1 && (p.g_Cs & 3)))
      BAD("a_ld=%d b_ld=%d g_Cs=%d must be multiples of 4", p.a_ld, p.b_ld, p.g_Cs);
    if (kind == KIND_DGRAD && (p.N & 3)) return mmvqa_set_error(MMVQA_ERR_ARG, "igemm dgrad: N=%d must be a multiple of 4", p.N);
  }
  if (p.a_pro == PRO_DZ && (!p.A2 || (!p.a_fold.stat && (!p.a_c0 || !p.a_c1 || !p.a_c2))))
    BAD("PRO_DZ needs A2 and three coefficient arrays (or a_fold)");
  if (p.g_SH <= 0 || p.g_SW <= 0 || p.g_OH <= 0 || p.g_OW <= 0 || p.g_Cs <= 0) BAD("gather geometry not set");
  return MMVQA_OK;
}

inline int validate_desc(const GemmParams& p, int kind, int nchw) {
  if (int r = validate_operands(p, kind, nchw)) return r;
  if (p.reserved0 != MMVQA_PREC_F32 && p.reserved0 != MMVQA_PREC_F16) BAD("unknown operand precision %d (reserved0)", p.reserved0);
  if (p.reserved1 != 0) BAD("reserved1=%d must be 0 (the persistent form was removed)", p.reserved1);
  if (p.reserved0 == MMVQA_PREC_F16 && (p.a_pro == PRO_AFFINE_SILU || p.a_pro == PRO_SILU_GATE || p.b_pro == PRO_AFFINE_SILU ||
                                        p.b_pro == PRO_SILU_GATE || p.gate))
    BAD("the f16 operand family has no SiLU / gate prologues (a_pro %d, b_pro %d)", p.a_pro, p.b_pro);
  const int KH = p.g_KH > 0 ? p.g_KH : 1, KW = p.g_KH > 0 ? p.g_KW : 1;
  const long taps = (long)KH * KW;
  if (KW <= 0 || (p.g_KH > 0 && (p.g_stride <= 0 || p.g_pad < 0))) BAD("bad geometry (KH=%d KW=%d Cs=%d stride=%d pad=%d)", p.g_KH, p.g_KW, p.g_Cs, p.g_stride, p.g_pad);
  const long ohw = (long)p.g_OH * p.g_OW;
  if (kind == KIND_WGRAD) {
    if ((long)p.N != taps * p.g_Cs) BAD("wgrad: N=%d != taps*Cs=%ld", p.N, taps * p.g_Cs);
    if (p.K % ohw) BAD("wgrad: K=%d is not a multiple of OH*OW=%ld", p.K, ohw);
    if (p.a_ld < p.M || (!nchw && p.b_ld < p.g_Cs) || p.c_ld < p.N) BAD("wgrad: leading dimension too small (a_ld=%d M=%d b_ld=%d Cs=%d c_ld=%d N=%d)", p.a_ld, p.M, p.b_ld, p.g_Cs, p.c_ld, p.N);
  } else {
    if ((long)p.K != taps * p.g_Cs) BAD("K=%d != taps*Cs=%ld", p.K, taps * p.g_Cs);
    if (p.M % ohw) BAD("M=%d is not a multiple of OH*OW=%ld", p.M, ohw);
    if (!nchw && p.a_ld < p.g_Cs) BAD("a_ld=%d < Cs=%d", p.a_ld, p.g_Cs);
    if (kind == KIND_FWD && p.b_ld < p.K) BAD("fwd: b_ld=%d < K=%d", p.b_ld, p.K);
    if (kind == KIND_DGRAD && ((long)p.b_ld < (taps - 1) * p.b_tapstride + p.N)) BAD("dgrad: b_ld=%d < (taps-1)*tapstride+N", p.b_ld);
    if (p.epi_mode == EPI_PLAIN && p.c_ld < p.N) BAD("c_ld=%d < N=%d", p.c_ld, p.N);
  }
  if (p.a_fold.stat) {
    const mmvqa_bn_fold& f = p.a_fold;
    if (f.slots <= 0 || f.slots > MMVQA_STAT_SLOTS || (f.slots & (f.slots - 1))) BAD("a_fold.slots=%d is not a power of two <= %d", f.slots, MMVQA_STAT_SLOTS);
    if (!(f.count > 0.0) || !f.gamma) BAD("a_fold without count / gamma");
    if (f.bwd ? (p.a_pro != PRO_DZ || !f.mean || !f.invstd) : (p.a_pro != PRO_AFFINE_RELU || !f.beta)) BAD("a_fold.bwd=%d does not match A prologue %d (or mean / invstd / beta missing)", f.bwd, p.a_pro);
    if (f.publish && (!f.out0 || !f.out1 || !f.out2 || (f.bwd ? (!f.dgamma || !f.dbeta) : !f.out3))) BAD("a_fold.publish without output arrays");
    if (nchw && kind != KIND_WGRAD) BAD("a_fold: not for the NCHW stem forward");
  } else if (p.a_pro != PRO_NONE && (!p.a_c0 || !p.a_c1)) BAD("A prologue %d without coefficients", p.a_pro);
  if (p.stat_slots < 0 || p.stat_slots > MMVQA_STAT_SLOTS || (p.stat_slots & (p.stat_slots - 1))) BAD("stat_slots=%d is not a power of two <= %d", p.stat_slots, MMVQA_STAT_SLOTS);
  if (p.b_pro != PRO_NONE && (!p.b_c0 || !p.b_c1)) BAD("B prologue %d without coefficients", p.b_pro);
  if ((p.a_pro == PRO_SILU_GATE || p.b_pro == PRO_SILU_GATE) && (!p.gate || p.gate_hw <= 0)) BAD("gate prologue without gate tensor");
  if (p.dact != ACT_NONE && !p.Pre) BAD("act' epilogue without the saved pre-activation");
  if (p.stat_bwd && p.stat1 && (!p.Z1 || !p.mean1 || !p.invstd1)) BAD("backward statistics without Z1 / mean / invstd");
  if (p.stat2 && (!p.stat1 || !p.Z2 || !p.mean2 || !p.invstd2)) BAD("second statistics set incomplete");
  if (p.epi_mode == EPI_TAP_FWD && (!p.tap_out || p.tap_HW <= 0)) BAD("tap epilogue without output / HW");
  if (p.epi_mode == EPI_TAP_BWD && (!p.tap_dv || p.tap_HW <= 0)) BAD("tap backward epilogue without dv / HW");
  if (p.Mk && p.mk_ld < p.N) BAD("mask tensor leading dimension %d < N=%d", p.mk_ld, p.N);
  if (p.R && p.r_ld < p.N) BAD("residual leading dimension %d < N=%d", p.r_ld, p.N);
  if (p.drop_p < 0.f || p.drop_p >= 1.f) BAD("dropout p=%g outside [0,1)", (double)p.drop_p);
#undef BAD
  return MMVQA_OK;
}

// --------------------------------------------------------------------------- the plan
// Plan of one launch of a non-empty product that validate_desc accepted.  tile: 0 = auto, else an IGEMM_TILES id.
inline int igemm_plan(const GemmParams& desc, int kind, int nchw, int tile, const IgemmSwitches& sw, IgemmPlan* out) {
  IgemmPlan& pl = *out;
  pl = IgemmPlan{};
  GemmParams& p = pl.p;
  GemmAux& x = pl.x;
  p = desc;
  if (p.g_KH <= 0) { p.g_KH = p.g_KW = 1; p.g_stride = 1; p.g_pad = 0; }
  const bool s2c = s2c_eligible(p, kind, nchw, sw);   // (a compact class has at most MAX_TAPS taps)
  if (!nchw && p.g_KH * p.g_KW > MAX_TAPS && !s2c)
    return mmvqa_set_error(MMVQA_ERR_ARG, "igemm: at most %d taps in the NHWC gather", MAX_TAPS);
  // 32-bit element offsets inside the loaders
  if ((double)p.M * p.a_ld > 2.0e9 && kind != KIND_WGRAD)
    return mmvqa_set_error(MMVQA_ERR_ARG, "igemm: operand A exceeds 2^31 elements");
  if (tile == 0) {
    // enough workgroups to fill 256 CUs (2 resident per CU) before growing the tile
    long t128 = (long)cdiv(p.M, 128) * cdiv(p.N, 128);
    long t12864 = (long)cdiv(p.M, 128) * cdiv(p.N, 64);
    if (t128 >= 384) tile = 1;
    else if (t12864 >= 384 || (p.N <= 64 && p.M >= 4096)) tile = 2;
    else tile = 3;
    // few workgroups and a long contraction: 8 waves per workgroup (two per SIMD)
    if (tile == 3 && kind != KIND_WGRAD && (long)cdiv(p.M, 64) * cdiv(p.N, 64) < 400 && p.K >= 512) tile = 5;
  }
  if (tile < 1 || tile > 6) tile = 3;
  if (nchw) tile = (kind == KIND_FWD) ? 2 : 6;   // the stem: 128x64x32 forward, 64x64x32 weight gradient
  const bool f16 = p.reserved0 == MMVQA_PREC_F16;
  if (f16 && tile == 5) tile = 3;   // the f16 family has no 8-wave variant
  const IgemmTile& t = IGEMM_TILES[tile];
  const int bm = t.bm, bn = t.bn, bk = t.bk;
  pl.shape = IgemmShape{bm, bn, bk, t.ks, kind, nchw ? 1 : 0, f16 ? MMVQA_PREC_F16 : MMVQA_PREC_F32, s2c ? 1 : 0};
  const int nkt = cdiv(p.K, bk);
  const bool ske = !nchw && sk_eligible(p, kind);
  if (p.splitk <= 0) {
    p.splitk = 1;
    const long tiles = (long)cdiv(p.M, bm) * cdiv(p.N, bn);
    if (kind == KIND_WGRAD) {
      int want = (int)((512 + tiles - 1) / tiles);
      int per = bk == 64 ? 2 : 4;                      // at least 128 rows of K per split
      int maxs = nkt / per > 0 ? nkt / per : 1;
      p.splitk = want < maxs ? want : maxs;
      if (p.splitk < 1) p.splitk = 1;
      if (p.splitk > 1) p.c_atomic = 1;
    } else if (ske && tiles <= 128 && p.K >= 1024) {
      // untuned default: fill the chip when the tile grid is small and every split keeps >= 256 of K
      int want = (int)((256 + tiles - 1) / tiles);
      const int maxs = p.K / 256;
      if (want > maxs) want = maxs;
      if (want > 8) want = 8;
      if (want > 1) p.splitk = want;
    }
  }
  if (kind != KIND_WGRAD && !nchw && p.splitk > 1 && !p.c_atomic) {
    if (!ske)
      return mmvqa_set_error(MMVQA_ERR_ARG, "igemm: split-K needs an accumulating epilogue or a scratch (sk_ws)");
    const long long cap = p.sk_ws_floats / ((long long)p.M * p.N);
    if (p.splitk > cap) p.splitk = (int)(cap < 1 ? 1 : cap);
    if (p.splitk > SK_MAX) p.splitk = SK_MAX;
  }
  p.ktiles_per_split = cdiv(nkt, p.splitk);
  p.splitk = cdiv(nkt, p.ktiles_per_split);
  if (p.splitk > 1 && !p.c_atomic && !ske)
    return mmvqa_set_error(MMVQA_ERR_ARG, "igemm: split-K needs an accumulating epilogue");
  if (nchw && kind == KIND_DGRAD) return mmvqa_set_error(MMVQA_ERR_ARG, "igemm: no NCHW dgrad");

  x.ohw = make_fastdiv(p.g_OH * p.g_OW);
  x.ow = make_fastdiv(p.g_OW);
  x.stagger = sw.no_stagger ? 0 : 1;
  x.part = (p.splitk > 1 && !p.c_atomic) ? p.sk_ws : nullptr;   // (ske holds: anything else was refused above)
  x.fast = (nchw || sw.general) ? 0 : igemm_loader_family(p, kind, bm, bn, bk);
  if (s2c && x.fast != 2)
    return mmvqa_set_error(MMVQA_ERR_ARG, "igemm: the compact stride-2 data gradient needs the uniform-tap loaders");
  // BatchNorm coefficients of the A prologue folded in the kernel's setup (mmvqa_bn_fold).  The K loop reads the LDS table
  // only in its uniform-tap forms; the weight gradient keeps its (loop-invariant) coefficients in registers.  Anything
  // else -- general loaders, a table beyond FOLD_MAX_FLOATS -- gets the coefficient launch in front.
  size_t fold_floats = 0;
  if (p.a_fold.stat) {
    const int ncoef = p.a_fold.bwd ? 3 : 2;
    const size_t need = kind != KIND_WGRAD ? (size_t)ncoef * p.g_Cs : (size_t)3 * bm;
    const bool pro_ok = p.a_fold.bwd ? p.a_pro == PRO_DZ : p.a_pro == PRO_AFFINE_RELU;
    if (pro_ok && need <= FOLD_MAX_FLOATS && (kind == KIND_WGRAD || x.fast != 0)) {
      x.ldsc = 1;
      fold_floats = need;
    } else {
      const BnFold& f = p.a_fold;
      if (!f.publish || !f.out0 || !f.out1 || !f.out2)
        return mmvqa_set_error(MMVQA_ERR_ARG, "igemm: this launch cannot fold its BatchNorm coefficients in the kernel and has nowhere to publish them");
      pl.coef_launch = f.bwd ? 2 : 1;
      pl.coef_stat = f.stat;
      p.a_c0 = f.out0; p.a_c1 = f.out1; p.a_c2 = f.out2;
      p.a_fold.stat = nullptr;
    }
  }
  pl.smem = igemm_smem_bytes(pl.shape, fold_floats);
  pl.threads = 256 * t.ks;
  pl.grid[0] = (unsigned)cdiv(p.N, bn); pl.grid[1] = (unsigned)cdiv(p.M, bm); pl.grid[2] = (unsigned)p.splitk;
  x.s2_hw = make_fastdiv(1); x.s2_w = make_fastdiv(1);
  if (s2c) {
    // four parity classes of M / 4 rows each in one grid; the class with the most taps first (its tiles run longest)
    x.s2_hw = make_fastdiv((p.g_OH / 2) * (p.g_OW / 2));
    x.s2_w = make_fastdiv(p.g_OW / 2);
    x.s2_M = p.M / 4;
    x.s2_tiles = cdiv(x.s2_M, bm);
    pl.grid[1] = 4u * (unsigned)x.s2_tiles;
    int cls[4] = {0, 1, 2, 3}, nt[4];
    for (int c = 0; c < 4; ++c) {
      const int h0 = ((c >> 1) + p.g_pad) & 1, w0 = ((c & 1) + p.g_pad) & 1;
      nt[c] = (h0 < p.g_KH ? (p.g_KH - h0 + 1) / 2 : 0) * (w0 < p.g_KW ? (p.g_KW - w0 + 1) / 2 : 0);
    }
    for (int i = 1; i < 4; ++i)
      for (int j = i; j > 0 && nt[cls[j]] > nt[cls[j - 1]]; --j) { const int c = cls[j]; cls[j] = cls[j - 1]; cls[j - 1] = c; }
    for (int i = 0; i < 4; ++i) x.s2_ord |= cls[i] << (2 * i);
  }
  x.sk_gx = (int)pl.grid[0]; x.sk_gy = (int)pl.grid[1];
  // split-K of a forward / data-gradient product: with the caller's tickets the last workgroup of a tile finishes it
  // (no second launch); the sk_finish switch keeps the finishing launch (A/B switch)
  if (x.part && !sw.sk_finish && p.sk_cnt && p.splitk <= SK_PART_MAX && p.epi_mode == EPI_PLAIN) {
    const long long tiles = (long long)pl.grid[0] * pl.grid[1];
    if (tiles <= p.sk_cnt_n && tiles * p.splitk * (long long)(bm * bn) <= p.sk_ws_floats) {
      x.tick = 1; x.part = nullptr; x.sk_slots = p.splitk; x.sk_part = p.sk_ws; x.sk_cnt = p.sk_cnt;
    }
  }
  pl.finish = x.part != nullptr;
  const long nwg = (long)pl.grid[0] * pl.grid[1] * pl.grid[2];
  if (!sw.no_xcd && nwg >= 32 && !nchw) {
    // bytes behind the row panels (A side) and the column panels (B side): keep the larger one XCD-local
    double a_bytes, b_bytes;
    if (kind == KIND_WGRAD) { a_bytes = (double)p.K * p.M * (p.a_pro == PRO_DZ ? 2 : 1); b_bytes = (double)p.K * p.g_Cs; }
    else if (kind == KIND_FWD) { a_bytes = (double)p.M * p.g_stride * p.g_stride * p.g_Cs; b_bytes = (double)p.N * p.K; }
    else { a_bytes = (double)p.M * p.g_Cs * (p.a_pro == PRO_DZ ? 2 : 1); b_bytes = (double)p.N * p.K; }
    x.xcd = (b_bytes > a_bytes && x.sk_gy > 1) ? 2 : (x.sk_gx > 1 ? 1 : 0);
  }
  return MMVQA_OK;
}

// --------------------------------------------------------------------------- tuner candidates
// (tile, split-K) pairs the per-shape tuner times for a product seen for the first time (NHWC, tile == 0)
inline std::vector<IgemmChoice> tune_candidates(const GemmParams& p, int kind) {
  std::vector<IgemmChoice> cands;
  if (kind == KIND_WGRAD && p.splitk <= 0) {
    for (int t = 1; t <= 6; ++t) for (int sk : {0, 1, 2, 3, 4, 6, 8, 12, 16}) cands.push_back({t, sk});
  } else if (sk_eligible(p, kind) && p.splitk <= 0 && (long)cdiv(p.M, 64) * cdiv(p.N, 64) <= 320) {
    // few output tiles: also try K split over workgroups (needs the caller's scratch)
    for (int t : {3, 5, 6}) for (int sk : {1, 2, 3, 4, 6, 8}) cands.push_back({t, sk});
    for (int t : {1, 2, 4}) cands.push_back({t, 1});
  } else {
    for (int t = 1; t <= 6; ++t) cands.push_back({t, p.splitk});
  }
  return cands;
}
