// Stand-alone driver of the implicit-GEMM launch plan (mm-vqa_amd/csrc/igemm_plan.h) for tests/test_igemm_plan_cpu.py:
// no HIP, no GPU.  Reads one case per line from stdin ("key=value" tokens), prints one JSON line per case.
//   mode=plan (default): validate_desc, then igemm_plan, as mmvqa_launch_igemm calls them; mode=tune: tune_candidates.
//   kind= nchw= tile=           the call's arguments
//   sw.general=1 ...            IgemmSwitches members (default: all off)
//   M=64 a_ld=64 ...            integer members of the descriptor (a_fold.* included); everything else is zero
//   A=1 sk_ws=1 ...             pointer members are FLAGS: 0 = null, 1 = a dummy address that names the member and
//                               points at nothing -- a plan that dereferenced one would trip the sanitizer
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <iostream>
#include <sstream>
#include <string>

#include "igemm_plan.h"

static char g_error[512];
int mmvqa_set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
  return code;
}

#define INT_FIELDS(F)                                                                                              \
  F(M) F(N) F(K) F(splitk) F(ktiles_per_split) F(a_pro) F(a_ld) F(b_pro) F(b_ld) F(b_tapstride) F(g_SH) F(g_SW)    \
  F(g_Cs) F(g_OH) F(g_OW) F(g_KH) F(g_KW) F(g_stride) F(g_pad) F(g_nchw) F(c_ld) F(c_atomic) F(act) F(dact)        \
  F(pre_ld) F(r_ld) F(epi_mode) F(tap_HW) F(mk_ld) F(stat_bwd) F(z1_ld) F(z2_ld) F(gate_hw) F(mk_mode)             \
  F(sk_ws_floats) F(stat_slots) F(reserved1) F(sk_cnt_n) F(reserved0) F(a_fold.slots) F(a_fold.bwd)                \
  F(a_fold.publish) F(a_fold.reps)
#define PTR_FIELDS(F)                                                                                              \
  F(A) F(A2) F(a_c0) F(a_c1) F(a_c2) F(B) F(b_c0) F(b_c1) F(C) F(Cpre) F(bias) F(Pre) F(R) F(tap_out) F(tap_dv)    \
  F(Mk) F(mk_s) F(mk_b) F(stat1) F(Z1) F(mean1) F(invstd1) F(stat2) F(Z2) F(mean2) F(invstd2) F(colsum) F(gate)    \
  F(pixmask) F(sk_ws) F(sk_cnt) F(a_fold.stat) F(a_fold.gamma) F(a_fold.beta) F(a_fold.mean) F(a_fold.invstd)      \
  F(a_fold.out0) F(a_fold.out1) F(a_fold.out2) F(a_fold.out3) F(a_fold.run_mean) F(a_fold.run_var) F(a_fold.nbt)   \
  F(a_fold.dgamma) F(a_fold.dbeta)

static const char* const PTR_NAMES[] = {
#define F(f) #f,
    PTR_FIELDS(F)
#undef F
};
constexpr int N_PTRS = sizeof(PTR_NAMES) / sizeof(PTR_NAMES[0]);
// unmapped, distinct, 64-byte aligned
static uintptr_t dummy_address(int idx) { return 0x10000u + 0x40u * (uintptr_t)idx; }
static std::string ptr_name(const void* q) {
  if (!q) return "null";
  for (int i = 0; i < N_PTRS; ++i)
    if ((uintptr_t)q == dummy_address(i)) return PTR_NAMES[i];
  return "?";
}

struct Case {
  std::string name, mode = "plan";
  int kind = 0, nchw = 0, tile = 0;
  IgemmSwitches sw{};
  GemmParams p{};
};

static bool parse_case(const std::string& line, Case* c) {
  std::istringstream in(line);
  std::string tok;
  while (in >> tok) {
    const size_t eq = tok.find('=');
    if (eq == std::string::npos) return false;
    const std::string key = tok.substr(0, eq), val = tok.substr(eq + 1);
    const long long iv = atoll(val.c_str());
    GemmParams& p = c->p;
    int idx = 0;
    bool found = true;
    if (key == "name") c->name = val;
    else if (key == "mode") c->mode = val;
    else if (key == "kind") c->kind = (int)iv;
    else if (key == "nchw") c->nchw = (int)iv;
    else if (key == "tile") c->tile = (int)iv;
    else if (key == "sw.general") c->sw.general = iv != 0;
    else if (key == "sw.no_stagger") c->sw.no_stagger = iv != 0;
    else if (key == "sw.sk_finish") c->sw.sk_finish = iv != 0;
    else if (key == "sw.no_xcd") c->sw.no_xcd = iv != 0;
    else if (key == "sw.s2_dense") c->sw.s2_dense = iv != 0;
    else if (key == "a_fold.count") p.a_fold.count = atof(val.c_str());
    else if (key == "drop_p") p.drop_p = (float)atof(val.c_str());
    else found = false;
#define F(f) if (key == #f) { p.f = (decltype(p.f))iv; found = true; }
    INT_FIELDS(F)
#undef F
#define F(f) if (key == #f) { p.f = iv ? (decltype(p.f))dummy_address(idx) : nullptr; found = true; } ++idx;
    PTR_FIELDS(F)
#undef F
    if (!found) return false;
  }
  return !c->name.empty();
}

// what a launch consists of, as the launcher of the recorded commit enqueued it
struct Rec {
  int rc = 0;
  IgemmShape shape{};
  unsigned grid[3] = {0, 0, 0};
  int threads = 0;
  size_t smem = 0;
  GemmParams p{};
  GemmAux x{};
  int coef = 0, finish = 0;
};

// ---- evaluate
static Rec evaluate(const Case& c) {
  Rec r;
  g_error[0] = 0;
  r.rc = validate_desc(c.p, c.kind, c.nchw);
  if (r.rc) return r;
  IgemmPlan pl;
  r.rc = igemm_plan(c.p, c.kind, c.nchw, c.tile, c.sw, &pl);
  if (r.rc) return r;
  r.shape = pl.shape;
  for (int i = 0; i < 3; ++i) r.grid[i] = pl.grid[i];
  r.threads = pl.threads;
  r.smem = pl.smem;
  r.p = pl.p;
  r.x = pl.x;
  r.coef = pl.coef_launch;
  r.finish = pl.finish ? 1 : 0;
  if (pl.coef_launch && !pl.coef_stat) r.coef = -1;   // the coefficient launch must keep the sums it reads
  return r;
}

static std::vector<IgemmChoice> candidates(const Case& c) { return tune_candidates(c.p, c.kind); }
// ---- end evaluate

static std::string json_escape(const char* s) {
  std::string o;
  for (; *s; ++s) {
    if (*s == '"' || *s == '\\') o += '\\';
    o += *s;
  }
  return o;
}

static void print_fastdiv(const char* name, const FastDiv& f) { printf("\"%s\": [%u, %u, %u], ", name, f.mul, f.shr, f.d); }

static void print_rec(const Case& c, const Rec& r) {
  printf("{\"name\": \"%s\", \"rc\": %d, ", c.name.c_str(), r.rc);
  if (r.rc) {
    printf("\"error\": \"%s\"}\n", json_escape(g_error).c_str());
    return;
  }
  const IgemmShape& s = r.shape;
  const GemmAux& x = r.x;
  const GemmParams& p = r.p;
  printf("\"shape\": {\"bm\": %d, \"bn\": %d, \"bk\": %d, \"ks\": %d, \"kind\": %d, \"nchw\": %d, \"prec\": %d, \"s2c\": %d}, ",
         s.bm, s.bn, s.bk, s.ks, s.kind, s.nchw, s.prec, s.s2c);
  printf("\"grid\": [%u, %u, %u], \"threads\": %d, \"smem\": %zu, \"x\": {", r.grid[0], r.grid[1], r.grid[2], r.threads, r.smem);
  print_fastdiv("ohw", x.ohw);
  print_fastdiv("ow", x.ow);
  printf("\"fast\": %d, \"stagger\": %d, \"part\": \"%s\", \"ldsc\": %d, \"pad0\": %d, \"sk_gx\": %d, \"sk_gy\": %d, \"sk_slots\": %d, ",
         x.fast, x.stagger, ptr_name(x.part).c_str(), x.ldsc, x.pad0, x.sk_gx, x.sk_gy, x.sk_slots);
  printf("\"sk_part\": \"%s\", \"sk_cnt\": \"%s\", \"tick\": %d, \"xcd\": %d, ", ptr_name(x.sk_part).c_str(),
         ptr_name(x.sk_cnt).c_str(), x.tick, x.xcd);
  print_fastdiv("s2_hw", x.s2_hw);
  print_fastdiv("s2_w", x.s2_w);
  printf("\"s2_M\": %d, \"s2_tiles\": %d, \"s2_ord\": %d}, ", x.s2_M, x.s2_tiles, x.s2_ord);
  printf("\"p\": {\"splitk\": %d, \"ktiles_per_split\": %d, \"c_atomic\": %d, \"g_KH\": %d, \"g_KW\": %d, \"g_stride\": %d, \"g_pad\": %d, ",
         p.splitk, p.ktiles_per_split, p.c_atomic, p.g_KH, p.g_KW, p.g_stride, p.g_pad);
  printf("\"a_c0\": \"%s\", \"a_c1\": \"%s\", \"a_c2\": \"%s\", \"a_fold.stat\": \"%s\"}, ", ptr_name(p.a_c0).c_str(),
         ptr_name(p.a_c1).c_str(), ptr_name(p.a_c2).c_str(), ptr_name(p.a_fold.stat).c_str());
  printf("\"coef_launch\": %d, \"finish\": %d}\n", r.coef, r.finish);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty() || line[0] == '#') continue;
    Case c;
    if (!parse_case(line, &c)) {
      fprintf(stderr, "bad case line: %s\n", line.c_str());
      return 2;
    }
    if (c.mode == "tune") {
      printf("{\"name\": \"%s\", \"candidates\": [", c.name.c_str());
      const std::vector<IgemmChoice> cands = candidates(c);
      for (size_t i = 0; i < cands.size(); ++i) printf("%s[%d, %d]", i ? ", " : "", cands[i].tile, cands[i].splitk);
      printf("]}\n");
    } else {
      print_rec(c, evaluate(c));
    }
  }
  return 0;
}
