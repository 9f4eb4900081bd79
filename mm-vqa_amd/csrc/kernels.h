// Host-side launchers that have no entry point of their own in the C ABI.  An operation of include/mmvqa.h is ONE function:
// the extern "C" mmvqa_* definition in the .hip file that launches its kernel, with its argument checks at the top; the
// engine calls those by their ABI names (common.h includes the public header).  What is declared here -- the k_ prefix --
// is what the ABI does not have: launchers with arguments the ABI twin lacks, plan-time predicates, engine-only kernels.
#pragma once
#include "common.h"
#include "igemm_plan.h"

#include <string>
#include <unordered_map>
#include <utility>

// per-shape (tile, split-K) choices of the implicit-GEMM launcher.  The launcher is three steps: validate_desc and
// igemm_plan (igemm_plan.h: pure host code, every per-launch decision) and igemm_run (igemm.hip: looks the planned
// instance up in one table and enqueues it).
struct IgemmTuner {
  bool tuning = false;
  std::unordered_map<std::string, IgemmChoice> table;
};
void mmvqa_set_tuner(IgemmTuner* t);
// operand precision the engine gives every implicit-GEMM launch of the calling thread (MMVQA_PREC_*): a launch whose
// descriptor says MMVQA_PREC_F32 takes this one (set around a forward / backward, like the tuner)
void mmvqa_set_igemm_precision(int prec);
// mmvqa_igemm / mmvqa_attention on a descriptor by value / reference: all their checks but the one for a null descriptor
int mmvqa_launch_igemm(GemmParams p, int kind, int nchw, int tile, hipStream_t stream);
int mmvqa_launch_attention(const AttnParams& p, int head_dim, int bwd, hipStream_t st);
// qkvattn.hip: whether mmvqa_qkv_attention_fwd takes the shape (T <= 32, head dimension 64)
bool k_qkv_attn_fwd_ok(int T, int H, int heads);

// elementwise.hip: mmvqa_bn_coef_fwd with (1 - momentum)^reps given directly (mmvqa_bn_fold carries it that way)
int k_bn_coef_fwd_keep(hipStream_t st, const double* stat, int C, double count, float eps, const float* gamma,
                       const float* beta, float* run_mean, float* run_var, long long* nbt, double keep, int reps,
                       int training, float* scale, float* shift, float* mean, float* invstd);
// mmvqa_se_dgate that also clears `nzero` floats at `zero` (the scratch of the squeeze-excite backward that follows)
int k_se_dgate(hipStream_t st, const float* t, const float* z, const float* s, const float* b, float* dgate, int N,
               int HW, int C, float* zero, int nzero);
int k_mul_dact(hipStream_t st, const float* x, const float* pre, int act, float* y, long n);
// fbattn.hip: rows of the Feedback Transformer between batch-major and window-major order
int k_fb_reorder(hipStream_t st, const float* src, float* dst, int B, int T, int H, int to_window);
// test-only: one wave that waits `us` microseconds (s_memrealtime), no memory access; us <= 0 enqueues nothing
int k_spin(hipStream_t st, int us);

// se.hip: the squeeze-excite fully connected layers (16-row problems) without the GEMM tile machinery
// (mmvqa_se_fc_fwd is two of these)
int k_skinny_fwd(hipStream_t st, const float* x, int x_ld, const float* W, const float* b, int act, float* pre,
                 float* y, int M, int N, int K);
bool k_se_fc_bwd_ok(int rd);   // the backward kernels keep an rd-wide tile in LDS: widths beyond their limit are refused at plan time
// mmvqa_se_fc_bwd with scratch_is_zero: the caller's previous kernel cleared the scratch (else a memset is queued)
int k_se_fc_bwd(hipStream_t st, const float* dgate, const float* gpre, const float* r, const float* rpre,
                const float* pool, const float* We, const float* Wr, float* dWe, float* dbe, float* dWr, float* dbr,
                float* dpool, float* scratch, int scratch_is_zero, int B, int mid, int rd);
