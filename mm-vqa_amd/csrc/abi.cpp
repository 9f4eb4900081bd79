// The engine's part of the extern "C" surface of libmmvqa_hip.so (declared in include/mmvqa.h), and the version / error /
// sizeof queries.  Every operation's entry point is defined in the .hip file that launches its kernel (see kernels.h).
#include <cstring>

#include "engine.h"

#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" {

int mmvqa_version(void) { return 100; }
const char* mmvqa_last_error(void) { return mmvqa_get_error(); }
size_t mmvqa_sizeof_gemm_desc(void) { return sizeof(mmvqa_gemm_desc); }
size_t mmvqa_sizeof_attn_desc(void) { return sizeof(mmvqa_attn_desc); }
size_t mmvqa_sizeof_model_desc(void) { return sizeof(mmvqa_model_desc); }
size_t mmvqa_sizeof_fb_attn_desc(void) { return sizeof(mmvqa_fb_attn_desc); }

// ---------------------------------------------------------------------------------- engine
void mmvqa_engine_destroy(mmvqa_engine* e) {
  if (!e) return;
  for (hipEvent_t ev : e->ev_pool) (void)hipEventDestroy(ev);
  if (e->side) (void)hipStreamDestroy(e->side);
  if (e->side2) (void)hipStreamDestroy(e->side2);
  delete e;
}
int mmvqa_engine_num_tensors(const mmvqa_engine* e) { return e ? (int)e->specs.size() : 0; }
int mmvqa_engine_tensor_info(const mmvqa_engine* e, int i, char* name, int name_cap, int* kind, int* ndim,
                             long long shape[4], long long* offset, int* channels_last) {
  if (!e || i < 0 || i >= (int)e->specs.size()) return mmvqa_set_error(MMVQA_ERR_ARG, "tensor_info: bad index");
  const TensorSpec& s = e->specs[i];
  if (name && name_cap > 0) {
    strncpy(name, s.name.c_str(), name_cap - 1);
    name[name_cap - 1] = 0;
  }
  if (kind) *kind = s.kind;
  if (ndim) *ndim = s.ndim;
  if (shape) for (int k = 0; k < 4; ++k) shape[k] = s.shape[k];
  if (offset) *offset = s.offset;
  if (channels_last) *channels_last = s.channels_last;
  return MMVQA_OK;
}
long long mmvqa_engine_param_floats(const mmvqa_engine* e) { return e ? e->n_params : 0; }
long long mmvqa_engine_buf_floats(const mmvqa_engine* e) { return e ? e->n_bufs : 0; }
long long mmvqa_engine_nbt_count(const mmvqa_engine* e) { return e ? e->n_nbt : 0; }
size_t mmvqa_engine_plan(mmvqa_engine* e, int B, int T, int img_h, int img_w) {
  if (!e) { mmvqa_set_error(MMVQA_ERR_ARG, "plan: null engine"); return 0; }
  return engine_plan(e, B, B, T, img_h, img_w, false);
}
size_t mmvqa_engine_plan_grouped(mmvqa_engine* e, int NI, int B, int T, int img_h, int img_w) {
  if (!e) { mmvqa_set_error(MMVQA_ERR_ARG, "plan_grouped: null engine"); return 0; }
  if (NI < 1 || NI > B) {
    mmvqa_set_error(MMVQA_ERR_ARG, "plan_grouped: NI=%d images for B=%d questions (1 <= NI <= B)", NI, B);
    return 0;
  }
  return engine_plan(e, NI, B, T, img_h, img_w, true);
}
int mmvqa_engine_bind(mmvqa_engine* e, float* params, float* grads, float* bufs, long long* nbt, void* workspace,
                      size_t workspace_bytes) {
  if (!e || !e->planned) return mmvqa_set_error(MMVQA_ERR_STATE, "bind: plan first");
  if (!params || !grads || !bufs || !nbt || !workspace) return mmvqa_set_error(MMVQA_ERR_ARG, "bind: null pointer");
  if (workspace_bytes < e->ws_floats * sizeof(float))
    return mmvqa_set_error(MMVQA_ERR_ARG, "bind: workspace too small (%zu < %zu)", workspace_bytes,
                           e->ws_floats * sizeof(float));
  if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)bufs | (uintptr_t)workspace) & 15)
    return mmvqa_set_error(MMVQA_ERR_ARG, "bind: buffers must be 16-byte aligned");
  e->params = params; e->grads = grads; e->bufs = bufs; e->nbt = nbt;
  e->ws = reinterpret_cast<float*>(workspace);
  e->ws_ready = false;        // tap-validity tables and tickets live in the (new) workspace: put in place by the next forward
  e->bound = true;
  e->img = nullptr;
  e->tokens_only = false;
  e->cached = false;
  return MMVQA_OK;
}
int mmvqa_engine_forward(mmvqa_engine* e, mmvqa_stream_t s, const float* img, const long long* ids,
                         const long long* seg, const long long* mask, float* logits, int logits_ld, float* feat,
                         int training, uint32_t seed) {
  if (!e || !img || !ids || !seg || !mask || !logits) return mmvqa_set_error(MMVQA_ERR_ARG, "forward: null pointer");
  return engine_forward(e, ST(s), img, ids, seg, mask, logits, logits_ld, feat, training, seed);
}
int mmvqa_engine_forward_grouped(mmvqa_engine* e, mmvqa_stream_t s, const float* img, const int* group,
                                 const int* offsets, const long long* ids, const long long* seg, const long long* mask,
                                 float* logits, int logits_ld, float* feat, int training, uint32_t seed) {
  if (!e || !img || !group || !offsets || !ids || !seg || !mask || !logits)
    return mmvqa_set_error(MMVQA_ERR_ARG, "forward_grouped: null pointer");
  return engine_forward(e, ST(s), img, ids, seg, mask, logits, logits_ld, feat, training, seed, group, offsets);
}
int mmvqa_engine_backward(mmvqa_engine* e, mmvqa_stream_t s, const float* dlogits, int dlogits_ld,
                          const float* dfeat) {
  if (!e || !dlogits) return mmvqa_set_error(MMVQA_ERR_ARG, "backward: null pointer");
  return engine_backward(e, ST(s), dlogits, dlogits_ld, dfeat);
}
int mmvqa_engine_backward_feature(mmvqa_engine* e, mmvqa_stream_t s, const float* dlogits, int dlogits_ld, float* dA) {
  if (!e) return mmvqa_set_error(MMVQA_ERR_ARG, "backward_feature: null engine");
  return engine_backward_feature(e, ST(s), dlogits, dlogits_ld, dA);
}
int mmvqa_engine_feature_map(mmvqa_engine* e, const float** A, int* H, int* W, int* C) {
  if (!e) return mmvqa_set_error(MMVQA_ERR_ARG, "feature_map: null engine");
  return engine_feature_map(e, A, H, W, C);
}
int mmvqa_engine_visual_tokens(mmvqa_engine* e, const float** vis) {
  if (!e) return mmvqa_set_error(MMVQA_ERR_ARG, "visual_tokens: null engine");
  return engine_visual_tokens(e, vis);
}
int mmvqa_engine_forward_tokens(mmvqa_engine* e, mmvqa_stream_t s, const float* vis, const long long* ids,
                                const long long* seg, const long long* mask, float* logits, int logits_ld, float* feat) {
  if (!e || !vis || !ids || !seg || !mask || !logits) return mmvqa_set_error(MMVQA_ERR_ARG, "forward_tokens: null pointer");
  return engine_forward_tokens(e, ST(s), vis, ids, seg, mask, logits, logits_ld, feat);
}
int mmvqa_engine_forward_cached(mmvqa_engine* e, mmvqa_stream_t s, const float* cache, int N, int K, const int* idx,
                                const int* view, const long long* ids, const long long* seg, const long long* mask,
                                float* logits, int logits_ld, float* feat, int training, uint32_t seed) {
  if (!e || !cache || !idx || !view || !ids || !seg || !mask || !logits)
    return mmvqa_set_error(MMVQA_ERR_ARG, "forward_cached: null pointer");
  return engine_forward_cached(e, ST(s), cache, N, K, idx, view, ids, seg, mask, logits, logits_ld, feat, training, seed);
}
int mmvqa_engine_backward_cached(mmvqa_engine* e, mmvqa_stream_t s, const float* dlogits, int dlogits_ld,
                                 const float* dfeat) {
  if (!e || !dlogits) return mmvqa_set_error(MMVQA_ERR_ARG, "backward_cached: null pointer");
  return engine_backward_cached(e, ST(s), dlogits, dlogits_ld, dfeat);
}
int mmvqa_engine_set_grad_callback(mmvqa_engine* e, mmvqa_grad_cb cb, void* user) {
  if (!e) return mmvqa_set_error(MMVQA_ERR_ARG, "set_grad_callback: null engine");
  e->grad_cb = cb;
  e->grad_cb_user = user;
  return MMVQA_OK;
}
int mmvqa_engine_set_precision(mmvqa_engine* e, int mode) {
  if (!e) return mmvqa_set_error(MMVQA_ERR_ARG, "set_precision: null engine");
  if (mode != MMVQA_PREC_F32 && mode != MMVQA_PREC_F16)
    return mmvqa_set_error(MMVQA_ERR_ARG, "set_precision: mode %d (0 = fp32, 1 = fp16 operands)", mode);
  if (mode == MMVQA_PREC_F16 && e->d.cnn != 0)
    return mmvqa_set_error(MMVQA_ERR_ARG, "set_precision: the fp16 operand mode covers the ResNet encoders only (EfficientNet's "
                                          "squeeze-excite, depthwise and thin tap products run outside the implicit GEMM)");
  e->prec = mode;
  return MMVQA_OK;
}
int mmvqa_engine_set_frozen(mmvqa_engine* e, int flags) {
  if (!e) return mmvqa_set_error(MMVQA_ERR_ARG, "set_frozen: null engine");
  if ((flags & ~(MMVQA_FREEZE_BACKBONE | MMVQA_FREEZE_BN_STATS)) || flags == MMVQA_FREEZE_BN_STATS)
    return mmvqa_set_error(MMVQA_ERR_ARG, "set_frozen: flags=%d (1 = backbone without gradient, 3 = and its BatchNorms on "
                                          "running statistics)", flags);
  e->frozen_next = flags;
  return MMVQA_OK;
}
int mmvqa_engine_tune(mmvqa_engine* e, int enable) {
  if (!e) return mmvqa_set_error(MMVQA_ERR_ARG, "tune: null engine");
  if (enable != 0 && enable != 1) return mmvqa_set_error(MMVQA_ERR_ARG, "tune: enable=%d is neither 0 nor 1", enable);
  e->tuner.tuning = enable != 0;
  return (int)e->tuner.table.size();
}
int mmvqa_engine_profile(mmvqa_engine* e, int enable) {
  if (!e) return mmvqa_set_error(MMVQA_ERR_ARG, "profile: null engine");
  e->prof_on = enable ? 1 : 0;
  e->use_side = enable == 2 ? 0 : 1;   // 2: one stream only, every launch has the chip to itself
  if (enable) {
    memset(e->prof_launch, 0, sizeof(e->prof_launch));
    memset(e->prof_ms, 0, sizeof(e->prof_ms));
    memset(e->prof_flops, 0, sizeof(e->prof_flops));
    memset(e->reg_launch, 0, sizeof(e->reg_launch));
    memset(e->reg_ms, 0, sizeof(e->reg_ms));
    memset(e->reg_flops, 0, sizeof(e->reg_flops));
    memset(e->tag_launch, 0, sizeof(e->tag_launch));
    memset(e->tag_ms, 0, sizeof(e->tag_ms));
    memset(e->tag_bytes, 0, sizeof(e->tag_bytes));
  }
  return MMVQA_OK;
}
int mmvqa_engine_profile_read_region(mmvqa_engine* e, int region, int cls, long long* launches, double* ms,
                                     double* flops) {
  if (!e || cls < 0 || cls >= PROF_NCLS || region < 0 || region >= REG_N)
    return mmvqa_set_error(MMVQA_ERR_ARG, "profile_read_region: bad region/class");
  int r = engine_profile_collect(e);
  if (r != MMVQA_OK) return r;
  if (launches) *launches = e->reg_launch[region][cls];
  if (ms) *ms = e->reg_ms[region][cls];
  if (flops) *flops = e->reg_flops[region][cls];
  return MMVQA_OK;
}
int mmvqa_engine_profile_read_hbm(mmvqa_engine* e, int kernel, long long* launches, double* ms, double* bytes) {
  if (!e || kernel <= HB_NONE || kernel >= HB_N) return mmvqa_set_error(MMVQA_ERR_ARG, "profile_read_hbm: bad kernel id");
  int r = engine_profile_collect(e);
  if (r != MMVQA_OK) return r;
  if (launches) *launches = e->tag_launch[kernel];
  if (ms) *ms = e->tag_ms[kernel];
  if (bytes) *bytes = e->tag_bytes[kernel];
  return MMVQA_OK;
}
int mmvqa_engine_profile_read(mmvqa_engine* e, int cls, long long* launches, double* ms, double* flops) {
  if (!e || cls < 0 || cls >= PROF_NCLS) return mmvqa_set_error(MMVQA_ERR_ARG, "profile_read: bad class");
  int r = engine_profile_collect(e);
  if (r != MMVQA_OK) return r;
  if (launches) *launches = e->prof_launch[cls];
  if (ms) *ms = e->prof_ms[cls];
  if (flops) *flops = e->prof_flops[cls];
  return MMVQA_OK;
}

}  // extern "C"
