// Forward-only BERT encoder (HF BertModel without the pooler: post-LN layers, absolute positions, erf GELU) for the
// frozen teacher of the distillation task (pretrain/roco_utils.py:112-132) and of the cosine SupCon mask
// (models/SupConLoss/supcon_utils.py:92-97, 140-159).  Built from the library's op-level entry points:
//   embeddings   mmvqa_embed_fwd (num_vis = 0, token type 0, no dropout)
//   per layer    mmvqa_igemm      qkv = x Wqkv^T + b      the three HF weights bound back to back: one product
//                mmvqa_attention_len_fwd                  per-sample key lengths, T <= 512 (bertattn.hip)
//                mmvqa_igemm      t = ctx Wo^T + b
//                mmvqa_layernorm_fwd  y = LN(t + x)
//                mmvqa_igemm      f = gelu(y Wi^T + b)
//                mmvqa_igemm      t = f Wd^T + b
//                mmvqa_layernorm_fwd  x = LN(t + y)       the last layer run writes the caller's buffer
// mmvqa_bert_forward_layers stops after the first n_layers layers (HF's hidden_states[n_layers], what BERTScore reads,
// supcon_utils.py:103-108); mmvqa_bert_forward is the same function with n_layers = layers.
// Everything is enqueued on the caller's stream; nothing synchronises, allocates or tunes.  Weights and workspace are
// borrowed device buffers.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "kernels.h"

#define BERT_MAX_T 512

namespace {

struct BertTensor {
  std::string name;
  int ndim;
  long long shape[2];
  long long offset;   // floats into the parameter buffer
};

struct BertLayerRef {
  long long wqkv, bqkv, wo, bo, ln1_g, ln1_b, wi, bi, wd, bd, ln2_g, ln2_b;
};

}  // namespace

struct mmvqa_bert {
  mmvqa_bert_desc d;
  std::vector<BertTensor> specs;
  long long n_params = 0;
  long long word = 0, pos = 0, type = 0, emb_g = 0, emb_b = 0;
  std::vector<BertLayerRef> layers;
  // plan
  bool planned = false, bound = false;
  int B = 0, T = 0;
  size_t ws_bytes = 0;
  size_t o_x = 0, o_qkv = 0, o_ctx = 0, o_t = 0, o_y = 0, o_ff = 0, o_mean = 0, o_rstd = 0, o_seg = 0;   // byte offsets
  const float* params = nullptr;
  char* ws = nullptr;
};

static long long bert_add(mmvqa_bert* e, const std::string& name, long long d0, long long d1) {
  BertTensor t;
  t.name = name;
  t.ndim = d1 > 0 ? 2 : 1;
  t.shape[0] = d0; t.shape[1] = d1 > 0 ? d1 : 0;
  t.offset = e->n_params;
  e->n_params += d0 * (d1 > 0 ? d1 : 1);
  e->specs.push_back(t);
  return t.offset;
}

// y[M][N] = act(x[M][K] W^T + b), W [N][K]
static int bert_linear(hipStream_t st, const float* x, int M, int K, const float* W, const float* b, int N, int act, float* y) {
  mmvqa_gemm_desc g;
  memset(&g, 0, sizeof(g));
  g.g_SH = g.g_SW = g.g_OH = g.g_OW = 1;
  g.g_KH = g.g_KW = 1; g.g_stride = 1; g.g_pad = 0;
  g.M = M; g.N = N; g.K = K;
  g.A = x; g.a_ld = K; g.g_Cs = K;
  g.B = W; g.b_ld = K;
  g.C = y; g.c_ld = N;
  g.bias = b;
  g.act = act;
  return mmvqa_igemm(&g, MMVQA_KIND_FWD, 0, 0, reinterpret_cast<mmvqa_stream_t>(st));
}

extern "C" {

size_t mmvqa_sizeof_bert_desc(void) { return sizeof(mmvqa_bert_desc); }

int mmvqa_bert_create(const mmvqa_bert_desc* d, mmvqa_bert** out) {
  const char* who = "bert_create";
  if (!d || !out) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: null pointer", who);
  if (d->layers < 1 || d->hidden < 1 || d->heads < 1 || d->inter < 1 || d->vocab < 1 || d->max_pos < 1 || d->type_vocab < 1)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: layers=%d hidden=%d heads=%d inter=%d vocab=%d max_pos=%d type_vocab=%d (all >= 1)",
                           who, d->layers, d->hidden, d->heads, d->inter, d->vocab, d->max_pos, d->type_vocab);
  if (d->hidden % 64 != 0 || d->heads != d->hidden / 64)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: hidden=%d heads=%d: the attention kernel has head dimension 64 (hidden %% 64 == 0, "
                                          "heads == hidden / 64)", who, d->hidden, d->heads);
  if (d->hidden > 1024) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: hidden=%d > 1024 (LayerNorm kernels)", who, d->hidden);
  if (d->inter % 4 != 0) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: inter=%d must be a multiple of 4", who, d->inter);
  if (!(d->eps > 0.f)) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: eps=%g must be positive", who, (double)d->eps);
  mmvqa_bert* e = new mmvqa_bert();
  e->d = *d;
  const long long H = d->hidden, I = d->inter;
  e->word = bert_add(e, "embeddings.word_embeddings.weight", d->vocab, H);
  e->pos = bert_add(e, "embeddings.position_embeddings.weight", d->max_pos, H);
  e->type = bert_add(e, "embeddings.token_type_embeddings.weight", d->type_vocab, H);
  e->emb_g = bert_add(e, "embeddings.LayerNorm.weight", H, 0);
  e->emb_b = bert_add(e, "embeddings.LayerNorm.bias", H, 0);
  for (int i = 0; i < d->layers; ++i) {
    const std::string p = "encoder.layer." + std::to_string(i) + ".";
    BertLayerRef L;
    // query, key, value back to back, weights then biases: one [3H][H] product
    L.wqkv = bert_add(e, p + "attention.self.query.weight", H, H);
    bert_add(e, p + "attention.self.key.weight", H, H);
    bert_add(e, p + "attention.self.value.weight", H, H);
    L.bqkv = bert_add(e, p + "attention.self.query.bias", H, 0);
    bert_add(e, p + "attention.self.key.bias", H, 0);
    bert_add(e, p + "attention.self.value.bias", H, 0);
    L.wo = bert_add(e, p + "attention.output.dense.weight", H, H);
    L.bo = bert_add(e, p + "attention.output.dense.bias", H, 0);
    L.ln1_g = bert_add(e, p + "attention.output.LayerNorm.weight", H, 0);
    L.ln1_b = bert_add(e, p + "attention.output.LayerNorm.bias", H, 0);
    L.wi = bert_add(e, p + "intermediate.dense.weight", I, H);
    L.bi = bert_add(e, p + "intermediate.dense.bias", I, 0);
    L.wd = bert_add(e, p + "output.dense.weight", H, I);
    L.bd = bert_add(e, p + "output.dense.bias", H, 0);
    L.ln2_g = bert_add(e, p + "output.LayerNorm.weight", H, 0);
    L.ln2_b = bert_add(e, p + "output.LayerNorm.bias", H, 0);
    e->layers.push_back(L);
  }
  *out = e;
  return MMVQA_OK;
}

void mmvqa_bert_destroy(mmvqa_bert* e) { delete e; }

int mmvqa_bert_num_tensors(const mmvqa_bert* e) { return e ? (int)e->specs.size() : 0; }

long long mmvqa_bert_param_floats(const mmvqa_bert* e) { return e ? e->n_params : 0; }

int mmvqa_bert_tensor_info(const mmvqa_bert* e, int i, char* name, int name_cap, int* ndim, long long shape[2],
                           long long* offset) {
  if (!e || i < 0 || i >= (int)e->specs.size()) return mmvqa_set_error(MMVQA_ERR_ARG, "bert_tensor_info: bad index");
  const BertTensor& t = e->specs[i];
  if (name && name_cap > 0) {
    strncpy(name, t.name.c_str(), name_cap - 1);
    name[name_cap - 1] = 0;
  }
  if (ndim) *ndim = t.ndim;
  if (shape) { shape[0] = t.shape[0]; shape[1] = t.shape[1]; }
  if (offset) *offset = t.offset;
  return MMVQA_OK;
}

size_t mmvqa_bert_plan(mmvqa_bert* e, int B, int T) {
  if (!e) { mmvqa_set_error(MMVQA_ERR_ARG, "bert_plan: null encoder"); return 0; }
  const int tmax = e->d.max_pos < BERT_MAX_T ? e->d.max_pos : BERT_MAX_T;
  if (B < 1 || B > 65535 || T < 1 || T > tmax) {
    mmvqa_set_error(MMVQA_ERR_ARG, "bert_plan: B=%d (1..65535) T=%d (1..min(%d, max_pos=%d))", B, T, BERT_MAX_T, e->d.max_pos);
    return 0;
  }
  const size_t M = (size_t)B * T, H = (size_t)e->d.hidden, I = (size_t)e->d.inter;
  size_t o = 0;
  auto take = [&o](size_t bytes) { size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
  e->o_x = take(M * H * 4);
  e->o_qkv = take(M * 3 * H * 4);
  e->o_ctx = take(M * H * 4);
  e->o_t = take(M * H * 4);
  e->o_y = take(M * H * 4);
  e->o_ff = take(M * I * 4);
  e->o_mean = take(M * 4);
  e->o_rstd = take(M * 4);
  e->o_seg = take(M * 8);
  e->ws_bytes = o;
  e->B = B; e->T = T;
  e->planned = true;
  e->bound = false;
  return o;
}

int mmvqa_bert_bind(mmvqa_bert* e, const float* params, void* workspace, size_t workspace_bytes) {
  if (!e) return mmvqa_set_error(MMVQA_ERR_ARG, "bert_bind: null encoder");
  if (!e->planned) return mmvqa_set_error(MMVQA_ERR_STATE, "bert_bind: plan first");
  if (!params || !workspace) return mmvqa_set_error(MMVQA_ERR_ARG, "bert_bind: null pointer");
  if (workspace_bytes < e->ws_bytes)
    return mmvqa_set_error(MMVQA_ERR_ARG, "bert_bind: workspace too small (%zu < %zu)", workspace_bytes, e->ws_bytes);
  if (((uintptr_t)params | (uintptr_t)workspace) & 15)
    return mmvqa_set_error(MMVQA_ERR_ARG, "bert_bind: buffers must be 16-byte aligned");
  e->params = params;
  e->ws = reinterpret_cast<char*>(workspace);
  e->bound = true;
  return MMVQA_OK;
}

// the embeddings and the first n_layers layers; the last LayerNorm of layer n_layers writes `out` (HF's hidden_states[n_layers])
static int bert_run(mmvqa_bert* e, mmvqa_stream_t s, const long long* ids, const int* len, int B, int T, int n_layers,
                    float* out, const char* who) {
  if (!e || !ids || !len || !out) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: null pointer", who);
  if (n_layers < 1 || n_layers > (int)e->layers.size())
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: n_layers=%d outside 1..%d (the encoder's depth)", who, n_layers,
                           (int)e->layers.size());
  if (!e->bound) return mmvqa_set_error(MMVQA_ERR_STATE, "%s: plan and bind first", who);
  if (B != e->B || T != e->T)
    return mmvqa_set_error(MMVQA_ERR_ARG, "%s: B=%d T=%d differ from the planned B=%d T=%d", who, B, T, e->B, e->T);
  if ((uintptr_t)out & 15) return mmvqa_set_error(MMVQA_ERR_ARG, "%s: out must be 16-byte aligned", who);
  hipStream_t st = reinterpret_cast<hipStream_t>(s);
  const int M = B * T, H = e->d.hidden, I = e->d.inter, heads = e->d.heads;
  const float* P = e->params;
  float* x = reinterpret_cast<float*>(e->ws + e->o_x);
  float* qkv = reinterpret_cast<float*>(e->ws + e->o_qkv);
  float* ctx = reinterpret_cast<float*>(e->ws + e->o_ctx);
  float* t = reinterpret_cast<float*>(e->ws + e->o_t);
  float* y = reinterpret_cast<float*>(e->ws + e->o_y);
  float* ff = reinterpret_cast<float*>(e->ws + e->o_ff);
  float* mean = reinterpret_cast<float*>(e->ws + e->o_mean);
  float* rstd = reinterpret_cast<float*>(e->ws + e->o_rstd);
  long long* seg = reinterpret_cast<long long*>(e->ws + e->o_seg);

  // token type 0 everywhere (the reference calls the model with input_ids and an attention mask only)
  HIP_CHECK_RET(hipMemsetAsync(seg, 0, (size_t)M * sizeof(long long), st));
  TRY(mmvqa_embed_fwd(s, ids, seg, P + e->word, P + e->pos, P + e->type, P + e->emb_g, P + e->emb_b, nullptr, x, nullptr,
                      nullptr, B, T, H, 0, e->d.eps, 0.f, 0u));
  for (int i = 0; i < n_layers; ++i) {
    const BertLayerRef& L = e->layers[i];
    TRY(bert_linear(st, x, M, H, P + L.wqkv, P + L.bqkv, 3 * H, MMVQA_ACT_NONE, qkv));
    TRY(mmvqa_attention_len_fwd(s, qkv, qkv + H, qkv + 2 * H, 3 * H, 64, ctx, H, 64, len, B, T, heads, 0.125f));
    TRY(bert_linear(st, ctx, M, H, P + L.wo, P + L.bo, H, MMVQA_ACT_NONE, t));
    TRY(mmvqa_layernorm_fwd(s, t, x, P + L.ln1_g, P + L.ln1_b, y, nullptr, mean, rstd, M, H, e->d.eps));
    TRY(bert_linear(st, y, M, H, P + L.wi, P + L.bi, I, MMVQA_ACT_GELU, ff));
    TRY(bert_linear(st, ff, M, I, P + L.wd, P + L.bd, H, MMVQA_ACT_NONE, t));
    TRY(mmvqa_layernorm_fwd(s, t, y, P + L.ln2_g, P + L.ln2_b, i + 1 == n_layers ? out : x, nullptr, mean, rstd, M, H,
                            e->d.eps));
  }
  return MMVQA_OK;
}

int mmvqa_bert_forward(mmvqa_bert* e, mmvqa_stream_t s, const long long* ids, const int* len, int B, int T, float* out) {
  return bert_run(e, s, ids, len, B, T, e ? (int)e->layers.size() : 1, out, "bert_forward");
}

int mmvqa_bert_forward_layers(mmvqa_bert* e, mmvqa_stream_t s, const long long* ids, const int* len, int B, int T,
                              int n_layers, float* out) {
  return bert_run(e, s, ids, len, B, T, n_layers, out, "bert_forward_layers");
}

}  // extern "C"
