/* mmvqa.h -- C ABI of the MI355X-native MMBERT hot path (libmmvqa_hip.so).
 *
 * The reference (DannielSilva/MM-VQA) has no FFI: its boundary is the Python object
 * protocol  Model(args) / model(img, ids, seg, mask) / state_dict  (models/mmbert.py:129-167,
 * pretrain/roco_utils.py:214-247, vqamed2019/utils.py:633-666).  This header is the native side of
 * that boundary: plain pointers + sizes + a hipStream_t, no torch types.  Every entry point
 *   - borrows raw DEVICE pointers (never allocates or frees caller memory),
 *   - enqueues on the given stream and returns without synchronising,
 *   - returns 0 on success or a negative code; mmvqa_last_error() gives the message.
 * INTEGRATION.md shows the ctypes binding the Python shim uses.
 *
 * Layout conventions: activations are NHWC ("channels last") fp32; conv weights are
 * [Cout][KH][KW][Cin]; linear weights [out][in]; ids/masks/labels int64.
 */
#ifndef MMVQA_H
#define MMVQA_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mmvqa_stream_t; /* hipStream_t */

#define MMVQA_ACT_NONE 0
#define MMVQA_ACT_RELU 1
#define MMVQA_ACT_GELU 2 /* models/transformer.py:7-8 */
#define MMVQA_ACT_SERF 3 /* models/serf.py:23-24 */
#define MMVQA_ACT_SILU 4 /* timm tf_efficientnetv2_m activations */
#define MMVQA_ACT_SIGMOID 5 /* squeeze-excite gate */

#define MMVQA_KIND_FWD 0   /* C[pix,co]      = sum X[pix@tap,ci] W[co,tap,ci]      */
#define MMVQA_KIND_DGRAD 1 /* C[pix_in,ci]   = sum dZ[pix_out,co] W[co,tap,ci]     */
#define MMVQA_KIND_WGRAD 2 /* C[co,(tap,ci)] = sum dZ[pix,co] X[pix@tap,ci]        */

#define MMVQA_STAT_SLOTS 16

/* BatchNorm coefficients folded inside the CONSUMING launch (training mode).
 * The launches that produce a BatchNorm's input accumulate its per-channel sums into `stat`
 * ([MMVQA_STAT_SLOTS][C][2] doubles, the first `slots` replicas in use: forward sum z / sum z^2, backward
 * sum g / sum g*xhat).  A launch whose operand prologue applies that BatchNorm can derive the coefficients
 * from the sums in its own setup phase, so that no coefficient launch (mmvqa_bn_coef_fwd / _bwd) sits between
 * producer and consumer on the dependency chain.  With `publish` one workgroup of the launch also writes what
 * the separate launch would have written: coefficients for later launches, running statistics with torch's
 * momentum rule applied `reps` times (models/image_encoding.py:72-86 runs the backbone prefix 5 times),
 * num_batches_tracked, and -- backward -- the gamma / beta gradients.  stat == NULL: no folding. */
typedef struct mmvqa_bn_fold {
  const double* stat;
  int slots;          /* replicas of the sums that are in use (power of two, <= MMVQA_STAT_SLOTS) */
  int bwd;            /* 0: -> scale, shift (and mean, invstd) ; 1: -> P, Q, R of dz = P*g + Q*z + R */
  int publish;
  int reps;
  double count;       /* elements per channel */
  double keep;        /* (1 - momentum)^reps */
  float eps;
  int reserved;
  const float* gamma;
  const float* beta;    /* forward */
  const float* mean;    /* backward: the forward pass's batch mean / 1/sqrt(var+eps) */
  const float* invstd;
  float* out0;          /* publish: forward scale | backward P */
  float* out1;          /*          forward shift | backward Q */
  float* out2;          /*          forward mean  | backward R */
  float* out3;          /*          forward invstd */
  float* run_mean;
  float* run_var;
  long long* nbt;
  float* dgamma;        /* backward publish: += sum g*xhat */
  float* dbeta;         /*                   += sum g */
} mmvqa_bn_fold;

/* Descriptor of one implicit-GEMM launch (see mm-vqa_amd/csrc/igemm.hip for the field semantics).
 * Replaces: torch.nn.Conv2d / nn.Linear forward+backward as used by models/image_encoding.py:53-86,
 * models/transformer.py:13-15,45-48, models/realformer.py:13-27, models/mmbert.py:133-148. */
typedef struct mmvqa_gemm_desc {
  int M, N, K;
  int splitk;
  int ktiles_per_split;
  const float* A;
  const float* A2;
  const float* a_c0;
  const float* a_c1;
  const float* a_c2;
  int a_pro;
  int a_ld;
  const float* B;
  const float* b_c0;
  const float* b_c1;
  int b_pro;
  int b_ld;
  int b_tapstride;
  int g_SH, g_SW, g_Cs, g_OH, g_OW, g_KH, g_KW, g_stride, g_pad;
  int g_nchw;
  float* C;
  int c_ld;
  int c_atomic;
  float* Cpre;
  const float* bias;
  int act;
  int dact;
  const float* Pre;
  int pre_ld;
  float drop_p;
  uint32_t drop_seed;
  const float* R;
  int r_ld;
  int epi_mode;
  int tap_HW;
  float* tap_out;
  const float* tap_dv;
  const float* Mk;
  int mk_ld;
  const float* mk_s;
  const float* mk_b;
  double* stat1;
  int stat_bwd;
  const float* Z1;
  int z1_ld;
  const float* mean1;
  const float* invstd1;
  double* stat2;
  const float* Z2;
  int z2_ld;
  const float* mean2;
  const float* invstd2;
  float* colsum;
  const float* gate; /* PRO_SILU_GATE: [image][g_Cs] squeeze-excite gates; image = pixel / gate_hw */
  int gate_hw;
  int mk_mode;       /* 0: ReLU mask (Mk*s+b > 0), 1: multiply by SiLU'(Mk*s+b) */
  const int* pixmask; /* optional, KIND_WGRAD of a stride-1 "same" convolution: per output pixel the bit mask of filter
                         taps that fall inside the image (mmvqa_pixmask); enables the uniform-tap weight-gradient loaders */
  float* sk_ws;       /* optional, KIND_FWD / KIND_DGRAD: scratch of sk_ws_floats floats.  With it a launch that has few
                         output tiles and a long contraction may split K over workgroups (splitk, or the launcher's /
                         tuner's choice when splitk <= 0): every workgroup of a tile writes its partial tile to the
                         scratch.  With sk_cnt the split is ticketed: the workgroup of a tile that arrives last sums the
                         partial tiles and applies the whole epilogue in the same kernel; without sk_cnt (or when the
                         tickets or the scratch are too small for the ticketed layout) a second launch does that.  Needs
                         splitk * M * N <= sk_ws_floats; one stream at a time. */
  long long sk_ws_floats;
  mmvqa_bn_fold a_fold; /* optional: the coefficients of the A prologue (a_pro AFFINE_RELU: scale/shift; DZ: P/Q/R) come
                           from raw sums instead of a_c0 / a_c1 / a_c2 (which may then be NULL) */
  int stat_slots;       /* replicas the statistics epilogue (stat1 / stat2) spreads its sums over; 0 = MMVQA_STAT_SLOTS */
  int reserved1;        /* must be 0 (a non-zero value is refused; the field keeps the struct layout unchanged) */
  unsigned int* sk_cnt; /* optional, with sk_ws: sk_cnt_n arrival tickets (one per 64x64 output tile at least) of the
                           ticketed split-K, ZERO before the first launch; every launch leaves them zero */
  int sk_cnt_n;
  int reserved0;        /* operand precision (the field keeps its name so that the struct layout is unchanged):
                           MMVQA_PREC_F32 (0) = fp32 operands, v_mfma_f32_32x32x2_f32;
                           MMVQA_PREC_F16 (1) = both operands rounded to fp16 (nearest-even, bit-equal to
                           torch's .half()) where the loader writes them to LDS, v_mfma_f32_32x32x16_f16, fp32
                           accumulation and epilogue.  The f16 family has no SiLU / gate prologues (refused),
                           and no 8-wave variant (tile 5 runs as tile 3). */
} mmvqa_gemm_desc;

#define MMVQA_PREC_F32 0
#define MMVQA_PREC_F16 1

/* Fused attention (models/transformer.py:19-30 and models/realformer.py:30-45). */
typedef struct mmvqa_attn_desc {
  const float* q;
  const float* k;
  const float* v;
  int row_stride, head_stride;
  float* out;
  int out_row_stride, out_head_stride;
  const long long* mask;
  int mask_on_query;
  const float* prev_in;
  float* prev_out;
  float* probs;
  int B, T, heads;
  float sqrt_d;
  float drop_p;
  uint32_t seed;
  const float* dout;
  float* dq;
  float* dk;
  float* dv;
  const float* dprev_in;
  float* dprev_out;
} mmvqa_attn_desc;

/* Attention of one Feedback-Transformer window (models/feedback_transformer_pytorch.py:160-193): n in {1, 2} queries per
 * sample and head (8 heads of width 64) against n_mem memory entries followed, when n == 2, by the window's own two keys.
 * Rows are window-major: row b*n + i of q / out / dout / dq, row b*2 + i of the self keys and values; memory entry j of
 * sample b lies at mem + (j/2)*mem_win + (b*2 + j%2)*mem_ld, head h at + h*64.  score = q.k * scale + bias[max(i - j, 0)][h]
 * (row 1 of the 32 x 8 table for (query 1, key 0), row 0 elsewhere; key 0 is the oldest memory entry); query 0 does not see
 * the window's second key (probability exactly 0).  probs[((b*8 + h)*n + i)*p_ld + j] keeps the probabilities before
 * dropout; the dropout index of (b, h, i, j) is ((b*8 + h)*T + n_mem + i)*T + j.
 * Backward: dq and the self dk / dv are written; rows < n_mem of dmem_k / dmem_v (addressed like mem_k) and rows 0, 1 of
 * dbias are ADDED to (dbias may be NULL: no bias-table gradient). */
typedef struct mmvqa_fb_attn_desc {
  const float* q;
  int q_ld;
  const float* mem_k;
  const float* mem_v;
  long long mem_win;
  int mem_ld;
  const float* self_k;
  const float* self_v;
  int self_ld;
  const float* bias;
  float* probs;
  int p_ld;
  float* out;
  int out_ld;
  int B, n, n_mem, T;
  float scale, drop_p;
  uint32_t seed;
  const float* dout;
  int dout_ld;
  float* dq;
  int dq_ld;
  float* dself_k;
  float* dself_v;
  int dself_ld;
  float* dmem_k;
  float* dmem_v;
  float* dbias;
} mmvqa_fb_attn_desc;

#define MMVQA_FB_MAX_HIDDENS 16   /* hiddens one aggregation takes: n_layers + 1 */
#define MMVQA_FB_MAX_T 256        /* mem_len of the reference (mmbert.py:118): memory truncation is not built */

/* Architecture of one Model(args) instance: the option surface of pretrain/roco_train.py:23-60,
 * vqamed2019/train.py:32-79 that the hot path reads (SURVEY.md section 5 "Config"). */
typedef struct mmvqa_model_desc {
  int cnn;              /* 0 = resnet (torchvision layout), 1 = tf_efficientnetv2_m (timm features_only) */
  int resnet_layers[4]; /* (3,8,36,3) = resnet152 */
  int resnet_width;     /* 64 */
  int effnet_depth_div; /* 1 = full depth; >1 divides stage repeats (tests) */
  int encoder;          /* 0 = transformer (BertLayer pre-LN), 1 = realformer, 2 = feedback-transformer */
  int hidden, heads, n_layers;
  int emb_vocab, max_pos, type_vocab;
  int num_vis;
  int head_kind;        /* 0 = roco (per-token MLM logits), 1 = VQA-Med (mean-pooled logits), 2 = headless (roco with
                         * task 'distillation', models/mmbert.py:159-161: the output is the encoder's h [B*T][hidden];
                         * fc1 / classifier keep their parameters and never receive a gradient; supcon is ignored) */
  int n_classes;        /* width of classifier[2] */
  int supcon, feat_dim;
  int use_relu;
  float p_drop;         /* --hidden_dropout_prob (BertLayer attention + residual dropouts) */
  float p_emb_drop;     /* BertEmbeddings dropout (0.1) */
  float p_rf_drop;      /* RealFormer dp1/dp2 (0.1) */
  float p_fb_drop;      /* Feedback Transformer attn_dropout / ff_dropout (0.1) */
  int fb_tokens;        /* Feedback Transformer num_tokens = args.vocab_size: rows of its never-used token_emb / to_logits.1
                         * (n_classes changes when classifier[2] is replaced, these do not) */
} mmvqa_model_desc;

/* Geometry of the forward-only BERT teacher (HF BertModel without the pooler; mm-vqa_amd/csrc/teacher.cpp):
 * hidden % 64 == 0 and heads == hidden / 64 (the attention kernel has head dimension 64), hidden <= 1024, inter % 4 == 0,
 * absolute position embeddings, erf GELU, LayerNorm eps (HF: 1e-12). */
typedef struct mmvqa_bert_desc {
  int layers, hidden, heads, inter, vocab, max_pos, type_vocab;
  float eps;
} mmvqa_bert_desc;

typedef struct mmvqa_bert mmvqa_bert;

/* gradient-ready notification of mmvqa_engine_set_grad_callback: grads[lo, hi) (float offsets) are final */
typedef void (*mmvqa_grad_cb)(void* user, long long lo, long long hi);

typedef struct mmvqa_engine mmvqa_engine;

/* ---- library ---------------------------------------------------------------------------- */
int mmvqa_version(void);
const char* mmvqa_last_error(void);
size_t mmvqa_sizeof_gemm_desc(void);
size_t mmvqa_sizeof_attn_desc(void);
size_t mmvqa_sizeof_model_desc(void);
size_t mmvqa_sizeof_fb_attn_desc(void);
size_t mmvqa_sizeof_bert_desc(void);

/* ---- op level (each is what one torch op of the reference's hot path lowers to) ------------ */
/* kind: MMVQA_KIND_*; nchw: 1 only for the 7x7 stem (NCHW image source); tile: 0 auto */
int mmvqa_igemm(const mmvqa_gemm_desc* d, int kind, int nchw, int tile, mmvqa_stream_t s);
int mmvqa_attention(const mmvqa_attn_desc* d, int head_dim, int backward, mmvqa_stream_t s);
/* Forward-only attention with per-sample key lengths, head dimension 64, 1 <= len[b] <= T <= 512, fp32 (bertattn.hip):
 *   out[b][i][h][:] = softmax_j(q_i . k_j * scale ; j < len[b]) . v_j
 * Row b*T + i of q / k / v starts at q + (b*T + i)*row_stride + h*head_stride (so the three may sit inside one fused
 * [B*T][3*hidden] buffer), of out at out + (b*T + i)*out_row_stride + h*out_head_stride; len is int32 [B] on the device.
 * No dropout, nothing saved, no score tensor in memory; online softmax over ceil(len[b] / 32) key tiles, bit-equal from
 * launch to launch.  Keys j >= len[b] have probability exactly 0 and are never read; query rows i >= len[b] are computed
 * like any other row, over the valid keys.  A len[b] outside [1, T] makes that sample's output rows NaN and reads nothing.
 * Refused on the host with MMVQA_ERR_ARG before any HIP call: a null pointer, B, T or heads < 1, T > 512, B or heads >
 * 65535, a row stride below 64, strides that are not multiples of 4.  q / k bases that are not 16-byte aligned are read
 * one element at a time. */
int mmvqa_attention_len_fwd(mmvqa_stream_t s, const float* q, const float* k, const float* v, int row_stride,
                            int head_stride, float* out, int out_row_stride, int out_head_stride, const int* len, int B,
                            int T, int heads, float scale);
/* BertLayer forward, projection and attention in ONE launch (models/transformer.py:19-30: proj_q / proj_k / proj_v,
 * split heads, scores / sqrt(d) - 10000 (1 - mask), softmax, dropout, @ v, merge heads) for T <= 32 and head dimension 64
 * (hidden = 64 * heads): xn [B*T, hidden] -> qkv [B*T, 3*hidden] (q | k | v, kept for the backward pass),
 * probs [B, heads, T(key), T(query)] (before dropout), ctx [B*T, hidden].  W = the three projection weights back to back
 * [3*hidden, hidden], bias [3*hidden] or NULL.  Same dropout stream as mmvqa_attention with the same seed. */
int mmvqa_qkv_attention_fwd(mmvqa_stream_t s, const float* xn, const float* W, const float* bias, const long long* mask,
                            float* qkv, float* probs, float* ctx, int B, int T, int hidden, int heads, float drop_p,
                            uint32_t seed);

/* ---- Feedback Transformer (each launch serves one window of two tokens, or the single token that ends an odd T) */
int mmvqa_fb_attention(const mmvqa_fb_attn_desc* d, int backward, mmvqa_stream_t s);
/* agg[rows][H] = sum_l softmax(layer_weight)_l * hid_l, hid_l = hid + l*hid_stride, n_hid <= MMVQA_FB_MAX_HIDDENS */
int mmvqa_fb_aggregate_fwd(mmvqa_stream_t s, const float* hid, long long hid_stride, int n_hid, const float* layer_weight,
                           float* agg, long rows, int H);
/* dh_l = softmax(layer_weight)_l * dagg written to dh + l*dh_stride; with dtop != NULL the share of the last hidden is
 * ADDED to dtop instead (and dh's last slot is left alone).  d_layer_weight (may be NULL) is ADDED to, through the softmax,
 * from the dot products <dagg, hid_l>: with float atomics, one per block and hidden. */
int mmvqa_fb_aggregate_bwd(mmvqa_stream_t s, const float* dagg, const float* hid, long long hid_stride, int n_hid,
                           const float* layer_weight, float* dh, long long dh_stride, float* dtop, float* d_layer_weight,
                           long rows, int H);
/* pre [M][2F] = (u | gate) -> y [M][F] = dropout(gelu(gate) * u), erf GELU; the dropout index of (r, c) is idx0 + r*F + c */
int mmvqa_geglu_fwd(mmvqa_stream_t s, const float* pre, float* y, long M, int F, float drop_p, uint32_t seed, uint32_t idx0);
int mmvqa_geglu_bwd(mmvqa_stream_t s, const float* dy, const float* pre, float* dpre, long M, int F, float drop_p,
                    uint32_t seed, uint32_t idx0);

/* BatchNorm2d (train: batch stats + running update repeated `reps` times; eval: running stats) */
int mmvqa_bn_coef_fwd(mmvqa_stream_t s, const double* stat, int C, double count, float eps, const float* gamma,
                      const float* beta, float* run_mean, float* run_var, long long* nbt, float momentum, int reps,
                      int training, float* scale, float* shift, float* mean, float* invstd);
int mmvqa_bn_coef_bwd(mmvqa_stream_t s, const double* stat, int C, double count, const float* gamma,
                      const float* mean, const float* invstd, int training, float* P, float* Q, float* R,
                      float* dgamma, float* dbeta);
int mmvqa_bn_add_relu(mmvqa_stream_t s, const float* z, const float* sc, const float* sh, const float* idn,
                      const float* id_sc, const float* id_sh, float* out, long rows, int C);
/* the same block end, relu(bn3(z) + [bn_d](idn)), with the BatchNorm coefficients folded from their raw sums inside the
 * launch (forward mmvqa_bn_fold; fd == NULL: the identity branch is added as it is) -- no coefficient launch between
 * conv3 and the block end (models/image_encoding.py:72-86 via torchvision Bottleneck.forward) */
int mmvqa_bn_add_relu_fold(mmvqa_stream_t s, const float* z, const mmvqa_bn_fold* f3, const float* idn,
                           const mmvqa_bn_fold* fd, float* out, long rows, int C);
int mmvqa_maxpool_fwd(mmvqa_stream_t s, const float* z, const float* sc, const float* sh, float* out,
                      unsigned char* idx, int N, int H, int W, int C, int OH, int OW);
int mmvqa_maxpool_bwd(mmvqa_stream_t s, const float* gp, const unsigned char* idx, const float* extra,
                      const float* z, const float* sc, const float* sh, const float* mean, const float* invstd,
                      float* g0, double* stat, int N, int H, int W, int C, int OH, int OW);
/* LayerNorm over the last axis, optional residual input (y = LN(x + res)).  H must be a multiple of 4 and at most
 * 1024; forward and backward refuse any other H with MMVQA_ERR_ARG and launch nothing. */
int mmvqa_layernorm_fwd(mmvqa_stream_t s, const float* x, const float* res, const float* gamma, const float* beta,
                        float* y, float* sum_out, float* mean, float* rstd, int rows, int H, float eps);
int mmvqa_layernorm_bwd(mmvqa_stream_t s, const float* dy, const float* x, const float* gamma, const float* mean,
                        const float* rstd, const float* dres, float* dx, float* dgamma, float* dbeta, int rows,
                        int H);
/* HF BertEmbeddings + visual-token overwrite (models/mmbert.py:60-67); vis is [num_vis][B][H].  H as for LayerNorm:
 * a multiple of 4, at most 1024, refused with MMVQA_ERR_ARG otherwise by the forward and the backward call alike. */
int mmvqa_embed_fwd(mmvqa_stream_t s, const long long* ids, const long long* seg, const float* word,
                    const float* pos, const float* type, const float* gamma, const float* beta, const float* vis,
                    float* out, float* xhat, float* rstd, int B, int T, int H, int num_vis, float eps,
                    float drop_p, uint32_t seed);
int mmvqa_embed_bwd(mmvqa_stream_t s, const float* dout, const long long* ids, const long long* seg,
                    const float* xhat, const float* rstd, const float* gamma, float* dword, float* dpos,
                    float* dtype, float* dgamma, float* dbeta, float* dvis, int B, int T, int H, int num_vis,
                    float drop_p, uint32_t seed, int pad_idx);
int mmvqa_meanpool_fwd(mmvqa_stream_t s, const float* h, const long long* mask, float* out, int B, int T, int H);
int mmvqa_meanpool_bwd(mmvqa_stream_t s, const float* dout, const long long* mask, float* dh, int B, int T, int H,
                       int accumulate);
/* log_softmax + NLLLoss() + masked argmax accuracy (pretrain/roco_utils.py:235-236,257-265).
 * out3 = {mean loss, #target>0, #correct}; row_lse (nullable) = log sum exp of each row, kept for mmvqa_mlm_grad;
 * dlogits (nullable) = (softmax - onehot) * (*gscale_ptr) * gscale_mul.  Rows that are 16-byte aligned with
 * ld >= round_up(V,4) take the single-pass float4 kernels (one read of the logits); others a scalar form. */
int mmvqa_mlm_loss(mmvqa_stream_t s, const float* logits, int ld, const long long* target, float* row_loss,
                   float* row_lse, long long* pred, float* dlogits, int dld, const float* gscale_ptr, float gscale_mul,
                   int rows, int V, float* out3);
/* backward of the above from the saved row_lse: dlogits = (exp(logits - lse) - onehot) * (*gscale_ptr) * gscale_mul
 * (gscale_ptr: device scalar = the upstream gradient of the mean loss, nullable); pad columns are zeroed.
 * Requires aligned rows (see above). */
int mmvqa_mlm_grad(mmvqa_stream_t s, const float* logits, int ld, const long long* target, const float* row_lse,
                   float* dlogits, int dld, const float* gscale_ptr, float gscale_mul, int rows, int V);
/* ASLSingleLabel (models/asl_singlelabel.py:23-53): per-sample losses + dlogits*gscale */
int mmvqa_asl_loss(mmvqa_stream_t s, const float* logits, int ld, const long long* target, float* row_loss,
                   float* dlogits, int dld, int rows, int C, float gamma_pos, float gamma_neg, float eps,
                   float gscale);
int mmvqa_l2norm_fwd(mmvqa_stream_t s, const float* x, float* y, float* nrm, int rows, int D);
int mmvqa_l2norm_bwd(mmvqa_stream_t s, const float* dy, const float* y, const float* nrm, float* dx, int rows,
                     int D);
/* SupConLoss.forward(features) without labels/mask = SimCLR (models/SupConLoss/loss.py:21-98);
 * f is [2N][D] view-major (loss.py:57), D <= 256; df (nullable) = dloss/df * gscale; ws = 4*N floats of scratch
 * (row log-sums and row losses).  Tiled over row blocks: any N (the all-gathered view set 2N*world of a
 * data-parallel job, SURVEY 8(e) collective 2).  Null f / loss / ws, N < 1, D < 1 or D > 256: MMVQA_ERR_ARG, before
 * anything is launched. */
int mmvqa_supcon_loss(mmvqa_stream_t s, const float* f, float* loss, float* df, float* ws, int N, int D, float temp,
                      float base_temp, float gscale);
/* SupConLoss.forward(features, mask=mask) (loss.py:21-98, contrast_mode 'all', two views): mask is [N][N] fp32, any
 * weights, may be asymmetric; it is tiled 2x2 over the 2N rows with the diagonal of the tiling zeroed, and weights the
 * positives of every anchor: loss = -(T/T_base) mean_a sum_b mt[a][b] (z[a][b] - lse[a]) / M[a], M[a] = sum_b mt[a][b].
 * A row with M[a] == 0 gives NaN, as the reference's division does.  f, df, N, D, gscale as mmvqa_supcon_loss;
 * ws = 6*N floats (2*N more than the unmasked call: the mask row sums M, which the gradient pass needs for both
 * mt[a][b] / M[a] and mt[b][a] / M[b]).  Null f / loss / ws, N < 1, D < 1 or D > 256: MMVQA_ERR_ARG, before anything
 * is launched, as mmvqa_supcon_loss; a null mask is refused the same way (it does not select the unmasked loss). */
int mmvqa_supcon_loss_masked(mmvqa_stream_t s, const float* f, const float* mask, float* loss, float* df, float* ws,
                             int N, int D, float temp, float base_temp, float gscale);
/* Jaccard mask of a batch (SimilarityCalculator.jaccard, supcon_utils.py:110-138) from a word-id CSR on the device:
 * text (row, col), col in 0..3 (caption, three translations), owns the sorted unique ids
 * ids[offsets[4*row+col] .. offsets[4*row+col+1]); offsets has 4*table_rows + 1 entries.  mask[i][j] (n x n fp32) = 1
 * for i == j, else |A_i & B_j| / |A_i | B_j| (0 when both are empty) with A_i = text (rowsA[i], colsA[i]),
 * B_j = text (rowsB[j], colsB[j]); the quotient is the double quotient rounded to fp32.  Sets of any length.  A row
 * or column outside the table gives NaN in the entries it touches.  All pointers are device pointers. */
int mmvqa_jaccard_mask(mmvqa_stream_t s, const int* offsets, const int* ids, const int* rowsA, const int* colsA,
                       const int* rowsB, const int* colsB, float* mask, int n, int table_rows);
/* Cosine mask of a batch from caption sentence embeddings resident on the device (SimilarityCalculator.sentence_trans /
 * bert_embedd, supcon_utils.py:140-168; the encoder itself is not run: the embeddings are computed offline).
 * mmvqa_normalize_rows, once per table, in place: x[r] = x[r] / max(|x[r]|_2, eps) for rows x D fp32 (eps > 0: a zero
 * row stays zero).  mmvqa_cosine_mask: table is [table_rows][4][D] fp32, already normalised, text (row, col) with col in
 * 0..3 (caption, three translations) as in mmvqa_jaccard_mask; mask[i][j] (n x n fp32) = 1 for i == j, else the dot
 * product of text (rowsA[i], colsA[i]) and text (rowsB[j], colsB[j]), one fmaf chain per lane and a fixed-order wave
 * reduction: the same inputs give the same bits on every launch.  Cosines may be negative; nothing is clamped.  A row
 * or column outside the table gives NaN in the entries it touches and reads nothing.  16-byte loads when D % 4 == 0 and
 * table is 16-byte aligned, scalar loads otherwise.  Refused on the host with MMVQA_ERR_ARG before any HIP call: a null
 * operand, rows / n / table_rows < 1, D < 1, D > 4096.  All pointers are device pointers. */
int mmvqa_normalize_rows(mmvqa_stream_t s, float* x, long long rows, int D, float eps);
int mmvqa_cosine_mask(mmvqa_stream_t s, const float* table, const int* rowsA, const int* colsA, const int* rowsB,
                      const int* colsB, float* mask, int n, int D, int table_rows);
/* BERTScore F1 mask of a batch (SimilarityCalculator.bert_score, supcon_utils.py:170-182, restated: the library's
 * greedy_cos_idf with idf = False, one candidate against one reference, bertscore.hip).  xa / xb are the token states of
 * the n candidates / n references, [n][T][D] fp32 each, rows ALREADY of unit length (mmvqa_normalize_rows); text i has
 * lenA[i] / lenB[i] positions, [CLS] first and [SEP] last.  For i != j, with S[t][u] = <xa[i][t], xb[j][u]> over ALL
 * positions t < lenA[i], u < lenB[j] (the specials are match targets):
 *   P = mean over t in 1..lenA[i]-2 of max_u S[t][u]      R = mean over u in 1..lenB[j]-2 of max_t S[t][u]
 *   F = 2 P R / (P + R), a NaN F becomes 0; an empty text (len == 2) gives P = R = F = 0;
 *   mask[i][j] = baseline == 0 ? F : (F - baseline) / (1 - baseline)
 * prec / rec ([n][n] each, both or neither) receive P and R, not rescaled.  mask[i][i] = prec[i][i] = rec[i][i] = 1, not
 * computed.  The score tiles are 32 x 32 products on v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain); no [n][n][T][T]
 * tensor exists anywhere; no atomics: the same inputs give the same bits on every launch.  Positions >= len are never
 * read, 32-row tiles wholly past a length are not visited.  A len outside [2, T] gives NaN in the row (lenA) or column
 * (lenB) it touches and reads nothing for it; the diagonal stays 1.  Refused on the host with MMVQA_ERR_ARG before any HIP
 * call: a null xa / xb / lenA / lenB / mask, exactly one of prec / rec null, n < 1, n > 65535, T < 2, T > 512, D < 64,
 * D % 64 != 0, D > 1024, xa or xb not 16-byte aligned.  All pointers are device pointers. */
int mmvqa_bertscore_mask(mmvqa_stream_t s, const float* xa, const int* lenA, const float* xb, const int* lenB, float* mask,
                         float* prec, float* rec, int n, int T, int D, float baseline);
/* Soft-target cross entropy over logits [rows][C] (leading dimension ld), forward AND backward in one launch, plus a
 * one-workgroup launch for the mean; the criteria vqamed2019/train.py:164-174 selects with --smoothing:
 *   mode 0 (MMVQA_SOFT_CE_HARD)      nn.CrossEntropyLoss, the eval branch (vqamed2019/utils.py:1261-1264)
 *   mode 1 (MMVQA_SOFT_CE_UNIFORM)   LabelSmoothing (utils.py:178-200): soft_j = smoothing / C + (1 - smoothing) [j == t]
 *   mode 2 (MMVQA_SOFT_CE_CATEGORY)  LabelSmoothByCategory, training branch (utils.py:1247-1260, 1296-1300):
 *                                    soft = table[category[row]] with soft_t OVERWRITTEN by 1 - smoothing (:1254);
 *                                    table [n_cat][table_ld] fp32 is computeCategoryTensors' (:1266-1293)
 * row_loss[r] = sum_j soft_j (lse - x_j); *loss = mean over the rows, added in a fixed order (bit-equal from run to
 * run); dlogits (nullable) [rows][dld] = (S p_j - soft_j) * gscale with S = sum_j soft_j (below 1 in mode 2 when t is
 * in its category's set), p = softmax(x).  target / category are int64 device arrays [rows]; category and table are
 * read in mode 2 only.  A target outside [0, C) or a category outside [0, n_cat) makes that row's loss and gradient NaN
 * and reads nothing outside the table.  16-byte accesses where a leading dimension is a multiple of 4 and its base is
 * 16-byte aligned (then the pad columns of dlogits up to round_up(C, 4) are written as 0), scalar otherwise.
 * Refused on the host with MMVQA_ERR_ARG: an unknown mode, rows < 1, C < 1, a null logits / target / row_loss / loss,
 * ld < C, dld < C with dlogits, mode 2 without table or category or with table_ld < C or n_cat < 1, smoothing outside
 * [0, 1]. */
#define MMVQA_SOFT_CE_HARD 0
#define MMVQA_SOFT_CE_UNIFORM 1
#define MMVQA_SOFT_CE_CATEGORY 2
int mmvqa_soft_ce_loss(mmvqa_stream_t s, const float* logits, int ld, const long long* target, const long long* category,
                       const float* table, int table_ld, int n_cat, int mode, double smoothing, float* row_loss,
                       float* loss, float* dlogits, int dld, int rows, int C, float gscale);
/* Distillation loss (pretrain/roco_train.py:94-95: nn.MSELoss; roco_utils.py:230-238: loss = MSELoss(h, target)) of the
 * headless model's output h [B*T][ld] fp32 against the teacher's per-token states (roco_utils.py:112-132), forward AND
 * backward in one launch plus a one-workgroup launch for the mean.  The states of every caption are resident on the
 * device: table [table_rows][H], fp32 or (table_f16 = 1) fp16, a half converting to fp32 exactly; start[b] (int64) is the
 * first table row of sample b's caption and count[b] (int32) its token count; first = num_vis + 2.  The dense target of
 * encode_text's distillation branch (roco_utils.py:162-199) is never stored: row r = b*T + t has the target
 * table[start[b] + t - first] for first <= t < first + n_b with n_b = min(count[b], T - first - 1) (the truncation of
 * :175-176) and a ZERO target everywhere else (:196-197) -- CLS, the visual rows, both SEPs and the padding are trained
 * towards zero, and the mean runs over all B*T*H elements (nn.MSELoss's default).
 * row_sq[r] = sum_j (h - target)^2; *loss = (sum_r row_sq[r]) / (B*T*H), added in a fixed order (bit-equal from run to
 * run); dh (nullable) [B*T][dld] = (h - target) * gscale, one subtraction and one multiplication in fp32 -- the caller
 * passes gscale = float(2 * upstream / (B*T*H)).  A sample with start < 0, count < 0 or start + n_b > table_rows gets NaN
 * in all its row_sq and dh rows and reads nothing from the table.  16-byte accesses of h / dh and whole-vector loads of
 * the table (16 bytes fp32, 8 bytes fp16) when H % 4 == 0, ld and dld are multiples of 4 and the bases are aligned to
 * the access; one element at a time otherwise.  With H % 4 == 0 no column lies between H and round_up(H, 4); columns
 * from H on are not written.  Refused on the host with MMVQA_ERR_ARG before any HIP call: a null h / table / start /
 * count / row_sq / loss, B, T, H or table_rows < 1, first outside [0, T), ld < H, dld < H with dh. */
int mmvqa_distill_mse(mmvqa_stream_t s, const float* h, int ld, const void* table, int table_f16, long long table_rows,
                      const long long* start, const int* count, int first, int B, int T, int H, float* row_sq, float* loss,
                      float* dh, int dld, float gscale);
/* ---- EfficientNetV2 (timm tf_efficientnetv2_m as models/image_encoding.py:15,26,100-115 instantiates it) pieces,
 * NHWC fp32; sc/sh = BatchNorm scale/shift of the producing conv (applied on load), stat = [16][C][2] doubles.
 * depthwise 3x3 (MBConv conv_dw): z2 = dw(silu(z1*s1+b1)), statistics of z2; TF "SAME" padding via pad (begin) */
int mmvqa_dwconv_fwd(mmvqa_stream_t s, const float* z1, const float* s1, const float* b1, const float* w, float* z2,
                     double* stat, int N, int H, int W, int C, int OH, int OW, int stride, int pad);
/* g1 = dw^T(P*g2 + Q*z2 + R) * silu'(z1*s1+b1); BatchNorm-backward sums of bn1 (sum g1, sum g1*xhat1) */
int mmvqa_dwconv_bwd_data(mmvqa_stream_t s, const float* g2, const float* z2, const float* P, const float* Q,
                          const float* R, const float* w, const float* z1, const float* s1, const float* b1,
                          const float* mean1, const float* invstd1, float* g1, double* stat, int N, int H, int W, int C,
                          int OH, int OW, int stride, int pad);
/* dw[c][tap] += sum_pix (P*g2 + Q*z2 + R)[pix,c] * silu(z1*s1+b1)[pix@tap,c] */
int mmvqa_dwconv_bwd_weight(mmvqa_stream_t s, const float* g2, const float* z2, const float* P, const float* Q,
                            const float* R, const float* z1, const float* s1, const float* b1, float* dw, int N, int H,
                            int W, int C, int OH, int OW, int stride, int pad);
/* squeeze-excite: pool[n][c] = mean_hw silu(z*sc+sh); dgate[n][c] = sum_hw t * silu(z*sc+sh) */
int mmvqa_se_pool(mmvqa_stream_t s, const float* z, const float* sc, const float* sh, float* pool, int N, int HW, int C);
int mmvqa_se_dgate(mmvqa_stream_t s, const float* t, const float* z, const float* sc, const float* sh, float* dgate,
                   int N, int HW, int C);
/* The same launches with the BatchNorm coefficients of their operand folded from the producer's raw sums inside the
 * launch (mmvqa_bn_fold; round 3): the FIRST consumer of a train-mode BatchNorm needs no coefficient launch in front.
 * Each workgroup derives the coefficients of its 32 / 64 channels once into LDS; with fold->publish the image-0
 * workgroup of a channel block writes what the coefficient launch would have (scale / shift / mean / invstd / running
 * statistics with the k-fold rule / batch counter; backward: P, Q, R and dgamma, dbeta) for the later consumers.
 * forward folds: (s1, b1) / (sc, sh) are ignored; backward folds (bwd_data publishes, bwd_weight never): (P, Q, R) are.
 * fold == NULL: identical to the plain entry.  (timm MBConv: conv_pw -> bn1 -> SiLU -> conv_dw -> bn2 -> SiLU -> SE) */
int mmvqa_dwconv_fwd_fold(mmvqa_stream_t s, const float* z1, const float* s1, const float* b1, const float* w, float* z2,
                          double* stat, int N, int H, int W, int C, int OH, int OW, int stride, int pad,
                          const mmvqa_bn_fold* fold);
int mmvqa_dwconv_bwd_data_fold(mmvqa_stream_t s, const float* g2, const float* z2, const float* P, const float* Q,
                               const float* R, const float* w, const float* z1, const float* s1, const float* b1,
                               const float* mean1, const float* invstd1, float* g1, double* stat, int N, int H, int W,
                               int C, int OH, int OW, int stride, int pad, const mmvqa_bn_fold* fold);
int mmvqa_dwconv_bwd_weight_fold(mmvqa_stream_t s, const float* g2, const float* z2, const float* P, const float* Q,
                                 const float* R, const float* z1, const float* s1, const float* b1, float* dw, int N,
                                 int H, int W, int C, int OH, int OW, int stride, int pad, const mmvqa_bn_fold* fold);
int mmvqa_se_pool_fold(mmvqa_stream_t s, const float* z, const float* sc, const float* sh, float* pool, int N, int HW,
                       int C, const mmvqa_bn_fold* fold);
/* visual-token tap of a feature map with few channels (models/image_encoding.py:53-62 at the stem: conv1x1 C -> N,
 * activation, global average pool): out[img][n] += mean_hw act(sum_c x'[pix][c] W[n][c]) with x' = x, or
 * relu(x*sc+sh) when sc/sh are given; x [M, C] NHWC rows, M = images*HW.  C in {24, 64}, M and HW multiples of 32,
 * M >= 32768 (mmvqa_tap_thin_ok); `out` [images, N] must be zero on entry. */
int mmvqa_tap_thin_ok(long M, int N, int C, int HW);
int mmvqa_tap_thin_fwd(mmvqa_stream_t s, const float* x, const float* sc, const float* sh, const float* W, float* out,
                       long M, int N, int C, int HW, int act);
/* backward recompute of the same tap: du[pix][n] = dv[img][n] / HW * act'(sum_c x'[pix][c] W[n][c]); du [M, N] */
int mmvqa_tap_thin_bwd(mmvqa_stream_t s, const float* x, const float* sc, const float* sh, const float* W,
                       const float* dv, float* du, long M, int N, int C, int HW, int act);
/* squeeze-excite fully connected layers (timm SqueezeExcite conv_reduce / conv_expand on the pooled [B, mid] tensor):
 *   rpre = pool Wr^T + br, r = silu(rpre)   [B, rd]   Wr [rd, mid]
 *   gpre = r We^T + be,    gate = sigmoid(gpre) [B, mid]   We [mid, rd]
 * backward: from dgate [B, mid] accumulates dWe, dbe, dWr, dbr (+=) and writes dpool [B, mid]; `scratch` holds
 * mmvqa_se_fc_bwd_scratch_floats(B, mid, rd) floats; rd <= 128. */
int mmvqa_se_fc_fwd(mmvqa_stream_t s, const float* pool, const float* Wr, const float* br, const float* We,
                    const float* be, float* rpre, float* r, float* gpre, float* gate, int B, int mid, int rd);
size_t mmvqa_se_fc_bwd_scratch_floats(int B, int mid, int rd);
int mmvqa_se_fc_bwd(mmvqa_stream_t s, const float* dgate, const float* gpre, const float* r, const float* rpre,
                    const float* pool, const float* We, const float* Wr, float* dWe, float* dbe, float* dWr, float* dbr,
                    float* dpool, float* scratch, int B, int mid, int rd);
/* out = (t * gate[n][c] + add[n][c] / HW) * act'(z*sc+sh) (gate/add nullable); BatchNorm-backward sums into stat */
int mmvqa_act_bwd_stats(mmvqa_stream_t s, const float* t, const float* gate, const float* add, const float* z,
                        const float* sc, const float* sh, const float* mean, const float* invstd, int act, float* out,
                        double* stat, long npix, int HW, int C);
/* block end: out = post(pre(z*sc+sh) + idn'), idn' = idn | iact(idn*ids+idb) | nothing */
int mmvqa_bn_act_add(mmvqa_stream_t s, const float* z, const float* sc, const float* sh, int pre_act, const float* idn,
                     const float* ids, const float* idb, int idn_act, int post_act, float* out, long rows, int C);
/* the block end with folded coefficients: out = post(pre(bn(z)) + [bn_d](idn)); idn / fd nullable; (pre, post) in
 * {(NONE, RELU): ResNet Bottleneck = mmvqa_bn_add_relu_fold, (SILU, NONE) and (NONE, NONE): EfficientNetV2 blocks} */
int mmvqa_bn_act_add_fold(mmvqa_stream_t s, const float* z, const mmvqa_bn_fold* f3, int pre_act, const float* idn,
                          const mmvqa_bn_fold* fd, int post_act, float* out, long rows, int C);
/* torch.optim.Adam defaults over a flat buffer; g is scaled by gscale first and zeroed when zero_grad != 0 */
int mmvqa_adam(mmvqa_stream_t s, float* p, float* g, float* m, float* v, long n, double lr, double b1, double b2,
               double eps, int step, float gscale, int zero_grad);
/* Adam with per-range learning rate, weight decay and mode (optimizer groups, no-decay tensors, frozen tensors) in ONE
 * launch over [lo, lo + n) of the flat buffers.  p / g / m / v are the bases of the WHOLE buffers; segs is the table on
 * the host, segs_dev the same table in device memory.  The caller uploads segs_dev when an entry changes (a learning
 * rate step, a tensor frozen) and not otherwise: the step-dependent factors are derived from the launch arguments, in
 * double as mmvqa_adam derives them, so the table does not change from step to step.  The call itself copies nothing
 * and waits for nothing.
 *   table: nseg entries (1..MMVQA_ADAM_MAX_SEGS), ascending, disjoint, non-empty, covering [0, end) without gaps with
 *          lo + n <= end; begin / end are float indices and multiples of 4 (the engine aligns every tensor to 4 floats:
 *          a 16-byte access never straddles two tensors).  Adjacent ranges with equal settings are merged by the caller.
 *   mode:  MMVQA_ADAM_L2        g += weight_decay * p on the scaled gradient (torch.optim.Adam(weight_decay=))
 *          MMVQA_ADAM_DECOUPLED p *= 1 - lr * weight_decay before the update (torch.optim.AdamW)
 *          MMVQA_ADAM_FROZEN    p, m, v are neither read nor written; g is zeroed when zero_grad != 0
 * betas, eps, step, gscale and zero_grad are shared by all segments.  One segment of mode 0 with weight_decay 0 gives
 * the bits of mmvqa_adam, and launches over pieces of a range give the bits of one launch over the range.
 * Refused on the host with MMVQA_ERR_ARG before any HIP call: a null pointer, lo or n negative or no multiple of 4, nseg
 * outside 1..MMVQA_ADAM_MAX_SEGS, a table that is unsorted, overlapping, gapped, misaligned or shorter than lo + n, an
 * unknown mode. */
#define MMVQA_ADAM_L2 0
#define MMVQA_ADAM_DECOUPLED 1
#define MMVQA_ADAM_FROZEN 2
#define MMVQA_ADAM_MAX_SEGS 4096
typedef struct mmvqa_adam_seg {
  long long begin, end;       /* [begin, end) in floats from the base of the buffers */
  double lr, weight_decay;
  int mode;                   /* MMVQA_ADAM_* */
  int reserved;               /* 0 */
} mmvqa_adam_seg;
size_t mmvqa_sizeof_adam_seg(void);
int mmvqa_adam_groups(mmvqa_stream_t s, float* p, float* g, float* m, float* v, long lo, long n,
                      const mmvqa_adam_seg* segs, const mmvqa_adam_seg* segs_dev, int nseg, double b1, double b2,
                      double eps, int step, float gscale, int zero_grad);
/* The two updates above with an exponential moving average of the parameters kept in the same pass: after an element's
 * update, ema = fmaf(p_new - ema, omd, ema) with omd = (float)(1.0 - ema_decay), every rounding the same in whichever
 * loop or ranged launch reaches the element.  p, g, m, v come out with the bits of the plain form.  ema is a flat
 * buffer like the others (the groups form: its base, indexed like p).  In a MMVQA_ADAM_FROZEN segment ema is neither
 * read nor written.  Checked as the plain forms are; refused in addition with MMVQA_ERR_ARG before any HIP call: a null
 * ema, an ema_decay outside [0, 1) or NaN, an ema range of the launch ([ema, ema + n), the groups form
 * [ema + lo, ema + lo + n)) that overlaps one of the other four buffers. */
int mmvqa_adam_ema(mmvqa_stream_t s, float* p, float* g, float* m, float* v, float* ema, long n, double lr, double b1,
                   double b2, double eps, int step, float gscale, int zero_grad, double ema_decay);
int mmvqa_adam_groups_ema(mmvqa_stream_t s, float* p, float* g, float* m, float* v, float* ema, long lo, long n,
                          const mmvqa_adam_seg* segs, const mmvqa_adam_seg* segs_dev, int nseg, double b1, double b2,
                          double eps, int step, float gscale, int zero_grad, double ema_decay);
/* exchange the contents of a[0..n) and b[0..n) in one launch, without a temporary buffer (16-byte accesses: n a
 * multiple of 4, both pointers aligned to 16 bytes, the buffers disjoint; anything else is MMVQA_ERR_ARG) */
int mmvqa_swap(mmvqa_stream_t s, float* a, float* b, long n);
/* loss scaling (torch.amp.GradScaler semantics): found_inf[0] = 1 if any of g[0..n) is inf / nan (left as it is
 * otherwise); with multiply != 0 also g *= inv_scale[0] in place.  Device pointers. */
int mmvqa_amp_unscale(mmvqa_stream_t s, float* g, long n, const float* inv_scale, float* found_inf, int multiply);
/* one-thread update of torch._amp_update_scale_: found_inf -> scale *= backoff, tracker = 0; else tracker + 1 and, at
 * growth_interval, scale *= growth (unless that overflows fp32), tracker = 0 */
int mmvqa_amp_update_scale(mmvqa_stream_t s, float* scale, int* growth_tracker, const float* found_inf,
                           double growth_factor, double backoff_factor, int growth_interval);
/* Per-tensor statistics of a flat fp32 buffer in at most three launches, whatever the number of tensors (the view of a
 * run that wandb.watch(model, log='all') gives the reference: pretrain/roco_train.py:80, vqamed2019/train.py:157).
 * One record per segment [offset, offset + numel) of `base`, in floats; what lies between segments is never read.
 *   counts  n_finite, n_nan, n_posinf, n_neginf; n_zero = finite values equal to +-0
 *   min/max over the finite values, exact (+inf / -inf when there is none)
 *   sum, sumsq over the finite values in fp64, each element converted first and squared in fp64 (exact)
 *   hist    MMVQA_TENSOR_HIST_BINS counts over the finite values between min and max, the position in fp64 with every
 *           operation rounded on its own:  scale = 64.0 / (double(max) - double(min))
 *                                          pos   = (double(x) - double(min)) * scale
 *                                          bin   = min(63, (int)pos)          x == max lands in bin 63
 *           max == min: every finite value in bin 0.
 * Results are bit-identical from call to call (no floating-point atomics; the sums are reduced in a fixed order).
 * flags & MMVQA_TENSOR_STATS_MOMENTS_ONLY: everything but the histogram, whose words are left as they are (two launches).
 * Table: nseg >= 1 entries, ascending and disjoint; numel == 0 is legal and gives zero counts and sums with min = +inf,
 * max = -inf.  A segment is cut into chunks of MMVQA_TENSOR_STATS_CHUNK floats, one workgroup each, and chunk0 is the
 * number of chunks before it (an empty segment counts as one): mmvqa_tensor_stats_workspace checks a host table, fills
 * chunk0 in every entry and returns the bytes of workspace a call needs (0: the table was refused, see
 * mmvqa_last_error).  The caller then uploads the table once: segs is the host copy, segs_dev the same bytes in device
 * memory; out (nseg records) and ws are device memory; n is the length of the buffer at base in floats.  The call
 * copies nothing and waits for nothing; one call at a time per workspace.
 * Refused on the host with MMVQA_ERR_ARG before any HIP call: a null pointer, nseg <= 0, a negative offset or numel, a
 * numel beyond 32 bits, a segment past n, segments that overlap or are unsorted, a chunk0 other than the query's, a
 * workspace that is too small, unknown flags. */
#define MMVQA_TENSOR_HIST_BINS 64
#define MMVQA_TENSOR_STATS_CHUNK 8192
#define MMVQA_TENSOR_STATS_MOMENTS_ONLY 1
typedef struct mmvqa_stat_seg {
  long long offset, numel;    /* in floats from base */
  long long chunk0;           /* filled by mmvqa_tensor_stats_workspace */
} mmvqa_stat_seg;
typedef struct mmvqa_tensor_stat {
  double sum, sumsq;
  long long n_finite, n_nan, n_posinf, n_neginf, n_zero;
  float min, max;
  unsigned int hist[MMVQA_TENSOR_HIST_BINS];
} mmvqa_tensor_stat;
size_t mmvqa_sizeof_stat_seg(void);
size_t mmvqa_sizeof_tensor_stat(void);
size_t mmvqa_tensor_stats_workspace(mmvqa_stat_seg* segs, int nseg);
int mmvqa_tensor_stats(mmvqa_stream_t s, const float* base, long long n, const mmvqa_stat_seg* segs,
                       const mmvqa_stat_seg* segs_dev, int nseg, mmvqa_tensor_stat* out, void* ws, size_t ws_bytes,
                       int flags);
int mmvqa_axpy(mmvqa_stream_t s, float* y, const float* x, float a, long n);
int mmvqa_colsum(mmvqa_stream_t s, const float* x, int ld, int rows, int cols, float* out);
int mmvqa_dropout(mmvqa_stream_t s, float* x, long n, float p, uint32_t seed);
/* y = dropout(x), x untouched: the form the engine's backward pass runs on the gradient of a residual branch, with the
 * (seed, linear index) stream of the forward epilogue that dropped the branch */
int mmvqa_dropout_copy(mmvqa_stream_t s, const float* x, float* y, long n, float p, uint32_t seed);
/* out[n*OH*OW + oy*OW + ox] = bit (kh*KW + kw) set iff input pixel (oy*stride - pad + kh, ox*stride - pad + kw) lies
 * inside the SH x SW image: the zero-padding pattern of torch.nn.Conv2d (torchvision Bottleneck.conv2), as consumed
 * by mmvqa_gemm_desc.pixmask */
int mmvqa_pixmask(mmvqa_stream_t s, int* out, int N, int OH, int OW, int SH, int SW, int KH, int KW, int stride,
                  int pad);
/* Grouped batches: NI images feed B >= NI questions.  Device pointers, fp32 rows of H floats
 * (H % 4 == 0), 16-byte aligned.  The kernels trust the CONTENTS of group / offsets: the caller validates them.
 * mmvqa_vis_expand: vis_q [num_vis][B][H], vis_q[t][b][:] = vis_i[t][group[b]][:] with vis_i [num_vis][NI][H] and
 * group int32 [B], every value in [0, NI).
 * mmvqa_dvis_group_sum: dvis_i [num_vis][NI][H], dvis_i[t][i][:] = the fp32 sum of dvis_q[t][b][:] over
 * offsets[i] <= b < offsets[i+1] (offsets int32 [NI+1], 0 = offsets[0] < ... < offsets[NI] = B), added in ascending b
 * starting from the first row, without atomics: bit-equal from run to run and to a sequential fp32 host loop.
 * MMVQA_ERR_ARG for a null pointer, NI < 1, B < NI, H % 4 != 0 or num_vis < 1. */
int mmvqa_vis_expand(mmvqa_stream_t s, const float* vis_i, const int* group, float* vis_q, int NI, int B, int H,
                     int num_vis);
int mmvqa_dvis_group_sum(mmvqa_stream_t s, const float* dvis_q, const int* offsets, float* dvis_i, int NI, int B, int H,
                         int num_vis);

/* ---- engine level: the whole Model.forward / backward (models/mmbert.py:150-167) ------------ */
int mmvqa_engine_create(const mmvqa_model_desc* desc, mmvqa_engine** out);
void mmvqa_engine_destroy(mmvqa_engine* e);
/* parameter / buffer table: names follow the reference state_dict.
 * kind: 0 = trainable fp32 (offset into params/grads), 1 = fp32 buffer (offset into bufs),
 *       2 = int64 buffer (offset into nbt).  shape is the LOGICAL torch shape; channels_last != 0
 *       means the physical order is [d0][d2][d3][d1]. */
int mmvqa_engine_num_tensors(const mmvqa_engine* e);
int mmvqa_engine_tensor_info(const mmvqa_engine* e, int i, char* name, int name_cap, int* kind, int* ndim,
                             long long shape[4], long long* offset, int* channels_last);
long long mmvqa_engine_param_floats(const mmvqa_engine* e);
long long mmvqa_engine_buf_floats(const mmvqa_engine* e);
long long mmvqa_engine_nbt_count(const mmvqa_engine* e);
/* plan for a batch geometry; returns workspace bytes needed (0 on error) */
size_t mmvqa_engine_plan(mmvqa_engine* e, int B, int T, int img_h, int img_w);
/* Plan for a GROUPED batch geometry: NI images feed B >= NI text rows.  The backbone, its taps
 * and their BatchNorm counts are laid out for NI images, the embedding, encoder and heads for B rows; the plan adds the
 * expanded tokens and their gradient [num_vis][B][hidden] and room for group[B] and offsets[NI+1].  Returns 0 with a
 * message for NI < 1 or NI > B.  After it mmvqa_engine_forward_grouped is the forward; mmvqa_engine_forward,
 * mmvqa_engine_forward_tokens, mmvqa_engine_feature_map and mmvqa_engine_backward_feature answer MMVQA_ERR_STATE.
 * mmvqa_engine_plan is the plan with NI == B and no grouping: no buffer and no launch more than before. */
size_t mmvqa_engine_plan_grouped(mmvqa_engine* e, int NI, int B, int T, int img_h, int img_w);
/* Borrowed buffers of the following forward / backward calls.  Part of the WORKSPACE holds state that must survive
 * between calls (tap-validity tables of the 3x3 weight gradients, the zeroed arrival tickets of the split-K GEMM
 * launches): the first forward after a bind puts it in place on that call's stream; the caller must not write to the
 * workspace while it is bound (re-bind after any such write). */
int mmvqa_engine_bind(mmvqa_engine* e, float* params, float* grads, float* bufs, long long* nbt, void* workspace,
                      size_t workspace_bytes);
/* img fp32 NCHW [B,3,h,w]; ids/seg/mask int64 [B,T]; logits [rows][ld] (rows = B*T or B);
 * feat [B][feat_dim] or NULL.  training != 0: batch-stat BN + dropout with `seed`.
 * head_kind 2: `logits` receives the encoder output h [B*T][ld], ld >= hidden and ld % 4 == 0 (columns from hidden on are
 * not written), and mmvqa_engine_backward takes the gradient of that buffer in the same layout. */
int mmvqa_engine_forward(mmvqa_engine* e, mmvqa_stream_t s, const float* img, const long long* ids,
                         const long long* seg, const long long* mask, float* logits, int logits_ld, float* feat,
                         int training, uint32_t seed);
/* The forward of a grouped plan: img [NI,3,h,w]; group int32 [B] (non-decreasing from 0 to NI-1 in steps of at most 1)
 * and offsets int32 [NI+1] (questions of image i: offsets[i] <= b < offsets[i+1]) are DEVICE pointers whose contents the
 * caller has validated; both are copied into the workspace on the stream, so the backward does not read the caller's
 * buffers.  Backbone and taps on the NI images, mmvqa_vis_expand, then embedding / encoder / heads on the B rows as in
 * mmvqa_engine_forward.  mmvqa_engine_backward after it sums the token gradients per image (mmvqa_dvis_group_sum) and
 * runs the backbone's backward once, on NI images.  mmvqa_engine_visual_tokens gives the [num_vis][NI][hidden] tokens.
 * MMVQA_ERR_STATE when the current plan is not grouped. */
int mmvqa_engine_forward_grouped(mmvqa_engine* e, mmvqa_stream_t s, const float* img, const int* group,
                                 const int* offsets, const long long* ids, const long long* seg, const long long* mask,
                                 float* logits, int logits_ld, float* feat, int training, uint32_t seed);
/* accumulates into grads; dlogits same layout as logits; dfeat nullable */
int mmvqa_engine_backward(mmvqa_engine* e, mmvqa_stream_t s, const float* dlogits, int dlogits_ld,
                          const float* dfeat);
/* Attribution: after an EVAL-mode mmvqa_engine_forward (training = 0, fp32 operands), writes dA = the gradient of
 * sum(dlogits * logits) with respect to the deepest backbone feature map A (ResNet: output of layer4, tapped by conv2;
 * EfficientNet: output of the last block = o[4], tapped by conv7), NHWC fp32 [B][H][W][C], into the caller's buffer.
 * Data gradients only (heads -> encoder -> one visual-token row -> one tap) on the given stream alone: parameters, the
 * gradient buffer, BatchNorm buffers are not written, no gradient callback is called.  MMVQA_ERR_STATE before any forward
 * or after a training-mode forward, MMVQA_ERR_ARG in the f16 operand mode. */
int mmvqa_engine_backward_feature(mmvqa_engine* e, mmvqa_stream_t s, const float* dlogits, int dlogits_ld, float* dA);
/* where A lives (inside the bound workspace: valid from a forward until the next one) and its dimensions */
int mmvqa_engine_feature_map(mmvqa_engine* e, const float** A, int* H, int* W, int* C);
/* Grad-CAM (vqamed2019/grad_cam2.py:139-176, batched per sample) from A and dA [B][H][W][C] (H * W <= 256, C % 4 == 0,
 * C <= 4096): w[c] = mean_hw dA, cam = relu(mean_c w[c] A) / max -> cam [B][H][W], valid[b] = 0 (and zeros) when the
 * maximum is not positive; up [B][IH][IW] = bilinear resize (half-pixel centres, edge clamp) or NULL; overlay
 * [B][IH][IW][3] uint8 = clip(alpha * jet[(uint8)(255 up)] + image_u8, 0, 255) or NULL (then image_u8 / jet may be
 * NULL); jet: 256 x 3 uint8 colour table on the device. */
int mmvqa_gradcam(mmvqa_stream_t s, const float* A, const float* dA, int B, int H, int W, int C, float* cam, int* valid,
                  float* up, int IH, int IW, const unsigned char* image_u8, const unsigned char* jet, float alpha,
                  unsigned char* overlay);
/* Forward from cached visual tokens.  mmvqa_engine_visual_tokens: where the last forward left the
 * num_vis visual tokens, [num_vis][B][hidden] as mmvqa_embed_fwd reads them, inside the bound workspace: valid until the
 * next forward.  mmvqa_engine_forward_tokens: the EVAL-mode forward (no dropout, no BatchNorm touched) with `vis` in that
 * layout in place of the backbone and its taps: the embedding with the overwrite, the encoder and the heads (or the
 * headless copy), all on the given stream; logits / feat as in mmvqa_engine_forward.  The backbone's activations in the
 * workspace are not those of `vis`: mmvqa_engine_backward and mmvqa_engine_backward_feature answer MMVQA_ERR_STATE
 * until the next mmvqa_engine_forward.  fp32 operands only: MMVQA_ERR_ARG in the f16 operand mode, and for a null pointer
 * or a bad logits_ld. */
int mmvqa_engine_visual_tokens(mmvqa_engine* e, const float** vis);
int mmvqa_engine_forward_tokens(mmvqa_engine* e, mmvqa_stream_t s, const float* vis, const long long* ids,
                                const long long* seg, const long long* mask, float* logits, int logits_ld, float* feat);
/* The visual-token cache: cache is one fp32 device array [N][K][num_vis][hidden] (N images, K
 * views of each); idx / view are int32 DEVICE arrays [B] whose contents the caller has validated on the host
 * (0 <= idx[b] < N, 0 <= view[b] < K): the kernels do not range-check them.
 * mmvqa_tokens_gather: out[t][b][:] = cache[idx[b]][view[b]][t][:], out in the engine's [num_vis][B][hidden] layout.
 * mmvqa_tokens_scatter: its inverse for ONE view (a host scalar) and distinct idx[b]: cache[idx[b]][view][t][:] = vis[t][b][:].
 * MMVQA_ERR_ARG before any HIP call for a null pointer, hidden % 8 != 0 or hidden > 1024, B / N / K / num_vis < 1, a
 * cache / out / vis that is not 16-byte aligned, a scalar view outside [0, K). */
int mmvqa_tokens_gather(mmvqa_stream_t s, const float* cache, int N, int K, const int* idx, const int* view, float* out,
                        int B, int hidden, int num_vis);
int mmvqa_tokens_scatter(mmvqa_stream_t s, const float* vis, const int* idx, int view, float* cache, int N, int K, int B,
                         int hidden, int num_vis);
/* Training from the cache.  mmvqa_engine_forward_cached: mmvqa_tokens_gather straight into the workspace's visual tokens,
 * then exactly the launches of mmvqa_engine_forward after the backbone (embedding, encoder, heads or the headless copy)
 * with the same dropout probabilities and per-site seeds, so `training` and `seed` mean what they mean there.  fp32
 * operands only (MMVQA_ERR_ARG in the f16 mode), ungrouped plan only (MMVQA_ERR_STATE).  The backbone's activations in
 * the workspace are not those of the tokens: mmvqa_engine_backward and mmvqa_engine_backward_feature answer
 * MMVQA_ERR_STATE after it, as after mmvqa_engine_forward_tokens.
 * mmvqa_engine_backward_cached: valid only directly after mmvqa_engine_forward_cached (MMVQA_ERR_STATE otherwise): heads,
 * encoder and embedding backward, accumulated into grads as mmvqa_engine_backward does; the gradient of the visual
 * tokens is computed into the workspace and dropped.  The backbone's and the five taps' range of grads and every
 * BatchNorm buffer are not written.  With a gradient callback, [enc_lo, n) and [0, emb_hi) are announced as in
 * mmvqa_engine_backward and the backbone + taps range [emb_hi, enc_lo) as it stands: one partition, as always. */
int mmvqa_engine_forward_cached(mmvqa_engine* e, mmvqa_stream_t s, const float* cache, int N, int K, const int* idx,
                                const int* view, const long long* ids, const long long* seg, const long long* mask,
                                float* logits, int logits_ld, float* feat, int training, uint32_t seed);
int mmvqa_engine_backward_cached(mmvqa_engine* e, mmvqa_stream_t s, const float* dlogits, int dlogits_ld,
                                 const float* dfeat);
/* Attribution methods beyond Grad-CAM (vqamed2019/grad_cam.py:65-72), maps as in mmvqa_gradcam
 * (H * W <= 256, C % 4 == 0, C <= 4096, else MMVQA_ERR_ARG before any HIP call).
 * mmvqa_cam_weights: w [B][C] of method 0 (gradcam: mean_p dA, bit-equal to mmvqa_gradcam's own), 1 (gradcam++:
 * sum_p max(g, 0) g^2 / (2 g^2 + S_c g^3 + 1e-7), 0 where g == 0) or 2 (xgradcam: sum_p g a / (S_c + 1e-7)), with
 * S_c = sum_p A[b][p][c].
 * mmvqa_cam_from_weights: the tail of mmvqa_gradcam (mean over channels of w * A, ReLU, division by the maximum, valid,
 * resize, overlay) with the channel weights w [B][C] from memory, or with the map before the ReLU raw [B][H][W] from
 * memory (then A may be NULL); exactly one of w and raw is non-NULL. */
int mmvqa_cam_weights(mmvqa_stream_t s, int method, const float* A, const float* dA, int B, int H, int W, int C, float* w);
int mmvqa_cam_from_weights(mmvqa_stream_t s, const float* A, const float* w, const float* raw, int B, int H, int W, int C,
                           float* cam, int* valid, float* up, int IH, int IW, const unsigned char* image_u8,
                           const unsigned char* jet, float alpha, unsigned char* overlay);
/* Eigen-CAM's map before the ReLU: raw [B][H][W] = X v1 with X = A[b] as [H*W][C], every column centred over the
 * positions, and v1 its first right singular vector, by 64 power iterations on the Gram matrix X X^T kept in
 * gram [B][H*W][H*W] (scratch).  Sign: the entry of largest magnitude is positive (ties: lowest position).
 * resid [B] = |G u - lambda u| / lambda of the result.  X all zero or H * W = 1: raw = 0 and resid = 0. */
int mmvqa_eigencam_raw(mmvqa_stream_t s, const float* A, int B, int H, int W, int C, float* gram, float* raw, float* resid);
/* Ablation-CAM's visual tokens: tokens [B][nc][hidden] = mean_p act(u[b][p][n] - Wt[n][c] A[b][p][c]) for the channels
 * c = c0 .. c0 + nc - 1 of A [B][HW][C], i.e. the token of a bias-free 1x1 tap Wt [hidden][C] with channel c zeroed;
 * act: 1 (ReLU) or 3 (SERF).  u [B * HW][hidden] = A Wt^T is scratch: computed first when compute_u != 0, reused
 * (from an earlier chunk of the same pass) otherwise.  mmvqa_ablation_weights: w [B][C] = (score[b] - score_abl[b][c]) /
 * score[b], zeros where score[b] == 0. */
int mmvqa_ablated_tokens(mmvqa_stream_t s, const float* A, const float* Wt, float* u, int B, int HW, int C, int hidden,
                         int act, int c0, int nc, int compute_u, float* tokens);
int mmvqa_ablation_weights(mmvqa_stream_t s, const float* score, const float* score_abl, int B, int C, float* w);
/* data-parallel overlap: cb(user, lo, hi) is called on the HOST thread inside mmvqa_engine_backward as soon as
 * the kernels completing grads[lo, hi) (float offsets) are enqueued and the given stream is ordered behind them, so
 * the caller can start the all-reduce of that range on its communication stream while backward continues.
 * The ranges of one backward partition [0, param_floats) exactly.  NULL disables. */
int mmvqa_engine_set_grad_callback(mmvqa_engine* e, mmvqa_grad_cb cb, void* user);
/* per-shape kernel configuration: while enabled, every implicit-GEMM shape met for the first time in
 * forward/backward is timed over its candidate (tile, split-K) set and the fastest is kept for later
 * calls.  A pass run with tuning enabled is a throw-away pass (outputs/statistics are garbage).
 * Returns the number of tuned shapes so far (>= 0) or a negative error.  enable is 0 or 1: any other value is
 * refused with MMVQA_ERR_ARG and changes nothing. */
int mmvqa_engine_tune(mmvqa_engine* e, int enable);
/* operand precision of every implicit GEMM of the following forward / backward calls: MMVQA_PREC_F32 (default) or
 * MMVQA_PREC_F16 (mixed precision: both operands of each contraction rounded to fp16 nearest-even, fp32 accumulation;
 * everything else -- storage, BatchNorm / LayerNorm, softmax, attention's QK^T and PV, epilogues, losses -- stays fp32).
 * The fused QKV + attention launch is replaced by the unfused route in f16 mode.  ResNet encoders only: an
 * EfficientNet engine refuses MMVQA_PREC_F16 (MMVQA_ERR_ARG). */
int mmvqa_engine_set_precision(mmvqa_engine* e, int mode);
/* Frozen backbone (the reference's commented-out `for p in self.parameters(): p.requires_grad = False`,
 * models/image_encoding.py:50-51).  flags are read by the next forward and recorded for its backward, as the precision
 * mode is; 0 (the default) is the full backward.
 *   MMVQA_FREEZE_BACKBONE: the parameters of the CNN body (transformer.trans.model.*, the floats between the embedding
 *     block and the first tap weight) receive no gradient.  The backward runs heads, encoder and the embedding as
 *     always, then only the weight gradient of the five taps (recompute of du, dW_tap; no data gradient), on the
 *     caller's stream: no convolution data or weight gradient, no BatchNorm-backward coefficients, no max-pool,
 *     depthwise or squeeze-excite backward.  The gradient callback still partitions the whole buffer; the frozen range
 *     is announced as it stands (this call never writes it).  The forward is unchanged: train-mode BatchNorm keeps
 *     using batch statistics and updating the running ones, as torch does with requires_grad=False under .train().
 *   MMVQA_FREEZE_BN_STATS (only with MMVQA_FREEZE_BACKBONE): the backbone's BatchNorms use their running statistics and
 *     leave running_mean / running_var / num_batches_tracked alone (backbone.eval()); dropout and everything outside
 *     the backbone stay as `training` says.
 * Any other bit, or MMVQA_FREEZE_BN_STATS alone, is refused with MMVQA_ERR_ARG and changes nothing. */
#define MMVQA_FREEZE_BACKBONE 1
#define MMVQA_FREEZE_BN_STATS 2
int mmvqa_engine_set_frozen(mmvqa_engine* e, int flags);
/* per-kernel-class timing (HIP events on the launch stream) of the NEXT forward+backward:
 * enable, run, then read back {n_launches, total_ms, algorithmic_flops} per class.
 * enable = 1: as the step normally runs (weight-gradient GEMMs on the second stream beside the data-gradient chain, so
 * a launch's time includes sharing the chip); enable = 2: everything on one stream; 0: off (both streams again) */
int mmvqa_engine_profile(mmvqa_engine* e, int enable);
int mmvqa_engine_profile_read(mmvqa_engine* e, int cls, long long* launches, double* ms, double* flops);
/* the same split by region of the step (SURVEY 8(d) per-block figures): 0 CNN backbone, 1 tap 1x1 convs
 * (image_encoding.py:53-62), 2 fused QKV / kqv projection (transformer.py:13-20, realformer.py:32-33) fwd+dgrad+wgrad,
 * 3 attention core (transformer.py:22-27, realformer.py:34-44), 4 rest of the encoder, 5 heads (mmbert.py:133-137,
 * 154-166), 6 embeddings, 7 BatchNorm coefficient kernels, 8 the fused QKV projection + attention launch (class 1, its
 * FLOPs = projection + attention) */
int mmvqa_engine_profile_read_region(mmvqa_engine* e, int region, int cls, long long* launches, double* ms,
                                     double* flops);
/* the HBM-bound kernels of the profiled step one by one: launches, total ms and ALGORITHMIC bytes (every tensor the
 * kernel has to read or write, once, fp32) -- bytes / ms against the 8 TB/s roofline.  kernel: 1 bn_add_relu (block end),
 * 2 / 3 maxpool fwd / bwd, 4 / 5 layernorm fwd / bwd, 6 dropout_copy, 7 bn_act_add, 8 / 9 / 10 dwconv fwd / bwd_data /
 * bwd_weight, 11 se_pool, 12 se_dgate, 13 act_bwd_stats, 14 / 15 tap_thin fwd / bwd */
int mmvqa_engine_profile_read_hbm(mmvqa_engine* e, int kernel, long long* launches, double* ms, double* bytes);

/* ---- BERT teacher: a frozen, forward-only HF BertModel (no pooler) on the device ------------------------------
 * The teacher of --task distillation (pretrain/roco_utils.py:112-132: last_hidden_state of every caption) and of the
 * cosine SupCon mask (models/SupConLoss/supcon_utils.py:140-159: mean hidden state of caption and translation).
 * Tensor table: HF names without the "bert." prefix, embeddings.word_embeddings.weight ...
 * encoder.layer.{i}.output.LayerNorm.bias, shapes as torch has them, offsets in floats into ONE parameter buffer; query /
 * key / value weights (then biases) of a layer lie back to back, so the projection is one product.
 * plan(B, T) -> workspace bytes (0 on error; T <= min(512, max_pos)); bind borrows the parameter buffer and the
 * workspace (both 16-byte aligned); forward enqueues on the given stream only, without synchronising or allocating:
 * ids int64 [B][T] (0 beyond a sample's length), len int32 [B] as in mmvqa_attention_len_fwd, token type 0, out
 * [B*T][hidden] fp32 = last_hidden_state including the padded rows.  ids outside the vocabulary are not checked.
 * forward_layers is forward stopped after the first n_layers layers (1..layers): the last LayerNorm of layer n_layers
 * writes out, which is HF's hidden_states[n_layers] (what BERTScore reads, supcon_utils.py:103-108); n_layers == layers is
 * forward itself, bit for bit; an n_layers outside 1..layers is refused with MMVQA_ERR_ARG before any HIP call. */
int mmvqa_bert_create(const mmvqa_bert_desc* desc, mmvqa_bert** out);
void mmvqa_bert_destroy(mmvqa_bert* e);
int mmvqa_bert_num_tensors(const mmvqa_bert* e);
long long mmvqa_bert_param_floats(const mmvqa_bert* e);
int mmvqa_bert_tensor_info(const mmvqa_bert* e, int i, char* name, int name_cap, int* ndim, long long shape[2],
                           long long* offset);
size_t mmvqa_bert_plan(mmvqa_bert* e, int B, int T);
int mmvqa_bert_bind(mmvqa_bert* e, const float* params, void* workspace, size_t workspace_bytes);
int mmvqa_bert_forward(mmvqa_bert* e, mmvqa_stream_t s, const long long* ids, const int* len, int B, int T, float* out);
int mmvqa_bert_forward_layers(mmvqa_bert* e, mmvqa_stream_t s, const long long* ids, const int* len, int B, int T,
                              int n_layers, float* out);

/* ---------------------------------------------------------------------------------------------------------------
 * Device input pipeline: the torchvision/PIL transforms of pretrain/roco_train.py:98-112 and
 * vqamed2019/train.py:179-200 on decoded uint8 RGB images in HBM, bit-exact with Pillow's arithmetic.
 * One job = PIL crop(box) -> resize((rw, rh), BILINEAR) -> keep the out_w x out_h window at (ox, oy):
 *   Resize(224)+CenterCrop(224): box = whole image, (rw, rh) = resized size, (ox, oy) = crop offset
 *   RandomResizedCrop          : box = sampled crop, (rw, rh) = (224, 224), (ox, oy) = (0, 0)
 * All pointers are device pointers; coefficient tables come from mmvqa_resample_coeffs (host) copied to the device. */
typedef struct mmvqa_resample_job {
  const unsigned char* src; int sh, sw, spitch;   /* source image, HWC uint8, row pitch in bytes */
  int bx, by, bw, bh;                             /* box of the source that is resized */
  int rw, rh;                                     /* size the box is resized to */
  int ox, oy;                                     /* window of the resized image that is produced */
  int ty0, tyn;                                   /* box rows [ty0, ty0+tyn) the vertical pass of the window reads */
  unsigned char* tmp;                             /* scratch [tyn][out_w][3] */
  unsigned char* dst; int dpitch;                 /* output [out_h][out_w][3] */
  const int* hb; const int* hk; int hks;          /* horizontal bounds [rw][2] / coefficients [rw][hks] */
  const int* vb; const int* vk; int vks;          /* vertical   bounds [rh][2] / coefficients [rh][vks] */
} mmvqa_resample_job;
size_t mmvqa_sizeof_resample_job(void);
/* HOST function: Pillow's bilinear resampling coefficients (Resample.c precompute_coeffs + normalize_coeffs_8bpc) of
 * resizing source range [in0, in1) of an axis of in_size pixels to out_size; returns taps per output (ksize);
 * with bounds == NULL only the size is returned */
int mmvqa_resample_coeffs(int in_size, double in0, double in1, int out_size, int* bounds, int* kk, int ksize_cap);
int mmvqa_aug_resample(mmvqa_stream_t s, const mmvqa_resample_job* jobs_dev, int njobs, int max_tmp_rows, int out_h,
                       int out_w);
/* Image.rotate(angle, NEAREST, expand=False, fillcolor=0) on [B][H][W][3]: fix_dev[b][6] = the 16.16 fixed-point
 * affine coefficients a0..a5 of Geometry.c affine_fixed (computed by the host side from the angle) */
int mmvqa_aug_rotate(mmvqa_stream_t s, const unsigned char* src, unsigned char* dst, const int* fix_dev, int B, int H,
                     int W);
/* one ColorJitter round in place: image b applies op_dev[b] (0 brightness, 1 contrast, 2 saturation, 3 hue with
 * factor = the uint8 hue shift, < 0 none) with factor_dev[b]; lsum_dev = B uint64 of scratch (L sums for contrast) */
int mmvqa_aug_jitter_round(mmvqa_stream_t s, unsigned char* img, const int* op_dev, const float* factor_dev,
                           unsigned long long* lsum_dev, int B, int npix);
/* ToTensor + Normalize: uint8 [B][npix][3] -> fp32 [B][3][npix], (x/255 - mean)/std; mean3/std3 are HOST pointers */
int mmvqa_aug_to_tensor(mmvqa_stream_t s, const unsigned char* img, float* out, int B, int npix, const float* mean3,
                        const float* std3);
/* Per-image parameters of mmvqa_aug_train_fused (the training chain after Resize + CenterCrop, in one launch).
 * Table fields are offsets in int32 elements into tables_dev, whose contents come from mmvqa_resample_coeffs (host):
 * hb / hk = bounds [S][2] / coefficients [S][hks] of resizing the box width to S, vb / vk the same for its height. */
typedef struct mmvqa_aug_record {
  int bx, by, bw, bh;                             /* RandomResizedCrop box in the S x S image (x, y, width, height) */
  int ty0, tyn;                                   /* box rows [ty0, ty0+tyn) the vertical pass reads */
  int hb, hk, hks;                                /* horizontal tables: offsets, taps per output */
  int vb, vk, vks;                                /* vertical tables: offsets, taps per output */
  int fix[6];                                     /* RandomRotation: affine_fixed 16.16 coefficients (mmvqa_aug_rotate) */
  int op[4];                                      /* ColorJitter order: op of round r (0..3 as in jitter_round, < 0 none) */
  float factor[4];                                /* factor of round r (hue: the uint8 shift) */
} mmvqa_aug_record;
size_t mmvqa_sizeof_aug_record(void);
/* RandomResizedCrop -> RandomRotation -> 4 ColorJitter rounds -> ToTensor + Normalize of B images in ONE launch, bit
 * for bit what mmvqa_aug_resample + _rotate + 4 x _jitter_round + _to_tensor compute.  src_u8 [B][S][S][3] is the
 * Resize + CenterCrop output; it is overwritten with the last byte stage.  out_f32 [B][3][S][S]; mean3/std3 are HOST
 * pointers.  Returns MMVQA_ERR_ARG for bad pointers or sizes and when S * S * 3 bytes do not fit the device's LDS.
 * The records are device data the call cannot check: the caller keeps every box inside the S x S image and the row
 * window [ty0, ty0 + tyn) inside the box.  An image whose record breaks that is skipped by the kernel: its slot of
 * out_f32 and of src_u8 is left as it was (no error is reported). */
int mmvqa_aug_train_fused(mmvqa_stream_t s, unsigned char* src_u8, float* out_f32, const mmvqa_aug_record* records_dev,
                          const int* tables_dev, int B, int S, const float* mean3, const float* std3);
/* mmvqa_aug_train_fused on V views of each of B images (SupCon's TwoCropTransform), in ONE launch: row v * B + n of
 * scratch_u8 [V*B][S][S][3] and out_f32 [V*B][3][S][S] is view v of image n, under record v * B + n of records_dev.
 * src_u8 [B][S][S][3] is the Resize + CenterCrop output; it is only read.  scratch_u8 ends holding each view's last
 * byte stage.  Every view is bit for bit what mmvqa_aug_train_fused gives for the same image and record.  Returns
 * MMVQA_ERR_ARG, with nothing enqueued, for null pointers, B, V or S <= 0, S * S * 3 bytes beyond the device's LDS,
 * and when the byte ranges of src_u8 and scratch_u8 overlap.  Records as for mmvqa_aug_train_fused: a view whose
 * record breaks the rules is skipped by the kernel, its rows of out_f32 and scratch_u8 left as they were. */
int mmvqa_aug_train_fused_views(mmvqa_stream_t s, const unsigned char* src_u8, unsigned char* scratch_u8, float* out_f32,
                                const mmvqa_aug_record* records_dev, const int* tables_dev, int B, int V, int S,
                                const float* mean3, const float* std3);
/* 1 if mmvqa_aug_train_fused takes images of S x S on the current device (S * S * 3 bytes fit its LDS), else 0 */
int mmvqa_aug_train_fused_fits(int S);
/* A non-blocking stream of the current device's LEAST priority (HIP: 1 = low, 0 = normal, negative = high), created
 * on first use and kept for the life of the process; *priority (may be NULL) receives the priority it has.  The input
 * pipeline runs on it so that its kernels yield to the training step's whenever both are ready. */
int mmvqa_low_priority_stream(mmvqa_stream_t* out, int* priority);
/* the priority of stream s (hipStreamGetPriority) */
int mmvqa_stream_priority(mmvqa_stream_t s, int* priority);

#ifdef __cplusplus
}
#endif
#endif /* MMVQA_H */
