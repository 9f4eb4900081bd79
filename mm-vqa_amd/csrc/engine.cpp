// Launch sequences of the MMBERT hot path (see engine.h).  Reference call stack: SURVEY.md 3.1-3.4.
//
//   forward : ResNet stem -> [tap] -> maxpool -> bottlenecks (+tap at every layer end)
//             -> BertEmbeddings + visual-token overwrite -> 4x BertLayer | 4x ResEncoderBlock
//             -> fc1/SERF/classifier (per token or mean-pooled) [+ SupCon head]
//   backward: the exact reverse, every BatchNorm/ReLU/residual backward folded into GEMM
//             prologues/epilogues (igemm.hip), weight gradients accumulated into `grads`.
#include "engine.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

// --------------------------------------------------------------------------- errors
static thread_local char g_err[1024] = "";
int mmvqa_set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
const char* mmvqa_get_error() { return g_err; }

// --------------------------------------------------------------------------- parameter table
namespace {

struct Builder {
  mmvqa_engine* e;
  long long align4(long long x) { return (x + 3) & ~3LL; }
  long long add(const std::string& name, int kind, std::initializer_list<long long> shape, int cl = 0) {
    TensorSpec s;
    s.name = name; s.kind = kind; s.ndim = (int)shape.size(); s.channels_last = cl;
    long long n = 1; int i = 0;
    for (auto v : shape) { s.shape[i++] = v; n *= v; }
    for (; i < 4; ++i) s.shape[i] = 1;
    long long& cur = kind == 0 ? e->n_params : (kind == 1 ? e->n_bufs : e->n_nbt);
    if (kind != 2) cur = align4(cur);
    s.offset = cur;
    cur += n;
    e->specs.push_back(s);
    return s.offset;
  }
  ConvRef conv(const std::string& name, int cin, int cout, int k, int stride, int pad) {
    ConvRef c; c.Cin = cin; c.Cout = cout; c.KH = k; c.stride = stride; c.pad = pad;
    c.w = add(name + ".weight", 0, {cout, cin, k, k}, 1);
    return c;
  }
  BNRef bn(const std::string& name, int C, int reps) {
    BNRef b; b.C = C; b.reps = reps;
    b.gamma = add(name + ".weight", 0, {C});
    b.beta = add(name + ".bias", 0, {C});
    b.rmean = add(name + ".running_mean", 1, {C});
    b.rvar = add(name + ".running_var", 1, {C});
    b.nbt = add(name + ".num_batches_tracked", 2, {});
    return b;
  }
  LinRef lin(const std::string& name, int in, int out, bool bias) {
    LinRef l; l.in = in; l.out = out;
    l.w = add(name + ".weight", 0, {out, in});
    l.b = bias ? add(name + ".bias", 0, {out}) : -1;
    return l;
  }
  LNRef ln(const std::string& name, int H) {
    LNRef l;
    l.g = add(name + ".weight", 0, {H});
    l.b = add(name + ".bias", 0, {H});
    return l;
  }
};

int build_tables(mmvqa_engine* e) {
  const mmvqa_model_desc& d = e->d;
  Builder b{e};
  const int H = d.hidden;
  // models/mmbert.py:52-56 -- HF BertEmbeddings
  const std::string be = "transformer.bert_embedding.";
  e->emb_word = b.add(be + "word_embeddings.weight", 0, {d.emb_vocab, H});
  e->emb_pos = b.add(be + "position_embeddings.weight", 0, {d.max_pos, H});
  e->emb_type = b.add(be + "token_type_embeddings.weight", 0, {d.type_vocab, H});
  e->emb_ln = b.ln(be + "LayerNorm", H);
  e->emb_hi = b.align4(e->n_params);
  // models/image_encoding.py:43-62 -- backbone + tap convs
  const std::string rm = "transformer.trans.model.";
  const int w = d.resnet_width;
  if (d.cnn == 1) {
    // timm tf_efficientnetv2_m(features_only=True) -- architecture: SURVEY.md Appendix B (wiring unpinned)
    struct St { int type, rep, stride, exp, out; bool se; };
    const St arch[7] = {{0, 3, 1, 1, 24, false}, {1, 5, 2, 4, 48, false}, {1, 5, 2, 4, 80, false}, {2, 7, 2, 4, 160, true},
                        {2, 14, 1, 6, 176, true}, {2, 18, 2, 6, 304, true}, {2, 5, 1, 6, 512, true}};
    const int feat_of_stage[7] = {0, 1, 2, -1, 3, -1, 4};
    const int div = d.effnet_depth_div > 0 ? d.effnet_depth_div : 1;
    e->stem_conv = b.conv(rm + "conv_stem", 3, 24, 3, 2, 0);
    e->stem_bn = b.bn(rm + "bn1", 24, 1);
    e->stem_bn.eps = 1e-3f;
    int cin = 24;
    for (int sI = 0; sI < 7; ++sI) {
      const St& a = arch[sI];
      const int reps = std::max(1, (a.rep + div - 1) / div);
      for (int k = 0; k < reps; ++k) {
        EffBlock blk;
        const std::string p = rm + "blocks." + std::to_string(sI) + "." + std::to_string(k) + ".";
        blk.type = a.type; blk.cin = cin; blk.cout = a.out; blk.stride = k == 0 ? a.stride : 1;
        blk.skip = blk.stride == 1 && cin == a.out;
        blk.mid = cin * a.exp;
        if (a.type == 0) {
          blk.c_a = b.conv(p + "conv", cin, a.out, 3, blk.stride, 0);
          blk.b_a = b.bn(p + "bn1", a.out, 1);
        } else if (a.type == 1) {
          blk.c_a = b.conv(p + "conv_exp", cin, blk.mid, 3, blk.stride, 0);
          blk.b_a = b.bn(p + "bn1", blk.mid, 1);
          blk.c_p = b.conv(p + "conv_pwl", blk.mid, a.out, 1, 1, 0);
          blk.b_p = b.bn(p + "bn2", a.out, 1);
        } else {
          blk.rd = (int)std::lround(cin * 0.25);
          blk.c_a = b.conv(p + "conv_pw", cin, blk.mid, 1, 1, 0);
          blk.b_a = b.bn(p + "bn1", blk.mid, 1);
          blk.dw_w = b.add(p + "conv_dw.weight", 0, {blk.mid, 1, 3, 3}, 1);
          blk.b_dw = b.bn(p + "bn2", blk.mid, 1);
          blk.se_r.in = blk.mid; blk.se_r.out = blk.rd;
          blk.se_r.w = b.add(p + "se.conv_reduce.weight", 0, {blk.rd, blk.mid, 1, 1}, 1);
          blk.se_r.b = b.add(p + "se.conv_reduce.bias", 0, {blk.rd});
          blk.se_e.in = blk.rd; blk.se_e.out = blk.mid;
          blk.se_e.w = b.add(p + "se.conv_expand.weight", 0, {blk.mid, blk.rd, 1, 1}, 1);
          blk.se_e.b = b.add(p + "se.conv_expand.bias", 0, {blk.mid});
          blk.c_p = b.conv(p + "conv_pwl", blk.mid, a.out, 1, 1, 0);
          blk.b_p = b.bn(p + "bn3", a.out, 1);
        }
        blk.b_a.eps = blk.b_dw.eps = blk.b_p.eps = 1e-3f;
        blk.feature = (k == reps - 1) ? feat_of_stage[sI] : -1;
        cin = a.out;
        e->eff.push_back(blk);
      }
    }
    const char* tapn[5] = {"conv2", "conv3", "conv4", "conv5", "conv7"};
    const int tapc[5] = {24, 48, 80, 176, 512};
    for (int k = 0; k < 5; ++k) {
      e->taps[k].C = tapc[k];
      e->taps[k].w = b.add(std::string("transformer.trans.") + tapn[k] + ".weight", 0, {H, tapc[k], 1, 1}, 1);
    }
  } else if (d.cnn == 0) {
  e->stem_conv = b.conv(rm + "conv1", 3, w, 7, 2, 3);
  e->stem_bn = b.bn(rm + "bn1", w, 5);
  int inpl = w;
  for (int l = 0; l < 4; ++l) {
    const int planes = w << l, stride = l == 0 ? 1 : 2, reps = 4 - l;
    for (int k = 0; k < d.resnet_layers[l]; ++k) {
      BlockRef blk;
      const std::string p = rm + "layer" + std::to_string(l + 1) + "." + std::to_string(k) + ".";
      const int s = k == 0 ? stride : 1;
      blk.c1 = b.conv(p + "conv1", inpl, planes, 1, 1, 0);
      blk.b1 = b.bn(p + "bn1", planes, reps);
      blk.c2 = b.conv(p + "conv2", planes, planes, 3, s, 1);
      blk.b2 = b.bn(p + "bn2", planes, reps);
      blk.c3 = b.conv(p + "conv3", planes, planes * 4, 1, 1, 0);
      blk.b3 = b.bn(p + "bn3", planes * 4, reps);
      blk.has_ds = (k == 0);
      if (blk.has_ds) {
        blk.cd = b.conv(p + "downsample.0", inpl, planes * 4, 1, s, 0);
        blk.bd = b.bn(p + "downsample.1", planes * 4, reps);
      }
      inpl = planes * 4;
      e->blocks.push_back(blk);
    }
    e->layer_end[l] = (int)e->blocks.size() - 1;
  }
  b.add(rm + "fc.weight", 0, {1000, (long long)w * 32});  // exists in the state_dict, never used (quirk 2)
  b.add(rm + "fc.bias", 0, {1000});
  const char* tapn[5] = {"conv2", "conv3", "conv4", "conv5", "conv7"};
  const int tapc[5] = {w * 32, w * 16, w * 8, w * 4, w};
  for (int k = 0; k < 5; ++k) {
    e->taps[k].C = tapc[k];
    e->taps[k].w = b.add(std::string("transformer.trans.") + tapn[k] + ".weight", 0, {H, tapc[k], 1, 1}, 1);
  }
  } else {
    return mmvqa_set_error(MMVQA_ERR_ARG, "engine: unknown cnn=%d", d.cnn);
  }
  // encoder
  e->enc_lo = b.align4(e->n_params);
  if (d.encoder == 0) {
    const std::string bl = "transformer.blocks.";
    e->norm1 = b.ln(bl + "norm1", H);
    e->norm2 = b.ln(bl + "norm2", H);
    e->bert.resize(d.n_layers);
    for (int i = 0; i < d.n_layers; ++i) {
      BertLayerRef& L = e->bert[i];
      const std::string a = bl + "attention." + std::to_string(i) + ".";
      // q,k,v weights (and biases) are laid out back to back: one fused [3H,H] projection
      L.qkv.in = H; L.qkv.out = 3 * H;
      L.qkv.w = b.add(a + "proj_q.weight", 0, {H, H});
      long long kw = b.add(a + "proj_k.weight", 0, {H, H});
      long long vw = b.add(a + "proj_v.weight", 0, {H, H});
      L.qkv.b = b.add(a + "proj_q.bias", 0, {H});
      long long kb = b.add(a + "proj_k.bias", 0, {H});
      long long vb = b.add(a + "proj_v.bias", 0, {H});
      if (kw != L.qkv.w + (long long)H * H || vw != kw + (long long)H * H || kb != L.qkv.b + H || vb != kb + H)
        return mmvqa_set_error(MMVQA_ERR_STATE, "engine: qkv parameters are not contiguous (H=%d)", H);
    }
    for (int i = 0; i < d.n_layers; ++i) e->bert[i].proj = b.lin(bl + "proj." + std::to_string(i), H, H, true);
    for (int i = 0; i < d.n_layers; ++i) {
      const std::string f = bl + "feedforward." + std::to_string(i) + ".";
      e->bert[i].fc1 = b.lin(f + "fc1", H, 4 * H, true);
      e->bert[i].fc2 = b.lin(f + "fc2", 4 * H, H, true);
    }
  } else if (d.encoder == 2) {
    // models/mmbert.py:110-127 -> FeedbackTransformer(num_tokens, dim, depth, seq_len=2, mem_len=256, dim_head=64, heads=8);
    // names of its state_dict.  to_kv is ONE tensor (attn.to_kv = shared_kv_proj, :229-230): it is listed under the
    // reference's first name, the Python shim adds the aliases (layers.l>0 and shared_kv_proj).
    const std::string fb = "transformer.block.";
    b.add(fb + "token_emb.weight", 0, {d.fb_tokens, H});                         // never used (:260 is commented out)
    e->fb_rel = b.add(fb + "pos_emb.relative_attention_bias.weight", 0, {32, 8});
    e->fb.resize(d.n_layers);
    for (int i = 0; i < d.n_layers; ++i) {
      FBLayerRef& L = e->fb[i];
      const std::string p = fb + "layers." + std::to_string(i) + ".";
      L.ln_a = b.ln(p + "0.fn.norm", H);
      L.to_q = b.lin(p + "0.fn.fn.to_q", H, 512, false);
      if (i == 0) e->fb_kv = b.lin(p + "0.fn.fn.to_kv", H, 1024, false);
      L.to_out = b.lin(p + "0.fn.fn.to_out", 512, H, true);
      L.ln_f = b.ln(p + "1.fn.norm", H);
      L.w1 = b.lin(p + "1.fn.fn.net.0", H, 8 * H, true);
      L.w2 = b.lin(p + "1.fn.fn.net.3", 4 * H, H, true);
    }
    e->fb_lw = b.add(fb + "layer_weight", 0, {d.n_layers + 1});
    b.ln(fb + "to_logits.0", H);                                                 // never used (to_logits_bool = False)
    b.lin(fb + "to_logits.1", H, d.fb_tokens, true);
  } else {
    e->rf.resize(d.n_layers);
    const int es = H / 8;
    for (int i = 0; i < d.n_layers; ++i) {
      RFLayerRef& L = e->rf[i];
      const std::string m = "transformer.mains." + std::to_string(i) + ".";
      L.kqv = b.lin(m + "kqv", es, 3 * es, false);
      L.proj = b.lin(m + "proj", H, H, false);
      L.ln1 = b.ln(m + "ln1", H);
      L.ln2 = b.ln(m + "ln2", H);
      L.ff0 = b.lin(m + "ff.0", H, 4 * H, true);
      L.ff2 = b.lin(m + "ff.2", 4 * H, H, true);
    }
  }
  // heads (models/mmbert.py:133-148)
  e->fc1 = b.lin("fc1", H, H, true);
  e->cls0 = b.lin("classifier.0", H, H, true);
  e->cls_ln = b.ln("classifier.1", H);
  e->cls2 = b.lin("classifier.2", H, d.n_classes, true);
  if (d.supcon) {
    e->head0 = b.lin("head.0", H, H, true);
    e->head2 = b.lin("head.2", H, d.feat_dim, true);
  }
  e->n_params = b.align4(e->n_params);
  e->n_bufs = b.align4(e->n_bufs);
  return MMVQA_OK;
}

// --------------------------------------------------------------------------- workspace plan
struct Arena {
  size_t cur = 0;
  size_t f(size_t n) {  // floats, 64-float (256 B) aligned
    cur = (cur + 63) & ~(size_t)63;
    size_t o = cur;
    cur += n;
    return o;
  }
};

// replicas of a folded BatchNorm's sums: every consumer workgroup reads slots x C x 16 bytes in its setup phase, every
// producer workgroup adds one value per channel and sum to ONE replica -- few replicas for the consumers' sake, enough
// of them that a replica does not collect more than a few dozen same-address atomics
int fold_slots(double rows) {
  static const int forced = getenv("MMVQA_BN_SLOTS") ? atoi(getenv("MMVQA_BN_SLOTS")) : 0;
  if (forced == 1 || forced == 2 || forced == 4 || forced == 8 || forced == 16) return forced;
  const double row_tiles = rows / 64.0;
  return row_tiles >= 32.0 ? 4 : (row_tiles >= 8.0 ? 2 : 1);
}

void plan_bn(Arena& a, BNRef& bn, double count) {
  bn.count = count;
  const size_t C = bn.C;
  bn.scale = a.f(C); bn.shift = a.f(C); bn.mean = a.f(C); bn.invstd = a.f(C);
  bn.P = a.f(C); bn.Q = a.f(C); bn.R = a.f(C);
}

}  // namespace

static inline int conv_out(int x, int k, int s, int p) { return (x + 2 * p - k) / s + 1; }

size_t engine_plan(mmvqa_engine* e, int NI, int B, int T, int IH, int IW, bool grouped) {
  const mmvqa_model_desc& d = e->d;
  if (d.encoder == 2 && (T < 2 || T > MMVQA_FB_MAX_T)) {
    mmvqa_set_error(MMVQA_ERR_ARG, "plan: the feedback-transformer takes 2 <= T <= %d tokens (T=%d): one token has no keys, "
                                   "beyond %d the reference truncates its memory, which is not built", MMVQA_FB_MAX_T, T, MMVQA_FB_MAX_T);
    return 0;
  }
  if (B <= 0 || T <= 0 || (T > 128 && d.encoder != 2) || T > d.max_pos || T <= d.num_vis) {
    mmvqa_set_error(MMVQA_ERR_ARG, "plan: bad B=%d T=%d (max_pos %d, num_vis %d, T<=128)", B, T, d.max_pos, d.num_vis);
    return 0;
  }
  if (NI < 1 || NI > B || (!grouped && NI != B)) {
    mmvqa_set_error(MMVQA_ERR_ARG, "plan: NI=%d images for B=%d text rows (1 <= NI <= B, NI == B unless grouped)", NI, B);
    return 0;
  }
  e->B = B; e->NI = NI; e->grouped = grouped; e->T = T; e->IH = IH; e->IW = IW;
  e->pixmask_off.clear(); e->ws_ready = false;
  Arena a;
  const int H = d.hidden;
  const size_t M = (size_t)B * T;
  // ---- backbone
  size_t max_io = 0, max_mid = 0, max_tapM = 0;
  if (d.cnn == 1) {
    // TensorFlow SAME padding: out = ceil(in/s); the odd padding element goes to the end, so the leading pad is
    // total/2 and the trailing one is implied by the bounds checks of the gather
    auto same = [](int in, int k, int s2, int* out) {
      *out = (in + s2 - 1) / s2;
      int total = std::max((*out - 1) * s2 + k - in, 0);
      return total / 2;
    };
    int ph = same(IH, 3, 2, &e->SH), pw = same(IW, 3, 2, &e->SW);
    if (ph != pw) { mmvqa_set_error(MMVQA_ERR_ARG, "plan: image %dx%d needs different SAME pads per axis", IH, IW); return 0; }
    e->stem_conv.pad = ph;
    const size_t M0 = (size_t)NI * e->SH * e->SW;
    e->z0 = a.f(M0 * 24);
    e->eff_a0 = a.f(M0 * 24);
    plan_bn(a, e->stem_bn, (double)M0);
    max_io = M0 * 24;
    int h = e->SH, wd = e->SW;
    size_t max_se = 0, max_separt = 0;
    for (auto& blk : e->eff) {
      blk.N = NI; blk.H = h; blk.W = wd;
      int p1 = same(h, 3, blk.stride, &blk.OH), p2 = same(wd, 3, blk.stride, &blk.OW);
      if (p1 != p2) { mmvqa_set_error(MMVQA_ERR_ARG, "plan: map %dx%d needs different SAME pads per axis", h, wd); return 0; }
      blk.pad = p1;
      const size_t Min = (size_t)NI * h * wd, Mout = (size_t)NI * blk.OH * blk.OW;
      if (blk.type == 0) {
        blk.c_a.pad = p1;
        blk.za = a.f(Mout * blk.cout); plan_bn(a, blk.b_a, (double)Mout);
      } else if (blk.type == 1) {
        blk.c_a.pad = p1;
        blk.za = a.f(Mout * blk.mid); plan_bn(a, blk.b_a, (double)Mout);
        blk.zp = a.f(Mout * blk.cout); plan_bn(a, blk.b_p, (double)Mout);
        max_mid = std::max(max_mid, Mout * blk.mid);
      } else {
        blk.za = a.f(Min * blk.mid); plan_bn(a, blk.b_a, (double)Min);
        blk.zdw = a.f(Mout * blk.mid); plan_bn(a, blk.b_dw, (double)Mout);
        blk.zp = a.f(Mout * blk.cout); plan_bn(a, blk.b_p, (double)Mout);
        blk.pool = a.f((size_t)NI * blk.mid); blk.gpre = a.f((size_t)NI * blk.mid); blk.gate = a.f((size_t)NI * blk.mid);
        blk.rpre = a.f((size_t)NI * blk.rd); blk.r = a.f((size_t)NI * blk.rd);
        max_mid = std::max(max_mid, std::max(Min, Mout) * blk.mid);
        max_se = std::max(max_se, (size_t)NI * blk.mid);
        max_separt = std::max(max_separt, mmvqa_se_fc_bwd_scratch_floats(NI, blk.mid, blk.rd));
        if (!k_se_fc_bwd_ok(blk.rd)) {   // refuse here, not at the first backward
          mmvqa_set_error(MMVQA_ERR_ARG, "plan: squeeze-excite reduce width %d exceeds what se_fc_bwd supports", blk.rd);
          return 0;
        }
      }
      blk.out = a.f(Mout * blk.cout);
      max_io = std::max(max_io, std::max(Min * blk.cin, Mout * blk.cout));
      if (blk.feature >= 0) { e->taps[blk.feature].HW = blk.OH * blk.OW; e->taps[blk.feature].M = (long)Mout; }
      h = blk.OH; wd = blk.OW;
    }
    for (int k = 0; k < 2; ++k) { e->eff_gA[k] = a.f(max_mid); e->eff_gB[k] = a.f(max_mid); }
    for (int i = 0; i < 6; ++i) e->eff_se[i] = a.f(max_se + 64);
    e->eff_separt = a.f(max_separt + 64);
    for (int k = 0; k < 5; ++k) {
      max_tapM = std::max(max_tapM, (size_t)e->taps[k].M);
      e->tapgrad[k] = a.f((size_t)e->taps[k].M * e->taps[k].C);
    }
  } else {
  e->SH = conv_out(IH, 7, 2, 3); e->SW = conv_out(IW, 7, 2, 3);
  e->PH = conv_out(e->SH, 3, 2, 1); e->PW = conv_out(e->SW, 3, 2, 1);
  const int w = d.resnet_width;
  const size_t M0 = (size_t)NI * e->SH * e->SW;
  e->z0 = a.f(M0 * w);
  plan_bn(a, e->stem_bn, (double)M0);
  e->p0 = a.f((size_t)NI * e->PH * e->PW * w);
  e->pool_idx = a.f(((size_t)NI * e->PH * e->PW * w + 3) / 4);
  int h = e->PH, wd = e->PW;
  max_io = M0 * w; max_tapM = M0;
  for (auto& blk : e->blocks) {
    blk.N = NI; blk.H = h; blk.W = wd;
    blk.OH = conv_out(h, 3, blk.c2.stride, 1); blk.OW = conv_out(wd, 3, blk.c2.stride, 1);
    const size_t Min = (size_t)NI * h * wd, Mout = (size_t)NI * blk.OH * blk.OW;
    blk.z1 = a.f(Min * blk.c1.Cout);
    if (blk.c2.stride == 1) {   // per-pixel tap-validity table of the 3x3 weight gradient: one per geometry, in the workspace
      char key[96];
      snprintf(key, sizeof(key), "%d,%d,%d,%d,%d", NI, blk.OH, blk.OW, blk.c2.KH, blk.c2.pad);
      if (!e->pixmask_off.count(key))
        e->pixmask_off[key] = mmvqa_engine::PixGeom{NI, blk.OH, blk.OW, h, wd, blk.c2.KH, blk.c2.stride, blk.c2.pad, a.f(Mout)};
    }
    blk.z2 = a.f(Mout * blk.c2.Cout);
    blk.z3 = a.f(Mout * blk.c3.Cout);
    blk.out = a.f(Mout * blk.c3.Cout);
    plan_bn(a, blk.b1, (double)Min);
    plan_bn(a, blk.b2, (double)Mout);
    plan_bn(a, blk.b3, (double)Mout);
    if (blk.has_ds) { blk.zd = a.f(Mout * blk.cd.Cout); plan_bn(a, blk.bd, (double)Mout); }
    if (e->bn_fold) {
      blk.b1.slots = fold_slots((double)Min);
      blk.b2.slots = blk.b3.slots = blk.bd.slots = fold_slots((double)Mout);
    }
    max_io = std::max(max_io, std::max(Min * blk.c1.Cin, Mout * blk.c3.Cout));
    max_mid = std::max(max_mid, std::max(Min * blk.c1.Cout, Mout * blk.c2.Cout));
    h = blk.OH; wd = blk.OW;
  }
  // taps: k=0..3 on the outputs of layer4..layer1, k=4 on the stem
  for (int k = 0; k < 4; ++k) {
    const BlockRef& blk = e->blocks[e->layer_end[3 - k]];
    e->taps[k].HW = blk.OH * blk.OW;
    e->taps[k].M = (long)NI * blk.OH * blk.OW;
  }
  e->taps[4].HW = e->SH * e->SW;
  e->taps[4].M = (long)M0;
  for (int k = 0; k < 5; ++k) {
    max_tapM = std::max(max_tapM, (size_t)e->taps[k].M);
    e->tapgrad[k] = a.f((size_t)e->taps[k].M * e->taps[k].C);
  }
  }
  e->vis = a.f((size_t)5 * NI * H);
  for (int i = 0; i < 3; ++i) e->sk_ws[i] = a.f(SK_WS_FLOATS);   // split-K partial tiles (caller's / side / tap stream)
  for (int i = 0; i < 3; ++i) e->sk_cnt[i] = a.f(SK_CNT_N);      // arrival tickets of ticketed split-K launches
  e->dvis = a.f((size_t)5 * NI * H);
  e->du = a.f(max_tapM * H);
  for (int i = 0; i < 3; ++i) e->gbuf[i] = a.f(max_io);
  e->g1buf = a.f(max_mid);
  e->g2buf = a.f(max_mid);
  e->dstmp = a.f(max_io);
  // ---- embeddings / encoder
  e->emb_out = a.f(M * H); e->emb_xhat = a.f(M * H); e->emb_rstd = a.f(M);
  if (d.encoder == 0) {
    for (auto& L : e->bert) {
      L.xn1 = a.f(M * H); L.mean1 = a.f(M); L.rstd1 = a.f(M);
      L.qkvo = a.f(M * 3 * H); L.probs = a.f((size_t)B * d.heads * T * T); L.ctx = a.f(M * H);
      L.y = a.f(M * H); L.xn2 = a.f(M * H); L.mean2 = a.f(M); L.rstd2 = a.f(M);
      L.pre1 = a.f(M * 4 * H); L.h1 = a.f(M * 4 * H); L.z = a.f(M * H);
    }
  } else if (d.encoder == 2) {
    const size_t nh = (size_t)d.n_layers + 1, W2 = (size_t)2 * B;
    e->fb_hid = a.f(nh * M * H); e->fb_ghid = a.f(nh * M * H);
    e->fb_mem = a.f(M * 1024); e->fb_dmem = a.f(M * 1024); e->fb_agg = a.f(M * H); e->fb_out = a.f(M * H);
    e->fb_dhs = a.f(nh * W2 * H);
    e->fb_s[0] = a.f(W2 * 4 * H); e->fb_s[1] = a.f(W2 * H); e->fb_s[2] = a.f(W2 * 512); e->fb_s[3] = a.f(W2 * H); e->fb_s[4] = a.f(W2 * H);
    for (auto& L : e->fb) {
      L.xn_a = a.f(M * H); L.mean_a = a.f(M); L.rstd_a = a.f(M);
      L.q = a.f(M * 512); L.kv = a.f(M * 1024); L.probs = a.f((size_t)B * 8 * (T + 1) * T); L.ctx = a.f(M * 512);
      L.xmid = a.f(M * H); L.xn_f = a.f(M * H); L.mean_f = a.f(M); L.rstd_f = a.f(M);
      L.pre = a.f(M * 8 * H); L.gg = a.f(M * 4 * H);
      L.g_pre = a.f(M * 8 * H); L.g_mid = a.f(M * H); L.g_q = a.f(M * 512); L.g_kv = a.f(M * 1024);
    }
  } else {
    for (auto& L : e->rf) {
      L.kqvo = a.f(M * 3 * H); L.probs = a.f((size_t)B * 8 * T * T); L.prev = a.f((size_t)B * T * T * 8);
      L.res = a.f(M * H); L.s1 = a.f(M * H); L.x1 = a.f(M * H); L.mean1 = a.f(M); L.rstd1 = a.f(M);
      L.pre = a.f(M * 4 * H); L.hact = a.f(M * 4 * H); L.s2 = a.f(M * H); L.x2 = a.f(M * H);
      L.mean2 = a.f(M); L.rstd2 = a.f(M);
    }
  }
  // ---- heads
  const size_t HM = d.head_kind == 0 ? M : (size_t)B;
  e->hd_pool = a.f((size_t)B * H);
  e->hd_upre = a.f(HM * H); e->hd_u = a.f(HM * H); e->hd_c0 = a.f(HM * H); e->hd_c1 = a.f(HM * H);
  e->hd_mean = a.f(HM); e->hd_rstd = a.f(HM);
  if (d.supcon) {
    e->sc_pool = a.f((size_t)B * H); e->sc_pre = a.f((size_t)B * H); e->sc_a = a.f((size_t)B * H);
    e->sc_f = a.f((size_t)B * d.feat_dim); e->sc_nrm = a.f(B); e->sc_y = a.f((size_t)B * d.feat_dim);
  }
  // ---- backward scratch
  e->t_a = a.f(M * H); e->t_b = a.f(M * H); e->t_c = a.f(M * H); e->t_d = a.f(M * H);
  e->t_big = a.f(M * 4 * H);
  e->t_dprev[0] = a.f((size_t)B * T * T * 8); e->t_dprev[1] = a.f((size_t)B * T * T * 8);
  // ---- BatchNorm statistic zones (doubles): [fwd of every BN][bwd of every BN]
  e->statzone = a.f(0);
  size_t sd = 0;  // in doubles
  auto take = [&](BNRef& bn, bool bwd) {
    (bwd ? bn.stat_b : bn.stat_f) = sd;
    sd += (size_t)MMVQA_STAT_SLOTS * bn.C * 2;
  };
  for (int pass = 0; pass < 2; ++pass) {
    const bool bw = pass == 1;
    take(e->stem_bn, bw);
    for (auto& blk : e->blocks) { take(blk.b1, bw); take(blk.b2, bw); take(blk.b3, bw); if (blk.has_ds) take(blk.bd, bw); }
    for (auto& blk : e->eff) { take(blk.b_a, bw); if (blk.type == 2) take(blk.b_dw, bw); if (blk.type != 0) take(blk.b_p, bw); }
  }
  const size_t half = sd / 2;
  if (sd != 2 * half) { mmvqa_set_error(MMVQA_ERR_STATE, "plan: stat zone mismatch"); return 0; }
  e->statzone_floats = sd * 2;
  a.f(e->statzone_floats);
  // ---- grouped batches: the tokens / their gradients per question, and the engine's copy of group[B] | offsets[NI+1]
  // (behind everything else: the ungrouped layout is the one it always was)
  e->vis_q = e->dvis_q = e->grp = 0;
  if (grouped) {
    e->vis_q = a.f((size_t)5 * B * H);
    e->dvis_q = a.f((size_t)5 * B * H);
    e->grp = a.f((size_t)B + NI + 1);
  }
  e->ws_floats = (a.cur + 63) & ~(size_t)63;
  e->planned = true;
  e->bound = false;
  return e->ws_floats * sizeof(float);
}

// --------------------------------------------------------------------------- launch helpers
#define WS(off) (e->ws + (off))
#define PRM(off) (e->params + (off))
#define GRD(off) (e->grads + (off))
static inline double* stat_ptr(mmvqa_engine* e, size_t doff) {
  return reinterpret_cast<double*>(e->ws + e->statzone) + doff;
}

static int prof_begin(mmvqa_engine* e, hipStream_t st, int cls, double flops, int tag = HB_NONE, double bytes = 0.0) {
  if (!e->prof_on) return MMVQA_OK;
  mmvqa_engine::ProfRec r;
  HIP_CHECK_RET(hipEventCreate(&r.a));
  HIP_CHECK_RET(hipEventCreate(&r.b));
  r.cls = cls; r.reg = e->prof_reg; r.flops = flops; r.tag = tag != HB_NONE ? tag : e->prof_tag; r.bytes = bytes;
  HIP_CHECK_RET(hipEventRecord(r.a, st));
  e->prof.push_back(r);
  return MMVQA_OK;
}
static int prof_end(mmvqa_engine* e, hipStream_t st) {
  if (!e->prof_on) return MMVQA_OK;
  HIP_CHECK_RET(hipEventRecord(e->prof.back().b, st));
  return MMVQA_OK;
}
struct RegScope {   // tags the launches of a scope with a profiler region
  mmvqa_engine* e; int old;
  RegScope(mmvqa_engine* e_, int r) : e(e_), old(e_->prof_reg) { e->prof_reg = r; }
  ~RegScope() { e->prof_reg = old; }
};
#define REG(r) RegScope _reg_scope(e, r)
// an HBM-bound launch: `bytes` = the tensors it has to read and write once (algorithmic bytes, fp32)
#define RUNB_ON(s, tag, bytes, call)                             \
  do {                                                           \
    TRY(prof_begin(e, s, PROF_OTHER, 0, tag, (double)(bytes)));  \
    TRY(call);                                                   \
    TRY(prof_end(e, s));                                         \
  } while (0)
#define RUN_ON(s, cls, flops, call)    \
  do {                                 \
    TRY(prof_begin(e, s, cls, flops)); \
    TRY(call);                         \
    TRY(prof_end(e, s));               \
  } while (0)
// the common case: the launch goes to the stream the enclosing function calls `st`
#define RUNB(tag, bytes, call) RUNB_ON(st, tag, bytes, call)
#define RUN(cls, flops, call) RUN_ON(st, cls, flops, call)

static GemmParams gp_linear_geom() {
  GemmParams g;
  memset(&g, 0, sizeof(g));
  g.g_SH = g.g_SW = g.g_OH = g.g_OW = 1;
  g.g_KH = g.g_KW = 1; g.g_stride = 1; g.g_pad = 0;
  return g;
}

// scratch for K split over workgroups (igemm.hip: partial tiles + finishing launch); one per stream
static void set_sk(mmvqa_engine* e, hipStream_t st, GemmParams& g) {
  static const bool off = getenv("MMVQA_NO_SK_WS") != nullptr;   // A/B switch: no K split of forward / data-gradient products
  if (off) return;
  const int which = (e->side && st == e->side) ? 1 : ((e->side2 && st == e->side2) ? 2 : 0);
  g.sk_ws = WS(e->sk_ws[which]);
  g.sk_ws_floats = (long long)SK_WS_FLOATS;
  g.sk_cnt = reinterpret_cast<unsigned int*>(WS(e->sk_cnt[which]));
  g.sk_cnt_n = SK_CNT_N;
}

struct EpiOpt {
  const float* R = nullptr; int r_ld = 0;
  const float* Mk = nullptr; int mk_ld = 0; const float* mk_s = nullptr; const float* mk_b = nullptr; int mk_mode = 0;
  BNRef* st1 = nullptr; const float* Z1 = nullptr;
  BNRef* st2 = nullptr; const float* Z2 = nullptr;
};

static void apply_epi(mmvqa_engine* e, GemmParams& g, const EpiOpt& o) {
  g.R = o.R; g.r_ld = o.r_ld;
  g.Mk = o.Mk; g.mk_ld = o.mk_ld; g.mk_s = o.mk_s; g.mk_b = o.mk_b; g.mk_mode = o.mk_mode;
  if (o.st1) {
    g.stat1 = stat_ptr(e, o.st1->stat_b); g.stat_bwd = 1; g.stat_slots = o.st1->slots;
    g.Z1 = o.Z1; g.z1_ld = o.st1->C; g.mean1 = WS(o.st1->mean); g.invstd1 = WS(o.st1->invstd);
  }
  if (o.st2) {
    g.stat2 = stat_ptr(e, o.st2->stat_b);
    g.Z2 = o.Z2; g.z2_ld = o.st2->C; g.mean2 = WS(o.st2->mean); g.invstd2 = WS(o.st2->invstd);
  }
}

// y[M,out] = act(x[M,in] W^T + b) (+dropout) (+R)
static int lin_fwd(mmvqa_engine* e, hipStream_t st, const float* x, int x_ld, long M, const LinRef& L, float* y,
                   int y_ld, int act, float* pre, float drop_p, uint32_t seed, const float* R, int r_ld) {
  GemmParams g = gp_linear_geom();
  g.M = (int)M; g.N = L.out; g.K = L.in;
  g.A = x; g.a_ld = x_ld; g.g_Cs = L.in;
  g.B = PRM(L.w); g.b_ld = L.in;
  g.C = y; g.c_ld = y_ld; g.Cpre = pre;
  g.bias = L.b >= 0 ? PRM(L.b) : nullptr;
  g.act = act; g.drop_p = drop_p; g.drop_seed = seed; g.R = R; g.r_ld = r_ld;
  set_sk(e, st, g);
  RUN(PROF_IGEMM, 2.0 * M * L.out * L.in, mmvqa_launch_igemm(g, KIND_FWD, 0, 0, st));
  return MMVQA_OK;
}

// dx[M,in] = dy[M,out] W  (optionally * act'(Pre), + R, column sums for the upstream bias)
static int lin_dgrad(mmvqa_engine* e, hipStream_t st, const float* dy, int dy_ld, long M, const LinRef& L, float* dx,
                     int dx_ld, int dact, const float* Pre, int pre_ld, float* colsum, const float* R, int r_ld) {
  GemmParams g = gp_linear_geom();
  g.M = (int)M; g.N = L.in; g.K = L.out;
  g.A = dy; g.a_ld = dy_ld; g.g_Cs = L.out;
  g.B = PRM(L.w); g.b_ld = L.in; g.b_tapstride = 0;
  g.C = dx; g.c_ld = dx_ld;
  g.dact = dact; g.Pre = Pre; g.pre_ld = pre_ld; g.colsum = colsum; g.R = R; g.r_ld = r_ld;
  // Few output tiles and a long contraction (the vocabulary-sized decoder: 96 tiles x 477 K-tiles): split K over
  // workgroups and accumulate with atomics into the zeroed output.  Only for a plain epilogue.
  const long tiles = ((M + 63) / 64) * ((L.in + 63) / 64);
  // (the vocabulary-sized contraction, L.out = 30522, is faster through the scratch + finishing launch that set_sk
  // enables below: heads 0.94 -> 0.90 ms per step; the QKV-sized one, 2304, is faster this way: 0.37 vs 0.40 ms)
  if (!dact && !colsum && !R && tiles < 256 && L.out >= 1536 && L.out <= 8192 && dx_ld == L.in) {
    int sk = (int)((512 + tiles - 1) / tiles);
    const int maxs = (L.out / 64) / 8;
    if (sk > maxs) sk = maxs;
    if (sk > 1) {
      HIP_CHECK_RET(hipMemsetAsync(dx, 0, sizeof(float) * (size_t)M * dx_ld, st));
      g.c_atomic = 1; g.splitk = sk;
    }
  }
  set_sk(e, st, g);
  RUN(PROF_IGEMM, 2.0 * M * L.out * L.in, mmvqa_launch_igemm(g, KIND_DGRAD, 0, 0, st));
  return MMVQA_OK;
}

// dW[out,in] += dy^T x ; db[out] += colsum(dy)
static int lin_wgrad(mmvqa_engine* e, hipStream_t st, const float* dy, int dy_ld, const float* x, int x_ld, long M,
                     const LinRef& L, bool bias_from_colsum) {
  GemmParams g = gp_linear_geom();
  g.M = L.out; g.N = L.in; g.K = (int)M;
  g.A = dy; g.a_ld = dy_ld;
  g.B = x; g.b_ld = x_ld; g.g_Cs = L.in;
  g.C = GRD(L.w); g.c_ld = L.in; g.c_atomic = 1;
  RUN(PROF_IGEMM, 2.0 * M * L.out * L.in, mmvqa_launch_igemm(g, KIND_WGRAD, 0, 0, st));
  if (bias_from_colsum && L.b >= 0) RUN(PROF_OTHER, 0, mmvqa_colsum(st, dy, dy_ld, (int)M, L.out, GRD(L.b)));
  return MMVQA_OK;
}

static int ln_fwd(mmvqa_engine* e, hipStream_t st, const float* x, const LNRef& ln, float* y, float* mean,
                  float* rstd, long rows, float eps) {
  RUNB(HB_LAYERNORM_FWD, 8.0 * rows * e->d.hidden, mmvqa_layernorm_fwd(st, x, nullptr, PRM(ln.g), PRM(ln.b), y, nullptr, mean, rstd, (int)rows,
                                     e->d.hidden, eps));
  return MMVQA_OK;
}
static int ln_bwd(mmvqa_engine* e, hipStream_t st, const float* dy, const float* x, const LNRef& ln,
                  const float* mean, const float* rstd, const float* dres, float* dx, long rows, bool data_only = false) {
  // data_only (mmvqa_engine_backward_feature): the gradient with respect to x alone, dgamma / dbeta are not accumulated
  RUNB(HB_LAYERNORM_BWD, (dres ? 16.0 : 12.0) * rows * e->d.hidden, mmvqa_layernorm_bwd(st, dy, x, PRM(ln.g), mean, rstd, dres, dx,
                                     data_only ? nullptr : GRD(ln.g), data_only ? nullptr : GRD(ln.b), (int)rows,
                                     e->d.hidden));
  return MMVQA_OK;
}

// --------------------------------------------------------------------------- convolution helpers
// the tensor the gather reads (SH x SW pixels of Cs channels) and the grid of positions the product's rows walk
static void conv_geom(GemmParams& g, const ConvRef& c, int SH, int SW, int Cs, int OH, int OW) {
  g.g_SH = SH; g.g_SW = SW; g.g_Cs = Cs; g.g_OH = OH; g.g_OW = OW;
  g.g_KH = g.g_KW = c.KH; g.g_stride = c.stride; g.g_pad = c.pad;
}

static int bn_coef_fwd(mmvqa_engine* e, hipStream_t st, BNRef& bn) {
  REG(REG_BNCOEF);
  RUN(PROF_OTHER, 0,
      mmvqa_bn_coef_fwd(st, stat_ptr(e, bn.stat_f), bn.C, bn.count, bn.eps, PRM(bn.gamma), PRM(bn.beta),
                    e->bufs + bn.rmean, e->bufs + bn.rvar, e->nbt + bn.nbt, 0.1f, bn.reps, e->bn_training,
                    WS(bn.scale), WS(bn.shift), WS(bn.mean), WS(bn.invstd)));
  return MMVQA_OK;
}
static int bn_coef_bwd(mmvqa_engine* e, hipStream_t st, BNRef& bn) {
  REG(REG_BNCOEF);
  RUN(PROF_OTHER, 0,
      mmvqa_bn_coef_bwd(st, stat_ptr(e, bn.stat_b), bn.C, bn.count, PRM(bn.gamma), WS(bn.mean), WS(bn.invstd),
                    e->bn_training, WS(bn.P), WS(bn.Q), WS(bn.R), GRD(bn.gamma), GRD(bn.beta)));
  return MMVQA_OK;
}

// The ResNet path in training mode folds the BatchNorm coefficients inside the launches that consume them
// (mmvqa_bn_fold: no coefficient launch between a convolution and its consumer on the dependency chain).
static inline bool folding(const mmvqa_engine* e) { return e->bn_fold && e->bn_training && e->d.cnn == 0; }
// The EfficientNet path folds where the FIRST consumer of a BatchNorm is an elementwise kernel (block end, depthwise
// convolution, squeeze-excite pooling: forward) -- later consumers read what that launch published.
static inline bool eff_folding(const mmvqa_engine* e) { return e->bn_fold && e->bn_training && e->d.cnn != 0; }

static void set_fold_fwd(mmvqa_engine* e, mmvqa_bn_fold& f, BNRef& bn) {
  memset(&f, 0, sizeof(f));
  f.stat = stat_ptr(e, bn.stat_f); f.slots = bn.slots; f.bwd = 0; f.publish = 1; f.reps = bn.reps;
  f.count = bn.count; f.keep = pow(1.0 - (double)0.1f, (double)bn.reps); f.eps = bn.eps;
  f.gamma = PRM(bn.gamma); f.beta = PRM(bn.beta);
  f.out0 = WS(bn.scale); f.out1 = WS(bn.shift); f.out2 = WS(bn.mean); f.out3 = WS(bn.invstd);
  f.run_mean = e->bufs + bn.rmean; f.run_var = e->bufs + bn.rvar; f.nbt = e->nbt + bn.nbt;
}
static void set_fold_bwd(mmvqa_engine* e, mmvqa_bn_fold& f, const BNRef& bn, bool publish) {
  memset(&f, 0, sizeof(f));
  f.stat = stat_ptr(e, bn.stat_b); f.slots = bn.slots; f.bwd = 1; f.publish = publish ? 1 : 0; f.reps = bn.reps;
  f.count = bn.count; f.keep = 1.0; f.eps = bn.eps;
  f.gamma = PRM(bn.gamma); f.mean = WS(bn.mean); f.invstd = WS(bn.invstd);
  f.out0 = WS(bn.P); f.out1 = WS(bn.Q); f.out2 = WS(bn.R);
  f.dgamma = GRD(bn.gamma); f.dbeta = GRD(bn.beta);
}

// Input side of a convolution product: x as stored (no BatchNorm), or act(bn(x)) [* squeeze-excite gate] applied on load.
// The ResNet path passes PRO_AFFINE_RELU, the EfficientNet path PRO_AFFINE_SILU, or PRO_SILU_GATE with the gate.
struct ConvIn {
  const BNRef* bn = nullptr;
  int pro = 0;
  const float* gate = nullptr;
  int gate_hw(int OH, int OW) const { return bn && pro != PRO_AFFINE_RELU ? OH * OW : 0; }   // (the SiLU loaders decode the image of a row)
};

// z = conv(x) with x as `in` describes it; accumulates the batch statistics of z.  !coef: the consumer of bn_out folds its
// coefficients itself (under folding(e) every consumer does: next convolution / block end)
static int conv_fwd(mmvqa_engine* e, hipStream_t st, const ConvRef& c, const float* x, const ConvIn& in, int N,
                    int H, int W, int OH, int OW, float* z, BNRef& bn_out, bool coef = true) {
  GemmParams g;
  memset(&g, 0, sizeof(g));
  g.M = N * OH * OW; g.N = c.Cout; g.K = c.KH * c.KH * c.Cin;
  g.A = x; g.a_ld = c.Cin;
  if (in.bn) {
    g.a_pro = in.pro; g.a_c0 = WS(in.bn->scale); g.a_c1 = WS(in.bn->shift);
    g.gate = in.gate; g.gate_hw = in.gate_hw(OH, OW);
    if (folding(e)) set_fold_fwd(e, g.a_fold, *const_cast<BNRef*>(in.bn));   // this launch is in.bn's first consumer
  }
  conv_geom(g, c, H, W, c.Cin, OH, OW);
  g.B = PRM(c.w); g.b_ld = g.K;
  g.C = z; g.c_ld = c.Cout;
  if (e->bn_training) { g.stat1 = stat_ptr(e, bn_out.stat_f); g.stat_bwd = 0; g.stat_slots = bn_out.slots; }
  set_sk(e, st, g);
  RUN(PROF_IGEMM, 2.0 * g.M * g.N * g.K, mmvqa_launch_igemm(g, KIND_FWD, 0, 0, st));
  return folding(e) || !coef ? MMVQA_OK : bn_coef_fwd(e, st, bn_out);
}

// dW += dz^T * x_gathered with dz = P*G + Q*z + R (BatchNorm backward of bn_out), x as `in` describes it
static int conv_wgrad(mmvqa_engine* e, hipStream_t st, const ConvRef& c, const float* G, const float* z,
                      const BNRef& bn_out, const float* x, const ConvIn& in, int N, int H, int W, int OH, int OW) {
  GemmParams g;
  memset(&g, 0, sizeof(g));
  g.M = c.Cout; g.N = c.KH * c.KH * c.Cin; g.K = N * OH * OW;
  g.A = G; g.A2 = z; g.a_ld = c.Cout; g.a_pro = PRO_DZ;
  g.a_c0 = WS(bn_out.P); g.a_c1 = WS(bn_out.Q); g.a_c2 = WS(bn_out.R);
  if (folding(e)) set_fold_bwd(e, g.a_fold, bn_out, false);   // (the data gradient of the same BatchNorm publishes)
  g.B = x; g.b_ld = c.Cin;
  if (in.bn) {
    g.b_pro = in.pro; g.b_c0 = WS(in.bn->scale); g.b_c1 = WS(in.bn->shift);
    g.gate = in.gate; g.gate_hw = in.gate_hw(OH, OW);
  }
  conv_geom(g, c, H, W, c.Cin, OH, OW);
  g.C = GRD(c.w); g.c_ld = g.N; g.c_atomic = 1;
  if (c.KH > 1 && c.stride == 1 && OH == H && OW == W) {
    // stride-1 "same" convolution: hand the kernel the per-pixel tap-validity table (one per geometry)
    char key[96];
    snprintf(key, sizeof(key), "%d,%d,%d,%d,%d", N, OH, OW, c.KH, c.pad);
    auto it = e->pixmask_off.find(key);
    if (it != e->pixmask_off.end()) g.pixmask = reinterpret_cast<int*>(WS(it->second.off));   // built by prepare_workspace()
  }
  RUN(PROF_IGEMM, 2.0 * (double)g.M * g.N * g.K, mmvqa_launch_igemm(g, KIND_WGRAD, 0, 0, st));
  return MMVQA_OK;
}

// dx[N,H,W,Cin] = conv_transpose(dz, W) with dz as above; epilogue options in `o`
static int conv_dgrad(mmvqa_engine* e, hipStream_t st, const ConvRef& c, const float* G, const float* z,
                      const BNRef& bn_out, int N, int H, int W, int OH, int OW, float* dx, const EpiOpt& o) {
  GemmParams g;
  memset(&g, 0, sizeof(g));
  g.M = N * H * W; g.N = c.Cin; g.K = c.KH * c.KH * c.Cout;
  g.A = G; g.A2 = z; g.a_ld = c.Cout; g.a_pro = PRO_DZ;
  g.a_c0 = WS(bn_out.P); g.a_c1 = WS(bn_out.Q); g.a_c2 = WS(bn_out.R);
  if (folding(e)) set_fold_bwd(e, g.a_fold, bn_out, true);
  conv_geom(g, c, OH, OW, c.Cout, H, W);   // gathers dz, one row per input pixel
  g.B = PRM(c.w); g.b_ld = c.KH * c.KH * c.Cin; g.b_tapstride = c.Cin;
  g.C = dx; g.c_ld = c.Cin;
  apply_epi(e, g, o);
  set_sk(e, st, g);
  RUN(PROF_IGEMM, 2.0 * (double)N * OH * OW * c.Cout * c.KH * c.KH * c.Cin,
      mmvqa_launch_igemm(g, KIND_DGRAD, 0, 0, st));
  return MMVQA_OK;
}

// The stem convolution of either backbone, gathered from the NCHW image.  KIND_FWD: z0 = conv(img) and the statistics of z0.
// KIND_WGRAD: dW += dz^T img, dz from g0 and z0 through the stem BatchNorm's backward coefficients.
static GemmParams stem_desc(mmvqa_engine* e, int kind, const float* g0 = nullptr) {
  const ConvRef& c = e->stem_conv;
  const int pixels = e->NI * e->SH * e->SW, taps = c.KH * c.KH * c.Cin;
  GemmParams g;
  memset(&g, 0, sizeof(g));
  g.g_nchw = 1;
  conv_geom(g, c, e->IH, e->IW, c.Cin, e->SH, e->SW);
  if (kind == KIND_FWD) {
    g.M = pixels; g.N = c.Cout; g.K = taps;
    g.A = e->img;
    g.B = PRM(c.w); g.b_ld = taps;
    g.C = WS(e->z0); g.c_ld = c.Cout;
    if (e->bn_training) g.stat1 = stat_ptr(e, e->stem_bn.stat_f);
  } else {
    g.M = c.Cout; g.N = taps; g.K = pixels;
    g.A = g0; g.A2 = WS(e->z0); g.a_ld = c.Cout; g.a_pro = PRO_DZ;
    g.a_c0 = WS(e->stem_bn.P); g.a_c1 = WS(e->stem_bn.Q); g.a_c2 = WS(e->stem_bn.R);
    g.B = e->img;
    g.C = GRD(c.w); g.c_ld = taps; g.c_atomic = 1;
  }
  return g;
}

// --------------------------------------------------------------------------- taps (models/image_encoding.py:53-62,72-86)
static int tap_act(const mmvqa_engine* e) { return e->d.use_relu ? ACT_RELU : ACT_SERF; }

// a tap with few channels on a huge map (EfficientNet's stem tap): weights stay in registers, no tile machinery (tapthin.hip)
// (C = 64 with BatchNorm+ReLU on load needs 256 VGPRs there and only ties the GEMM kernel: measured, round 2)
// (fp32 operands: not in the f16 mode, whose contract rounds every tap product's operands -- the implicit GEMM)
static bool tap_is_thin(const mmvqa_engine* e, const TapRef& t) {
  static const bool thin_off = getenv("MMVQA_NO_TAP_THIN") != nullptr;   // A/B switch
  return !thin_off && e->prec == MMVQA_PREC_F32 && t.C <= 32 && mmvqa_tap_thin_ok(t.M, e->d.hidden, t.C, t.HW);
}

// u = act(fmap W_tap^T), consumed by the epilogue: EPI_TAP_FWD pools it into the visual token, EPI_TAP_BWD turns it into du.
// The caller sets the epilogue's pointers and C.
static GemmParams tap_desc(mmvqa_engine* e, hipStream_t st, const TapRef& t, const float* fmap, const BNRef* bn_in, int epi_mode) {
  GemmParams g = gp_linear_geom();
  g.M = (int)t.M; g.N = e->d.hidden; g.K = t.C;
  g.A = fmap; g.a_ld = t.C; g.g_Cs = t.C;
  if (bn_in) { g.a_pro = PRO_AFFINE_RELU; g.a_c0 = WS(bn_in->scale); g.a_c1 = WS(bn_in->shift); }
  g.B = PRM(t.w); g.b_ld = t.C;
  g.epi_mode = epi_mode; g.act = tap_act(e); g.tap_HW = t.HW;
  g.c_ld = g.N;
  set_sk(e, st, g);
  return g;
}

static int tap_fwd(mmvqa_engine* e, hipStream_t st, int k, const float* fmap, const BNRef* bn_in) {
  REG(REG_TAP);
  const TapRef& t = e->taps[k];
  float* vis = WS(e->vis) + (size_t)k * e->NI * e->d.hidden;
  if (tap_is_thin(e, t)) {
    TRY(prof_begin(e, st, PROF_MATRIX, 2.0 * (double)t.M * e->d.hidden * t.C, HB_TAP_THIN_FWD, 4.0 * (double)t.M * t.C));
    TRY(mmvqa_tap_thin_fwd(st, fmap, bn_in ? WS(bn_in->scale) : nullptr, bn_in ? WS(bn_in->shift) : nullptr,
                                      PRM(t.w), vis, t.M, e->d.hidden, t.C, t.HW, tap_act(e)));
    TRY(prof_end(e, st));
    return MMVQA_OK;
  }
  GemmParams g = tap_desc(e, st, t, fmap, bn_in, EPI_TAP_FWD);
  g.tap_out = vis;
  g.C = vis;  // unused by this epilogue
  RUN(PROF_IGEMM, 2.0 * (double)g.M * g.N * g.K, mmvqa_launch_igemm(g, KIND_FWD, 0, 0, st));
  return MMVQA_OK;
}

// backward of one tap: du (recompute), dW_tap, and the gradient wrt the feature map (T_k or masked G)
// (data_only: the recompute and the data gradient, no weight gradient -- mmvqa_engine_backward_feature;
//  weight_only, its mirror: the recompute and dW_tap, no data gradient and dfmap unused -- the frozen backbone)
static int tap_bwd(mmvqa_engine* e, hipStream_t st, int k, const float* fmap, const BNRef* bn_in, float* dfmap,
                   const EpiOpt& o, bool data_only = false, bool weight_only = false) {
  REG(REG_TAP);
  const TapRef& t = e->taps[k];
  const int Hd = e->d.hidden;
  const float* dv = WS(e->dvis) + (size_t)k * e->NI * Hd;
  if (tap_is_thin(e, t)) {
    TRY(prof_begin(e, st, PROF_MATRIX, 2.0 * (double)t.M * Hd * t.C, HB_TAP_THIN_BWD, 4.0 * (double)t.M * (t.C + Hd)));
    TRY(mmvqa_tap_thin_bwd(st, fmap, bn_in ? WS(bn_in->scale) : nullptr, bn_in ? WS(bn_in->shift) : nullptr,
                       PRM(t.w), dv, WS(e->du), t.M, Hd, t.C, t.HW, tap_act(e)));
    TRY(prof_end(e, st));
  } else {
    GemmParams g = tap_desc(e, st, t, fmap, bn_in, EPI_TAP_BWD);
    g.tap_dv = dv;
    g.C = WS(e->du);
    RUN(PROF_IGEMM, 2.0 * (double)g.M * g.N * g.K, mmvqa_launch_igemm(g, KIND_FWD, 0, 0, st));
  }
  if (!data_only) {
  // dW_tap[Hd][C] += du^T fmap
  GemmParams w = gp_linear_geom();
  w.M = Hd; w.N = t.C; w.K = (int)t.M;
  w.A = WS(e->du); w.a_ld = Hd;
  w.B = fmap; w.b_ld = t.C; w.g_Cs = t.C;
  if (bn_in) { w.b_pro = PRO_AFFINE_RELU; w.b_c0 = WS(bn_in->scale); w.b_c1 = WS(bn_in->shift); }
  w.C = GRD(t.w); w.c_ld = t.C; w.c_atomic = 1;
  RUN(PROF_IGEMM, 2.0 * (double)w.M * w.N * w.K, mmvqa_launch_igemm(w, KIND_WGRAD, 0, 0, st));
  }
  if (weight_only) return MMVQA_OK;
  // dfmap[M][C] = du W_tap
  GemmParams dg = gp_linear_geom();
  dg.M = (int)t.M; dg.N = t.C; dg.K = Hd;
  dg.A = WS(e->du); dg.a_ld = Hd; dg.g_Cs = Hd;
  dg.B = PRM(t.w); dg.b_ld = t.C;
  dg.C = dfmap; dg.c_ld = t.C;
  apply_epi(e, dg, o);
  set_sk(e, st, dg);
  RUN(PROF_IGEMM, 2.0 * (double)dg.M * dg.N * dg.K, mmvqa_launch_igemm(dg, KIND_DGRAD, 0, 0, st));
  return MMVQA_OK;
}

// --------------------------------------------------------------------------- side stream (backward overlap)
// Test-only lag injection (tests/test_hip_schedule.py): MMVQA_SIDE_LAG_US=n enqueues an n-microsecond spin on the side /
// tap stream right behind every fork, MMVQA_MAIN_LAG_US=n on the caller's stream right after the fork's event.  A missing
// need() / SideReads::write() / join then loses its race every time instead of now and then.  Read once, clamped to
// [0, 2000]; unset (the default) enqueues nothing.
static int lag_us(const char* name) {
  const char* v = getenv(name);
  if (!v) return 0;
  const int n = atoi(v);
  return n < 0 ? 0 : (n > 2000 ? 2000 : n);
}
// The data-gradient chain (dgrad -> BN coefficients -> dgrad ...) is the critical path of the backward pass
// and, on the 14x14 / 7x7 layers, fills well under one workgroup per CU; the weight-gradient GEMMs and
// the tap backward only feed the optimizer, so they run on a second HIP stream and fill the idle CUs.
// Ordering is by events: fork() makes the side stream wait for everything enqueued so far on the main
// stream, mark() hands out an event for the side work enqueued so far, need() makes the main stream wait
// for such an event before it overwrites a buffer the side work reads.
struct SideCtx {
  mmvqa_engine* e;
  hipStream_t st, sd;
  bool on;
  // the side streams carry work with slack (weight gradients, taps, downsample branches): lowest priority, so that the
  // dependency chain on the caller's stream is dispatched first whenever both have kernels ready.  A stream that cannot
  // be made is no ordering loss: its work goes where it went without it.
  static bool make_stream(hipStream_t* s, bool low_prio) {
    int least = 0, greatest = 0;
    const hipError_t r = low_prio && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest
                             ? hipStreamCreateWithPriority(s, hipStreamNonBlocking, least)
                             : hipStreamCreateWithFlags(s, hipStreamNonBlocking);
    if (r != hipSuccess) *s = nullptr;
    return r == hipSuccess;
  }
  SideCtx(mmvqa_engine* e_, hipStream_t st_, bool allow = true) : e(e_), st(st_) {
    on = allow && e->use_side && !e->tuner.tuning;   // (the per-launch profiler records its events on the launching stream)
    static const bool prio_off = getenv("MMVQA_SIDE_PRIO_OFF") != nullptr;   // A/B switch (this stream only)
    if (on && !e->side) on = make_stream(&e->side, !prio_off);
    sd = on ? e->side : st;
  }
  // third stream for the tap backward: four long launch groups (2.4 ms per config-2 step) that are needed only when the
  // chain reaches their layer; queued on `sd` they sat in front of the first weight gradients, whose completion the chain
  // waits for before it reuses a gradient buffer.  MMVQA_TAP_STREAM_OFF=1 puts them back on `sd` (A/B switch): 24.46 ms
  // against 24.15 ms per config-2 step.  (More launches share the chip this way and each launch's own duration stretches:
  // the bench line's per-launch figure `roofline.frac` reads lower on the faster step; `roofline.step_level` and
  // `roofline.single_stream` do not have that blind spot.  DESIGN 7.5.)
  hipStream_t tap_stream() {
    static const bool want = getenv("MMVQA_TAP_STREAM_OFF") == nullptr;
    if (!on || !want) return sd;
    if (!e->side2 && !make_stream(&e->side2, true)) return sd;
    return e->side2;
  }
  // Every edge returns a status: a HIP call that fails ends the step with an error instead of dropping the ordering.
  int fork_to(hipStream_t s) {   // s starts behind everything queued on the caller's stream so far
    if (!on || s == st) return MMVQA_OK;
    hipEvent_t ev;
    TRY(next_event(&ev));
    HIP_CHECK_RET(hipEventRecord(ev, st));
    TRY(lag(st, false));
    HIP_CHECK_RET(hipStreamWaitEvent(s, ev, 0));
    return lag(s, true);
  }
  int fork() { return fork_to(sd); }
  static int lag(hipStream_t s, bool side) {   // (test-only, see lag_us)
    static const int side_us = lag_us("MMVQA_SIDE_LAG_US"), main_us = lag_us("MMVQA_MAIN_LAG_US");
    const int us = side ? side_us : main_us;
    return us > 0 ? k_spin(s, us) : MMVQA_OK;
  }
  int mark_on(hipStream_t s, hipEvent_t* ev) {   // *ev: the work queued on s so far (null without a side stream)
    *ev = nullptr;
    if (!on) return MMVQA_OK;
    TRY(next_event(ev));
    HIP_CHECK_RET(hipEventRecord(*ev, s));
    return MMVQA_OK;
  }
  int mark(hipEvent_t* ev) { return mark_on(sd, ev); }
  int next_event(hipEvent_t* ev) {
    if (e->ev_next == e->ev_pool.size()) {
      HIP_CHECK_RET(hipEventCreateWithFlags(ev, hipEventDisableTiming));
      e->ev_pool.push_back(*ev);
    }
    *ev = e->ev_pool[e->ev_next++];
    return MMVQA_OK;
  }
  int need(hipEvent_t ev) {
    if (on && ev) HIP_CHECK_RET(hipStreamWaitEvent(st, ev, 0));
    return MMVQA_OK;
  }
  int join() {   // the caller's stream waits for everything queued on the side stream so far
    hipEvent_t ev;
    TRY(mark(&ev));
    return need(ev);
  }
};

// Weight gradients of the linear layers (heads, encoder) on the side stream: the 512-row products of the encoder fill
// 96-384 of 256 CUs x 2 slots, so a weight gradient beside the data gradient it shares its input with is nearly free.
// SideReads remembers, per scratch buffer, the event of the last side launch that READS it; the chain calls write(ptr)
// before it overwrites that buffer.  MMVQA_ENC_SIDE_OFF=1: everything on the caller's stream (A/B switch).
struct SideReads {
  SideCtx& sc;
  bool on;
  std::vector<std::pair<const void*, hipEvent_t>> rd;
  bool data_only;   // data gradients only (mmvqa_engine_backward_feature): no weight / bias / LayerNorm-parameter gradient
  explicit SideReads(SideCtx& s, bool data_only_ = false) : sc(s), data_only(data_only_) {
    static const bool off = getenv("MMVQA_ENC_SIDE_OFF") != nullptr;
    on = sc.on && !off && !data_only;
  }
  float* bias_grad(float* g) const { return data_only ? nullptr : g; }
  int read(const void* p) {
    hipEvent_t ev;
    TRY(sc.mark(&ev));
    for (auto& kv : rd) if (kv.first == p) { kv.second = ev; return MMVQA_OK; }
    rd.emplace_back(p, ev);
    return MMVQA_OK;
  }
  int write(const void* p) {
    for (auto& kv : rd) if (kv.first == p && kv.second) { TRY(sc.need(kv.second)); kv.second = nullptr; }
    return MMVQA_OK;
  }
  int join() { return on ? sc.join() : MMVQA_OK; }
};
// dW += dy^T x (+ bias gradient) beside the chain: starts behind everything queued on the caller's stream so far
static int lin_wgrad_side(mmvqa_engine* e, SideReads& sr, hipStream_t st, const float* dy, int dy_ld, const float* x, int x_ld, long M,
                          const LinRef& L, bool bias_from_colsum) {
  if (sr.data_only) return MMVQA_OK;
  if (!sr.on) return lin_wgrad(e, st, dy, dy_ld, x, x_ld, M, L, bias_from_colsum);
  TRY(sr.sc.fork());
  TRY(lin_wgrad(e, sr.sc.sd, dy, dy_ld, x, x_ld, M, L, bias_from_colsum));
  return sr.read(dy);
}

static int notify(mmvqa_engine* e, SideCtx& sc, long long lo, long long hi) {
  if (!e->grad_cb || hi <= lo) return MMVQA_OK;
  TRY(sc.join());   // weight gradients of the range may still be queued on the side stream
  e->grad_cb(e->grad_cb_user, lo, hi);
  return MMVQA_OK;
}

// --------------------------------------------------------------------------- ResNet forward / backward
static int resnet_forward(mmvqa_engine* e, hipStream_t st) {
  const mmvqa_model_desc& d = e->d;
  const int B = e->NI, w = d.resnet_width;   // the backbone's batch: the images
  if (e->bn_training)
    HIP_CHECK_RET(hipMemsetAsync(stat_ptr(e, 0), 0, e->statzone_floats / 2 * sizeof(float), st));
  HIP_CHECK_RET(hipMemsetAsync(WS(e->vis), 0, (size_t)5 * B * d.hidden * sizeof(float), st));
  {  // stem 7x7/2 on the NCHW image
    const GemmParams g = stem_desc(e, KIND_FWD);
    RUN(PROF_IGEMM, 2.0 * (double)g.M * g.N * g.K, mmvqa_launch_igemm(g, KIND_FWD, 1, 0, st));
    TRY(bn_coef_fwd(e, st, e->stem_bn));
  }
  // The five taps (1x1 conv -> act -> global average pool) and the downsample convolutions do not feed the
  // bottleneck chain: they run on the side stream beside it (most of the chain's launches fill 196 of 256 CUs).
  SideCtx sc(e, st);
  // A tap is queued on the side stream BEHIND the next block's downsample convolution (MMVQA_TAP_FIRST=1: in front of it, as
  // before round 3's last change): the block end of that block waits for the downsample branch, and a 0.1-0.6 ms tap in
  // front of it stalled the chain at every layer start (the stem tap alone is 634 us against 220 us of layer1.0's
  // three convolutions).
  static const bool tap_first = getenv("MMVQA_TAP_FIRST") != nullptr;
  int pend_tap = -1;
  const float* pend_x = nullptr;
  const BNRef* pend_bn = nullptr;
  if (tap_first) {
    TRY(sc.fork());
    TRY(tap_fwd(e, sc.sd, 4, WS(e->z0), &e->stem_bn));
  } else {
    pend_tap = 4; pend_x = WS(e->z0); pend_bn = &e->stem_bn;
  }
  RUNB(HB_MAXPOOL_FWD, 4.0 * B * e->SH * e->SW * w + 5.0 * B * e->PH * e->PW * w, mmvqa_maxpool_fwd(st, WS(e->z0), WS(e->stem_bn.scale), WS(e->stem_bn.shift), WS(e->p0),
                                   reinterpret_cast<unsigned char*>(WS(e->pool_idx)), B, e->SH, e->SW, w, e->PH,
                                   e->PW));
  const float* x = WS(e->p0);
  int layer = 0;
  for (size_t i = 0; i < e->blocks.size(); ++i) {
    BlockRef& b = e->blocks[i];
    hipEvent_t ev_ds = nullptr;
    if (b.has_ds) {
      TRY(sc.fork());
      TRY(conv_fwd(e, sc.sd, b.cd, x, {}, B, b.H, b.W, b.OH, b.OW, WS(b.zd), b.bd));
      TRY(sc.mark(&ev_ds));
    }
    if (pend_tap >= 0) {   // the tap on the previous layer's output (or the stem's), behind this block's downsample branch
      if (!b.has_ds) TRY(sc.fork());
      TRY(tap_fwd(e, sc.sd, pend_tap, pend_x, pend_bn));
      pend_tap = -1;
    }
    TRY(conv_fwd(e, st, b.c1, x, {}, B, b.H, b.W, b.H, b.W, WS(b.z1), b.b1));
    TRY(conv_fwd(e, st, b.c2, WS(b.z1), {&b.b1, PRO_AFFINE_RELU}, B, b.H, b.W, b.OH, b.OW, WS(b.z2), b.b2));
    TRY(conv_fwd(e, st, b.c3, WS(b.z2), {&b.b2, PRO_AFFINE_RELU}, B, b.OH, b.OW, b.OH, b.OW, WS(b.z3), b.b3));
    const long rows = (long)B * b.OH * b.OW;
    if (folding(e)) {
      mmvqa_bn_fold f3, fd;
      set_fold_fwd(e, f3, b.b3);
      if (b.has_ds) { TRY(sc.need(ev_ds)); set_fold_fwd(e, fd, b.bd); }
      RUNB(HB_BN_ADD_RELU, 12.0 * rows * b.c3.Cout, mmvqa_bn_add_relu_fold(st, WS(b.z3), &f3, b.has_ds ? WS(b.zd) : x, b.has_ds ? &fd : nullptr,
                                            WS(b.out), rows, b.c3.Cout));
    } else if (b.has_ds) {
      TRY(sc.need(ev_ds));
      RUNB(HB_BN_ADD_RELU, 12.0 * rows * b.c3.Cout, mmvqa_bn_add_relu(st, WS(b.z3), WS(b.b3.scale), WS(b.b3.shift), WS(b.zd), WS(b.bd.scale),
                                       WS(b.bd.shift), WS(b.out), rows, b.c3.Cout));
    } else {
      RUNB(HB_BN_ADD_RELU, 12.0 * rows * b.c3.Cout, mmvqa_bn_add_relu(st, WS(b.z3), WS(b.b3.scale), WS(b.b3.shift), x, nullptr, nullptr,
                                       WS(b.out), rows, b.c3.Cout));
    }
    x = WS(b.out);
    if ((int)i == e->layer_end[layer]) {
      if (tap_first) {
        TRY(sc.fork());
        TRY(tap_fwd(e, sc.sd, 3 - layer, x, nullptr));
      } else {
        pend_tap = 3 - layer; pend_x = x; pend_bn = nullptr;
      }
      ++layer;
    }
  }
  if (pend_tap >= 0) {   // the tap on the last layer's output
    TRY(sc.fork());
    TRY(tap_fwd(e, sc.sd, pend_tap, pend_x, pend_bn));
  }
  TRY(sc.join());   // join: the embedding reads the visual tokens
  return MMVQA_OK;
}

static int resnet_backward(mmvqa_engine* e, hipStream_t st) {
  const int B = e->NI, w = e->d.resnet_width;
  HIP_CHECK_RET(hipMemsetAsync(stat_ptr(e, 0) + e->statzone_floats / 4, 0,
                               e->statzone_floats / 2 * sizeof(float), st));
  SideCtx sc(e, st);
  hipStream_t sd = sc.sd;
  const int nb = (int)e->blocks.size();
  int cur = 0;
  {  // the layer4 tap starts the main chain
    BlockRef& last = e->blocks[nb - 1];
    EpiOpt o;
    o.Mk = WS(last.out); o.mk_ld = last.c3.Cout;
    o.st1 = &last.b3; o.Z1 = WS(last.z3);
    if (last.has_ds) { o.st2 = &last.bd; o.Z2 = WS(last.zd); }
    TRY(tap_bwd(e, st, 0, WS(last.out), nullptr, WS(e->gbuf[cur]), o));
  }
  // taps on layer1..3 and the stem produce side gradients T_k that are only needed when the chain reaches
  // their layer: side stream (they share the `du` scratch with the tap above, hence the fork after it)
  hipEvent_t ev_tap[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  hipStream_t ts = sc.tap_stream();
  TRY(sc.fork_to(ts));
  for (int k = 1; k <= 3; ++k) {
    const BlockRef& blk = e->blocks[e->layer_end[3 - k]];
    TRY(tap_bwd(e, ts, k, WS(blk.out), nullptr, WS(e->tapgrad[k]), EpiOpt()));
    TRY(sc.mark_on(ts, &ev_tap[k]));
  }
  TRY(tap_bwd(e, ts, 4, WS(e->z0), &e->stem_bn, WS(e->tapgrad[4]), EpiOpt()));
  TRY(sc.mark_on(ts, &ev_tap[4]));
  hipEvent_t ev_g1 = nullptr, ev_g2 = nullptr, ev_prevG = nullptr;   // side readers of g1buf / g2buf / previous G
  // gradients in [enc_lo, end) were announced by the caller; the tap weights sit in [taps[0].w, enc_lo) (fc below them).
  // Their gradients come from the tap stream, which notify() does not join: that range is announced after the stem,
  // whose chain waits for the last tap, and the block ranges end below it
  long long hi_mark = e->taps[0].w;
  for (int i = nb - 1; i >= 0; --i) {
    BlockRef& b = e->blocks[i];
    const float* G = WS(e->gbuf[cur]);
    const float* x = i == 0 ? WS(e->p0) : WS(e->blocks[i - 1].out);
    float* Gprev = WS(e->gbuf[cur ^ 1]);
    // side gradient arriving at this block's input from a tap (only where the previous block ends a layer)
    const float* extra = nullptr;
    hipEvent_t ev_extra = nullptr;
    for (int l = 0; l < 3; ++l)
      if (i - 1 == e->layer_end[l]) { extra = WS(e->tapgrad[3 - l]); ev_extra = ev_tap[3 - l]; }
    hipEvent_t evG = nullptr;   // side readers of this block's G
    // conv3 / bn3
    if (!folding(e)) TRY(bn_coef_bwd(e, st, b.b3));
    TRY(sc.fork());
    TRY(conv_wgrad(e, sd, b.c3, G, WS(b.z3), b.b3, WS(b.z2), {&b.b2, PRO_AFFINE_RELU}, B, b.OH, b.OW, b.OH, b.OW));
    TRY(sc.mark(&evG));
    {
      EpiOpt o;
      o.Mk = WS(b.z2); o.mk_ld = b.c2.Cout; o.mk_s = WS(b.b2.scale); o.mk_b = WS(b.b2.shift);
      o.st1 = &b.b2; o.Z1 = WS(b.z2);
      TRY(sc.need(ev_g2));
      TRY(conv_dgrad(e, st, b.c3, G, WS(b.z3), b.b3, B, b.OH, b.OW, b.OH, b.OW, WS(e->g2buf), o));
    }
    // conv2 / bn2
    if (!folding(e)) TRY(bn_coef_bwd(e, st, b.b2));
    TRY(sc.fork());
    TRY(conv_wgrad(e, sd, b.c2, WS(e->g2buf), WS(b.z2), b.b2, WS(b.z1), {&b.b1, PRO_AFFINE_RELU}, B, b.H, b.W, b.OH, b.OW));
    TRY(sc.mark(&ev_g2));
    {
      EpiOpt o;
      o.Mk = WS(b.z1); o.mk_ld = b.c1.Cout; o.mk_s = WS(b.b1.scale); o.mk_b = WS(b.b1.shift);
      o.st1 = &b.b1; o.Z1 = WS(b.z1);
      TRY(sc.need(ev_g1));
      TRY(conv_dgrad(e, st, b.c2, WS(e->g2buf), WS(b.z2), b.b2, B, b.H, b.W, b.OH, b.OW, WS(e->g1buf), o));
    }
    // conv1 / bn1
    if (!folding(e)) TRY(bn_coef_bwd(e, st, b.b1));
    TRY(sc.fork());
    TRY(conv_wgrad(e, sd, b.c1, WS(e->g1buf), WS(b.z1), b.b1, x, {}, B, b.H, b.W, b.H, b.W));
    TRY(sc.mark(&ev_g1));
    // gradient wrt the block input: conv1 path + identity/downsample path (+ tap side gradient)
    EpiOpt o;
    if (i > 0) {
      BlockRef& pb = e->blocks[i - 1];
      o.Mk = x; o.mk_ld = b.c1.Cin;
      o.st1 = &pb.b3; o.Z1 = WS(pb.z3);
      if (pb.has_ds) { o.st2 = &pb.bd; o.Z2 = WS(pb.zd); }
    }
    if (b.has_ds) {
      if (!folding(e)) TRY(bn_coef_bwd(e, st, b.bd));
      TRY(sc.fork());
      TRY(conv_wgrad(e, sd, b.cd, G, WS(b.zd), b.bd, x, {}, B, b.H, b.W, b.OH, b.OW));
      TRY(sc.mark(&evG));
      EpiOpt od;
      od.R = extra; od.r_ld = b.cd.Cin;
      TRY(sc.need(ev_extra));
      TRY(conv_dgrad(e, st, b.cd, G, WS(b.zd), b.bd, B, b.H, b.W, b.OH, b.OW, WS(e->dstmp), od));
      o.R = WS(e->dstmp); o.r_ld = b.c1.Cin;
    } else {
      if (extra) return mmvqa_set_error(MMVQA_ERR_STATE, "resnet_backward: tap gradient without downsample");
      o.R = G; o.r_ld = b.c1.Cin;
    }
    TRY(sc.need(ev_prevG));   // the buffer written next was the G of the block before: its side readers must be done
    TRY(conv_dgrad(e, st, b.c1, WS(e->g1buf), WS(b.z1), b.b1, B, b.H, b.W, b.H, b.W, Gprev, o));
    ev_prevG = evG;
    cur ^= 1;
    // announce finished gradient ranges every ~12 blocks and at layer starts (large, few all-reduces)
    bool layer_start = false;
    for (int l = 0; l < 3; ++l) layer_start |= (i - 1 == e->layer_end[l]);
    if (i > 0 && (layer_start || (nb - i) % 12 == 0)) { TRY(notify(e, sc, b.c1.w, hi_mark)); hi_mark = b.c1.w; }
  }
  // stem: max-pool backward + stem-tap gradient + ReLU mask + BN statistics, then the 7x7 weight gradient
  float* g0 = WS(e->gbuf[cur ^ 1]);
  TRY(sc.need(ev_prevG));
  TRY(sc.need(ev_tap[4]));
  RUNB(HB_MAXPOOL_BWD, 12.0 * B * e->SH * e->SW * w + 5.0 * B * e->PH * e->PW * w,
      mmvqa_maxpool_bwd(st, WS(e->gbuf[cur]), reinterpret_cast<unsigned char*>(WS(e->pool_idx)), WS(e->tapgrad[4]),
                    WS(e->z0), WS(e->stem_bn.scale), WS(e->stem_bn.shift), WS(e->stem_bn.mean),
                    WS(e->stem_bn.invstd), g0, stat_ptr(e, e->stem_bn.stat_b), B, e->SH, e->SW, w, e->PH, e->PW));
  TRY(bn_coef_bwd(e, st, e->stem_bn));
  const GemmParams g = stem_desc(e, KIND_WGRAD, g0);
  RUN(PROF_IGEMM, 2.0 * (double)g.M * g.N * g.K, mmvqa_launch_igemm(g, KIND_WGRAD, 1, 0, st));
  TRY(sc.join());   // join: everything after the backward (all-reduce, Adam) sees the side stream's gradients
  TRY(notify(e, sc, e->taps[0].w, e->enc_lo));   // tap weights: the caller's stream is behind ev_tap[4], the last tap launch
  TRY(notify(e, sc, e->emb_hi, hi_mark));
  return MMVQA_OK;
}

// Backward of a frozen backbone (MMVQA_FREEZE_BACKBONE): nothing below the taps receives a gradient, so no gradient has to
// reach a feature map.  What is left is the weight gradient of the five taps, from the feature maps the forward kept.
// The taps share the `du` scratch, so they run one after the other, and there is nothing to run beside them: all on the
// caller's stream, no side stream to join before the announcements.
static int frozen_backbone_backward(mmvqa_engine* e, hipStream_t st) {
  if (e->d.cnn == 1) {
    for (auto& b : e->eff)
      if (b.feature >= 0) TRY(tap_bwd(e, st, b.feature, WS(b.out), nullptr, nullptr, EpiOpt(), false, true));
  } else {
    TRY(tap_bwd(e, st, 0, WS(e->blocks.back().out), nullptr, nullptr, EpiOpt(), false, true));
    for (int k = 1; k <= 3; ++k)
      TRY(tap_bwd(e, st, k, WS(e->blocks[e->layer_end[3 - k]].out), nullptr, nullptr, EpiOpt(), false, true));
    TRY(tap_bwd(e, st, 4, WS(e->z0), &e->stem_bn, nullptr, EpiOpt(), false, true));
  }
  if (e->grad_cb) {
    e->grad_cb(e->grad_cb_user, e->taps[0].w, e->enc_lo);   // tap weights
    e->grad_cb(e->grad_cb_user, e->emb_hi, e->taps[0].w);   // the frozen range, as it stands: this backward wrote none of it
  }
  return MMVQA_OK;
}

// --------------------------------------------------------------------------- EfficientNetV2 forward / backward
static int effnet_forward(mmvqa_engine* e, hipStream_t st) {
  const mmvqa_model_desc& d = e->d;
  const int B = e->NI;
  if (e->bn_training)
    HIP_CHECK_RET(hipMemsetAsync(stat_ptr(e, 0), 0, e->statzone_floats / 2 * sizeof(float), st));
  HIP_CHECK_RET(hipMemsetAsync(WS(e->vis), 0, (size_t)5 * B * d.hidden * sizeof(float), st));
  const long M0 = (long)B * e->SH * e->SW;
  const bool fold = eff_folding(e);
  // out = act(bn(z)) + idn: with folding, this launch derives bn's coefficients from the raw sums and publishes them
  auto block_end = [&](BNRef& bn, const float* z, int act, const float* idn, float* out, long rows, int C, bool have_coef) -> int {
    if (fold && !have_coef) {
      mmvqa_bn_fold f;
      set_fold_fwd(e, f, bn);
      RUNB(HB_BN_ACT_ADD, (idn ? 12.0 : 8.0) * rows * C, mmvqa_bn_act_add_fold(st, z, &f, act, idn, nullptr, ACT_NONE, out, rows, C));
    } else {
      if (!have_coef) TRY(bn_coef_fwd(e, st, bn));
      RUNB(HB_BN_ACT_ADD, (idn ? 12.0 : 8.0) * rows * C, mmvqa_bn_act_add(st, z, WS(bn.scale), WS(bn.shift), act, idn, nullptr, nullptr, 0,
                                      ACT_NONE, out, rows, C));
    }
    return MMVQA_OK;
  };
  {  // conv_stem 3x3/2 SAME on the NCHW image
    const GemmParams g = stem_desc(e, KIND_FWD);
    RUN(PROF_IGEMM, 2.0 * (double)g.M * g.N * g.K, mmvqa_launch_igemm(g, KIND_FWD, 1, 0, st));
    TRY(block_end(e->stem_bn, WS(e->z0), ACT_SILU, nullptr, WS(e->eff_a0), M0, g.N, false));
  }
  const float* x = WS(e->eff_a0);
  SideCtx sc(e, st);
  for (auto& b : e->eff) {
    const long Mout = (long)B * b.OH * b.OW;
    const float* idn = b.skip ? x : nullptr;
    if (b.type == 0) {
      TRY(conv_fwd(e, st, b.c_a, x, {}, B, b.H, b.W, b.OH, b.OW, WS(b.za), b.b_a, false));
      TRY(block_end(b.b_a, WS(b.za), ACT_SILU, idn, WS(b.out), Mout, b.cout, false));
    } else if (b.type == 1) {
      TRY(conv_fwd(e, st, b.c_a, x, {}, B, b.H, b.W, b.OH, b.OW, WS(b.za), b.b_a));
      TRY(conv_fwd(e, st, b.c_p, WS(b.za), {&b.b_a, PRO_AFFINE_SILU}, B, b.OH, b.OW, b.OH, b.OW, WS(b.zp), b.b_p, false));
      TRY(block_end(b.b_p, WS(b.zp), ACT_NONE, idn, WS(b.out), Mout, b.cout, false));
    } else {
      mmvqa_bn_fold fa, fdw;
      if (fold) { set_fold_fwd(e, fa, b.b_a); set_fold_fwd(e, fdw, b.b_dw); }
      TRY(conv_fwd(e, st, b.c_a, x, {}, B, b.H, b.W, b.H, b.W, WS(b.za), b.b_a, !fold));
      RUNB(HB_DWCONV_FWD, 4.0 * ((double)B * b.H * b.W + (double)Mout) * b.mid, mmvqa_dwconv_fwd_fold(st, WS(b.za), WS(b.b_a.scale), WS(b.b_a.shift), PRM(b.dw_w), WS(b.zdw),
                                      e->bn_training ? stat_ptr(e, b.b_dw.stat_f) : nullptr, B, b.H, b.W, b.mid, b.OH, b.OW,
                                      b.stride, b.pad, fold ? &fa : nullptr));
      if (!fold) TRY(bn_coef_fwd(e, st, b.b_dw));
      // squeeze-excite: gate = sigmoid(W_e silu(W_r mean_hw(a2) + b_r) + b_e)
      RUNB(HB_SE_POOL, 4.0 * Mout * b.mid, mmvqa_se_pool_fold(st, WS(b.zdw), WS(b.b_dw.scale), WS(b.b_dw.shift), WS(b.pool), B, b.OH * b.OW, b.mid,
                                      fold ? &fdw : nullptr));
      RUN(PROF_MATRIX, 2.0 * B * b.mid * b.rd, k_skinny_fwd(st, WS(b.pool), b.mid, PRM(b.se_r.w), PRM(b.se_r.b), ACT_SILU, WS(b.rpre), WS(b.r),
                                      B, b.rd, b.mid));
      RUN(PROF_MATRIX, 2.0 * B * b.mid * b.rd, k_skinny_fwd(st, WS(b.r), b.rd, PRM(b.se_e.w), PRM(b.se_e.b), ACT_SIGMOID, WS(b.gpre),
                                      WS(b.gate), B, b.mid, b.rd));
      TRY(conv_fwd(e, st, b.c_p, WS(b.zdw), {&b.b_dw, PRO_SILU_GATE, WS(b.gate)}, B, b.OH, b.OW, b.OH, b.OW, WS(b.zp), b.b_p, false));
      TRY(block_end(b.b_p, WS(b.zp), ACT_NONE, idn, WS(b.out), Mout, b.cout, false));
    }
    x = WS(b.out);
    // the taps feed only the encoder: side stream, beside the chain of (mostly sub-chip-sized) launches
    if (b.feature >= 0) { TRY(sc.fork()); TRY(tap_fwd(e, sc.sd, b.feature, x, nullptr)); }
  }
  TRY(sc.join());   // join: the embedding reads the visual tokens
  return MMVQA_OK;
}

static int effnet_backward(mmvqa_engine* e, hipStream_t st) {
  const int B = e->NI;
  HIP_CHECK_RET(hipMemsetAsync(stat_ptr(e, 0) + e->statzone_floats / 4, 0,
                               e->statzone_floats / 2 * sizeof(float), st));
  const int nb = (int)e->eff.size();
  // BatchNorm-backward coefficients folded where both consumers are elementwise kernels (the depthwise BatchNorm).  Folding
  // in the convolutions' weight / data gradients as the ResNet path does was measured and dropped here: these BatchNorms
  // keep 16 replicas of their sums and have up to 3072 channels, every workgroup of a data gradient folds all of them, and
  // the step got 0.2 ms slower than with the coefficient launches (config 3, same box).
  const bool fold = eff_folding(e);
  // Weight gradients (convolutions, depthwise, taps) only feed the optimizer: they run on the side stream beside the
  // data-gradient chain, whose launches are mostly smaller than the chip.  A side launch starts after everything the
  // caller's stream had queued when it was issued (fork) and leaves an event behind; the chain waits for that event before
  // it overwrites a buffer the side launch reads (G alternates between the two gbuf, gA / gB between two copies by block
  // parity, so the wait is for the launch of two blocks ago).
  SideCtx scx(e, st);
  hipStream_t sd = scx.sd;
  hipEvent_t ev_G[2] = {nullptr, nullptr}, ev_gA[2] = {nullptr, nullptr}, ev_gB[2] = {nullptr, nullptr};
  hipEvent_t ev_tap[4] = {nullptr, nullptr, nullptr, nullptr};
  long long hi_mark = e->enc_lo;
  // a block whose last op is a BatchNorm (er / ir) expects the BN-backward sums of that BN with its gradient
  auto producer_opts = [&](int i, EpiOpt& o) {
    if (i < 0) return;
    EffBlock& pb = e->eff[i];
    if (pb.type != 0) { o.st1 = &pb.b_p; o.Z1 = WS(pb.zp); }
  };
  int cur = 0;
  {
    EpiOpt o;
    producer_opts(nb - 1, o);
    TRY(tap_bwd(e, st, 4, WS(e->eff[nb - 1].out), nullptr, WS(e->gbuf[cur]), o));
  }
  // the other taps produce side gradients that are needed when the chain reaches their block (they share the `du`
  // scratch with the tap above, hence the fork after it)
  TRY(scx.fork());
  for (auto& b : e->eff)
    if (b.feature >= 0 && b.feature < 4) {
      TRY(tap_bwd(e, sd, b.feature, WS(b.out), nullptr, WS(e->tapgrad[b.feature]), EpiOpt()));
      TRY(scx.mark(&ev_tap[b.feature]));
    }
  // (a stream of their own for these taps, as the ResNet path has, measured neutral here: 22.74 / 22.76 / 22.84 vs 22.67 / 22.75 / 22.72 ms)
  for (int i = nb - 1; i >= 0; --i) {
    EffBlock& b = e->eff[i];
    const float* G = WS(e->gbuf[cur]);
    const float* x = i == 0 ? WS(e->eff_a0) : WS(e->eff[i - 1].out);
    float* Gprev = WS(e->gbuf[cur ^ 1]);
    const float* extra = (i > 0 && e->eff[i - 1].feature >= 0) ? WS(e->tapgrad[e->eff[i - 1].feature]) : nullptr;
    if (extra && b.skip) return mmvqa_set_error(MMVQA_ERR_STATE, "effnet_backward: tap gradient into a skip block");
    const long Min = (long)B * b.H * b.W, Mout = (long)B * b.OH * b.OW;
    const int pi = i & 1;
    float* gA = WS(e->eff_gA[pi]);
    float* gB = WS(e->eff_gB[pi]);
    const float* dz_first = nullptr;   // gradient tensor feeding the block's first convolution
    if (b.type == 0) {
      // out = silu(bn(za)) + x
      TRY(scx.need(ev_gA[pi]));
      RUNB(HB_ACT_BWD_STATS, 12.0 * Mout * b.cout, mmvqa_act_bwd_stats(st, G, nullptr, nullptr, WS(b.za), WS(b.b_a.scale), WS(b.b_a.shift),
                                         WS(b.b_a.mean), WS(b.b_a.invstd), ACT_SILU, gA, stat_ptr(e, b.b_a.stat_b), Mout,
                                         b.OH * b.OW, b.cout));
      dz_first = gA;
    } else if (b.type == 1) {
      TRY(bn_coef_bwd(e, st, b.b_p));
      TRY(scx.fork());
      TRY(conv_wgrad(e, sd, b.c_p, G, WS(b.zp), b.b_p, WS(b.za), {&b.b_a, PRO_AFFINE_SILU}, B, b.OH, b.OW, b.OH, b.OW));
      TRY(scx.mark(&ev_G[cur]));
      TRY(scx.need(ev_gA[pi]));
      EpiOpt o;
      o.Mk = WS(b.za); o.mk_ld = b.mid; o.mk_s = WS(b.b_a.scale); o.mk_b = WS(b.b_a.shift); o.mk_mode = 1;
      o.st1 = &b.b_a; o.Z1 = WS(b.za);
      TRY(conv_dgrad(e, st, b.c_p, G, WS(b.zp), b.b_p, B, b.OH, b.OW, b.OH, b.OW, gA, o));
      dz_first = gA;
    } else {
      TRY(bn_coef_bwd(e, st, b.b_p));
      TRY(scx.fork());
      TRY(conv_wgrad(e, sd, b.c_p, G, WS(b.zp), b.b_p, WS(b.zdw), {&b.b_dw, PRO_SILU_GATE, WS(b.gate)}, B, b.OH, b.OW, b.OH, b.OW));
      TRY(scx.mark(&ev_G[cur]));
      TRY(scx.need(ev_gA[pi]));
      TRY(conv_dgrad(e, st, b.c_p, G, WS(b.zp), b.b_p, B, b.OH, b.OW, b.OH, b.OW, gA, EpiOpt()));   // t = d(a2*gate)
      // squeeze-excite backward
      float* dgate = WS(e->eff_se[0]); float* dpool = WS(e->eff_se[3]);
      RUNB(HB_SE_DGATE, 8.0 * Mout * b.mid, k_se_dgate(st, gA, WS(b.zdw), WS(b.b_dw.scale), WS(b.b_dw.shift), dgate, B, b.OH * b.OW, b.mid,
                                    WS(e->eff_separt), B * b.rd));
      RUN(PROF_MATRIX, 8.0 * B * b.mid * b.rd, k_se_fc_bwd(st, dgate, WS(b.gpre), WS(b.r), WS(b.rpre), WS(b.pool), PRM(b.se_e.w), PRM(b.se_r.w),
                                     GRD(b.se_e.w), GRD(b.se_e.b), GRD(b.se_r.w), GRD(b.se_r.b), dpool,
                                     WS(e->eff_separt), 1, B, b.mid, b.rd));
      // du2 = (t*gate + dpool/HW) * silu'(bn2(zdw)); BN2 sums
      TRY(scx.need(ev_gB[pi]));
      RUNB(HB_ACT_BWD_STATS, 12.0 * Mout * b.mid, mmvqa_act_bwd_stats(st, gA, WS(b.gate), dpool, WS(b.zdw), WS(b.b_dw.scale), WS(b.b_dw.shift),
                                         WS(b.b_dw.mean), WS(b.b_dw.invstd), ACT_SILU, gB, stat_ptr(e, b.b_dw.stat_b), Mout,
                                         b.OH * b.OW, b.mid));
      mmvqa_bn_fold fdw_w, fdw_d;
      if (fold) { set_fold_bwd(e, fdw_w, b.b_dw, false); set_fold_bwd(e, fdw_d, b.b_dw, true); }
      else TRY(bn_coef_bwd(e, st, b.b_dw));
      TRY(scx.fork());
      RUNB_ON(sd, HB_DWCONV_BWD_WEIGHT, 4.0 * (2.0 * Mout + (double)Min) * b.mid, mmvqa_dwconv_bwd_weight_fold(sd, gB, WS(b.zdw), WS(b.b_dw.P), WS(b.b_dw.Q), WS(b.b_dw.R), WS(b.za),
                                           WS(b.b_a.scale), WS(b.b_a.shift), GRD(b.dw_w), B, b.H, b.W, b.mid, b.OH, b.OW,
                                           b.stride, b.pad, fold ? &fdw_w : nullptr));
      TRY(scx.mark(&ev_gB[pi]));
      RUNB(HB_DWCONV_BWD_DATA, 4.0 * (2.0 * Mout + 2.0 * (double)Min) * b.mid, mmvqa_dwconv_bwd_data_fold(st, gB, WS(b.zdw), WS(b.b_dw.P), WS(b.b_dw.Q), WS(b.b_dw.R), PRM(b.dw_w),
                                           WS(b.za), WS(b.b_a.scale), WS(b.b_a.shift), WS(b.b_a.mean), WS(b.b_a.invstd), gA,
                                           stat_ptr(e, b.b_a.stat_b), B, b.H, b.W, b.mid, b.OH, b.OW, b.stride, b.pad, fold ? &fdw_d : nullptr));
      dz_first = gA;
    }
    // first convolution of the block: weight gradient, then the gradient wrt the block input
    TRY(bn_coef_bwd(e, st, b.b_a));
    const int fo_h = b.type == 2 ? b.H : b.OH, fo_w = b.type == 2 ? b.W : b.OW;   // its output resolution
    TRY(scx.fork());
    TRY(conv_wgrad(e, sd, b.c_a, dz_first, WS(b.za), b.b_a, x, {}, B, b.H, b.W, fo_h, fo_w));
    TRY(scx.mark(&ev_gA[pi]));
    EpiOpt o;
    producer_opts(i - 1, o);
    if (b.skip) { o.R = G; o.r_ld = b.cin; }
    else if (extra) { o.R = extra; o.r_ld = b.cin; TRY(scx.need(ev_tap[e->eff[i - 1].feature])); }
    TRY(scx.need(ev_G[cur ^ 1]));   // the buffer written next was the G of the block before: its side reader must be done
    TRY(conv_dgrad(e, st, b.c_a, dz_first, WS(b.za), b.b_a, B, b.H, b.W, fo_h, fo_w, Gprev, o));
    (void)Min;
    cur ^= 1;
    if (i > 0 && (nb - i) % 12 == 0) { TRY(notify(e, scx, b.c_a.w, hi_mark)); hi_mark = b.c_a.w; }
  }
  // stem: du0 = G(a0) * silu'(bn1(z0)); BN sums; 3x3 weight gradient on the NCHW image
  float* g0 = WS(e->gbuf[cur ^ 1]);
  const long M0 = (long)B * e->SH * e->SW;
  const int C0 = e->stem_conv.Cout;
  TRY(scx.need(ev_G[cur ^ 1]));
  RUNB(HB_ACT_BWD_STATS, 12.0 * M0 * C0, mmvqa_act_bwd_stats(st, WS(e->gbuf[cur]), nullptr, nullptr, WS(e->z0), WS(e->stem_bn.scale),
                                     WS(e->stem_bn.shift), WS(e->stem_bn.mean), WS(e->stem_bn.invstd), ACT_SILU, g0,
                                     stat_ptr(e, e->stem_bn.stat_b), M0, e->SH * e->SW, C0));
  TRY(bn_coef_bwd(e, st, e->stem_bn));
  const GemmParams g = stem_desc(e, KIND_WGRAD, g0);
  RUN(PROF_IGEMM, 2.0 * (double)g.M * g.N * g.K, mmvqa_launch_igemm(g, KIND_WGRAD, 1, 0, st));
  TRY(scx.join());   // join: everything after the backward (all-reduce, Adam) sees the side stream's gradients
  TRY(notify(e, scx, e->emb_hi, hi_mark));
  return MMVQA_OK;
}

// --------------------------------------------------------------------------- encoders
static inline uint32_t site_seed(const mmvqa_engine* e, int layer, int site) {
  return e->seed + 0x9E3779B9u * (uint32_t)(layer * 8 + site + 1);
}

static int attn_call(mmvqa_engine* e, hipStream_t st, AttnParams& a, int head_dim, int bwd) {
  REG(REG_ATTN);
  const double fl = (bwd ? 10.0 : 4.0) * (double)e->B * a.heads * e->T * e->T * head_dim;
  RUN(PROF_ATTN, fl, mmvqa_launch_attention(a, head_dim, bwd, st));
  return MMVQA_OK;
}

// The attention descriptors of the two encoders as the forward fills them; the backward adds only its d* pointers.
static AttnParams bert_attn_desc(mmvqa_engine* e, const BertLayerRef& L, int layer, float p) {
  const int H = e->d.hidden, hd = H / e->d.heads;
  AttnParams a;
  memset(&a, 0, sizeof(a));
  a.q = WS(L.qkvo); a.k = a.q + H; a.v = a.q + 2 * H;
  a.row_stride = 3 * H; a.head_stride = hd;
  a.out = WS(L.ctx); a.out_row_stride = H; a.out_head_stride = hd;
  a.mask = e->mask; a.mask_on_query = 0; a.probs = WS(L.probs);
  a.B = e->B; a.T = e->T; a.heads = e->d.heads; a.sqrt_d = sqrtf((float)hd);
  a.drop_p = p; a.seed = site_seed(e, layer, 0);
  return a;
}
static AttnParams rf_attn_desc(mmvqa_engine* e, const RFLayerRef& L, int layer) {
  const int H = e->d.hidden, es = H / 8;
  AttnParams a;
  memset(&a, 0, sizeof(a));
  a.k = WS(L.kqvo); a.q = a.k + es; a.v = a.k + 2 * es;
  a.row_stride = 8 * 3 * es; a.head_stride = 3 * es;
  a.out = WS(L.res); a.out_row_stride = H; a.out_head_stride = es;
  a.mask = e->mask; a.mask_on_query = 1;
  a.prev_in = layer > 0 ? WS(e->rf[layer - 1].prev) : nullptr;
  a.prev_out = WS(L.prev); a.probs = WS(L.probs);
  a.B = e->B; a.T = e->T; a.heads = 8; a.sqrt_d = sqrtf((float)es);
  return a;
}

// dropout on a gradient [B*T, hidden] on its way into a linear: *out = g itself where nothing is dropped, else a masked copy in t_b
static int drop_grad(mmvqa_engine* e, hipStream_t st, SideReads& sr, const float* g, float p, uint32_t seed, const float** out) {
  *out = g;
  if (p > 0.f) {
    const long n = (long)e->B * e->T * e->d.hidden;
    TRY(sr.write(WS(e->t_b)));
    RUNB(HB_DROPOUT_COPY, 8.0 * n, mmvqa_dropout_copy(st, g, WS(e->t_b), n, p, seed));
    *out = WS(e->t_b);
  }
  return MMVQA_OK;
}

// models/transformer.py:75-86 (pre-LN, norm1 for both sub-layers, shared by all layers)
static int bert_forward(mmvqa_engine* e, hipStream_t st, const float* x_in, const float** x_out) {
  REG(REG_ENC);
  const mmvqa_model_desc& d = e->d;
  const int H = d.hidden;
  const long M = (long)e->B * e->T;
  const float p = e->training ? d.p_drop : 0.f;
  const float* x = x_in;
  for (int i = 0; i < d.n_layers; ++i) {
    BertLayerRef& L = e->bert[i];
    TRY(ln_fwd(e, st, x, e->norm1, WS(L.xn1), WS(L.mean1), WS(L.rstd1), M, 1e-12f));
    static const bool fused_off = getenv("MMVQA_NO_FUSED_QKV") != nullptr;   // A/B switch
    // (its projection is an fp32 MFMA: in f16 mode the projection goes through the implicit GEMM, the unfused route)
    if (!fused_off && e->prec == MMVQA_PREC_F32 && k_qkv_attn_fwd_ok(e->T, H, d.heads)) {
      // projection + attention of every (sample, head) in one launch (qkvattn.hip): a profiler region of its own (the
      // north-star block = QKV products + attention, whichever launches carry them: bench.py adds the three regions)
      REG(REG_QKV_ATTN);
      RUN(PROF_ATTN, 2.0 * M * 3 * H * H + 4.0 * e->B * d.heads * (double)e->T * e->T * (H / d.heads),
          mmvqa_qkv_attention_fwd(st, WS(L.xn1), PRM(L.qkv.w), PRM(L.qkv.b), e->mask, WS(L.qkvo), WS(L.probs), WS(L.ctx), e->B, e->T,
                         H, d.heads, p, site_seed(e, i, 0)));
    } else {
    { REG(REG_QKV); TRY(lin_fwd(e, st, WS(L.xn1), H, M, L.qkv, WS(L.qkvo), 3 * H, ACT_NONE, nullptr, 0.f, 0, nullptr, 0)); }
    AttnParams a = bert_attn_desc(e, L, i, p);
    TRY(attn_call(e, st, a, H / d.heads, 0));
    }
    TRY(lin_fwd(e, st, WS(L.ctx), H, M, L.proj, WS(L.y), H, ACT_NONE, nullptr, p, site_seed(e, i, 1), x, H));
    TRY(ln_fwd(e, st, WS(L.y), e->norm1, WS(L.xn2), WS(L.mean2), WS(L.rstd2), M, 1e-12f));
    TRY(lin_fwd(e, st, WS(L.xn2), H, M, L.fc1, WS(L.h1), 4 * H, ACT_GELU, WS(L.pre1), 0.f, 0, nullptr, 0));
    TRY(lin_fwd(e, st, WS(L.h1), 4 * H, M, L.fc2, WS(L.z), H, ACT_NONE, nullptr, p, site_seed(e, i, 2), WS(L.y), H));
    x = WS(L.z);
  }
  *x_out = x;
  return MMVQA_OK;
}

// dz (in t_a) -> dx (left in t_a)
static int bert_backward(mmvqa_engine* e, hipStream_t st, const float* x_in, SideReads& sr) {
  REG(REG_ENC);
  const mmvqa_model_desc& d = e->d;
  const int H = d.hidden;
  const long M = (long)e->B * e->T;
  const float p = e->training ? d.p_drop : 0.f;
  float* dz = WS(e->t_a);
  for (int i = d.n_layers - 1; i >= 0; --i) {
    BertLayerRef& L = e->bert[i];
    const float* x = i == 0 ? x_in : WS(e->bert[i - 1].z);
    // FFN branch: z = y + drop(fc2(gelu(fc1(norm1(y)))))
    const float* dzd;
    TRY(drop_grad(e, st, sr, dz, p, site_seed(e, i, 2), &dzd));
    TRY(lin_wgrad_side(e, sr, st, dzd, H, WS(L.h1), 4 * H, M, L.fc2, true));
    TRY(sr.write(WS(e->t_big)));
    TRY(lin_dgrad(e, st, dzd, H, M, L.fc2, WS(e->t_big), 4 * H, ACT_GELU, WS(L.pre1), 4 * H, sr.bias_grad(GRD(L.fc1.b)), nullptr, 0));
    TRY(lin_wgrad_side(e, sr, st, WS(e->t_big), 4 * H, WS(L.xn2), H, M, L.fc1, false));
    TRY(sr.write(WS(e->t_c)));
    TRY(lin_dgrad(e, st, WS(e->t_big), 4 * H, M, L.fc1, WS(e->t_c), H, 0, nullptr, 0, nullptr, nullptr, 0));
    // dy = LN'(dxn2) + dz
    TRY(sr.write(WS(e->t_d)));
    TRY(ln_bwd(e, st, WS(e->t_c), WS(L.y), e->norm1, WS(L.mean2), WS(L.rstd2), dz, WS(e->t_d), M, sr.data_only));
    float* dy = WS(e->t_d);
    // attention branch: y = x + drop(proj(attn(norm1(x))))
    const float* dyd;
    TRY(drop_grad(e, st, sr, dy, p, site_seed(e, i, 1), &dyd));
    TRY(lin_wgrad_side(e, sr, st, dyd, H, WS(L.ctx), H, M, L.proj, true));
    TRY(sr.write(WS(e->t_c)));
    TRY(lin_dgrad(e, st, dyd, H, M, L.proj, WS(e->t_c), H, 0, nullptr, 0, nullptr, nullptr, 0));  // dctx
    AttnParams a = bert_attn_desc(e, L, i, p);
    a.dout = WS(e->t_c);
    float* dqkv = WS(e->t_big);
    a.dq = dqkv; a.dk = dqkv + H; a.dv = dqkv + 2 * H;
    TRY(sr.write(dqkv));
    TRY(attn_call(e, st, a, H / d.heads, 1));
    { REG(REG_QKV);
      TRY(lin_wgrad_side(e, sr, st, dqkv, 3 * H, WS(L.xn1), H, M, L.qkv, true));
      TRY(sr.write(WS(e->t_c)));
      TRY(lin_dgrad(e, st, dqkv, 3 * H, M, L.qkv, WS(e->t_c), H, 0, nullptr, 0, nullptr, nullptr, 0)); }  // dxn1
    TRY(sr.write(dz));
    TRY(ln_bwd(e, st, WS(e->t_c), x, e->norm1, WS(L.mean1), WS(L.rstd1), dy, dz, M, sr.data_only));
  }
  return MMVQA_OK;
}

// models/realformer.py:30-51 (post-LN, shared per-head kqv, residual scores, query-axis mask)
static int rf_forward(mmvqa_engine* e, hipStream_t st, const float* x_in, const float** x_out) {
  REG(REG_ENC);
  const mmvqa_model_desc& d = e->d;
  const int H = d.hidden, es = H / 8;
  const long M = (long)e->B * e->T;
  const float p = e->training ? d.p_rf_drop : 0.f;
  const float* x = x_in;
  for (int i = 0; i < d.n_layers; ++i) {
    RFLayerRef& L = e->rf[i];
    { REG(REG_QKV); TRY(lin_fwd(e, st, x, es, M * 8, L.kqv, WS(L.kqvo), 3 * es, ACT_NONE, nullptr, 0.f, 0, nullptr, 0)); }
    AttnParams a = rf_attn_desc(e, L, i);
    TRY(attn_call(e, st, a, es, 0));
    // s1 = x + drop(proj(res)); x1 = ln1(s1)
    TRY(lin_fwd(e, st, WS(L.res), H, M, L.proj, WS(L.s1), H, ACT_NONE, nullptr, p, site_seed(e, i, 1), x, H));
    TRY(ln_fwd(e, st, WS(L.s1), L.ln1, WS(L.x1), WS(L.mean1), WS(L.rstd1), M, 1e-5f));
    TRY(lin_fwd(e, st, WS(L.x1), H, M, L.ff0, WS(L.hact), 4 * H, ACT_SERF, WS(L.pre), 0.f, 0, nullptr, 0));
    TRY(lin_fwd(e, st, WS(L.hact), 4 * H, M, L.ff2, WS(L.s2), H, ACT_NONE, nullptr, p, site_seed(e, i, 2), WS(L.x1), H));
    TRY(ln_fwd(e, st, WS(L.s2), L.ln2, WS(L.x2), WS(L.mean2), WS(L.rstd2), M, 1e-5f));
    x = WS(L.x2);
  }
  *x_out = x;
  return MMVQA_OK;
}

static int rf_backward(mmvqa_engine* e, hipStream_t st, const float* x_in, SideReads& sr) {
  REG(REG_ENC);
  const mmvqa_model_desc& d = e->d;
  const int H = d.hidden, es = H / 8;
  const long M = (long)e->B * e->T;
  const float p = e->training ? d.p_rf_drop : 0.f;
  float* dx2 = WS(e->t_a);
  for (int i = d.n_layers - 1; i >= 0; --i) {
    RFLayerRef& L = e->rf[i];
    const float* x = i == 0 ? x_in : WS(e->rf[i - 1].x2);
    // x2 = ln2(s2), s2 = x1 + drop(ff2(serf(ff0(x1))))
    TRY(sr.write(WS(e->t_d)));
    TRY(ln_bwd(e, st, dx2, WS(L.s2), L.ln2, WS(L.mean2), WS(L.rstd2), nullptr, WS(e->t_d), M, sr.data_only));
    float* ds2 = WS(e->t_d);
    const float* dff;
    TRY(drop_grad(e, st, sr, ds2, p, site_seed(e, i, 2), &dff));
    TRY(lin_wgrad_side(e, sr, st, dff, H, WS(L.hact), 4 * H, M, L.ff2, true));
    TRY(sr.write(WS(e->t_big)));
    TRY(lin_dgrad(e, st, dff, H, M, L.ff2, WS(e->t_big), 4 * H, ACT_SERF, WS(L.pre), 4 * H, sr.bias_grad(GRD(L.ff0.b)), nullptr, 0));
    TRY(lin_wgrad_side(e, sr, st, WS(e->t_big), 4 * H, WS(L.x1), H, M, L.ff0, false));
    TRY(sr.write(WS(e->t_c)));
    TRY(lin_dgrad(e, st, WS(e->t_big), 4 * H, M, L.ff0, WS(e->t_c), H, 0, nullptr, 0, nullptr, ds2, H));  // dx1 total
    // x1 = ln1(s1), s1 = x + drop(proj(res))
    TRY(sr.write(WS(e->t_d)));
    TRY(ln_bwd(e, st, WS(e->t_c), WS(L.s1), L.ln1, WS(L.mean1), WS(L.rstd1), nullptr, WS(e->t_d), M, sr.data_only));
    float* ds1 = WS(e->t_d);
    const float* dr;
    TRY(drop_grad(e, st, sr, ds1, p, site_seed(e, i, 1), &dr));
    TRY(lin_wgrad_side(e, sr, st, dr, H, WS(L.res), H, M, L.proj, false));
    TRY(sr.write(WS(e->t_c)));
    TRY(lin_dgrad(e, st, dr, H, M, L.proj, WS(e->t_c), H, 0, nullptr, 0, nullptr, nullptr, 0));  // dres
    AttnParams a = rf_attn_desc(e, L, i);
    a.dout = WS(e->t_c);
    float* dkqv = WS(e->t_big);
    a.dk = dkqv; a.dq = dkqv + es; a.dv = dkqv + 2 * es;
    a.dprev_in = (i < d.n_layers - 1) ? WS(e->t_dprev[(i + 1) & 1]) : nullptr;
    a.dprev_out = i > 0 ? WS(e->t_dprev[i & 1]) : nullptr;
    TRY(sr.write(dkqv));
    TRY(attn_call(e, st, a, es, 1));
    { REG(REG_QKV);
      TRY(lin_wgrad_side(e, sr, st, dkqv, 3 * es, x, es, M * 8, L.kqv, false));
      TRY(sr.write(dx2));
      TRY(lin_dgrad(e, st, dkqv, 3 * es, M * 8, L.kqv, dx2, es, 0, nullptr, 0, nullptr, ds1, es)); }  // dx total
  }
  return MMVQA_OK;
}

// models/feedback_transformer_pytorch.py:257-312 with seq_len = 2: a recurrence over windows of two tokens (an odd T ends in
// a window of one).  Rows are window-major: window w holds rows [w*2B, w*2B + n*B), row b*n + i, so that every linear of a
// window is one product with M = n*B.  DESIGN.md section 15.
static inline int fb_windows(int T) { return (T + 1) / 2; }
static inline int fb_tokens(int T, int w) { return 2 * w + 1 < T ? 2 : 1; }

static void fb_attn_fill(mmvqa_engine* e, const FBLayerRef& L, int layer, int w, int n, float p, mmvqa_fb_attn_desc& a) {
  const size_t r0 = (size_t)w * 2 * e->B;
  memset(&a, 0, sizeof(a));
  a.q = WS(L.q) + r0 * 512; a.q_ld = 512;
  a.mem_k = WS(e->fb_mem); a.mem_v = a.mem_k + 512; a.mem_win = (long long)2 * e->B * 1024; a.mem_ld = 1024;
  if (n == 2) { a.self_k = WS(L.kv) + r0 * 1024; a.self_v = a.self_k + 512; a.self_ld = 1024; }
  a.bias = PRM(e->fb_rel);
  a.probs = WS(L.probs) + (size_t)w * e->B * 8 * 2 * e->T; a.p_ld = e->T;
  a.out = WS(L.ctx) + r0 * 512; a.out_ld = 512;
  a.B = e->B; a.n = n; a.n_mem = 2 * w; a.T = e->T;
  a.scale = 0.125f;   // dim_head ** -0.5
  a.drop_p = p; a.seed = site_seed(e, layer, 0);
}
static int fb_attn_call(mmvqa_engine* e, hipStream_t st, const mmvqa_fb_attn_desc& a, int bwd) {
  REG(REG_ATTN);
  const double fl = (bwd ? 10.0 : 4.0) * (double)a.B * 8 * a.n * (a.n_mem + (a.n == 2 ? 2 : 0)) * 64;
  RUN(PROF_ATTN, fl, mmvqa_fb_attention(&a, bwd, st));
  return MMVQA_OK;
}

static int fb_forward(mmvqa_engine* e, hipStream_t st, const float* x_in, const float** x_out) {
  REG(REG_ENC);
  const mmvqa_model_desc& d = e->d;
  const int H = d.hidden, B = e->B, T = e->T, NL = d.n_layers, nwin = fb_windows(T);
  const size_t M = (size_t)B * T;
  const float p = e->training ? d.p_fb_drop : 0.f;
  RUN(PROF_OTHER, 0, k_fb_reorder(st, x_in, WS(e->fb_hid), B, T, H, 1));
  for (int w = 0; w < nwin; ++w) {
    const int n = fb_tokens(T, w);
    const long Mw = (long)n * B;
    const size_t r0 = (size_t)w * 2 * B;
    for (int i = 0; i < NL; ++i) {
      FBLayerRef& L = e->fb[i];
      const float* x = WS(e->fb_hid) + i * M * H + r0 * H;
      // x = x + to_out(attn(LN_a(x)))
      TRY(ln_fwd(e, st, x, L.ln_a, WS(L.xn_a) + r0 * H, WS(L.mean_a) + r0, WS(L.rstd_a) + r0, Mw, 1e-5f));
      { REG(REG_QKV);
        TRY(lin_fwd(e, st, WS(L.xn_a) + r0 * H, H, Mw, L.to_q, WS(L.q) + r0 * 512, 512, ACT_NONE, nullptr, 0.f, 0, nullptr, 0));
        if (n == 2)   // "only self attend if going at greater than 1 token at a time" (:163)
          TRY(lin_fwd(e, st, WS(L.xn_a) + r0 * H, H, Mw, e->fb_kv, WS(L.kv) + r0 * 1024, 1024, ACT_NONE, nullptr, 0.f, 0, nullptr, 0)); }
      mmvqa_fb_attn_desc a;
      fb_attn_fill(e, L, i, w, n, p, a);
      TRY(fb_attn_call(e, st, a, 0));
      TRY(lin_fwd(e, st, WS(L.ctx) + r0 * 512, 512, Mw, L.to_out, WS(L.xmid) + r0 * H, H, ACT_NONE, nullptr, 0.f, 0, x, H));
      // x = x + W2(drop(gelu(gate) * u)), (u | gate) = W1 LN_f(x)
      TRY(ln_fwd(e, st, WS(L.xmid) + r0 * H, L.ln_f, WS(L.xn_f) + r0 * H, WS(L.mean_f) + r0, WS(L.rstd_f) + r0, Mw, 1e-5f));
      TRY(lin_fwd(e, st, WS(L.xn_f) + r0 * H, H, Mw, L.w1, WS(L.pre) + r0 * 8 * H, 8 * H, ACT_NONE, nullptr, 0.f, 0, nullptr, 0));
      RUN(PROF_OTHER, 0, mmvqa_geglu_fwd(st, WS(L.pre) + r0 * 8 * H, WS(L.gg) + r0 * 4 * H, Mw, 4 * H, p, site_seed(e, i, 1),
                                     (uint32_t)(r0 * 4 * H)));
      TRY(lin_fwd(e, st, WS(L.gg) + r0 * 4 * H, 4 * H, Mw, L.w2, WS(e->fb_hid) + (i + 1) * M * H + r0 * H, H, ACT_NONE, nullptr, 0.f,
                  0, WS(L.xmid) + r0 * H, H));
    }
    if (w + 1 < nwin) {   // the memory the last window would write is never read
      RUN(PROF_OTHER, 0, mmvqa_fb_aggregate_fwd(st, WS(e->fb_hid) + r0 * H, (long long)(M * H), NL + 1, PRM(e->fb_lw),
                                            WS(e->fb_agg) + r0 * H, Mw, H));
      REG(REG_QKV);
      TRY(lin_fwd(e, st, WS(e->fb_agg) + r0 * H, H, Mw, e->fb_kv, WS(e->fb_mem) + r0 * 1024, 1024, ACT_NONE, nullptr, 0.f, 0, nullptr, 0));
    }
  }
  RUN(PROF_OTHER, 0, k_fb_reorder(st, WS(e->fb_hid) + NL * M * H, WS(e->fb_out), B, T, H, 0));
  *x_out = WS(e->fb_out);
  return MMVQA_OK;
}

// dh (in t_a, [B][T][H]) -> dx (left in t_a).  The time loop (windows last to first, layers last to first) runs the data
// gradients only and leaves every linear's output gradient in a buffer of the full B*T rows; the weight gradients follow the
// loop, one product over all rows per linear, on the side stream.
static int fb_backward(mmvqa_engine* e, hipStream_t st, const float* x_in, SideReads& sr) {
  (void)x_in;
  REG(REG_ENC);
  const mmvqa_model_desc& d = e->d;
  const int H = d.hidden, B = e->B, T = e->T, NL = d.n_layers, nwin = fb_windows(T);
  const size_t M = (size_t)B * T;
  const float p = e->training ? d.p_fb_drop : 0.f;
  float* ghid = WS(e->fb_ghid);
  RUN(PROF_OTHER, 0, k_fb_reorder(st, WS(e->t_a), ghid + NL * M * H, B, T, H, 1));
  HIP_CHECK_RET(hipMemsetAsync(WS(e->fb_dmem), 0, M * 1024 * sizeof(float), st));
  float *s1 = WS(e->fb_s[0]), *s2 = WS(e->fb_s[1]), *s3 = WS(e->fb_s[2]), *s4 = WS(e->fb_s[3]), *s5 = WS(e->fb_s[4]);
  for (int w = nwin - 1; w >= 0; --w) {
    const int n = fb_tokens(T, w);
    const long Mw = (long)n * B;
    const size_t r0 = (size_t)w * 2 * B;
    const bool wrote_mem = w + 1 < nwin;
    if (wrote_mem) {
      // every later window has added its share: rows r0.. of dmem are final.  dagg through the shared projection, then
      // softmax(layer_weight)_l * dagg into each hidden's gradient (the top one at once, the others when the loop gets there)
      { REG(REG_QKV);
        TRY(lin_dgrad(e, st, WS(e->fb_dmem) + r0 * 1024, 1024, Mw, e->fb_kv, s2, H, 0, nullptr, 0, nullptr, nullptr, 0)); }
      RUN(PROF_OTHER, 0, mmvqa_fb_aggregate_bwd(st, s2, WS(e->fb_hid) + r0 * H, (long long)(M * H), NL + 1, PRM(e->fb_lw),
                                            WS(e->fb_dhs), (long long)2 * B * H, ghid + NL * M * H + r0 * H,
                                            sr.data_only ? nullptr : GRD(e->fb_lw), Mw, H));
    }
    for (int i = NL - 1; i >= 0; --i) {
      FBLayerRef& L = e->fb[i];
      const float* gout = ghid + (i + 1) * M * H + r0 * H;
      TRY(lin_dgrad(e, st, gout, H, Mw, L.w2, s1, 4 * H, 0, nullptr, 0, nullptr, nullptr, 0));
      RUN(PROF_OTHER, 0, mmvqa_geglu_bwd(st, s1, WS(L.pre) + r0 * 8 * H, WS(L.g_pre) + r0 * 8 * H, Mw, 4 * H, p, site_seed(e, i, 1),
                                     (uint32_t)(r0 * 4 * H)));
      TRY(lin_dgrad(e, st, WS(L.g_pre) + r0 * 8 * H, 8 * H, Mw, L.w1, s2, H, 0, nullptr, 0, nullptr, nullptr, 0));
      TRY(ln_bwd(e, st, s2, WS(L.xmid) + r0 * H, L.ln_f, WS(L.mean_f) + r0, WS(L.rstd_f) + r0, gout, WS(L.g_mid) + r0 * H, Mw,
                 sr.data_only));
      TRY(lin_dgrad(e, st, WS(L.g_mid) + r0 * H, H, Mw, L.to_out, s3, 512, 0, nullptr, 0, nullptr, nullptr, 0));
      mmvqa_fb_attn_desc a;
      fb_attn_fill(e, L, i, w, n, p, a);
      a.dout = s3; a.dout_ld = 512;
      a.dq = WS(L.g_q) + r0 * 512; a.dq_ld = 512;
      if (n == 2) { a.dself_k = WS(L.g_kv) + r0 * 1024; a.dself_v = a.dself_k + 512; a.dself_ld = 1024; }
      a.dmem_k = WS(e->fb_dmem); a.dmem_v = a.dmem_k + 512;
      a.dbias = sr.data_only ? nullptr : GRD(e->fb_rel);
      TRY(fb_attn_call(e, st, a, 1));
      const float* dxn = s4;
      { REG(REG_QKV);
        TRY(lin_dgrad(e, st, WS(L.g_q) + r0 * 512, 512, Mw, L.to_q, s4, H, 0, nullptr, 0, nullptr, nullptr, 0));
        if (n == 2) {
          TRY(lin_dgrad(e, st, WS(L.g_kv) + r0 * 1024, 1024, Mw, e->fb_kv, s5, H, 0, nullptr, 0, nullptr, s4, H));
          dxn = s5;
        } }
      TRY(ln_bwd(e, st, dxn, WS(e->fb_hid) + i * M * H + r0 * H, L.ln_a, WS(L.mean_a) + r0, WS(L.rstd_a) + r0,
                 WS(L.g_mid) + r0 * H, ghid + i * M * H + r0 * H, Mw, sr.data_only));
      if (wrote_mem)
        RUN(PROF_OTHER, 0, mmvqa_axpy(st, ghid + i * M * H + r0 * H, WS(e->fb_dhs) + (size_t)i * 2 * B * H, 1.0f, Mw * H));
    }
  }
  if (!sr.data_only) {
    // weight gradients: the same sums over the windows, each formed in one product over all rows.  The shared to_kv weight
    // collects one product per layer (self keys / values: the rows of the two-token windows, which come first) and one for
    // the memory projection (input agg, every window but the last).
    const long Mfull = (long)2 * B * (T / 2), Mmem = (long)2 * B * (nwin - 1);
    struct TagScope { mmvqa_engine* e; TagScope(mmvqa_engine* e_) : e(e_) { e->prof_tag = HB_FB_WGRAD; } ~TagScope() { e->prof_tag = HB_NONE; } } tag(e);
    for (int i = NL - 1; i >= 0; --i) {
      FBLayerRef& L = e->fb[i];
      TRY(lin_wgrad_side(e, sr, st, ghid + (i + 1) * M * H, H, WS(L.gg), 4 * H, (long)M, L.w2, true));
      TRY(lin_wgrad_side(e, sr, st, WS(L.g_pre), 8 * H, WS(L.xn_f), H, (long)M, L.w1, true));
      TRY(lin_wgrad_side(e, sr, st, WS(L.g_mid), H, WS(L.ctx), 512, (long)M, L.to_out, true));
      REG(REG_QKV);
      TRY(lin_wgrad_side(e, sr, st, WS(L.g_q), 512, WS(L.xn_a), H, (long)M, L.to_q, false));
      TRY(lin_wgrad_side(e, sr, st, WS(L.g_kv), 1024, WS(L.xn_a), H, Mfull, e->fb_kv, false));
    }
    if (Mmem > 0) {
      REG(REG_QKV);
      TRY(lin_wgrad_side(e, sr, st, WS(e->fb_dmem), 1024, WS(e->fb_agg), H, Mmem, e->fb_kv, false));
    }
  }
  TRY(sr.write(WS(e->t_a)));
  RUN(PROF_OTHER, 0, k_fb_reorder(st, ghid, WS(e->t_a), B, T, H, 0));
  return MMVQA_OK;
}

// --------------------------------------------------------------------------- heads (models/mmbert.py:150-167)
static int heads_forward(mmvqa_engine* e, hipStream_t st, const float* h) {
  REG(REG_HEAD);
  const mmvqa_model_desc& d = e->d;
  const int H = d.hidden;
  const long M = (long)e->B * e->T;
  const float* hin = h;
  long HM = M;
  if (d.head_kind == 1) {
    RUN(PROF_OTHER, 0, mmvqa_meanpool_fwd(st, h, e->mask, WS(e->hd_pool), e->B, e->T, H));
    hin = WS(e->hd_pool);
    HM = e->B;
  }
  TRY(lin_fwd(e, st, hin, H, HM, e->fc1, WS(e->hd_u), H, ACT_SERF, WS(e->hd_upre), 0.f, 0, nullptr, 0));
  TRY(lin_fwd(e, st, WS(e->hd_u), H, HM, e->cls0, WS(e->hd_c0), H, ACT_NONE, nullptr, 0.f, 0, nullptr, 0));
  TRY(ln_fwd(e, st, WS(e->hd_c0), e->cls_ln, WS(e->hd_c1), WS(e->hd_mean), WS(e->hd_rstd), HM, 1e-12f));
  TRY(lin_fwd(e, st, WS(e->hd_c1), H, HM, e->cls2, e->logits, e->logits_ld, ACT_NONE, nullptr, 0.f, 0, nullptr, 0));
  if (d.supcon && e->feat) {
    RUN(PROF_OTHER, 0, mmvqa_meanpool_fwd(st, h, e->mask, WS(e->sc_pool), e->B, e->T, H));
    TRY(lin_fwd(e, st, WS(e->sc_pool), H, e->B, e->head0, WS(e->sc_a), H, ACT_SERF, WS(e->sc_pre), 0.f, 0, nullptr, 0));
    TRY(lin_fwd(e, st, WS(e->sc_a), H, e->B, e->head2, WS(e->sc_f), d.feat_dim, ACT_NONE, nullptr, 0.f, 0, nullptr, 0));
    // the normalised features stay in the engine's workspace for the backward pass: the caller may drop its
    // `feat` tensor before backward (supcon_utils.py:283-284 rebinds it to split_feat(feat))
    RUN(PROF_OTHER, 0, mmvqa_l2norm_fwd(st, WS(e->sc_f), WS(e->sc_y), WS(e->sc_nrm), e->B, d.feat_dim));
    HIP_CHECK_RET(hipMemcpyAsync(e->feat, WS(e->sc_y), (size_t)e->B * d.feat_dim * sizeof(float),
                                 hipMemcpyDeviceToDevice, st));
  }
  return MMVQA_OK;
}

// produces dh (gradient wrt the encoder output) in t_a
static int heads_backward(mmvqa_engine* e, hipStream_t st, const float* h, const float* dlogits, int dl_ld,
                          const float* dfeat, SideReads& sr) {
  REG(REG_HEAD);
  const mmvqa_model_desc& d = e->d;
  const int H = d.hidden;
  const long M = (long)e->B * e->T;
  const long HM = d.head_kind == 1 ? e->B : M;
  const float* hin = d.head_kind == 1 ? WS(e->hd_pool) : h;
  if (!sr.data_only) {  // classifier[2]: logits = c1 W^T + b  (beside the data gradient of the same layer: both read dlogits, nobody writes it)
    if (sr.on) TRY(sr.sc.fork());
    hipStream_t wst = sr.on ? sr.sc.sd : st;
    GemmParams g = gp_linear_geom();
    g.M = d.n_classes; g.N = H; g.K = (int)HM;
    g.A = dlogits; g.a_ld = dl_ld;
    g.B = WS(e->hd_c1); g.b_ld = H; g.g_Cs = H;
    g.C = GRD(e->cls2.w); g.c_ld = H; g.c_atomic = 1;
    RUN_ON(wst, PROF_IGEMM, 2.0 * HM * d.n_classes * H, mmvqa_launch_igemm(g, KIND_WGRAD, 0, 0, wst));
    RUN_ON(wst, PROF_OTHER, 0, mmvqa_colsum(wst, dlogits, dl_ld, (int)HM, d.n_classes, GRD(e->cls2.b)));
  }
  TRY(lin_dgrad(e, st, dlogits, dl_ld, HM, e->cls2, WS(e->t_b), H, 0, nullptr, 0, nullptr, nullptr, 0));  // dc1
  TRY(ln_bwd(e, st, WS(e->t_b), WS(e->hd_c0), e->cls_ln, WS(e->hd_mean), WS(e->hd_rstd), nullptr, WS(e->t_c), HM, sr.data_only));
  TRY(lin_wgrad_side(e, sr, st, WS(e->t_c), H, WS(e->hd_u), H, HM, e->cls0, true));
  TRY(lin_dgrad(e, st, WS(e->t_c), H, HM, e->cls0, WS(e->t_b), H, ACT_SERF, WS(e->hd_upre), H, sr.bias_grad(GRD(e->fc1.b)), nullptr, 0));
  TRY(lin_wgrad_side(e, sr, st, WS(e->t_b), H, hin, H, HM, e->fc1, false));
  float* dh = WS(e->t_a);
  if (d.head_kind == 1) {
    TRY(sr.write(WS(e->t_c)));
    TRY(lin_dgrad(e, st, WS(e->t_b), H, HM, e->fc1, WS(e->t_c), H, 0, nullptr, 0, nullptr, nullptr, 0));
    RUN(PROF_OTHER, 0, mmvqa_meanpool_bwd(st, WS(e->t_c), e->mask, dh, e->B, e->T, H, 0));
  } else {
    TRY(lin_dgrad(e, st, WS(e->t_b), H, HM, e->fc1, dh, H, 0, nullptr, 0, nullptr, nullptr, 0));
  }
  if (d.supcon && dfeat) {
    TRY(sr.write(WS(e->t_b))); TRY(sr.write(WS(e->t_c)));
    float* df = WS(e->t_b);  // [B][feat_dim]
    RUN(PROF_OTHER, 0, mmvqa_l2norm_bwd(st, dfeat, WS(e->sc_y), WS(e->sc_nrm), df, e->B, d.feat_dim));
    TRY(lin_wgrad(e, st, df, d.feat_dim, WS(e->sc_a), H, e->B, e->head2, true));
    TRY(lin_dgrad(e, st, df, d.feat_dim, e->B, e->head2, WS(e->t_c), H, ACT_SERF, WS(e->sc_pre), H, GRD(e->head0.b), nullptr, 0));
    TRY(lin_wgrad(e, st, WS(e->t_c), H, WS(e->sc_pool), H, e->B, e->head0, false));
    TRY(lin_dgrad(e, st, WS(e->t_c), H, e->B, e->head0, WS(e->t_d), H, 0, nullptr, 0, nullptr, nullptr, 0));
    RUN(PROF_OTHER, 0, mmvqa_meanpool_bwd(st, WS(e->t_d), e->mask, dh, e->B, e->T, H, 1));
  }
  return MMVQA_OK;
}

// rows x cols floats between two row-major buffers on `st`.  Equal leading dimensions (what the Python shim passes:
// hidden is a multiple of 8) make it one linear copy, which the runtime enqueues without waiting for the stream; the
// strided form is correct for any ld but the runtime may hold the host until the stream has drained.
static int copy_rows(hipStream_t st, float* dst, size_t dst_ld, const float* src, size_t src_ld, size_t rows, size_t cols) {
  if (dst_ld == cols && src_ld == cols)
    HIP_CHECK_RET(hipMemcpyAsync(dst, src, rows * cols * sizeof(float), hipMemcpyDeviceToDevice, st));
  else
    HIP_CHECK_RET(hipMemcpy2DAsync(dst, dst_ld * sizeof(float), src, src_ld * sizeof(float), cols * sizeof(float), rows,
                                   hipMemcpyDeviceToDevice, st));
  return MMVQA_OK;
}

// --------------------------------------------------------------------------- whole model
// State that lives in the caller's workspace ACROSS calls (mmvqa.h, mmvqa_engine_bind): the tap-validity tables of the
// 3x3 weight gradients and the (zero) arrival tickets of the ticketed split-K launches.  Put in place on the caller's stream
// by the first forward after a bind, i.e. before the side stream exists for that workspace.
static int prepare_workspace(mmvqa_engine* e, hipStream_t st) {
  if (e->ws_ready) return MMVQA_OK;
  for (auto& kv : e->pixmask_off) {
    const mmvqa_engine::PixGeom& q = kv.second;
    TRY(mmvqa_pixmask(st, reinterpret_cast<int*>(WS(q.off)), q.N, q.OH, q.OW, q.H, q.W, q.KH, q.KH, q.stride, q.pad));
  }
  for (int i = 0; i < 3; ++i) HIP_CHECK_RET(hipMemsetAsync(WS(e->sk_cnt[i]), 0, SK_CNT_N * sizeof(unsigned int), st));
  e->ws_ready = true;
  return MMVQA_OK;
}

// One entry point's launches: every implicit GEMM inside takes the engine's tuner and the given operand precision, and the
// event pool is handed out from its start again
struct StepScope {
  StepScope(mmvqa_engine* e, int prec) { mmvqa_set_tuner(&e->tuner); mmvqa_set_igemm_precision(prec); e->ev_next = 0; }
  ~StepScope() { mmvqa_set_igemm_precision(MMVQA_PREC_F32); mmvqa_set_tuner(nullptr); }
};

static int encoder_forward(mmvqa_engine* e, hipStream_t st, const float** h) {
  if (e->d.encoder == 0) return bert_forward(e, st, WS(e->emb_out), h);
  if (e->d.encoder == 2) return fb_forward(e, st, WS(e->emb_out), h);
  return rf_forward(e, st, WS(e->emb_out), h);
}
static int encoder_backward(mmvqa_engine* e, hipStream_t st, SideReads& sr) {
  if (e->d.encoder == 0) return bert_backward(e, st, WS(e->emb_out), sr);
  if (e->d.encoder == 2) return fb_backward(e, st, WS(e->emb_out), sr);
  return rf_backward(e, st, WS(e->emb_out), sr);
}

int engine_forward(mmvqa_engine* e, hipStream_t st, const float* img, const long long* ids, const long long* seg,
                   const long long* mask, float* logits, int logits_ld, float* feat, int training, uint32_t seed,
                   const int* group, const int* offsets) {
  if (!e->planned || !e->bound) return mmvqa_set_error(MMVQA_ERR_STATE, "engine_forward: plan/bind first");
  if (e->grouped != (group != nullptr))
    return mmvqa_set_error(MMVQA_ERR_STATE, e->grouped ? "engine_forward: the plan is grouped (NI=%d images, B=%d rows): call "
                                                         "mmvqa_engine_forward_grouped, or plan again"
                                                       : "engine_forward_grouped: the plan is not grouped (NI=%d, B=%d): call "
                                                         "mmvqa_engine_plan_grouped first", e->NI, e->B);
  TRY(prepare_workspace(e, st));
  const mmvqa_model_desc& d = e->d;
  const int out_w = d.head_kind == 2 ? d.hidden : d.n_classes;   // headless: the caller's buffer receives h
  if (logits_ld < out_w || (logits_ld & 3))
    return mmvqa_set_error(MMVQA_ERR_ARG, "engine_forward: logits_ld=%d must be >= %s=%d and %%4==0", logits_ld,
                           d.head_kind == 2 ? "hidden" : "n_classes", out_w);
  e->img = img; e->ids = ids; e->seg = seg; e->mask = mask;
  e->logits = logits; e->logits_ld = logits_ld; e->feat = feat;
  e->training = training; e->seed = seed; e->tokens_only = false; e->cached = false;
  e->frozen = e->frozen_next;
  // `training` means dropout everywhere and batch statistics in the backbone's BatchNorms; the two part only under
  // MMVQA_FREEZE_BN_STATS (backbone.eval() inside model.train())
  e->bn_training = training && !(e->frozen & MMVQA_FREEZE_BN_STATS);
  if (e->prec != MMVQA_PREC_F32 && d.cnn != 0)
    return mmvqa_set_error(MMVQA_ERR_ARG, "engine_forward: f16 operand mode covers the ResNet encoders only");
  StepScope scope(e, e->prec);
  if (e->grouped) {   // the engine's own copy of the maps: the backward reads offsets long after the caller's buffers may be gone
    int* grp = reinterpret_cast<int*>(WS(e->grp));
    HIP_CHECK_RET(hipMemcpyAsync(grp, group, (size_t)e->B * sizeof(int), hipMemcpyDeviceToDevice, st));
    HIP_CHECK_RET(hipMemcpyAsync(grp + e->B, offsets, ((size_t)e->NI + 1) * sizeof(int), hipMemcpyDeviceToDevice, st));
  }
  if (d.cnn == 1) TRY(effnet_forward(e, st)); else TRY(resnet_forward(e, st));
  const float pe = training ? d.p_emb_drop : 0.f;
  e->prof_reg = REG_EMBED;
  const float* vis = WS(e->vis);
  if (e->grouped) {   // question b reads the tokens of image group[b]
    RUNB(HB_NONE, 8.0 * d.num_vis * e->B * d.hidden,
         mmvqa_vis_expand(st, WS(e->vis), reinterpret_cast<const int*>(WS(e->grp)), WS(e->vis_q), e->NI, e->B, d.hidden, d.num_vis));
    vis = WS(e->vis_q);
  }
  RUN(PROF_OTHER, 0,
      mmvqa_embed_fwd(st, ids, seg, PRM(e->emb_word), PRM(e->emb_pos), PRM(e->emb_type), PRM(e->emb_ln.g),
                  PRM(e->emb_ln.b), vis, WS(e->emb_out), WS(e->emb_xhat), WS(e->emb_rstd), e->B, e->T,
                  d.hidden, d.num_vis, 1e-12f, pe, site_seed(e, 100, 0)));
  e->prof_reg = REG_BACKBONE;
  const float* h = nullptr;
  TRY(encoder_forward(e, st, &h));
  e->enc_out_final = (size_t)(h - e->ws);
  if (d.head_kind == 2) {   // models/mmbert.py:159-161: logits = h; fc1 / classifier / head are not run
    return copy_rows(st, logits, (size_t)logits_ld, h, (size_t)d.hidden, (size_t)e->B * e->T, (size_t)d.hidden);
  }
  return heads_forward(e, st, h);
}

// Where the last forward left the num_vis visual tokens: [num_vis][NI][hidden] inside the bound workspace (NI == B unless
// the plan is grouped), as the taps write them; valid until the next forward.
int engine_visual_tokens(mmvqa_engine* e, const float** vis) {
  if (!e->planned || !e->bound || (!e->img && !e->tokens_only))
    return mmvqa_set_error(MMVQA_ERR_STATE, "engine_visual_tokens: plan/bind and run a forward first");
  if (!vis) return mmvqa_set_error(MMVQA_ERR_ARG, "engine_visual_tokens: null pointer");
  *vis = WS(e->vis);
  return MMVQA_OK;
}

// The eval-mode forward from given visual tokens: `vis` [num_vis][B][hidden] takes the place of what the backbone and
// its taps write, then exactly the launches of engine_forward after the backbone run on the caller's stream.  The
// backbone's activations in the workspace are NOT those of these tokens afterwards: both backward entry points refuse.
int engine_forward_tokens(mmvqa_engine* e, hipStream_t st, const float* vis, const long long* ids, const long long* seg,
                          const long long* mask, float* logits, int logits_ld, float* feat) {
  if (e->prec != MMVQA_PREC_F32)
    return mmvqa_set_error(MMVQA_ERR_ARG, "engine_forward_tokens: runs with fp32 operands, not in the f16 operand mode");
  if (!e->planned || !e->bound) return mmvqa_set_error(MMVQA_ERR_STATE, "engine_forward_tokens: plan/bind first");
  if (e->grouped) return mmvqa_set_error(MMVQA_ERR_STATE, "engine_forward_tokens: the plan is grouped; plan again with mmvqa_engine_plan");
  const mmvqa_model_desc& d = e->d;
  const int out_w = d.head_kind == 2 ? d.hidden : d.n_classes;
  if (logits_ld < out_w || (logits_ld & 3))
    return mmvqa_set_error(MMVQA_ERR_ARG, "engine_forward_tokens: logits_ld=%d must be >= %s=%d and %%4==0", logits_ld,
                           d.head_kind == 2 ? "hidden" : "n_classes", out_w);
  TRY(prepare_workspace(e, st));
  e->img = nullptr; e->tokens_only = true; e->cached = false;   // no backward of any kind after this forward
  e->ids = ids; e->seg = seg; e->mask = mask;
  e->logits = logits; e->logits_ld = logits_ld; e->feat = feat;
  e->training = 0; e->bn_training = 0; e->seed = 0;
  StepScope scope(e, MMVQA_PREC_F32);
  const size_t n_vis = (size_t)d.num_vis * e->B * d.hidden;
  if (vis != WS(e->vis)) HIP_CHECK_RET(hipMemcpyAsync(WS(e->vis), vis, n_vis * sizeof(float), hipMemcpyDeviceToDevice, st));
  e->prof_reg = REG_EMBED;
  RUN(PROF_OTHER, 0,
      mmvqa_embed_fwd(st, ids, seg, PRM(e->emb_word), PRM(e->emb_pos), PRM(e->emb_type), PRM(e->emb_ln.g),
                  PRM(e->emb_ln.b), WS(e->vis), WS(e->emb_out), WS(e->emb_xhat), WS(e->emb_rstd), e->B, e->T,
                  d.hidden, d.num_vis, 1e-12f, 0.f, site_seed(e, 100, 0)));
  e->prof_reg = REG_BACKBONE;
  const float* h = nullptr;
  TRY(encoder_forward(e, st, &h));
  e->enc_out_final = (size_t)(h - e->ws);
  if (d.head_kind == 2)
    return copy_rows(st, logits, (size_t)logits_ld, h, (size_t)d.hidden, (size_t)e->B * e->T, (size_t)d.hidden);
  return heads_forward(e, st, h);
}

// The forward of a training step from the token cache: the gather writes the workspace's visual
// tokens, then exactly the launches of engine_forward after the backbone, with its dropout probabilities and site seeds.
// Like engine_forward_tokens it leaves the backbone's activations foreign to these tokens (tokens_only: engine_backward and
// engine_backward_feature refuse); unlike it, it keeps `training` and allows engine_backward_cached.
int engine_forward_cached(mmvqa_engine* e, hipStream_t st, const float* cache, int N, int K, const int* idx, const int* view,
                          const long long* ids, const long long* seg, const long long* mask, float* logits, int logits_ld,
                          float* feat, int training, uint32_t seed) {
  if (e->prec != MMVQA_PREC_F32)
    return mmvqa_set_error(MMVQA_ERR_ARG, "engine_forward_cached: runs with fp32 operands, not in the f16 operand mode");
  if (!e->planned || !e->bound) return mmvqa_set_error(MMVQA_ERR_STATE, "engine_forward_cached: plan/bind first");
  if (e->grouped) return mmvqa_set_error(MMVQA_ERR_STATE, "engine_forward_cached: the plan is grouped; plan again with mmvqa_engine_plan");
  const mmvqa_model_desc& d = e->d;
  const int out_w = d.head_kind == 2 ? d.hidden : d.n_classes;
  if (logits_ld < out_w || (logits_ld & 3))
    return mmvqa_set_error(MMVQA_ERR_ARG, "engine_forward_cached: logits_ld=%d must be >= %s=%d and %%4==0", logits_ld,
                           d.head_kind == 2 ? "hidden" : "n_classes", out_w);
  if (N < 1 || K < 1) return mmvqa_set_error(MMVQA_ERR_ARG, "engine_forward_cached: N=%d K=%d must both be at least 1", N, K);
  if ((uintptr_t)cache & 15) return mmvqa_set_error(MMVQA_ERR_ARG, "engine_forward_cached: cache must be 16-byte aligned");
  TRY(prepare_workspace(e, st));
  e->img = nullptr; e->tokens_only = true; e->cached = false;   // (cached: set once every launch below is queued)
  e->ids = ids; e->seg = seg; e->mask = mask;
  e->logits = logits; e->logits_ld = logits_ld; e->feat = feat;
  e->training = training; e->bn_training = 0; e->seed = seed;
  StepScope scope(e, MMVQA_PREC_F32);
  // (the gather belongs to none of the profiler's regions: the regions above the tokens count what they count in a full
  // step; tools/cached_bench.py times it alone)
  TRY(mmvqa_tokens_gather(st, cache, N, K, idx, view, WS(e->vis), e->B, d.hidden, d.num_vis));
  const float pe = training ? d.p_emb_drop : 0.f;
  e->prof_reg = REG_EMBED;
  RUN(PROF_OTHER, 0,
      mmvqa_embed_fwd(st, ids, seg, PRM(e->emb_word), PRM(e->emb_pos), PRM(e->emb_type), PRM(e->emb_ln.g),
                  PRM(e->emb_ln.b), WS(e->vis), WS(e->emb_out), WS(e->emb_xhat), WS(e->emb_rstd), e->B, e->T,
                  d.hidden, d.num_vis, 1e-12f, pe, site_seed(e, 100, 0)));
  e->prof_reg = REG_BACKBONE;
  const float* h = nullptr;
  TRY(encoder_forward(e, st, &h));
  e->enc_out_final = (size_t)(h - e->ws);
  if (d.head_kind == 2)
    TRY(copy_rows(st, logits, (size_t)logits_ld, h, (size_t)d.hidden, (size_t)e->B * e->T, (size_t)d.hidden));
  else
    TRY(heads_forward(e, st, h));
  e->cached = true;
  return MMVQA_OK;
}

// The backward of engine_forward_cached: engine_backward up to and including the embedding, then nothing.  The gradient of
// the visual tokens lands in the workspace and is dropped; the backbone + taps range [emb_hi, enc_lo) of the gradient
// buffer is announced as it stands (as frozen_backbone_backward announces the backbone), so every range is announced once.
int engine_backward_cached(mmvqa_engine* e, hipStream_t st, const float* dlogits, int dl_ld, const float* dfeat) {
  if (!e->planned || !e->bound || !e->cached)
    return mmvqa_set_error(MMVQA_ERR_STATE, "engine_backward_cached: run mmvqa_engine_forward_cached first");
  const mmvqa_model_desc& d = e->d;
  StepScope scope(e, MMVQA_PREC_F32);
  const float* h = WS(e->enc_out_final);
  SideCtx sc_enc(e, st);
  SideReads sr(sc_enc);
  if (d.head_kind == 2) {
    if (dl_ld < d.hidden)
      return mmvqa_set_error(MMVQA_ERR_ARG, "engine_backward_cached: dlogits_ld=%d < hidden=%d", dl_ld, d.hidden);
    TRY(copy_rows(st, WS(e->t_a), (size_t)d.hidden, dlogits, (size_t)dl_ld, (size_t)e->B * e->T, (size_t)d.hidden));
  } else {
    TRY(heads_backward(e, st, h, dlogits, dl_ld, dfeat, sr));
  }
  TRY(encoder_backward(e, st, sr));
  if (e->grad_cb) {
    TRY(sr.join());   // the weight gradients of the range may still be queued on the side stream
    e->grad_cb(e->grad_cb_user, e->enc_lo, e->n_params);   // heads + encoder gradients are final
  }
  const float pe = e->training ? d.p_emb_drop : 0.f;
  e->prof_reg = REG_EMBED;
  RUN(PROF_OTHER, 0,
      mmvqa_embed_bwd(st, WS(e->t_a), e->ids, e->seg, WS(e->emb_xhat), WS(e->emb_rstd), PRM(e->emb_ln.g),
                  GRD(e->emb_word), GRD(e->emb_pos), GRD(e->emb_type), GRD(e->emb_ln.g), GRD(e->emb_ln.b),
                  WS(e->dvis), e->B, e->T, d.hidden, d.num_vis, pe, site_seed(e, 100, 0), 0));
  e->prof_reg = REG_BACKBONE;
  // nothing follows that would join the side stream (engine_backward's backbone does): whatever comes after this
  // backward (Adam, a reduction) sees the weight gradients; the embedding backward above ran beside the last of them
  TRY(sr.join());
  if (e->grad_cb) {
    e->grad_cb(e->grad_cb_user, 0, e->emb_hi);            // embedding tables + LayerNorm
    e->grad_cb(e->grad_cb_user, e->emb_hi, e->enc_lo);    // backbone and taps, as they stand: this backward wrote none of it
  }
  return MMVQA_OK;
}

int engine_backward(mmvqa_engine* e, hipStream_t st, const float* dlogits, int dl_ld, const float* dfeat) {
  if (!e->planned || !e->bound || !e->img) return mmvqa_set_error(MMVQA_ERR_STATE, "engine_backward: run forward first");
  const mmvqa_model_desc& d = e->d;
  if (e->prec != MMVQA_PREC_F32 && d.cnn != 0)
    return mmvqa_set_error(MMVQA_ERR_ARG, "engine_backward: f16 operand mode covers the ResNet encoders only");
  StepScope scope(e, e->prec);
  const float* h = WS(e->enc_out_final);
  SideCtx sc_enc(e, st);
  SideReads sr(sc_enc);
  if (d.head_kind == 2) {
    // the caller's gradient IS dh: it goes where heads_backward leaves it; the head parameters' gradient ranges are not
    // touched and are announced with the encoder's below, as always
    if (dl_ld < d.hidden)
      return mmvqa_set_error(MMVQA_ERR_ARG, "engine_backward: dlogits_ld=%d < hidden=%d", dl_ld, d.hidden);
    TRY(copy_rows(st, WS(e->t_a), (size_t)d.hidden, dlogits, (size_t)dl_ld, (size_t)e->B * e->T, (size_t)d.hidden));
  } else {
    TRY(heads_backward(e, st, h, dlogits, dl_ld, dfeat, sr));
  }
  TRY(encoder_backward(e, st, sr));
  if (e->grad_cb) {
    TRY(sr.join());   // the weight gradients of the range may still be queued on the side stream
    e->grad_cb(e->grad_cb_user, e->enc_lo, e->n_params);   // heads + encoder gradients are final
  }
  const float pe = e->training ? d.p_emb_drop : 0.f;
  e->prof_reg = REG_EMBED;
  RUN(PROF_OTHER, 0,
      mmvqa_embed_bwd(st, WS(e->t_a), e->ids, e->seg, WS(e->emb_xhat), WS(e->emb_rstd), PRM(e->emb_ln.g),
                  GRD(e->emb_word), GRD(e->emb_pos), GRD(e->emb_type), GRD(e->emb_ln.g), GRD(e->emb_ln.b),
                  WS(e->grouped ? e->dvis_q : e->dvis), e->B, e->T, d.hidden, d.num_vis, pe, site_seed(e, 100, 0), 0));
  if (e->grouped)   // the gradient of an image's token: the sum over its questions
    RUNB(HB_NONE, 4.0 * d.num_vis * (e->B + e->NI) * d.hidden,
         mmvqa_dvis_group_sum(st, WS(e->dvis_q), reinterpret_cast<const int*>(WS(e->grp)) + e->B, WS(e->dvis), e->NI, e->B,
                              d.hidden, d.num_vis));
  e->prof_reg = REG_BACKBONE;
  if (e->grad_cb) e->grad_cb(e->grad_cb_user, 0, e->emb_hi);            // embedding tables + LayerNorm
  if (e->frozen & MMVQA_FREEZE_BACKBONE) return frozen_backbone_backward(e, st);
  return d.cnn == 1 ? effnet_backward(e, st) : resnet_backward(e, st);
}

// The deepest backbone feature map A (the one map that feeds nothing but its own tap) and the index of that tap =
// the visual-token row it fills: ResNet layer4 -> conv2 -> row 0, EfficientNet last block (o[4]) -> conv7 -> row 4.
static int feature_tap(const mmvqa_engine* e, size_t* off, int* H, int* W, int* C) {
  if (e->d.cnn == 1) { const EffBlock& b = e->eff.back(); *off = b.out; *H = b.OH; *W = b.OW; *C = b.cout; return 4; }
  const BlockRef& b = e->blocks.back(); *off = b.out; *H = b.OH; *W = b.OW; *C = b.c3.Cout; return 0;
}

int engine_feature_map(mmvqa_engine* e, const float** A, int* H, int* W, int* C) {
  if (!e->planned || !e->bound) return mmvqa_set_error(MMVQA_ERR_STATE, "engine_feature_map: plan/bind and run a forward first");
  if (e->grouped) return mmvqa_set_error(MMVQA_ERR_STATE, "engine_feature_map: attribution on a grouped plan is not built; plan again with mmvqa_engine_plan");
  size_t off = 0; int h = 0, w = 0, c = 0;
  (void)feature_tap(e, &off, &h, &w, &c);
  if (A) *A = WS(off);
  if (H) *H = h;
  if (W) *W = w;
  if (C) *C = c;
  return MMVQA_OK;
}

// Gradient of sum(dlogits * logits) with respect to the deepest feature map, after an eval-mode forward: the data
// gradients of heads -> encoder -> one visual-token row -> one tap, on the caller's stream alone.  The eval forward
// already leaves everything this reads (attention probabilities, LayerNorm statistics, pre-activations: nothing in the
// forward is conditional on `training` except dropout probabilities and BatchNorm statistics).  Parameters, gradient
// buffer and BatchNorm buffers are not written.
int engine_backward_feature(mmvqa_engine* e, hipStream_t st, const float* dlogits, int dl_ld, float* dA) {
  if (e->planned && e->grouped)
    return mmvqa_set_error(MMVQA_ERR_STATE, "engine_backward_feature: attribution on a grouped plan is not built; plan again with "
                                            "mmvqa_engine_plan and run an eval-mode forward");
  if (e->planned && e->bound && e->tokens_only)
    return mmvqa_set_error(MMVQA_ERR_STATE, "engine_backward_feature: the last forward ran from given visual tokens, so the "
                                            "feature map in the workspace is not theirs; run an eval-mode forward first");
  if (!e->planned || !e->bound || !e->img)
    return mmvqa_set_error(MMVQA_ERR_STATE, "engine_backward_feature: run an eval-mode forward first");
  if (e->training)
    return mmvqa_set_error(MMVQA_ERR_STATE, "engine_backward_feature: the last forward ran in training mode (dropout and batch "
                                            "statistics couple the samples); run an eval-mode forward first");
  if (e->prec != MMVQA_PREC_F32)
    return mmvqa_set_error(MMVQA_ERR_ARG, "engine_backward_feature: attribution runs with fp32 operands, not in the f16 operand mode");
  const mmvqa_model_desc& d = e->d;
  if (d.head_kind == 2) return mmvqa_set_error(MMVQA_ERR_ARG, "engine_backward_feature: the headless model has no logits");
  if (!dlogits || !dA) return mmvqa_set_error(MMVQA_ERR_ARG, "engine_backward_feature: null pointer");
  if (dl_ld < d.n_classes || (dl_ld & 3))
    return mmvqa_set_error(MMVQA_ERR_ARG, "engine_backward_feature: dlogits_ld=%d must be >= n_classes and %%4==0", dl_ld);
  StepScope scope(e, MMVQA_PREC_F32);
  SideCtx sc(e, st, false);
  SideReads sr(sc, true);
  TRY(heads_backward(e, st, WS(e->enc_out_final), dlogits, dl_ld, nullptr, sr));
  TRY(encoder_backward(e, st, sr));
  size_t off = 0; int h = 0, w = 0, C = 0;
  const int k = feature_tap(e, &off, &h, &w, &C);
  // the visual tokens overwrite rows 0..4 after the embedding LayerNorm: dvis[k][b] is row k of sample b, copied
  HIP_CHECK_RET(hipMemcpy2DAsync(WS(e->dvis) + (size_t)k * e->B * d.hidden, (size_t)d.hidden * sizeof(float),
                                 WS(e->t_a) + (size_t)k * d.hidden, (size_t)e->T * d.hidden * sizeof(float),
                                 (size_t)d.hidden * sizeof(float), (size_t)e->B, hipMemcpyDeviceToDevice, st));
  e->prof_reg = REG_BACKBONE;
  return tap_bwd(e, st, k, WS(off), nullptr, dA, EpiOpt(), true);
}

extern "C" int mmvqa_engine_create(const mmvqa_model_desc* desc, mmvqa_engine** out) {
  if (!desc || !out) return mmvqa_set_error(MMVQA_ERR_ARG, "engine_create: null argument");
  const mmvqa_model_desc& d = *desc;
  if (d.hidden % 8 != 0 || d.hidden > 1024 || d.n_layers < 1 || d.num_vis != 5)
    return mmvqa_set_error(MMVQA_ERR_ARG, "engine_create: hidden=%d n_layers=%d num_vis=%d unsupported", d.hidden,
                           d.n_layers, d.num_vis);
  if (d.encoder == 0 && (d.heads < 1 || d.hidden % d.heads != 0))
    return mmvqa_set_error(MMVQA_ERR_ARG, "engine_create: heads=%d does not divide hidden=%d", d.heads, d.hidden);
  if (d.encoder < 0 || d.encoder > 2)
    return mmvqa_set_error(MMVQA_ERR_ARG, "engine_create: encoder=%d (0 = transformer, 1 = realformer, 2 = feedback-transformer)", d.encoder);
  if (d.encoder == 2 && (d.n_layers + 1 > MMVQA_FB_MAX_HIDDENS || d.fb_tokens < 1))
    return mmvqa_set_error(MMVQA_ERR_ARG, "engine_create: feedback-transformer with n_layers=%d (at most %d) fb_tokens=%d", d.n_layers,
                           MMVQA_FB_MAX_HIDDENS - 1, d.fb_tokens);
  if (d.cnn == 0 && d.resnet_width % 8 != 0)
    return mmvqa_set_error(MMVQA_ERR_ARG, "engine_create: resnet_width=%d must be a multiple of 8", d.resnet_width);
  if (d.head_kind < 0 || d.head_kind > 2)
    return mmvqa_set_error(MMVQA_ERR_ARG, "engine_create: head_kind=%d (0 = MLM, 1 = VQA, 2 = headless)", d.head_kind);
  mmvqa_engine* e = new mmvqa_engine();
  e->d = d;
  if (d.head_kind == 2) e->d.supcon = 0;   // models/mmbert.py:159-161 returns h alone, whatever args.supcon says
  if (getenv("MMVQA_NO_SIDE_STREAM")) e->use_side = 0;   // A/B switch: everything on the caller's stream
  if (getenv("MMVQA_NO_BN_FOLD")) e->bn_fold = 0;        // A/B switch: separate BatchNorm coefficient launches everywhere
  int r = build_tables(e);
  if (r != MMVQA_OK) { delete e; return r; }
  *out = e;
  return MMVQA_OK;
}

int engine_profile_collect(mmvqa_engine* e) {
  for (auto& r : e->prof) {
    HIP_CHECK_RET(hipEventSynchronize(r.b));
    float ms = 0.f;
    HIP_CHECK_RET(hipEventElapsedTime(&ms, r.a, r.b));
    e->prof_launch[r.cls] += 1;
    e->prof_ms[r.cls] += ms;
    e->prof_flops[r.cls] += r.flops;
    e->reg_launch[r.reg][r.cls] += 1;
    e->reg_ms[r.reg][r.cls] += ms;
    e->reg_flops[r.reg][r.cls] += r.flops;
    if (r.tag > HB_NONE && r.tag < HB_N) { e->tag_launch[r.tag] += 1; e->tag_ms[r.tag] += ms; e->tag_bytes[r.tag] += r.bytes; }
    hipEventDestroy(r.a);
    hipEventDestroy(r.b);
  }
  e->prof.clear();
  return MMVQA_OK;
}
