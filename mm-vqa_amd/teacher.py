"""The frozen BERT teacher on the device (C ABI: mmvqa_bert_* in include/mmvqa.h, csrc/teacher.cpp).

Two of the reference's recipes run a stock HF BertModel (`args.clinicalbert`) beside the model:
  --task distillation   pretrain/roco_utils.py:112-132: the target of a caption is last_hidden_state[1:len-1]
  --similarity cosine   models/SupConLoss/supcon_utils.py:92-97, 140-159: the positive mask is the cosine of the mean
                        hidden state of caption and translation, the mean taken over ALL padded positions
and a third scores the token states of an inner layer (BERTScorer, supcon_utils.py:103-108, 170-182):
  --similarity bert_score   the positive mask is the BERTScore F1 of caption against translation: forward(layer=N) and
                        bertscore_mask below (csrc/bertscore.hip), the library's greedy matching restated

BertTeacher is that model, forward only: post-LN layers, absolute positions, erf GELU, no pooler, token type 0.  Its
weights are one flat fp32 buffer; it has no parameters (nothing for an optimiser), its state_dict() is empty (the
reference keeps the teacher in the dataset / the SimilarityCalculator and never saves it), and it belongs to no Model.
"""
from __future__ import annotations

import ctypes as C
import re

import torch

from . import _lib as L
from .checkpoint import read_state_dict

MAX_T = 512


def _canonical(sd):
    """HF names without a `bert.` / `module.` prefix, LayerNorm.gamma / beta as weight / bias; pooler, heads (cls.*) and
    the position_ids buffer dropped"""
    out = {}
    for k, v in sd.items():
        if not torch.is_tensor(v):
            continue
        k = k.replace("LayerNorm.gamma", "LayerNorm.weight").replace("LayerNorm.beta", "LayerNorm.bias")
        for p in ("module.", "bert."):
            if k.startswith(p):
                k = k[len(p):]
        if k.startswith(("pooler.", "cls.")) or k.endswith("position_ids"):
            continue
        if k.startswith(("embeddings.", "encoder.layer.")):
            out[k] = v
    return out


class BertTeacher(torch.nn.Module):
    def __init__(self, layers, hidden, inter, vocab, max_pos, type_vocab=2, eps=1e-12):
        super().__init__()
        if hidden % 64 != 0 or hidden < 64:
            raise ValueError(f"BertTeacher: hidden = {hidden} is not a multiple of 64 (the attention kernel's head dimension)")
        d = L.BertDesc(int(layers), int(hidden), int(hidden) // 64, int(inter), int(vocab), int(max_pos), int(type_vocab),
                       float(eps))
        lib = L.lib()
        h = C.c_void_p()
        L.check(lib.mmvqa_bert_create(C.byref(d), C.byref(h)))
        self._handle = h
        self.layers, self.hidden, self.heads, self.inter = d.layers, d.hidden, d.heads, d.inter
        self.vocab, self.max_pos, self.type_vocab, self.eps = d.vocab, d.max_pos, d.type_vocab, float(eps)
        self._specs = {}
        name = C.create_string_buffer(256)
        nd, shape, off = C.c_int(), (C.c_longlong * 2)(), C.c_longlong()
        for i in range(lib.mmvqa_bert_num_tensors(h)):
            L.check(lib.mmvqa_bert_tensor_info(h, i, name, 256, C.byref(nd), C.byref(shape), C.byref(off)))
            self._specs[name.value.decode()] = (off.value, tuple(shape[k] for k in range(nd.value)))
        self.register_buffer("flat", torch.zeros(lib.mmvqa_bert_param_floats(h), dtype=torch.float32), persistent=False)
        self._ws = None
        self._bound = None

    def __del__(self):
        try:                                            # (at interpreter exit torch's own globals may be gone already)
            h = self.__dict__.pop("_handle", None)
            if h is not None and h.value:
                L.lib().mmvqa_bert_destroy(h)
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def tensor_names(self):
        return list(self._specs)

    def tensor(self, name):
        """view of one HF-named tensor inside the flat buffer"""
        off, shape = self._specs[name]
        n = 1
        for s in shape:
            n *= s
        return self.flat[off:off + n].view(shape)

    @classmethod
    def from_state_dict(cls, path_or_dict, eps=1e-12):
        """from a local HF BertModel / BertForMaskedLM state dict (.bin / .pt / .safetensors or a dict).  The geometry is
        read from the tensors' shapes; a `bert.` prefix, gamma / beta names and a pooler are accepted and ignored."""
        sd = _canonical(read_state_dict(path_or_dict))
        emb = ("embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight",
               "embeddings.token_type_embeddings.weight")
        l0 = "encoder.layer.0.intermediate.dense.weight"
        missing = [k for k in emb + (l0,) if k not in sd]
        if missing:
            raise KeyError(f"BertTeacher: no tensors {missing} in the state dict (a HF BertModel is expected)")
        vocab, hidden = sd[emb[0]].shape
        idx = {int(m.group(1)) for m in (re.match(r"encoder\.layer\.(\d+)\.", k) for k in sd) if m}
        layers = max(idx) + 1
        if hidden % 64 != 0:
            raise ValueError(f"BertTeacher: hidden = {hidden} is not a multiple of 64 (the attention kernel's head dimension)")
        t = cls(layers, hidden, sd[l0].shape[0], vocab, sd[emb[1]].shape[0], sd[emb[2]].shape[0], eps)
        missing = [k for k in t._specs if k not in sd]
        if missing:
            raise KeyError(f"BertTeacher: the state dict lacks {missing[:5]} ({len(missing)} tensors)")
        bad = [(k, tuple(sd[k].shape), s) for k, (_, s) in t._specs.items() if tuple(sd[k].shape) != s]
        if bad:
            raise ValueError(f"BertTeacher: shapes differ (name, checkpoint, expected): {bad[:5]}")
        with torch.no_grad():
            for k in t._specs:
                t.tensor(k).copy_(sd[k].to(torch.float32))
        return t

    @classmethod
    def random(cls, layers, hidden, inter, vocab, max_pos, seed=0, type_vocab=2, eps=1e-12):
        """a seeded random teacher (HF's initialisation: normal(0, 0.02), LayerNorm near identity) for synthetic runs"""
        t = cls(layers, hidden, inter, vocab, max_pos, type_vocab, eps)
        g = torch.Generator().manual_seed(int(seed))
        with torch.no_grad():
            for k in t._specs:
                v = t.tensor(k)
                if k.endswith("LayerNorm.weight"):
                    v.copy_(1.0 + 0.05 * torch.randn(v.shape, generator=g))
                elif k.endswith("LayerNorm.bias") or k.endswith(".bias"):
                    v.copy_(0.02 * torch.randn(v.shape, generator=g))
                else:
                    v.copy_(0.02 * torch.randn(v.shape, generator=g))
        return t

    def hf_state_dict(self):
        """copies of the weights under their HF names (tests, export)"""
        return {k: self.tensor(k).detach().clone() for k in self._specs}

    # ------------------------------------------------------------------ forward
    def _check(self, ids, lens):
        if not self.flat.is_cuda:
            raise L.MMVQAError("BertTeacher: GPU tensors only (no CPU fallback); move the teacher with .to(device)")
        if not torch.is_tensor(ids) or ids.dtype != torch.int64 or ids.dim() != 2:
            raise ValueError("BertTeacher: `ids` must be an int64 tensor [B, T]")
        B, T = ids.shape
        if not torch.is_tensor(lens) or lens.dtype != torch.int32 or tuple(lens.shape) != (B,):
            raise ValueError(f"BertTeacher: `lens` must be an int32 tensor [{B}]")
        if ids.device != self.flat.device or lens.device != self.flat.device:
            raise ValueError(f"BertTeacher: `ids` and `lens` must be on the teacher's device {self.flat.device}")
        if B < 1 or T < 1 or T > min(MAX_T, self.max_pos):
            raise ValueError(f"BertTeacher: B = {B}, T = {T}: T must lie in 1..min({MAX_T}, max_pos = {self.max_pos})")
        return B, T

    def _plan(self, B, T):
        lib = L.lib()
        key = (B, T, self.flat.data_ptr())
        if self._bound == key:
            return
        need = lib.mmvqa_bert_plan(self._handle, B, T)
        if need == 0:
            L.check(-1)
        if self._ws is None or self._ws.numel() < need or self._ws.device != self.flat.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.flat.device)
        L.check(lib.mmvqa_bert_bind(self._handle, L.ptr(self.flat), L.ptr(self._ws), self._ws.numel()))
        self._bound = key

    @torch.no_grad()
    def forward(self, ids, lens, layer=None):
        """last_hidden_state [B, T, hidden] of ids int64 [B, T] with per-sample lengths lens int32 [B] (1 <= len <= T;
        positions from len on are padding: never attended to, but their own rows are computed, as HF computes them).
        With layer = N (1..layers) the encoder stops after its first N layers: HF's hidden_states[N], which is what
        BERTScore reads; None runs all layers.  Runs on the current stream; nothing is synchronised.  ids outside the
        vocabulary are not checked."""
        B, T = self._check(ids, lens)
        if layer is not None and not 1 <= int(layer) <= self.layers:
            raise ValueError(f"BertTeacher: layer = {layer} is outside 1..{self.layers} (the checkpoint's depth)")
        self._plan(B, T)
        ids, lens = ids.contiguous(), lens.contiguous()
        out = torch.empty(B, T, self.hidden, dtype=torch.float32, device=self.flat.device)
        if layer is None:
            L.check(L.lib().mmvqa_bert_forward(self._handle, L.stream_ptr(), L.ptr(ids), L.ptr(lens), B, T, L.ptr(out)))
        else:
            L.check(L.lib().mmvqa_bert_forward_layers(self._handle, L.stream_ptr(), L.ptr(ids), L.ptr(lens), B, T, int(layer),
                                                      L.ptr(out)))
        return out

    @torch.no_grad()
    def sentence_means(self, ids, lens):
        """[B, hidden]: the plain mean of the hidden states over all T positions, padded ones included (`f1.mean(1)`,
        supcon_utils.py:147).  The reference tokenises a batch with padding=True, so the mean depends on the batch's
        longest text: T must be exactly that length."""
        h = self.forward(ids, lens)
        B, T, H = h.shape
        ones = torch.ones(B, T, dtype=torch.int64, device=h.device)
        out = torch.empty(B, H, dtype=torch.float32, device=h.device)
        L.check(L.lib().mmvqa_meanpool_fwd(L.stream_ptr(), L.ptr(h), L.ptr(ones), L.ptr(out), B, T, H))
        return out


def attention_len_fwd(q, k, v, lens, scale=0.125, out=None):
    """mmvqa_attention_len_fwd on [B, T, heads, 64] fp32 views (unit stride along the last axis, one row stride and one
    head stride shared by q, k and v: separate tensors or slices of one fused [B, T, 3 * hidden] buffer) -> [B, T, heads, 64]"""
    B, T, heads, D = q.shape
    if D != 64 or any(t.dtype != torch.float32 or t.shape != q.shape or t.stride() != q.stride() for t in (q, k, v)):
        raise ValueError("attention_len_fwd: q, k, v must be fp32 [B, T, heads, 64] with equal strides")
    if not q.is_cuda:
        raise L.MMVQAError("attention_len_fwd: GPU tensors only (no CPU fallback)")
    if q.stride(3) != 1 or q.stride(0) != T * q.stride(1):
        raise ValueError("attention_len_fwd: rows must be evenly spaced over [B, T] with unit stride inside a head")
    if lens.dtype != torch.int32 or tuple(lens.shape) != (B,) or lens.device != q.device:
        raise ValueError(f"attention_len_fwd: `lens` must be int32 [{B}] on q's device")
    if out is None:
        out = torch.empty(B, T, heads, 64, dtype=torch.float32, device=q.device)
    L.check(L.lib().mmvqa_attention_len_fwd(L.stream_ptr(), L.ptr(q), L.ptr(k), L.ptr(v), q.stride(1), q.stride(2), L.ptr(out),
                                            out.stride(1), out.stride(2), L.ptr(lens.contiguous()), B, T, heads, float(scale)))
    return out


def cosine_mask_from_means(means, n=None):
    """the cosine mask of SimilarityCalculator.bert_embedd (supcon_utils.py:140-159) from the 2n mean vectors
    [captions 0..n-1 | translations n..2n-1]: rows to unit length (eps 1e-8), mask[i][j] = <caption i, translation j>,
    unit diagonal.  -> [n, n] fp32.  Runs on the current stream."""
    two_n, D = means.shape
    n = two_n // 2 if n is None else n
    if two_n != 2 * n or means.dtype != torch.float32 or not means.is_cuda:
        raise ValueError("cosine_mask_from_means: `means` must be fp32 [2n, D] on the GPU")
    rows = (two_n + 3) // 4
    table = torch.zeros(rows * 4, D, dtype=torch.float32, device=means.device)   # (row, col) table of mmvqa_cosine_mask
    table[:two_n] = means
    lib = L.lib()
    L.check(lib.mmvqa_normalize_rows(L.stream_ptr(), L.ptr(table), rows * 4, D, 1e-8))
    r = torch.arange(two_n, dtype=torch.int32, device=means.device)
    ra, ca = (r[:n] // 4).contiguous(), (r[:n] % 4).contiguous()
    rb, cb = (r[n:] // 4).contiguous(), (r[n:] % 4).contiguous()
    mask = torch.empty(n, n, dtype=torch.float32, device=means.device)
    L.check(lib.mmvqa_cosine_mask(L.stream_ptr(), L.ptr(table), L.ptr(ra), L.ptr(ca), L.ptr(rb), L.ptr(cb), L.ptr(mask), n, D,
                                  rows))
    return mask


BERTSCORE_EPS = 1e-12      # the library divides by the plain norm; BERT states are far from zero


def normalize_states_(x):
    """rows of fp32 [..., D] to unit length in place (x / max(|x|, 1e-12), mmvqa_normalize_rows); current stream"""
    if x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous():
        raise ValueError("normalize_states_: a contiguous fp32 GPU tensor is expected")
    D = x.shape[-1]
    L.check(L.lib().mmvqa_normalize_rows(L.stream_ptr(), L.ptr(x), x.numel() // D, D, BERTSCORE_EPS))
    return x


def bertscore_mask_unit(xa, lenA, xb, lenB, baseline=0.0, return_pr=False):
    """mmvqa_bertscore_mask on states whose rows are already of unit length (see bertscore_mask)"""
    if xa.dim() != 3 or xb.shape != xa.shape or xa.dtype != torch.float32 or xb.dtype != torch.float32:
        raise ValueError("bertscore_mask: `xa` and `xb` must be fp32 [n, T, D] tensors of one shape")
    if not xa.is_cuda or xb.device != xa.device:
        raise L.MMVQAError("bertscore_mask: GPU tensors only (no CPU fallback)")
    n, T, D = xa.shape
    for ln in (lenA, lenB):
        if not torch.is_tensor(ln) or ln.dtype != torch.int32 or tuple(ln.shape) != (n,) or ln.device != xa.device:
            raise ValueError(f"bertscore_mask: the lengths must be int32 [{n}] tensors on the states' device")
    xa, xb, lenA, lenB = xa.contiguous(), xb.contiguous(), lenA.contiguous(), lenB.contiguous()
    mask = torch.empty(n, n, dtype=torch.float32, device=xa.device)
    pr = torch.empty(2, n, n, dtype=torch.float32, device=xa.device) if return_pr else None
    L.check(L.lib().mmvqa_bertscore_mask(L.stream_ptr(), L.ptr(xa), L.ptr(lenA), L.ptr(xb), L.ptr(lenB), L.ptr(mask),
                                         L.ptr(pr[0]) if return_pr else None, L.ptr(pr[1]) if return_pr else None, n, T, D,
                                         float(baseline)))
    return (mask, pr[0], pr[1]) if return_pr else mask


def bertscore_mask(xa, lenA, xb, lenB, baseline=0.0, return_pr=False):
    """the BERTScore F1 mask of SimilarityCalculator.bert_score (supcon_utils.py:170-182), the library's greedy matching
    restated (idf off, one candidate against one reference): xa / xb fp32 [n, T, D] are the token states of the n
    candidates / references (position 0 [CLS], position len - 1 [SEP]), lenA / lenB int32 [n].  Copies of the states are
    brought to unit length (eps 1e-12); S = all cosines of text i against text j over positions < len, specials
    included as match targets; P / R = the mean over the word pieces 1..len-2 of the row / column maxima; mask[i][j] =
    2PR / (P + R) (NaN -> 0, an empty text -> 0), then (F - baseline) / (1 - baseline) when baseline != 0; unit diagonal.
    -> mask [n, n] fp32, with return_pr also P and R (not rescaled).  Positions >= len are never read by the score
    kernel.  Runs on the current stream; nothing is synchronised."""
    if xa.dtype != torch.float32 or xb.dtype != torch.float32:
        raise ValueError("bertscore_mask: `xa` and `xb` must be fp32 [n, T, D] tensors of one shape")
    if not xa.is_cuda or not xb.is_cuda:
        raise L.MMVQAError("bertscore_mask: GPU tensors only (no CPU fallback)")
    return bertscore_mask_unit(normalize_states_(xa.contiguous().clone()), lenA, normalize_states_(xb.contiguous().clone()),
                               lenB, baseline, return_pr)
