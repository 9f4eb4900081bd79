"""Shared pieces of the BERT-teacher tests: a plain-torch restatement of HF's BertModel forward (no pooler) in any
dtype, written independently of mmvqa_amd, the float64 attention the kernel is compared with, and the fixture."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F


def load(golden_dir, name="teacher"):
    return dict(np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False))


def fixture_state_dict(fx, dtype=torch.float32):
    """the fixture's weights (stored as float16, every value fp16-representable) under their HF names"""
    return {k[2:].replace("__", "."): torch.from_numpy(v.astype(np.float32)).to(dtype) for k, v in fx.items() if k.startswith("w_")}


def attention_ref(q, k, v, lens, scale=0.125):
    """softmax(q k^T scale over keys j < len[b]) v for [B, T, heads, D] tensors, in their dtype; every query row i < T
    is computed; a len outside [1, T] gives NaN rows"""
    B, T, nh, D = q.shape
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    keep = torch.arange(T)[None, :] < torch.as_tensor(lens).long()[:, None]          # [B, T]
    s = s.masked_fill(~keep[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    out = torch.einsum("bhij,bjhd->bihd", p, v)
    for b, n in enumerate(lens):
        if not 1 <= int(n) <= T:
            out[b] = float("nan")
    return out


def bert_forward(sd, ids, lens, eps=1e-12, dtype=torch.float32):
    """last_hidden_state [B, T, hidden] of HF BertModel (post-LN layers, absolute positions, erf GELU, token type 0) from
    a state dict with HF names; keys j >= len[b] are masked out, padded query rows are computed.  Heads of width 64."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    B, T = ids.shape
    H = sd["embeddings.word_embeddings.weight"].shape[1]
    nh = H // 64
    x = (sd["embeddings.word_embeddings.weight"][ids] + sd["embeddings.token_type_embeddings.weight"][0]
         + sd["embeddings.position_embeddings.weight"][:T][None])
    x = F.layer_norm(x, (H,), sd["embeddings.LayerNorm.weight"], sd["embeddings.LayerNorm.bias"], eps)
    i = 0
    while f"encoder.layer.{i}.attention.self.query.weight" in sd:
        p = f"encoder.layer.{i}."
        lin = lambda t, n: F.linear(t, sd[p + n + ".weight"], sd[p + n + ".bias"])   # noqa: E731
        q = lin(x, "attention.self.query").view(B, T, nh, 64)
        k = lin(x, "attention.self.key").view(B, T, nh, 64)
        v = lin(x, "attention.self.value").view(B, T, nh, 64)
        ctx = attention_ref(q, k, v, lens, 1.0 / math.sqrt(64.0)).reshape(B, T, H)
        y = F.layer_norm(lin(ctx, "attention.output.dense") + x, (H,), sd[p + "attention.output.LayerNorm.weight"],
                         sd[p + "attention.output.LayerNorm.bias"], eps)
        f = lin(y, "intermediate.dense")
        f = f * 0.5 * (1.0 + torch.erf(f / math.sqrt(2.0)))
        x = F.layer_norm(lin(f, "output.dense") + y, (H,), sd[p + "output.LayerNorm.weight"], sd[p + "output.LayerNorm.bias"],
                         eps)
        i += 1
    return x


def random_state_dict(layers, hidden, inter, vocab, max_pos, seed, type_vocab=2):
    """HF-named random weights at HF's initialisation scale, LayerNorm near identity"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: 0.02 * torch.randn(*s, generator=g)   # noqa: E731
    sd = {"embeddings.word_embeddings.weight": r(vocab, hidden), "embeddings.position_embeddings.weight": r(max_pos, hidden),
          "embeddings.token_type_embeddings.weight": r(type_vocab, hidden),
          "embeddings.LayerNorm.weight": 1.0 + 0.05 * torch.randn(hidden, generator=g), "embeddings.LayerNorm.bias": r(hidden)}
    for i in range(layers):
        p = f"encoder.layer.{i}."
        for n, (o, k) in (("attention.self.query", (hidden, hidden)), ("attention.self.key", (hidden, hidden)),
                          ("attention.self.value", (hidden, hidden)), ("attention.output.dense", (hidden, hidden)),
                          ("intermediate.dense", (inter, hidden)), ("output.dense", (hidden, inter))):
            # projections large enough for attention to be far from uniform
            sd[p + n + ".weight"] = (0.08 if "self" in n else 0.02) * torch.randn(o, k, generator=g)
            sd[p + n + ".bias"] = r(o)
        for n in ("attention.output.LayerNorm", "output.LayerNorm"):
            sd[p + n + ".weight"] = 1.0 + 0.05 * torch.randn(hidden, generator=g)
            sd[p + n + ".bias"] = r(hidden)
    return sd


def pad_ids(rows, T=None):
    """list of id lists -> (int64 [B, T] zero-padded, int32 lens [B])"""
    T = max(len(r) for r in rows) if T is None else T
    ids = torch.zeros(len(rows), T, dtype=torch.int64)
    for b, r in enumerate(rows):
        ids[b, :len(r)] = torch.as_tensor(r, dtype=torch.int64)
    return ids, torch.tensor([len(r) for r in rows], dtype=torch.int32)
