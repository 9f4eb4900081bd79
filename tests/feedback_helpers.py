"""Oracle of the Feedback-Transformer fusion encoder (models/feedback_transformer_pytorch.py, models/mmbert.py:110-127).

oracle.OracleModel refuses this encoder, so the restatement lives here: `FeedbackBlock` is the reference's class in plain
torch (no einops) with the reference's parameter names and its one shared to_kv weight; tests/test_feedback_cpu.py pins it
to the reference through tests/golden/feedback*.npz.  `OracleFeedback` owns it as `.block` below
oracle.mmbert_oracle._Abstract, and `oracle_model` swaps it into an OracleModel.  With `drop_seed` set the block draws the
engine's dropout masks (DESIGN.md "Dropout stream") instead of torch's."""
import copy

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from dropout_helpers import rng_uniform, site_seed, inject_dropout
from oracle import mmbert_oracle as O

HEADS, DIM_HEAD, MEM_LEN = 8, 64, 256


class _Residual(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x, **kw):
        return self.fn(x, **kw) + x


class _PreNorm(nn.Module):
    def __init__(self, dim, fn):
        super().__init__()
        self.fn = fn
        self.norm = nn.LayerNorm(dim)

    def forward(self, x, **kw):
        return self.fn(self.norm(x), **kw)


class _Bias(nn.Module):
    """RelativePositionBias(causal=True): bucket = max(query - key, 0) for the two query positions a window has."""

    def __init__(self):
        super().__init__()
        self.relative_attention_bias = nn.Embedding(32, HEADS)

    def forward(self, i, j):
        n = (torch.arange(i)[:, None] - torch.arange(j)[None, :]).clamp_min(0)
        assert int(n.max()) < 16   # the exact buckets: a window has at most two queries
        return self.relative_attention_bias(n).permute(2, 0, 1)[None]   # [1, h, i, j]


class _Attention(nn.Module):
    def __init__(self, dim, p):
        super().__init__()
        inner = HEADS * DIM_HEAD
        self.to_q = nn.Linear(dim, inner, bias=False)
        self.to_kv = nn.Linear(dim, 2 * inner, bias=False)
        self.to_out = nn.Linear(inner, dim)
        self.dropout = nn.Dropout(p)

    def forward(self, x, memory=None, pos_emb=None, keep=None):
        B, n, _ = x.shape
        q = self.to_q(x) * DIM_HEAD ** -0.5
        k, v = memory if memory is not None else (None, None)
        if n > 1:
            sk, sv = self.to_kv(x).chunk(2, dim=-1)
            k = sk if k is None else torch.cat((k, sk), 1)
            v = sv if v is None else torch.cat((v, sv), 1)
        q, k, v = (t.view(B, t.shape[1], HEADS, DIM_HEAD).transpose(1, 2) for t in (q, k, v))
        sim = q @ k.transpose(-1, -2)
        j = sim.shape[-1]
        sim = sim + pos_emb(n, j)
        if n > 1:
            mask = torch.ones(n, j).triu_(j - n + 1).bool()
            sim = sim.masked_fill(mask, -torch.finfo(q.dtype).max)
        attn = sim.softmax(-1)
        attn = self.dropout(attn) if keep is None else attn * keep.to(attn.dtype)
        out = (attn @ v).transpose(1, 2).reshape(B, n, HEADS * DIM_HEAD)
        return self.to_out(out)


class _GEGLU(nn.Module):
    def forward(self, x):
        u, gate = x.chunk(2, dim=-1)
        return F.gelu(gate) * u


class _FeedForward(nn.Module):
    def __init__(self, dim, p):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(dim, dim * 8), _GEGLU(), nn.Dropout(p), nn.Linear(dim * 4, dim))

    def forward(self, x, keep=None):
        if keep is None:
            return self.net(x)
        return self.net[3](self.net[1](self.net[0](x)) * keep.to(x.dtype))


def attn_keep(seed, layer, p, B, T, w, n, keys):
    """the engine's mask of the attention probabilities of (layer, window w), scaled: element (b, h, i, j) has index
    ((b*8 + h)*T + 2w + i)*T + j in stream (layer, site 0)"""
    b, h, i, j = np.meshgrid(np.arange(B), np.arange(HEADS), np.arange(n), np.arange(keys), indexing="ij")
    idx = ((b * HEADS + h) * T + 2 * w + i) * T + j
    keep = rng_uniform(site_seed(seed, layer, 0), idx.astype(np.uint32)) >= np.float32(p)
    return torch.from_numpy(keep.astype(np.float64) / (1.0 - p))


def geglu_keep(seed, layer, p, B, w, n, F4):
    """the engine's mask after GEGLU: element (b, i, c) has index (w*2B + b*n + i)*4H + c in stream (layer, site 1)"""
    b, i, c = np.meshgrid(np.arange(B), np.arange(n), np.arange(F4), indexing="ij")
    idx = (w * 2 * B + b * n + i) * F4 + c
    keep = rng_uniform(site_seed(seed, layer, 1), idx.astype(np.uint32)) >= np.float32(p)
    return torch.from_numpy(keep.astype(np.float64) / (1.0 - p))


class FeedbackBlock(nn.Module):
    """FeedbackTransformer(num_tokens, dim, depth, seq_len=2, mem_len=256, heads=8, dim_head=64) applied to float input"""

    def __init__(self, num_tokens, dim, depth, p=0.1):
        super().__init__()
        self.token_emb = nn.Embedding(num_tokens, dim)
        self.pos_emb = _Bias()
        self.layers = nn.ModuleList()
        shared = None
        for _ in range(depth):
            attn = _Attention(dim, p)
            shared = attn.to_kv if shared is None else shared
            attn.to_kv = shared
            self.layers.append(nn.ModuleList([_Residual(_PreNorm(dim, attn)), _Residual(_PreNorm(dim, _FeedForward(dim, p)))]))
        self.layer_weight = nn.Parameter(torch.ones(depth + 1))
        self.shared_kv_proj = shared
        self.to_logits = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, num_tokens))
        self.p = p
        self.drop_seed = None   # set: training-mode dropout draws the engine's masks of a step with this base seed

    def forward(self, x):
        B, T, dim = x.shape
        if T < 2:
            raise ValueError("one token has no keys")
        lw = self.layer_weight.softmax(-1)
        mk = mv = None
        outs = []
        masks = self.drop_seed is not None and self.training and self.p > 0
        for w, x in enumerate(x.split(2, dim=1)):
            n = x.shape[1]
            hiddens = [x]
            memory = None if mk is None else (mk, mv)
            keys = (0 if mk is None else mk.shape[1]) + (n if n > 1 else 0)
            for l, (attn, ff) in enumerate(self.layers):
                ka = attn_keep(self.drop_seed, l, self.p, B, T, w, n, keys) if masks else None
                kf = geglu_keep(self.drop_seed, l, self.p, B, w, n, 4 * dim) if masks else None
                x = attn(x, memory=memory, pos_emb=self.pos_emb, keep=ka)
                x = ff(x, keep=kf)
                hiddens.append(x)
            outs.append(x)
            agg = (torch.stack(hiddens) * lw[:, None, None, None]).sum(0)
            k, v = self.shared_kv_proj(agg).chunk(2, dim=-1)
            mk = k if mk is None else torch.cat((mk, k), 1)
            mv = v if mv is None else torch.cat((mv, v), 1)
            mk, mv = mk[:, -MEM_LEN:], mv[:, -MEM_LEN:]
        return torch.cat(outs, 1)


def seeded_weights(block, seed):
    """weights of a FeedbackBlock from numpy.random.RandomState(seed), in named_parameters() order: the golden generator and
    the test draw the same ones (in the order of the sorted names), so the fixture stores results only"""
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        for name, prm in sorted(block.named_parameters()):
            scale = 1.0 if (name.endswith("norm.weight") or name == "layer_weight") else 0.0
            spread = 0.3 if prm.dim() < 2 else 1.0 / np.sqrt(prm.shape[-1])
            if "relative_attention_bias" in name:
                spread = 1.0
            prm.copy_(torch.from_numpy(scale + spread * rs.standard_normal(tuple(prm.shape))).to(prm.dtype))
    return block


class OracleFeedback(O._Abstract):
    """models/mmbert.py:110-127 (FeedBackTransformer): prepare_input, then the block on the float h; the mask is not used"""

    def __init__(self, args):
        super().__init__(args)
        self.block = FeedbackBlock(args.vocab_size, args.hidden_size, args.n_layers, getattr(args, "fb_dropout_prob", 0.1))

    def forward(self, img, input_ids, token_type_ids, mask):
        return self.block(self.prepare_input(img, input_ids, token_type_ids, mask))


def oracle_model(args, feat_dim=128):
    """OracleModel with the feedback encoder: built for `transformer` (heads, losses, protocol), encoder swapped"""
    a = copy.copy(args)
    a.transformer_model = "transformer"
    m = O.OracleModel(a, feat_dim) if feat_dim != 128 else O.OracleModel(a)
    m.transformer = OracleFeedback(args)
    return m


def inject_feedback_dropout(orc, seed):
    """dropout_helpers.inject_dropout for the sites the other encoders share (the embedding), and the engine's masks for
    the two sites of every feedback layer"""
    for m in orc.modules():
        if isinstance(m, FeedbackBlock):
            m.drop_seed = int(seed)
            for attn, ff in m.layers:            # the block draws the masks itself: these modules are never called with one
                attn.fn.fn.dropout = nn.Identity()
                ff.fn.fn.net[2] = nn.Identity()
    return inject_dropout(orc, seed)
