#!/usr/bin/env python3
"""Golden vectors for the SupCon mask from caption sentence embeddings, produced by the REFERENCE's own code:

    models/SupConLoss/supcon_utils.py:140-159  SimilarityCalculator.bert_embedd
        a / max(|a|, 1e-8), b / max(|b|, 1e-8), mm, fill_diagonal_(1) -- what sentence_trans (:162-168) gets from
        util.cos_sim, written out

Run ONCE in the build container:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_supcon_embed.py

No language model is loaded.  The calculator is constructed with similarity="jaccard" (the "cosine" constructor calls
from_pretrained) and its .tokenizer / .model / .device are set by hand to NAME-ONLY stand-ins: the "tokenizer" turns a
list of (row, column) keys into an index tensor, the "model" returns last_hidden_state = E[index][:, None, :], a
sequence of length 1, so that bert_embedd's .mean(1) is exact and everything after it is the reference's arithmetic.
Packages the image lacks are stubbed as in make_golden_supcon_mask.py.  Stored in supcon_embed.npz, per D in {5, 384}:
the embedding table emb_D [6, 4, D], the translation columns drawn cols_D_k [6] and the reference's matrix ref_D_k
[6, 6] of caption i against translation (j, cols[j]).  Data only.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from transformers import BertTokenizer, BertModel, AutoTokenizer, AutoModel  # noqa: E402,F401
import make_golden as MG  # noqa: E402  (stubs torchvision/timm, imports the reference model modules)
from make_golden_text import stub, register_stubs  # noqa: E402

register_stubs()
sys.modules["torchvision"].models = sys.modules["torchvision.models"]
stub("sentence_transformers", SentenceTransformer=object, util=object)
stub("googletrans", Translator=object)
stub("bert_score", BERTScorer=object)
sys.path.insert(0, os.path.join(MG.REF, "pretrain"))
sys.path.insert(0, os.path.join(MG.REF, "models", "SupConLoss"))
import importlib  # noqa: E402

importlib.import_module("roco_utils")               # (supcon_utils does `from roco_utils import encode_text`)
SU = importlib.import_module("supcon_utils")

N = 6
COLS = ([1] * N, [1, 2, 3, 1, 2, 3], [3, 3, 2, 2, 1, 1])


class Keys(dict):
    """what the stand-in tokenizer returns: bert_embedd calls .to(device) on it and splats it into the model"""

    def to(self, _device):
        return self


def table(D, seed):
    """signed embeddings with per-text scales in (0, 3); caption 2 all zero; translation (4, c) = 2.5 x caption 1 for
    every column c, so that mask[1][4] is a cosine of 1 off the diagonal"""
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(N, 4, D, generator=g) * (3.0 * torch.rand(N, 4, 1, generator=g)).clamp_min(0.05)
    e[2, 0] = 0.0
    e[4, 1:] = 2.5 * e[1, 0]
    return e


def main():
    calc = SU.SimilarityCalculator(argparse.Namespace(similarity="jaccard"), "cpu")     # never "cosine": that downloads
    out = {}
    for D, seed in ((5, 51), (384, 52)):
        E = table(D, seed)
        flat = E.reshape(N * 4, D)
        calc.device = "cpu"
        calc.tokenizer = lambda keys, **_kw: Keys(index=torch.tensor([r * 4 + c for r, c in keys]))
        calc.model = _Model(flat)
        out[f"emb_{D}"] = E
        for k, cols in enumerate(COLS):
            captions = [(i, 0) for i in range(N)]
            augs = [(j, cols[j]) for j in range(N)]
            out[f"cols_{D}_{k}"] = np.asarray(cols, dtype=np.int32)
            out[f"ref_{D}_{k}"] = calc.bert_embedd(captions, augs, N).clone()
    MG.save("supcon_embed", **out)


class _Model:
    """stand-in for the language model: one "token" per text whose hidden state is the text's embedding"""

    def __init__(self, flat):
        self.flat = flat

    def eval(self):
        return self

    def __call__(self, index):
        return types.SimpleNamespace(last_hidden_state=self.flat[index][:, None, :])


if __name__ == "__main__":
    main()
