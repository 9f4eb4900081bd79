#!/usr/bin/env python3
"""Golden vectors for the label-smoothing criteria of the VQA-Med loop, produced by the REFERENCE's own classes:

    vqamed2019/utils.py:1234-1300  LabelSmoothByCategory (training branch, eval branch, computeCategoryTensors)
    vqamed2019/utils.py:178-200    LabelSmoothing (fed the one-hot target its training branch multiplies by, :172-175)

Run ONCE in the build container:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_label_smoothing.py

Packages the image lacks are NAME-ONLY stubs, as in make_golden_loops.py.  The train frame of each case lists the five
categories in the order the reference hard-codes (plane, modality, binary, organ, abnormality, utils.py:1292-1293), gives
`organ` a single answer, shares one answer between two categories and leaves the last answer indices out of every train
row.  The batch holds targets inside their category's answer set, targets of another category, and targets no train row
has.  Stored in label_smoothing.npz per case (C = 23, C = 1552): the frame (category names, answers), logits, targets,
categories, the reference's five table rows, the training-branch loss with its autograd gradient, the eval-branch loss,
and the same three for LabelSmoothing.  Data only.
"""
import os
import sys

import numpy as np
import pandas as pd
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
sys.modules["nltk.translate.bleu_score"].sentence_bleu = lambda *a, **k: 0.0
sys.modules["torchvision"].models = sys.modules["torchvision.models"]
stub("sentence_transformers", SentenceTransformer=object, util=object)
stub("googletrans", Translator=object)
stub("bert_score", BERTScorer=object)
sys.modules["torchvision.models"].resnet152 = lambda **kw: None
sys.path.insert(0, os.path.join(MG.REF, "vqamed2019"))
import importlib  # noqa: E402

VU = importlib.import_module("vqamed2019.utils")

ORDER = ["plane", "modality", "binary", "organ", "abnormality"]      # utils.py:1292-1293
SMOOTHING = 0.1


def frame(C):
    """(category, answer) rows: the categories first appear in ORDER; organ has ONE answer; one `binary` answer (9 / 61)
    also occurs in a modality row; the last answers (C - 1 at C = 23, 1500.. at C = 1552) are in no row"""
    if C == 23:
        sets = {"plane": [0, 1, 2, 3], "modality": [4, 5, 6, 7, 8, 4, 9], "binary": [9, 10, 9], "organ": [11, 11],
                "abnormality": list(range(12, 22))}
    else:
        sets = {"plane": list(range(0, 16)), "modality": list(range(16, 61)) + [61], "binary": [61, 62], "organ": [63],
                "abnormality": list(range(64, 1500))}
    rows = [(c, sets[c][0]) for c in ORDER]                          # first appearances, in the reference's order
    for c in reversed(ORDER):
        rows += [(c, a) for a in sets[c][1:]]
    return pd.DataFrame({"category": [r[0] for r in rows], "answer": [r[1] for r in rows]}), sets


def main():
    out = {}
    for C, B, scale, seed in ((23, 12, 3.0, 71), (1552, 12, 4.0, 72)):
        df, sets = frame(C)
        assert list(df.category.unique()) == ORDER
        crit = VU.LabelSmoothByCategory(df, C, "cpu", smoothing=SMOOTHING)
        tables = torch.stack([crit.idx2vector[i] for i in range(5)])
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, C, generator=g) * scale
        cat = torch.arange(B) % 5
        tgt = torch.empty(B, dtype=torch.long)
        for b in range(B):
            own = sorted(set(sets[ORDER[int(cat[b])]]))
            other = sorted(set(sets[ORDER[(int(cat[b]) + 1) % 5]]) - set(own))
            # rows 0-4 inside the category's set, 5-9 in another category's, the rest in no train row
            tgt[b] = own[int(torch.randint(0, len(own), (1,), generator=g))] if b < 5 else \
                other[int(torch.randint(0, len(other), (1,), generator=g))] if b < 10 else C - 1
        t = f"c{C}_"
        crit.train()
        xr = x.clone().requires_grad_(True)
        loss = crit(xr, tgt, cat)
        loss.backward()
        crit.eval()
        out.update({t + "train_category": np.array(df.category.tolist()), t + "train_answer": df.answer.to_numpy(),
                    t + "logits": x, t + "target": tgt, t + "category": cat, t + "tables": tables,
                    t + "loss": loss.detach(), t + "dlogits": xr.grad, t + "eval_loss": crit(x, tgt, cat).detach()})
        uni = VU.LabelSmoothing(smoothing=SMOOTHING)
        uni.train()
        xr = x.clone().requires_grad_(True)
        onehot = torch.stack([VU.onehot(C, int(v)) for v in tgt])
        loss = uni(xr, onehot)
        loss.backward()
        uni.eval()
        out.update({t + "uniform_loss": loss.detach(), t + "uniform_dlogits": xr.grad,
                    t + "uniform_eval_loss": uni(x, tgt).detach()})
    out["smoothing"] = np.float64(SMOOTHING)
    MG.save("label_smoothing", **out)


if __name__ == "__main__":
    main()
