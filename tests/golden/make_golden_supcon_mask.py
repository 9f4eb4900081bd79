#!/usr/bin/env python3
"""Golden vectors for SupCon with a positive mask, produced by the REFERENCE's own code:

    models/SupConLoss/loss.py:21-98            SupConLoss()(features, mask=m) and (features, labels=y)
    models/SupConLoss/supcon_utils.py:110-138  SimilarityCalculator.jaccard / jaccard_similarity

Run ONCE in the build container:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_supcon_mask.py

Packages the image lacks are NAME-ONLY stubs, as in make_golden_loops.py.  Stored in supcon_mask.npz: the features,
masks and labels, the reference's loss and feature gradient for each, and the Jaccard matrix of a handful of caption /
translation strings (the strings themselves in supcon_mask_texts.json).  Data only.
"""
import argparse
import json
import os
import sys

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
from models.SupConLoss.loss import SupConLoss  # noqa: E402

# caption i against translation j: mixed case, repeated words, tabs and double spaces, an empty caption AND an empty
# translation (pair (4, 5): the empty-union branch), identical texts off the diagonal (caption 1 == translation 2)
CAPTIONS = [
    "Chest X-ray showing a LEFT pleural effusion",
    "axial ct of the abdomen",
    "MRI  of the\tbrain brain Brain with contrast",
    "Ultrasound of the liver, the liver is enlarged",
    "",
    "no acute finding",
]
AUGS = [
    "chest x-ray shows a pleural effusion on the left",
    "Axial CT scan of the  abdomen",
    "axial ct of the abdomen",
    "ultrasound\tof the LIVER , enlarged liver",
    "with contrast: mri of the brain",
    "",
]


def soft_mask(n, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(n, n, generator=g)
    m = m * (torch.rand(n, n, generator=g) < 0.6).float()       # asymmetric, about 40 % zeros
    m.fill_diagonal_(1.0)
    return m


def loss_and_grad(f, **kw):
    f = f.clone().requires_grad_(True)
    l = SupConLoss(temperature=0.07)(f, **kw)
    l.backward()
    return l.detach(), f.grad


def main():
    out = {}
    for tag, n, d, seed in (("a", 5, 16, 31), ("b", 16, 128, 32)):
        g = torch.Generator().manual_seed(seed)
        f = torch.nn.functional.normalize(torch.randn(n, 2, d, generator=g), dim=2)
        m = soft_mask(n, seed + 100)
        y = torch.randint(0, 3, (n,), generator=g)
        lm, gm = loss_and_grad(f, mask=m)
        ly, gy = loss_and_grad(f, labels=y)
        out.update({f"{tag}_feat": f, f"{tag}_mask": m, f"{tag}_labels": y, f"{tag}_loss_mask": lm, f"{tag}_dfeat_mask": gm,
                    f"{tag}_loss_labels": ly, f"{tag}_dfeat_labels": gy})
    calc = SU.SimilarityCalculator(argparse.Namespace(similarity="jaccard"), "cpu")
    out["jaccard"] = calc.jaccard(CAPTIONS, AUGS, len(CAPTIONS))
    MG.save("supcon_mask", **out)
    with open(os.path.join(HERE, "supcon_mask_texts.json"), "w") as fh:
        json.dump({"captions": CAPTIONS, "augs": AUGS}, fh, indent=1)


if __name__ == "__main__":
    main()
