#!/usr/bin/env python3
"""Golden vectors of the BERT teacher, produced by HF's BertModel and by the REFERENCE's own functions:

    (a) last_hidden_state of a padded batch                 transformers BertModel (what args.clinicalbert loads)
    (b) pretrain/roco_utils.py:112-132                      distillation(caption, tokenizer, clinicalbert, args)
    (c) models/SupConLoss/supcon_utils.py:140-159           SimilarityCalculator.bert_embedd(doc1, doc2, bsz)

Run ONCE in the build container:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_teacher.py

Nothing is downloaded: the model is a seeded BertModel (2 layers, hidden 128, 2 heads, intermediate 128, 64 positions,
no pooler) over tests/golden/text_vocab.txt, its weights rounded to fp16-representable values and stored as float16; the
tokenizer is HF's BertTokenizer on that vocabulary, cased, as the clinical checkpoints are.  The calculator is built with
similarity="jaccard" (the "cosine" constructor calls from_pretrained) and gets .tokenizer / .model / .device by hand.
Packages the image lacks are stubbed as in make_golden_supcon_embed.py.  Beside each fp32 result the float64 value of
tests/teacher_helpers.py's plain-torch restatement is stored, with the distance between the two (e0, e_mask): the bounds
of the GPU tests are multiples of it.  Data only, written to teacher.npz.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

from transformers import BertConfig, BertModel, BertTokenizer, AutoTokenizer, AutoModel  # noqa: E402,F401
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

RU = importlib.import_module("roco_utils")
SU = importlib.import_module("supcon_utils")
import teacher_helpers as TH  # noqa: E402

WORDS = ("heart liver kidney spleen lung lungs bone fracture mass lesion nodule opacity effusion pleural pneumonia edema "
         "tumor cyst normal abnormal axial coronal sagittal contrast enhanced patient year old male female").split()
MAX_POS = 64


def build_model(vocab_size):
    cfg = BertConfig(vocab_size=vocab_size, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128,
                     max_position_embeddings=MAX_POS, type_vocab_size=2, hidden_dropout_prob=0.0,
                     attention_probs_dropout_prob=0.0, layer_norm_eps=1e-12, hidden_act="gelu")
    torch.manual_seed(1234)
    model = BertModel(cfg, add_pooling_layer=False).eval()
    g = torch.Generator().manual_seed(4321)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if not v.is_floating_point():
                continue
            if k.endswith("LayerNorm.weight"):
                v.copy_(1.0 + 0.1 * torch.randn(v.shape, generator=g))
            elif k.endswith(".bias"):
                v.copy_(0.05 * torch.randn(v.shape, generator=g))     # HF starts them at zero: a swapped bias would not show
            elif "embeddings" in k:
                v.copy_(0.5 * torch.randn(v.shape, generator=g))
            elif "attention.self" in k:
                v.copy_(0.12 * torch.randn(v.shape, generator=g))     # scores of a few units: attention far from uniform
            else:
                v.copy_(0.08 * torch.randn(v.shape, generator=g))
            v.copy_((torch.round(v * 1024.0) / 1024.0).half().float())   # fp16-representable, on a 2^-10 grid (the file compresses)
    return model


def main():
    vocab = [t for t in open(os.path.join(HERE, "text_vocab.txt"), encoding="utf-8").read().split("\n") if t]
    tok = BertTokenizer(vocab={t: i for i, t in enumerate(vocab)}, do_lower_case=False, model_max_length=MAX_POS)
    model = build_model(len(vocab))
    sd = {k: v for k, v in model.state_dict().items() if v.is_floating_point()}
    arrs = {"w_" + k.replace(".", "__"): v.half() for k, v in sd.items()}
    for k, v in sd.items():
        assert torch.equal(v.half().float(), v), k
    arrs.update(max_pos=MAX_POS, cls_id=tok.cls_token_id, sep_id=tok.sep_token_id, eps=1e-12)

    # ---------------------------------------------------------------- (a) hidden states of a padded batch
    g = torch.Generator().manual_seed(7)
    lens = [37, 33, 2]
    rows = [[tok.cls_token_id] + torch.randint(5, len(vocab), (n - 2,), generator=g).tolist() + [tok.sep_token_id] for n in lens]
    ids, ln = TH.pad_ids(rows)
    mask = (torch.arange(ids.shape[1])[None] < ln[:, None].long()).long()
    with torch.no_grad():
        hf = model(input_ids=ids, attention_mask=mask).last_hidden_state
        r32 = TH.bert_forward(sd, ids, ln, dtype=torch.float32)
        r64 = TH.bert_forward(sd, ids, ln, dtype=torch.float64)
        alone = model(input_ids=ids[1:2, :33]).last_hidden_state
    e0 = float((hf.double() - r64).abs().max())
    print(f"(a) |out| max {float(r64.abs().max()):.3f}  HF vs restatement fp32 {float((hf - r32).abs().max()):.2e}  "
          f"fp32 vs fp64 e0 {e0:.2e}  unpadded vs padded {float((alone[0] - hf[1, :33]).abs().max()):.2e}")
    assert float((hf - r32).abs().max()) <= 2 * e0
    arrs.update(a_ids=ids, a_lens=ln, a_hf=hf, a_f64=r64, e0=e0)

    # ---------------------------------------------------------------- (b) the reference's distillation()
    a = types.SimpleNamespace(task="distillation", max_token_length=MAX_POS, num_vis=5, max_position_embeddings=MAX_POS)
    # the longest caption has exactly max_token_length - 2 pieces: tokenize() ignores truncation=True / max_length, so one
    # piece more trips distillation()'s own assertion (roco_utils.py:130) -- the reference cannot produce that case
    captions = ["", WORDS[0], " ".join(WORDS[:6]), " ".join((WORDS * 3)[:MAX_POS - 2])]
    try:
        RU.distillation(" ".join((WORDS * 3)[:MAX_POS - 1]), tok, model, a)
        raise SystemExit("the reference now truncates: store the over-long case as well")
    except AssertionError:
        pass
    arrs["b_captions"] = np.array(captions)
    for c, cap in enumerate(captions):
        pieces, states = RU.distillation(cap, tok, model, a)
        states = states.reshape(-1, 128)
        print(f"(b) caption {c}: {len(pieces)} pieces")
        assert len(pieces) == (0, 1, 6, MAX_POS - 2)[c]
        arrs[f"b_ids{c}"] = np.asarray(tok.convert_tokens_to_ids(pieces), dtype=np.int64)
        arrs[f"b_states{c}"] = states

    # ---------------------------------------------------------------- (c) the reference's bert_embedd()
    n = 8
    doc1 = [" ".join(WORDS[i:i + 2 + 3 * i]) for i in range(n)]
    doc2 = [" ".join(WORDS[(2 * i + 3) % 11:(2 * i + 3) % 11 + 1 + (5 * i) % 13]) for i in range(n)]
    doc2[5] = doc1[2]                                   # mask[2][5] is the cosine of a text with itself at another padding
    calc = SU.SimilarityCalculator(argparse.Namespace(similarity="jaccard"), "cpu")     # never "cosine": that downloads
    calc.device, calc.tokenizer, calc.model = "cpu", tok, model
    ref = calc.bert_embedd(doc1, doc2, n).clone()
    enc = tok(list(doc1) + list(doc2), return_tensors="pt", truncation=True, padding=True)
    cids = enc["input_ids"]
    clens = enc["attention_mask"].sum(1).to(torch.int32)
    with torch.no_grad():
        h64 = TH.bert_forward(sd, cids, clens, dtype=torch.float64)
    f = h64.mean(1)
    f = f / f.norm(dim=1, keepdim=True).clamp_min(1e-8)
    m64 = (f[:n] @ f[n:].T).fill_diagonal_(1.0)
    e_mask = float((ref.double() - m64).abs().max())
    print(f"(c) T = {cids.shape[1]}, lens {clens.tolist()}, mask range [{float(m64.min()):.3f}, {float(m64.max()):.3f}], e_mask {e_mask:.2e}")
    arrs.update(c_doc1=np.array(doc1), c_doc2=np.array(doc2), c_ids=cids, c_lens=clens, c_ref=ref, c_f64=m64, e_mask=e_mask)
    MG.save("teacher", **arrs)
    print("bytes", os.path.getsize(os.path.join(HERE, "teacher.npz")))


if __name__ == "__main__":
    main()
