#!/usr/bin/env python3
"""Golden vectors of the distillation task, produced by the REFERENCE's own functions:

    distill_text.npz   pretrain/roco_utils.py:112-132, 162-199   encode_text(..., task='distillation')
    loop_distill.npz   pretrain/roco_utils.py:207-290            train_one_epoch with task='distillation', nn.MSELoss

Run ONCE in the build container:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_distill.py

The stubs are make_golden_loops.py's.  The tokenizer is HF's BertTokenizer on tests/golden/text_vocab.txt; the stand-in
`clinicalbert` returns (E[input_ids],) for a seeded E [vocab, 768]: the teacher's state of a token is then a function of
its id alone, which is all encode_text's layout needs.  The loop runs the reference Model (task='distillation': it returns
the encoder output, models/mmbert.py:159-161) for two Adam steps, once per encoder, on batches whose dense target is the
gather of a small teacher table (stored with start / count, the form the hot path reads).  The same loop is run again in
float64; the generator asserts that the fp32 run stays well inside the cap the replay test applies.  Data only.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden_loops as ML  # noqa: E402  (registers the stubs, imports the reference's roco_utils as ML.RU)
from make_golden_loops import MG, O, RU, synth, LR, PICK_COMMON, Recorder, sample  # noqa: E402
from transformers import BertTokenizer  # noqa: E402

D = 768
WORDS = ("heart liver kidney spleen lung lungs bone fracture mass lesion nodule opacity effusion pleural pneumonia edema "
         "tumor cyst normal abnormal axial coronal sagittal contrast enhanced patient year old male female").split()


def distill_text():
    vocab = [t for t in open(os.path.join(HERE, "text_vocab.txt"), encoding="utf-8").read().split("\n") if t]
    tok = BertTokenizer(vocab={t: i for i, t in enumerate(vocab)})
    g = torch.Generator().manual_seed(97)
    E = torch.randn(len(vocab), D, generator=g)
    teacher = lambda input_ids, attention_mask, output_hidden_states=True: (E[input_ids],)   # noqa: E731
    captions = [" ".join(WORDS[:n]) for n in (0, 1, 4, 5, 24, 26)]      # pieces: 0, 1, T - 8 and more, for T = 12 and 32
    arrs = dict(captions=np.array(captions), cls_id=tok.cls_token_id, sep_id=tok.sep_token_id, vocab=len(vocab), Ts=[12, 32])
    for c, cap in enumerate(captions):
        a = types.SimpleNamespace(task="distillation", max_token_length=512, num_vis=5, max_position_embeddings=32)
        pieces, states = RU.distillation(cap, tok, teacher, a)          # what the file format holds per caption
        assert len(pieces) == (0, 1, 4, 5, 24, 26)[c]
        arrs[f"ids{c}"] = np.asarray(tok.convert_tokens_to_ids(pieces), dtype=np.int64)
        arrs[f"states{c}"] = states.reshape(-1, D)
        for T in (12, 32):
            a.max_position_embeddings = T
            tokens, seg, mask, labels = RU.encode_text(cap, tok, None, a, teacher)
            assert tokens.shape == (T,) and labels.shape == (T, D)
            arrs[f"tokens{c}_{T}"], arrs[f"seg{c}_{T}"], arrs[f"mask{c}_{T}"] = tokens, seg, mask
            arrs[f"labels{c}_{T}"] = labels
    MG.save("distill_text", **arrs)


def dense_target(table, start, count, T, first=7):
    """the target of roco_utils.py:196-197 from a table of states"""
    out = torch.zeros(len(start), T, table.shape[1], dtype=table.dtype)
    for b in range(len(start)):
        n = min(int(count[b]), T - first - 1)
        out[b, first:first + n] = table[int(start[b]):int(start[b]) + n]
    return out


def run_loop(tm, batches, dtype):
    V = 64
    kw = dict(transformer_model=tm, dataset="roco", task="distillation", hidden_size=D, n_layers=2, heads=12,
              hidden_dropout_prob=0.0, vocab_size=V, resnet_layers=(1, 1, 1, 1), resnet_width=64, bert_max_pos=32,
              use_relu=False, cnn_encoder="resnet152")
    args = O.make_args(**kw)
    torch.manual_seed(61)
    orc = O.OracleModel(args)
    ref = MG.build_ref_model(args, orc)
    MG.zero_dropout(ref)
    ref = ref.to(dtype)
    start_sd = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    loader = [(img.to(dtype), ids.unsqueeze(1), seg, mask.unsqueeze(1), dense_target(table, st, ct, ids.shape[1]).to(dtype))
              for (img, ids, seg, mask, st, ct), table in batches]
    crit = Recorder(torch.nn.MSELoss())                                      # roco_train.py:94-95
    opt = torch.optim.Adam(ref.parameters(), lr=LR)                          # roco_train.py:90
    a = types.SimpleNamespace(mixed_precision=False, task="distillation")
    mean_loss, total_acc = RU.train_one_epoch(loader, ref, crit, opt, None, "cpu", a, 0)
    assert total_acc is None                                                 # roco_utils.py:287-288
    return ref, crit.values, float(mean_loss), start_sd


def loop_distill():
    B, T, hw, V = 3, 12, 64, 64
    batches = [synth.distill_batch(B, T, hw, vocab=V, D=D, seed=170 + i) for i in range(2)]
    arrs = dict(seed=61, dims=[B, T, hw, V], lr=LR, total_acc_is_none=True)
    for i, ((img, ids, seg, mask, st, ct), table) in enumerate(batches):
        for n, t in zip(("img", "ids", "seg", "mask", "start", "count", "table"), (img, ids, seg, mask, st, ct, table)):
            arrs[f"{n}{i}"] = t
    extra = {"transformer": ["transformer.blocks.norm1.weight", "transformer.blocks.attention.1.proj_v.weight"],
             "realformer": ["transformer.mains.0.kqv.weight", "transformer.mains.1.ln2.weight"]}
    for tm in ("transformer", "realformer"):
        ref, losses, mean_loss, start_sd = run_loop(tm, batches, torch.float32)
        ref64, losses64, _, _ = run_loop(tm, batches, torch.float64)
        sd, sd64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
        for k in ("fc1.weight", "classifier.2.weight"):                      # no gradient: Adam leaves them alone
            assert torch.equal(sd[k].detach(), start_sd[k]), k
        for i in range(2):                                                   # a third of the replay's 1e-3
            assert abs(losses[i] - losses64[i]) <= (1e-3 / 3) * abs(losses64[i]), (tm, i, losses[i], losses64[i])
        arrs[f"{tm}_losses"], arrs[f"{tm}_mean_loss"] = np.array(losses), mean_loss
        for k in PICK_COMMON + extra[tm]:
            s32, s64 = sample(sd[k]), sample(sd64[k])
            off = ((s32.double() - s64).abs() > 0.5 * LR).double().mean().item()
            assert off <= 0.01, f"{tm} {k}: {off:.4f} of the sampled elements of the fp32 run are off the fp64 run"   # a third of 3 %
            arrs[f"{tm}_p_" + k.replace(".", "__")] = s32
        bsd = ref.state_dict()
        for k in ("transformer.trans.model.bn1.running_mean", "transformer.trans.model.bn1.num_batches_tracked"):
            arrs[f"{tm}_b_" + k.replace(".", "__")] = bsd[k]
    MG.save("loop_distill", **arrs)


if __name__ == "__main__":
    distill_text()
    loop_distill()
