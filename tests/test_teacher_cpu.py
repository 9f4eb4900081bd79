"""The BERT teacher without a GPU: the plain-torch restatement against HF's own output (fixture (a) of
tests/golden/teacher.npz), BertTeacher's constructors, the host-side refusals of mmvqa_attention_len_fwd and mmvqa_bert_*,
the tokenisation and layout of the online distillation data against the reference's distillation() (fixture (b)) and
HF's padded batch (fixture (c)), and the parser rules of the new options."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import teacher_helpers as TH
from mmvqa_amd import _lib as L
from mmvqa_amd import data as D
from mmvqa_amd import train
from mmvqa_amd.teacher import BertTeacher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, "tests", "golden", "text_vocab.txt")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return TH.load(golden_dir)


def test_restatement_against_hf(fx):
    sd = TH.fixture_state_dict(fx)
    ids, lens = torch.from_numpy(fx["a_ids"]), torch.from_numpy(fx["a_lens"])
    e0 = float(fx["e0"])
    r32 = TH.bert_forward(sd, ids, lens, eps=float(fx["eps"]))
    r64 = TH.bert_forward(sd, ids, lens, eps=float(fx["eps"]), dtype=torch.float64)
    assert float((r32 - torch.from_numpy(fx["a_hf"])).abs().max()) <= 2.0 * e0
    assert float((r64 - torch.from_numpy(fx["a_f64"])).abs().max()) <= 1e-12
    assert 1e-7 < e0 < 1e-5 and float(np.abs(fx["a_f64"]).max()) > 2.0
    # an unpadded run of a sample is its padded valid rows
    alone = TH.bert_forward(sd, ids[1:2, :33], lens[1:2], dtype=torch.float64)
    assert float((alone[0] - r64[1, :33]).abs().max()) <= 1e-12


def _variants(sd):
    yield "plain", dict(sd)
    yield "bert. prefix", {"bert." + k: v for k, v in sd.items()}
    yield "gamma / beta", {k.replace("LayerNorm.weight", "LayerNorm.gamma").replace("LayerNorm.bias", "LayerNorm.beta"): v
                           for k, v in sd.items()}
    extra = {"bert." + k: v for k, v in sd.items()}
    extra.update({"bert.pooler.dense.weight": torch.zeros(128, 128), "bert.pooler.dense.bias": torch.zeros(128),
                  "bert.embeddings.position_ids": torch.arange(64)[None], "cls.predictions.bias": torch.zeros(213)})
    yield "pooler, heads and position_ids", extra
    yield "a recorder-style wrapper", {"state_dict": dict(sd)}


def test_from_state_dict_variants_and_refusals(fx, tmp_path):
    sd = TH.fixture_state_dict(fx)
    want = None
    for name, v in _variants(sd):
        t = BertTeacher.from_state_dict(v)
        assert (t.layers, t.hidden, t.heads, t.inter, t.vocab, t.max_pos, t.type_vocab) == (2, 128, 2, 128, 213, 64, 2), name
        want = t.flat.clone() if want is None else want
        assert torch.equal(t.flat, want), name
        for k, w in sd.items():
            assert torch.equal(t.tensor(k), w), (name, k)
    torch.save(sd, tmp_path / "teacher.pt")
    assert torch.equal(BertTeacher.from_state_dict(str(tmp_path / "teacher.pt")).flat, want)
    # query / key / value of a layer lie back to back in the flat buffer: one [3H][H] product
    t = BertTeacher.from_state_dict(sd)
    p = "encoder.layer.1.attention.self."
    o = t._specs[p + "query.weight"][0]
    assert t._specs[p + "key.weight"][0] == o + 128 * 128 and t._specs[p + "value.weight"][0] == o + 2 * 128 * 128
    ob = t._specs[p + "query.bias"][0]
    assert ob == o + 3 * 128 * 128 and t._specs[p + "key.bias"][0] == ob + 128 and t._specs[p + "value.bias"][0] == ob + 256
    assert set(t.tensor_names()) == set(sd) and list(t.parameters()) == [] and t.state_dict() == {}
    # refusals
    lack = {k: v for k, v in sd.items() if k != "encoder.layer.1.output.dense.bias"}
    with pytest.raises(KeyError, match="encoder.layer.1.output.dense.bias"):
        BertTeacher.from_state_dict(lack)
    with pytest.raises(KeyError, match="word_embeddings"):
        BertTeacher.from_state_dict({k: v for k, v in sd.items() if "word_embeddings" not in k})
    with pytest.raises(KeyError):
        BertTeacher.from_state_dict({"fc.weight": torch.zeros(3, 3)})
    odd = TH.random_state_dict(1, 96, 128, 50, 16, seed=1)
    with pytest.raises(ValueError, match="multiple of 64"):
        BertTeacher.from_state_dict(odd)
    bad = dict(sd)
    bad["encoder.layer.0.attention.self.key.weight"] = torch.zeros(128, 64)
    with pytest.raises(ValueError, match="shapes differ"):
        BertTeacher.from_state_dict(bad)
    with pytest.raises(ValueError, match="multiple of 64"):
        BertTeacher.random(1, 100, 128, 50, 16, seed=0)
    # random teachers: seeded, and a CPU forward is refused (no fallback)
    a, b, c = (BertTeacher.random(1, 64, 128, 50, 16, seed=s) for s in (3, 3, 4))
    assert torch.equal(a.flat, b.flat) and not torch.equal(a.flat, c.flat)
    with pytest.raises(L.MMVQAError, match="no CPU fallback"):
        a(torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, dtype=torch.int32))


def test_attention_len_fwd_refuses_bad_arguments_on_the_host():
    lib = L.lib()
    p = 0x1000                                  # never dereferenced: every call is refused before any HIP call
    ok = dict(q=p, k=p, v=p, rs=192, hs=64, out=p, ors=64, ohs=64, len=p, B=2, T=37, heads=1, scale=0.125)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.mmvqa_attention_len_fwd(None, a["q"], a["k"], a["v"], a["rs"], a["hs"], a["out"], a["ors"], a["ohs"], a["len"],
                                         a["B"], a["T"], a["heads"], a["scale"])
        return rc, lib.mmvqa_last_error()

    for kw, what in ((dict(q=None), b"null"), (dict(k=None), b"null"), (dict(v=None), b"null"), (dict(out=None), b"null"),
                     (dict(len=None), b"null"), (dict(B=0), b"B=0"), (dict(T=0), b"T=0"), (dict(heads=0), b"heads=0"),
                     (dict(T=513), b"T=513"), (dict(rs=190), b"multiples of 4"), (dict(hs=62), b"multiples of 4"),
                     (dict(ors=66), b"multiples of 4"), (dict(ohs=2), b"multiples of 4"), (dict(rs=32), b"below the head dimension"),
                     (dict(B=70000), b"65535")):
        rc, err = call(**kw)
        assert rc == -1 and err.startswith(b"attention_len_fwd: ") and what in err, (kw, rc, err)


def test_bert_entry_points_refuse_bad_arguments_on_the_host():
    lib = L.lib()
    good = (2, 128, 2, 128, 50, 64, 2, 1e-12)
    h = C.c_void_p()
    for i, v, what in ((0, 0, b"layers=0"), (1, 96, b"head dimension 64"), (2, 3, b"head dimension 64"), (3, 0, b"inter=0"),
                       (3, 130, b"multiple of 4"), (4, 0, b"vocab=0"), (5, 0, b"max_pos=0"), (6, 0, b"type_vocab=0"),
                       (7, 0.0, b"eps"), (1, 2048, b"1024")):
        f = list(good)
        f[i] = v
        if i == 1 and v % 64 == 0:
            f[2] = v // 64
        d = L.BertDesc(*f)
        rc = lib.mmvqa_bert_create(C.byref(d), C.byref(h))
        assert rc == -1 and lib.mmvqa_last_error().startswith(b"bert_create: ") and what in lib.mmvqa_last_error(), (i, v, lib.mmvqa_last_error())
    assert lib.mmvqa_bert_create(None, C.byref(h)) == -1
    d = L.BertDesc(*good)
    assert lib.mmvqa_bert_create(C.byref(d), C.byref(h)) == 0
    try:
        assert lib.mmvqa_sizeof_bert_desc() == C.sizeof(L.BertDesc) == 32
        n = lib.mmvqa_bert_num_tensors(h)
        assert n == 5 + 2 * 16
        name = C.create_string_buffer(128)
        nd, shape, off = C.c_int(), (C.c_longlong * 2)(), C.c_longlong()
        total = 0
        for i in range(n):
            assert lib.mmvqa_bert_tensor_info(h, i, name, 128, C.byref(nd), C.byref(shape), C.byref(off)) == 0
            assert off.value == total and off.value % 4 == 0 and not name.value.startswith(b"pooler")
            total += shape[0] * (shape[1] if nd.value == 2 else 1)
        assert total == lib.mmvqa_bert_param_floats(h)
        assert name.value == b"encoder.layer.1.output.LayerNorm.bias"
        assert lib.mmvqa_bert_tensor_info(h, n, name, 128, None, None, None) == -1
        p = 0x1000
        assert lib.mmvqa_bert_bind(h, p, p, 1 << 30) == -3 and b"plan first" in lib.mmvqa_last_error()
        assert lib.mmvqa_bert_forward(h, None, p, p, 1, 8, p) == -3
        for B, T in ((0, 8), (1, 0), (1, 65), (70000, 8)):          # T <= min(512, max_pos = 64)
            assert lib.mmvqa_bert_plan(h, B, T) == 0 and b"bert_plan" in lib.mmvqa_last_error(), (B, T)
        need = lib.mmvqa_bert_plan(h, 3, 37)
        assert need >= 3 * 37 * 128 * 4 * (1 + 3 + 1 + 1 + 1 + 1)
        assert lib.mmvqa_bert_bind(h, None, p, need) == -1 and lib.mmvqa_bert_bind(h, p, None, need) == -1
        assert lib.mmvqa_bert_bind(h, p, p, need - 1) == -1 and b"too small" in lib.mmvqa_last_error()
        assert lib.mmvqa_bert_bind(h, p + 4, p, need) == -1 and b"aligned" in lib.mmvqa_last_error()
        assert lib.mmvqa_bert_bind(h, p, p, need) == 0
        for args in ((None, p, 3, 37, p), (p, None, 3, 37, p), (p, p, 3, 37, None), (p, p, 2, 37, p), (p, p, 3, 36, p),
                     (p, p, 3, 37, p + 4)):
            assert lib.mmvqa_bert_forward(h, None, *args) == -1, args
    finally:
        lib.mmvqa_bert_destroy(h)
    big = L.BertDesc(1, 64, 1, 64, 50, 1024, 2, 1e-12)             # more positions than the attention kernel takes
    assert lib.mmvqa_bert_create(C.byref(big), C.byref(h)) == 0
    assert lib.mmvqa_bert_plan(h, 1, 512) > 0 and lib.mmvqa_bert_plan(h, 1, 513) == 0
    lib.mmvqa_bert_destroy(h)


def test_online_distill_dataset_against_the_reference(fx):
    """the teacher's input ids and the student's layout are those of the reference's distillation() + encode_text"""
    tok = D.text.BertWordPiece(VOCAB, do_lower_case=False)
    cls_id, sep_id = int(fx["cls_id"]), int(fx["sep_id"])
    assert (tok.cls_token_id, tok.sep_token_id) == (cls_id, sep_id)
    caps = [str(c) for c in fx["b_captions"]]
    L_, T = int(fx["max_pos"]), 24
    ds = D.OnlineDistillDataset([("img%d.jpg" % i, c) for i, c in enumerate(caps)], tok, 5, T, L_)
    for c in range(len(caps)):
        pieces = fx[f"b_ids{c}"].tolist()
        ids, seg, mask, row = ds.encode(c)
        assert row.dtype == torch.int64 and tuple(row.shape) == (1 + L_,)
        n = len(pieces) + 2
        assert int(row[0]) == n and row[1:1 + n].tolist() == [cls_id] + pieces + [sep_id] and not row[1 + n:].any()
        part2 = pieces[:T - 8]                                                      # roco_utils.py:174-175
        want = [cls_id] + [0] * 5 + [sep_id] + part2 + [sep_id]
        assert ids.tolist() == want + [0] * (T - len(want))
        assert seg.tolist() == [0] * 7 + [1] * (len(part2) + 1) + [0] * (T - len(want))
        assert mask.tolist() == [1] * len(want) + [0] * (T - len(want))
        assert fx[f"b_states{c}"].shape == (len(pieces), 128)
    # a caption of more pieces than the teacher takes is cut at max_token_length - 2 (the reference's tokenize() call
    # asks for that truncation, but its assertion fails on such a caption: there is no reference value to compare with)
    long_ds = D.OnlineDistillDataset([("x.jpg", caps[3] + " heart liver kidney")], tok, 5, T, L_)
    row = long_ds.encode(0)[3]
    assert int(row[0]) == L_ and row[1:].tolist() == [cls_id] + fx["b_ids3"].tolist() + [sep_id]
    with pytest.raises(ValueError, match="max_token_length"):
        D.OnlineDistillDataset([], tok, 5, T, 1)
    # collate: one shape for every batch, the longest length travels on the host
    items = [(np.zeros((4, 4, 3), np.uint8),) + ds.encode(i) + (i,) for i in (1, 2)]
    b = ds.collate(items)
    assert tuple(b["target"].shape) == (2, 1 + L_) and int(b["teacher_T"]) == 8


def test_cosine_mask_tokenisation_matches_hf_padding(fx):
    """list(doc1) + list(doc2) with padding=True: teacher_row of every text, cut at the longest, is HF's input_ids"""
    tok = D.text.BertWordPiece(VOCAB, do_lower_case=False)
    texts = [str(t) for t in fx["c_doc1"]] + [str(t) for t in fx["c_doc2"]]
    rows = torch.stack([D.teacher_row(tok, t, int(fx["max_pos"])) for t in texts])
    ids, lens, Tp = train.teacher_inputs(rows, int(rows[:, 0].max()))
    assert Tp == fx["c_ids"].shape[1] and torch.equal(ids, torch.from_numpy(fx["c_ids"]))
    assert torch.equal(lens, torch.from_numpy(fx["c_lens"])) and lens.dtype == torch.int32
    assert train.teacher_inputs(rows)[2] == Tp                                      # without the host figure: read from the rows
    m = fx["c_ref"]
    assert (np.diag(m) == 1.0).all() and float(fx["e_mask"]) < 2e-6 and m[2, 5] > 0.9 and m.min() < 0.9


def test_parser_rules(capsys):
    tw = ["--teacher_weights", "w.pt", "--teacher_vocab_file", "v.txt"]
    bad = (
        (["distill", "--data_dir", "x"] + tw + ["--teacher_states", "a.npz"], "exclude each other"),
        (["distill", "--data_dir", "x"] + tw + ["--val_teacher_states", "a.npz"], "exclude each other"),
        (["distill"] + tw, "--data_dir only"),
        (["distill", "--data_dir", "x", "--teacher_weights", "w.pt"], "needs both"),
        (["distill", "--data_dir", "x", "--teacher_vocab_file", "v.txt"], "needs both"),
        (["distill", "--data_dir", "x", "--teacher_layers", "2"], "synthetic batches"),
        (["distill", "--teacher_layers", "2", "--hidden_size", "96"], "multiple of 64"),
        (["distill", "--data_dir", "x"], "needs --teacher_states"),                         # the earlier rule stands
        (["distill", "--data_dir", "x"] + tw + ["--max_token_length", "1"], "no room"),
        (["supcon", "--supcon_mask", "cosine"] + tw, "needs --data_dir"),
        (["supcon", "--supcon_mask", "cosine", "--data_dir", "x", "--con_task", "simclr"] + tw, "contradicts"),
        (["supcon", "--supcon_mask", "cosine", "--data_dir", "x"], "--teacher_weights FILE and --teacher_vocab_file FILE"),
        (["supcon", "--supcon_mask", "cosine", "--data_dir", "x", "--teacher_weights", "w.pt"], "--teacher_vocab_file FILE"),
        (["supcon", "--supcon_mask", "jaccard", "--data_dir", "x"] + tw, "cosine only"),
        (["supcon"] + tw, "cosine only"),
        (["mlm"] + tw, "unrecognized arguments"),
    )
    for argv, msg in bad:
        with pytest.raises(SystemExit) as e:
            train.parse_args(argv)
        assert e.value.code == 2 and msg in capsys.readouterr().err, argv
    mode, a = train.parse_args(["distill", "--data_dir", "x"] + tw)
    assert a.max_token_length == 512 and not a.teacher_lower_case and a.teacher_layers == 0 and a.teacher_states is None
    mode, a = train.parse_args(["supcon", "--supcon_mask", "cosine", "--data_dir", "x", "--teacher_lower_case", "--max_token_length", "64"] + tw)
    assert a.supcon_mask == "cosine" and a.teacher_lower_case and a.max_token_length == 64
    mode, a = train.parse_args(["distill", "--teacher_layers", "2", "--hidden_size", "128"])
    assert a.teacher_layers == 2
    mode, a = train.parse_args(["distill"])                                              # defaults unchanged
    assert a.teacher_weights is None and a.teacher_layers == 0
