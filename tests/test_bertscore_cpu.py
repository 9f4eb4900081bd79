"""BERTScore without a GPU: hand-worked known answers that anchor the restatement of tests/bertscore_helpers.py (the
library is not installed, so nothing pins it), the host-side refusals of mmvqa_bertscore_mask and
mmvqa_bert_forward_layers, and the command line of `train supcon --supcon_mask bert_score`."""
import ctypes as C
import math

import pytest
import torch

import bertscore_helpers as BH
from mmvqa_amd import train


def e(k, D=8):
    v = torch.zeros(D, dtype=torch.float64)
    v[k] = 1.0
    return v


def text(*rows):
    return torch.stack([torch.as_tensor(r, dtype=torch.float64) for r in rows])


def test_identical_texts_score_one():
    g = torch.Generator().manual_seed(0)
    c = torch.randn(6, 8, generator=g, dtype=torch.float64)
    P, R, F = BH.pair(c, c.clone())
    # every position's best match is itself, cosine 1
    assert abs(float(P) - 1) < 1e-14 and abs(float(R) - 1) < 1e-14 and abs(float(F) - 1) < 1e-14


def test_orthogonal_texts_score_zero():
    # candidate [CLS] w w [SEP] = e0 e1 e2 e3, reference = e4 e5 e6 e7: every cosine is 0, P = R = 0, F = 0/0 -> 0
    P, R, F = BH.pair(text(e(0), e(1), e(2), e(3)), text(e(4), e(5), e(6), e(7)))
    assert float(P) == 0.0 and float(R) == 0.0 and float(F) == 0.0


# candidate: 2 word pieces, reference: 3; the specials are orthogonal to everything (e4..e7), so they match nothing.
#   c1 = e0                 c2 = (0, 3, 4) / 5         (given unnormalised: the restatement divides by the norm)
#   r1 = (1, 1, 0) / sqrt 2 r2 = e2     r3 = e3
#   S (words) = [[1/sqrt 2, 0, 0], [0.6/sqrt 2, 0.8, 0]]
#   row maxima 1/sqrt 2, 0.8             -> P = (1/sqrt 2 + 0.8) / 2
#   column maxima 1/sqrt 2, 0.8, 0       -> R = (1/sqrt 2 + 0.8) / 3
#   with s = 1/sqrt 2 + 0.8: F = 2 (s/2)(s/3) / (5s/6) = 2s/5
CAND = text(e(6), e(0), [0, 3, 4, 0, 0, 0, 0, 0], e(7))
REF = text(e(4), [2, 2, 0, 0, 0, 0, 0, 0], e(2), e(3), e(5))
S_ = math.sqrt(0.5) + 0.8


def test_two_by_three_pieces_by_hand():
    P, R, F = BH.pair(CAND, REF)
    assert abs(float(P) - S_ / 2) < 1e-14 and abs(float(R) - S_ / 3) < 1e-14 and abs(float(F) - 2 * S_ / 5) < 1e-14
    # the same through the batched form, padded with rows that must not matter, and in fp32
    xa, xb = torch.full((2, 6, 8), 7.0, dtype=torch.float64), torch.full((2, 6, 8), -3.0, dtype=torch.float64)
    xa[0, :4], xb[1, :5] = CAND, REF
    xa[1, :3], xb[0, :3] = text(e(6), e(1), e(7)), text(e(4), e(1), e(5))
    la, lb = torch.tensor([4, 3]), torch.tensor([3, 5])
    Pm, Rm, Fm = BH.bertscore(xa, la, xb, lb)
    assert abs(float(Pm[0, 1]) - S_ / 2) < 1e-14 and abs(float(Rm[0, 1]) - S_ / 3) < 1e-14 and abs(float(Fm[0, 1]) - 2 * S_ / 5) < 1e-14
    assert float(Pm[0, 0]) == 1.0 and float(Fm[1, 1]) == 1.0                     # the diagonal is set, not computed
    # text 1 (word e1) against reference 0 (word e1): 1
    assert abs(float(Fm[1, 0]) - 1.0) < 1e-14
    (ref, e_cpu) = BH.cpu_error(xa, la, xb, lb)
    assert e_cpu < 1e-6 and torch.equal(ref[2], Fm)


def test_baseline_rescaling():
    b = 0.25
    _, _, F = BH.pair(CAND, REF, baseline=b)
    assert abs(float(F) - (2 * S_ / 5 - b) / (1 - b)) < 1e-14
    # an empty text scores 0 and is rescaled like every other score
    _, _, F0 = BH.pair(text(e(6), e(7)), REF, baseline=b)
    assert abs(float(F0) - (0 - b) / (1 - b)) < 1e-14


def test_specials_are_match_targets():
    # the candidate's only word is e0; the reference's [CLS] is e0 too, its only word is e1.  The word's best match is
    # the [CLS]: P = 1.  Were the specials no targets, P would be 0.
    P, R, F = BH.pair(text(e(6), e(0), e(7)), text(e(0), e(1), e(5)))
    assert float(P) == 1.0 and float(R) == 0.0 and float(F) == 0.0


def test_specials_carry_no_weight():
    ref = text(e(4), e(1), e(5))
    P0, R0, _ = BH.pair(text(e(6), e(0), e(7)), ref)          # the [CLS] row e6 matches nothing
    P1, R1, _ = BH.pair(text(e(1), e(0), e(7)), ref)          # the [CLS] row e1 now matches the reference's word with 1
    assert float(P0) == float(P1) == 0.0                      # its own best match is not averaged: P is unchanged
    assert float(R0) == 0.0 and float(R1) == 1.0              # but as a target it raises the reference word's recall


def test_empty_text_scores_zero():
    for c, r in ((text(e(6), e(7)), REF), (CAND, text(e(4), e(5))), (text(e(6), e(7)), text(e(4), e(5)))):
        P, R, F = BH.pair(c, r)
        assert float(P) == 0.0 and float(R) == 0.0 and float(F) == 0.0


def test_bad_lengths_give_nan_rows_and_columns():
    xa, xb = BH.positive_states(3, 5, 64, seed=1)
    P, R, F = BH.bertscore(xa, torch.tensor([1, 4, 5]), xb, torch.tensor([3, 6, 5]))
    nan = torch.isnan(F)
    want = torch.tensor([[False, True, True], [False, False, False], [False, True, False]])
    assert torch.equal(nan, want) and torch.equal(torch.isnan(P), want)


def test_host_refusals_without_a_gpu():
    from mmvqa_amd import _lib as L
    lib = L.lib()
    p = 0x1000                                            # never dereferenced: every call is refused first
    ok = dict(xa=p, lenA=p, xb=p, lenB=p, mask=p, prec=None, rec=None, n=4, T=16, D=128, baseline=0.0)
    bad = [dict(xa=None), dict(xb=None), dict(lenA=None), dict(lenB=None), dict(mask=None), dict(prec=p), dict(rec=p),
           dict(n=0), dict(n=65536), dict(T=1), dict(T=513), dict(D=32), dict(D=96), dict(D=1088), dict(xa=p + 4), dict(xb=p + 8)]
    for change in bad:
        a = {**ok, **change}
        rc = lib.mmvqa_bertscore_mask(None, a["xa"], a["lenA"], a["xb"], a["lenB"], a["mask"], a["prec"], a["rec"], a["n"],
                                      a["T"], a["D"], a["baseline"])
        assert rc == -1 and lib.mmvqa_last_error().startswith(b"bertscore_mask: "), (change, rc, lib.mmvqa_last_error())
    # the teacher at a layer: a depth outside 1..layers is refused before anything else is looked at
    d = L.BertDesc(2, 64, 1, 128, 30, 16, 2, 1e-12)
    h = C.c_void_p()
    assert lib.mmvqa_bert_create(C.byref(d), C.byref(h)) == 0
    try:
        for nl in (0, 3, -1):
            assert lib.mmvqa_bert_forward_layers(h, None, p, p, 1, 8, nl, p) == -1
            assert b"bert_forward_layers: n_layers=" in lib.mmvqa_last_error()
    finally:
        lib.mmvqa_bert_destroy(h)


def test_train_bert_score_arguments(capsys):
    tw = ["--teacher_weights", "w.pt", "--teacher_vocab_file", "v.txt"]
    base = ["supcon", "--data_dir", "x"]
    bad = (
        (base + ["--supcon_mask", "bert_score"], "invalid choice"),
        (base + ["--supcon_mask", "bert_score", "--teacher_weights", "w.pt"], "invalid choice"),
        (["supcon", "--supcon_mask", "bert_score"] + tw, "needs --data_dir"),
        (base + ["--supcon_mask", "cosine", "--bert_score_layer", "8"] + tw, "bert_score only"),
        (base + ["--supcon_mask", "jaccard", "--bert_score_baseline", "0.3"], "bert_score only"),
        (["supcon", "--bert_score_layer", "8"], "bert_score only"),
        (base + ["--supcon_mask", "bert_score", "--bert_score", "bert"] + tw, "BPE"),
        (base + ["--supcon_mask", "bert_score", "--bert_score", "bert"] + tw, "baseline file"),
        (base + ["--supcon_mask", "bert_score", "--bert_score", "roberta"] + tw, "invalid choice"),
        (base + ["--supcon_mask", "bert_score", "--bert_score_layer", "0"] + tw, "at least 1"),
        (base + ["--supcon_mask", "bert_score", "--bert_score_baseline", "1.0"] + tw, "below 1"),
        (base + ["--supcon_mask", "jaccard"] + tw, "cosine only"),
    )
    for argv, msg in bad:
        with pytest.raises(SystemExit) as ex:
            train.parse_args(argv)
        assert ex.value.code == 2 and msg in capsys.readouterr().err, argv
    mode, a = train.parse_args(base + ["--supcon_mask", "bert_score", "--teacher_lower_case"] + tw)
    assert mode == "supcon" and a.supcon_mask == "bert_score" and a.bert_score_layer == 8 and a.bert_score_baseline == 0.0
    mode, a = train.parse_args(base + ["--supcon_mask", "bert_score", "--bert_score", "scibert", "--bert_score_layer", "3",
                                       "--bert_score_baseline", "0.4", "--similarity", "bert_score"] + tw)
    assert a.bert_score_layer == 3 and a.bert_score_baseline == 0.4 and a.bert_score == "scibert"
    mode, a = train.parse_args(["supcon", "--bert_score", "scibert"])                # accepted and not read
    assert a.supcon_mask == "none" and a.bert_score_layer is None
