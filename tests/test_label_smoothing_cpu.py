"""Label smoothing by question category (vqamed2019/utils.py:1234-1300, :178-200), everything that needs no GPU: the
fp64 restatement against the reference's own numbers (tests/golden/label_smoothing.npz), the table builder, the host-side
argument checks of mmvqa_soft_ce_loss, the parser, the dataset / collate with the category map."""
import ctypes as C

import numpy as np
import pytest
import torch

import mmvqa_amd
from mmvqa_amd import _lib as L
from mmvqa_amd import data as D
from mmvqa_amd import synth, train
import label_smoothing_helpers as H


@pytest.fixture(scope="module")
def gold():
    return H.fixture()


@pytest.mark.parametrize("Cn", [23, 1552])
def test_restatement_reproduces_the_reference(gold, Cn):
    g, t = gold, f"c{Cn}_"
    sm = float(g["smoothing"])
    x, tgt, cat = (torch.from_numpy(g[t + k]) for k in ("logits", "target", "category"))
    table = torch.from_numpy(g[t + "tables"])
    # the reference ran in fp32: the logits and their log-sum-exp are below 32 in magnitude, where an fp32 ulp is 2^-19;
    # log_softmax rounds there up to four times (x - max, the log-sum, their difference, the exp's argument), and an
    # absolute error of the exponent is a relative error of p = softmax(x), hence of the gradient's largest entries
    tol = 4.0 * 2.0 ** -19
    assert float(x.abs().max()) < 32
    for dtype in (torch.float32, torch.float64):
        for mode, lk, gk in ((H.CATEGORY, "loss", "dlogits"), (H.UNIFORM, "uniform_loss", "uniform_dlogits")):
            soft = H.soft_targets(mode, tgt, Cn, sm, table, cat, dtype)
            loss, grad = H.loss_and_grad(x.to(dtype), soft)
            assert abs(float(loss) - float(g[t + lk])) <= tol * abs(float(g[t + lk])), (mode, dtype)
            ref = torch.from_numpy(g[t + gk]).double()
            assert float((grad.double() - ref).abs().max()) <= tol * float(ref.abs().max()), (mode, dtype)
            closed = H.closed_form_grad(x.double(), soft.double())
            assert float((closed - ref).abs().max()) <= tol * float(ref.abs().max()), (mode, "closed form")
        hard = H.soft_ce(x.to(dtype), H.soft_targets(H.HARD, tgt, Cn, dtype=dtype))
        for k in ("eval_loss", "uniform_eval_loss"):
            assert abs(float(hard) - float(g[t + k])) <= tol * abs(float(g[t + k]))
    # the consequence the kernel must get right: a target inside its category's set is overwritten, the row sums below 1
    soft = H.soft_targets(H.CATEGORY, tgt, Cn, sm, table, cat)
    S = soft.sum(1)
    assert bool((S[:5] < 1.0).all())
    assert float((S[5:] - 1.0).abs().max()) < 1e-6


@pytest.mark.parametrize("Cn", [23, 1552])
def test_category_smoothing_table_is_the_references(gold, Cn):
    g, t = gold, f"c{Cn}_"
    rows = H.fixture_rows(g, Cn)
    crit = mmvqa_amd.CategorySmoothing(rows, Cn, smoothing=float(g["smoothing"]))
    assert crit.categories == H.ORDER
    assert crit.cat2idx == D.category_ids(rows) == {c: i for i, c in enumerate(H.ORDER)}
    assert crit.table.dtype == torch.float32
    assert np.array_equal(crit.table.numpy().view(np.uint32), g[t + "tables"].view(np.uint32))      # bit for bit
    names, table = H.category_table(rows, Cn, float(g["smoothing"]))
    assert names == H.ORDER and torch.equal(table, crit.table)
    assert int((crit.table[3] > 0).sum()) == 1                       # organ: one answer carries the whole smoothing mass
    assert float(crit.table[:, Cn - 1].abs().max()) == 0.0           # an answer of no train row is in no set


def test_empty_category_gives_a_zero_row():
    rows = [("a.jpg", "q", 2, "plane", "train"), ("b.jpg", "q", 0, "organ", "train"), ("c.jpg", "q", 2, "plane", "train")]
    crit = mmvqa_amd.CategorySmoothing(rows, 4, smoothing=0.2, categories=["plane", "binary", "organ"])
    assert crit.categories == ["plane", "binary", "organ"]
    assert torch.equal(crit.table, torch.tensor([[0, 0, 0.2, 0], [0, 0, 0, 0], [0.2, 0, 0, 0]], dtype=torch.float32))
    none = mmvqa_amd.CategorySmoothing([], 4)
    assert none.categories == [] and float(none.table.abs().max()) == 0.0


def test_soft_ce_refuses_inconsistent_arguments_without_gpu():
    lib = L.lib()
    ok = dict(logits=0x1000, ld=24, target=0x2000, category=0x3000, table=0x4000, table_ld=24, n_cat=5, mode=2,
              smoothing=0.1, row_loss=0x5000, loss=0x6000, dlogits=0x7000, dld=24, rows=4, C=23, gscale=0.25)

    def refused(what, **kw):
        a = {**ok, **kw}                      # never dereferenced: every case is refused before a launch
        rc = lib.mmvqa_soft_ce_loss(None, a["logits"], a["ld"], a["target"], a["category"], a["table"], a["table_ld"],
                                    a["n_cat"], a["mode"], a["smoothing"], a["row_loss"], a["loss"], a["dlogits"], a["dld"],
                                    a["rows"], a["C"], a["gscale"])
        assert rc == -1, f"{what}: rc {rc}"
        assert b"soft_ce_loss:" in lib.mmvqa_last_error(), what
        with pytest.raises(L.MMVQAError):
            L.check(rc)

    refused("mode 2 without table", table=None)
    refused("mode 2 without category", category=None)
    refused("ld < C", ld=20)
    refused("table_ld < C", table_ld=22)
    refused("rows = 0", rows=0)
    refused("rows < 0", rows=-3)
    refused("unknown mode", mode=3)
    refused("negative mode", mode=-1)
    refused("dld < C", dld=16)
    refused("n_cat = 0", n_cat=0)
    refused("null logits", logits=None)
    refused("smoothing > 1", smoothing=1.5)


def test_cpu_tensors_are_refused():
    x, t = torch.zeros(2, 5), torch.zeros(2, dtype=torch.long)
    with pytest.raises(mmvqa_amd.MMVQAError, match="no CPU fallback"):
        mmvqa_amd.soft_ce_loss(x, t)
    with pytest.raises(mmvqa_amd.MMVQAError, match="no CPU fallback"):
        mmvqa_amd.LabelSmoothing(0.1)(x, t)
    crit = mmvqa_amd.CategorySmoothing(synth.vqa_category_rows(5), 5)
    with pytest.raises(mmvqa_amd.MMVQAError, match="no CPU fallback"):
        crit(x, t, torch.zeros(2, dtype=torch.long))
    with pytest.raises(ValueError, match="category ids"):
        crit.to("cpu")(x, t)


def test_vqa_parser_accepts_smoothing():
    mode, args = train.parse_args(["vqa", "--smoothing", "0.1", "--loss", "ASLSingleLabel"])
    assert mode == "vqa" and args.smoothing == 0.1
    assert train.parse_args(["vqa"])[1].smoothing is None
    assert train.parse_args(["eval", "--smoothing", "0.2"])[1].smoothing == 0.2
    with pytest.raises(SystemExit):
        train.parse_args(["vqa", "--smoothing", "1.5"])
    with pytest.raises(SystemExit):
        train.parse_args(["mlm", "--smoothing", "0.1"])


def test_synthetic_categories_follow_the_table_partition():
    rows = synth.vqa_category_rows(23)
    crit = mmvqa_amd.CategorySmoothing(rows, 23)
    assert crit.categories == list(synth.VQA_CATEGORIES)
    tgt = synth.vqa_batch(6, 10, 8, vocab=50, n_classes=23, seed=5)[4]
    cat = synth.vqa_categories(6, 23, seed=5)
    assert cat.dtype == torch.int64 and torch.equal(cat, tgt % 5)
    assert bool((crit.table[cat, tgt] > 0).all())                   # every target lies in its category's set


def _dataset_rows(tmp_path):
    from PIL import Image
    rows = []
    for i, (cat, ans) in enumerate([("plane", 0), ("organ", 1), ("plane", 2), ("binary", 3), ("organ", 1)]):
        p = tmp_path / f"im{i}.png"
        Image.fromarray(np.full((4 + i, 5, 3), 10 * i, dtype=np.uint8)).save(p)
        rows.append((str(p), f"what is {i}?", ans, cat, "train"))
    return rows


def test_dataset_and_collate_with_the_category_map(tmp_path, golden_dir):
    import os
    from mmvqa_amd import text
    tok = text.BertWordPiece(os.path.join(golden_dir, "text_vocab.txt"))
    rows = _dataset_rows(tmp_path)
    ids = D.category_ids(rows)
    assert ids == {"plane": 0, "organ": 1, "binary": 2}               # first appearance, row order
    plain = D.VqaDataset(rows, tok, 12)
    withcat = D.VqaDataset(rows, tok, 12, categories=ids)
    items = [plain[(0, i)] for i in range(5)]
    citems = [withcat[(0, i)] for i in range(5)]
    assert all(len(it) == 6 for it in items) and all(len(it) == 7 for it in citems)
    assert [it[6] for it in citems] == [0, 1, 0, 2, 1]
    for a, b in zip(items, citems):                                   # the first six elements are the default item
        assert np.array_equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1:5], b[1:5])) and a[5] == b[5]
    assert getattr(plain, "collate", None) is None and withcat.collate is D.collate_category
    base, cb = D.collate(items), D.collate_category(citems)
    assert set(base) == {"pixels", "shapes", "ids", "seg", "mask", "target", "index"}
    assert set(cb) == set(base) | {"category"}
    assert all(torch.equal(base[k], cb[k]) for k in base)
    assert cb["category"].dtype == torch.int64 and cb["category"].tolist() == [0, 1, 0, 2, 1]
    with pytest.raises(ValueError, match="not in the category map"):
        D.VqaDataset(rows, tok, 12, categories={"plane": 0})
