"""Grouped batches without a GPU: the table grouping, the sampler's packing and collate_grouped on a
hand-written table with 1, 3 and 4 questions per image; the host validation of `group`; the refusals of
Model.forward_grouped, of the command line and of mmvqa_engine_plan_grouped."""
import numpy as np
import pytest
import torch

import mmvqa_amd
from mmvqa_amd import _lib as L, data as D, train
from mmvqa_amd.model import group_maps
from oracle import mmbert_oracle as O

T = 12
# (image, question, answer index, category, mode) as data.vqa_tables returns rows; the questions of an image need not be
# adjacent in the table
TABLE = [("a.jpg", "what organ is this", 0, "organ", "train"),
         ("b.jpg", "which plane", 1, "plane", "train"),
         ("a.jpg", "which modality", 2, "modality", "train"),
         ("c.jpg", "what organ is this", 3, "organ", "train"),
         ("b.jpg", "which modality", 2, "modality", "train"),
         ("a.jpg", "which plane", 1, "plane", "train"),
         ("b.jpg", "what is abnormal", 4, "abnormality", "train"),
         ("a.jpg", "what is abnormal", 5, "abnormality", "train")]
SHAPES = {"a.jpg": (6, 4), "b.jpg": (3, 5), "c.jpg": (2, 2)}


class Tok:
    """stands in for the WordPiece tokenizer behind text.encode_text_vqa"""

    def tokenize(self, s):
        return s.split()

    def convert_tokens_to_ids(self, toks):
        return [10 + len(t) for t in toks]


@pytest.fixture
def dataset(monkeypatch):
    def fake_decode(path):
        h, w = SHAPES[path]
        return np.full((h, w, 3), ord(path[0]), dtype=np.uint8)
    monkeypatch.setattr(D, "decode", fake_decode)
    monkeypatch.setattr(D.text, "encode_text_vqa",
                        lambda q, tok, T_: ([len(q)] * T_, [0] * T_, [1] * T_))
    return D.VqaGroupedDataset(TABLE, Tok(), T)


def test_group_rows_by_image():
    assert D.group_rows_by_image(TABLE) == [("a.jpg", [0, 2, 5, 7]), ("b.jpg", [1, 4, 6]), ("c.jpg", [3])]
    assert D.group_rows_by_image([]) == []


def test_dataset_item_and_collate(dataset):
    assert len(dataset) == 3 and dataset.counts() == [4, 3, 1]
    items = [dataset[(0, 2)], dataset[(0, 0)], dataset[(0, 1)]]          # c (1 question), a (4), b (3)
    assert [tuple(it[1].shape) for it in items] == [(1, T), (4, T), (3, T)]
    batch = D.collate_grouped(items)
    assert batch["shapes"].tolist() == [[2, 2], [6, 4], [3, 5]]
    assert batch["pixels"].numel() == 3 * (4 + 24 + 15)
    assert [a.shape for a in D.unpack(batch)] == [(2, 2, 3), (6, 4, 3), (3, 5, 3)]
    for k in ("ids", "seg", "mask"):
        assert tuple(batch[k].shape) == (8, T) and batch[k].dtype == torch.int64
    assert batch["group"].tolist() == [0, 1, 1, 1, 1, 2, 2, 2] and batch["group"].dtype == torch.int64
    assert not batch["group"].is_cuda
    assert batch["index"].tolist() == [3, 0, 2, 5, 7, 1, 4, 6]                # table rows, table order inside an image
    assert batch["target"].tolist() == [TABLE[r][2] for r in batch["index"].tolist()]
    assert batch["ids"][:, 0].tolist() == [len(TABLE[r][1]) for r in batch["index"].tolist()]
    assert "category" not in batch
    group_maps(batch["group"], 3, 8)                                          # what forward_grouped accepts


def test_categories(dataset):
    cats = D.category_ids(TABLE)
    ds = D.VqaGroupedDataset(TABLE, Tok(), T, categories=cats)
    batch = D.collate_grouped([ds[(0, 1)], ds[(0, 0)]])
    assert batch["category"].tolist() == [cats[TABLE[r][3]] for r in batch["index"].tolist()]
    with pytest.raises(ValueError, match="abnormality"):
        D.VqaGroupedDataset(TABLE, Tok(), T, categories={k: v for k, v in cats.items() if k != "abnormality"})


@pytest.mark.parametrize("bs", [4, 5, 7, 8, 100])
def test_sampler_packs_by_questions(bs):
    counts = [4, 3, 1, 4, 1, 3, 4]
    for shuffle in (False, True):
        s = D.GroupedBatchSampler(counts, bs, shuffle, seed=3)
        s.epoch = 2
        batches = [[i for _, i in b] for b in s]
        assert len(batches) == len(s)
        assert sorted(i for b in batches for i in b) == list(range(len(counts)))       # every image once
        assert [i for b in batches for i in b] == s.order() == D.EpochBatchSampler.indices(s)   # in the epoch order
        assert all(b and sum(counts[i] for i in b) <= bs for b in batches)
        # a batch is closed only when the next image would not fit
        for b, nxt in zip(batches, batches[1:]):
            assert sum(counts[i] for i in b) + counts[nxt[0]] > bs
        assert all(e == 2 for b in s for e, _ in b)


def test_sampler_is_a_function_of_seed_epoch_rank():
    counts = [4, 3, 1, 4, 1, 3, 4, 2, 2]

    def draw(seed, epoch, rank):
        s = D.GroupedBatchSampler(counts, 6, True, seed=seed, rank=rank, world=2)
        s.epoch = epoch
        return list(s)
    assert draw(5, 1, 0) == draw(5, 1, 0)
    assert draw(5, 1, 0) != draw(5, 2, 0) and draw(5, 1, 0) != draw(6, 1, 0) and draw(5, 1, 0) != draw(5, 1, 1)
    both = [i for r in (0, 1) for b in draw(5, 1, r) for _, i in b]
    assert set(both) == set(range(len(counts)))                                      # the two shards cover the table


@pytest.mark.parametrize("world", [2, 3, 4])
@pytest.mark.parametrize("bs", [4, 7, 16])
def test_every_rank_runs_the_same_number_of_steps(world, bs):
    """a data-parallel step is one gradient all-reduce: ranks with different numbers of batches would fall out of step.
    Uneven counts, where ranks packing their own image shards would close their batches at different places (at
    batch size 16 and two ranks, the file-order shards of this table pack into 4 and 5 batches)."""
    counts = [4, 3, 4, 4, 1, 4, 3, 3, 4, 2, 4, 4, 3, 4, 1, 1, 4, 4, 3, 4, 4, 4, 2, 4, 3, 4, 4, 4, 1, 4, 4, 3, 4, 4, 4, 4, 3]
    for shuffle in (False, True):
        for epoch in (0, 1, 5):
            ranks = []
            for r in range(world):
                s = D.GroupedBatchSampler(counts, bs, shuffle, seed=11, rank=r, world=world)
                s.epoch = epoch
                ranks.append(s)
            per_rank = [[[i for _, i in b] for b in s] for s in ranks]
            assert len({len(b) for b in per_rank}) == 1, [len(b) for b in per_rank]
            assert all(len(s) == len(b) for s, b in zip(ranks, per_rank))
            whole = ranks[0].all_batches()
            assert all(b.all_batches() == whole for b in ranks)                          # one packing, dealt out
            n = len(per_rank[0])
            dealt = [per_rank[j % world][j // world] for j in range(n * world)]
            assert dealt[:len(whole)] == whole and dealt[len(whole):] == whole[:n * world - len(whole)]   # padded from the head
            assert all(b and sum(counts[i] for i in b) <= bs for bs_ in per_rank for b in bs_)
            assert {i for bs_ in per_rank for b in bs_ for i in b} == set(range(len(counts)))


def test_oversized_image_is_refused(dataset):
    with pytest.raises(ValueError, match="4 questions"):
        D.GroupedBatchSampler([1, 4, 2], 3, False)
    with pytest.raises(ValueError, match="batch_size 3"):
        D.HostLoader(dataset, 3, shuffle=False, num_workers=0, pin_memory=False)
    host = D.HostLoader(dataset, 4, shuffle=False, num_workers=0, pin_memory=False)
    assert [b["group"].tolist() for b, _, _ in host] == [[0, 0, 0, 0], [0, 0, 0, 1]]


def test_host_loader_draws_one_augment_set_per_image(dataset):
    host = D.HostLoader(dataset, 8, shuffle=True, seed=1, num_workers=0, pin_memory=False, aug=D.VQA_AUG, size=16)
    (batch, params, meta), = list(host)
    assert batch["ids"].shape[0] == 8 and batch["shapes"].shape[0] == 3
    assert len(params) == 3                                                          # per image, not per question


@pytest.mark.parametrize("group,NI,B,what", [
    ([0, 1, 1], 2, 4, "3 entries"),                    # wrong length
    ([0, -1, 1], 2, 3, "negative"),
    ([0, 1, 0, 1], 2, 4, "decreases"),
    ([0, 2, 2], 3, 3, "skips"),                        # a gap: image 1 has no question
    ([0, 0, 1], 3, 3, "ends at image 1"),              # the last value is not NI - 1
    ([1, 1, 2], 3, 3, "start at image 0"),
    ([0, 1], 3, 2, "images <= questions"),
    ([0.5, 1], 2, 2, "integers"),
])
def test_malformed_group_raises(group, NI, B, what):
    with pytest.raises(ValueError, match=what):
        group_maps(group, NI, B)
    if all(isinstance(v, int) for v in group):
        with pytest.raises(ValueError, match=what):
            group_maps(torch.tensor(group), NI, B)


def test_group_maps():
    m = group_maps(torch.tensor([0, 1, 1, 1, 2, 2]), 3, 6)
    assert m.dtype == torch.int32 and m.tolist() == [0, 1, 1, 1, 2, 2, 0, 1, 4, 6]
    assert group_maps([0], 1, 1).tolist() == [0, 0, 1]
    assert group_maps(np.array([0, 0, 1]).tolist(), 2, 3).tolist() == [0, 0, 1, 0, 2, 3]
    with pytest.raises(ValueError, match="integer"):
        group_maps(torch.tensor([0.0, 1.0]), 2, 2)


def mini_model():
    args = O.make_args(resnet_layers=(1, 1, 1, 1), resnet_width=8, hidden_size=96, n_layers=2, heads=12, vocab_size=23,
                       emb_vocab=50, bert_max_pos=32, dataset="VQA-Med")
    return mmvqa_amd.Model(args)


def test_forward_grouped_on_cpu_tensors():
    m = mini_model()
    img = torch.zeros(2, 3, 32, 32)
    ids = torch.zeros(3, 10, dtype=torch.long)
    with pytest.raises(L.MMVQAError, match="no CPU fallback"):
        m.forward_grouped(img, [0, 0, 1], ids, ids, ids)
    with pytest.raises(ValueError, match="decreases"):          # the map is validated first, before any device is asked for
        m.forward_grouped(img, [0, 1, 0], ids, ids, ids)
    with pytest.raises(ValueError, match="ends at image 0"):
        m.forward_grouped(img, torch.tensor([0, 0, 0]), ids, ids, ids)


def test_plan_grouped_refusals_and_size():
    m = mini_model()
    lib = L.lib()
    for NI, B in ((0, 4), (5, 4), (-1, 4)):
        assert lib.mmvqa_engine_plan_grouped(m._handle, NI, B, 10, 32, 32) == 0
        err = lib.mmvqa_last_error()
        assert b"plan_grouped" in err and f"NI={NI}".encode() in err, err
    assert lib.mmvqa_engine_plan_grouped(None, 2, 4, 10, 32, 32) == 0
    plain = lib.mmvqa_engine_plan(m._handle, 4, 10, 32, 32)
    same = lib.mmvqa_engine_plan_grouped(m._handle, 4, 4, 10, 32, 32)
    fewer = lib.mmvqa_engine_plan_grouped(m._handle, 2, 4, 10, 32, 32)
    assert plain > 0 and same >= plain                       # NI == B: the same layout plus the grouped buffers
    assert same - plain >= 2 * 5 * 4 * 96 * 4 + (4 + 4 + 1) * 4
    assert 0 < fewer < same                                  # the backbone is laid out for the images
    assert lib.mmvqa_engine_plan(m._handle, 4, 10, 32, 32) == plain   # and planning back gives the old size


def test_command_line():
    for mode in ("vqa", "eval"):
        m, a = train.parse_args([mode, "--group_by_image"])
        assert m == mode and a.group_by_image is True
        assert train.parse_args([mode])[1].group_by_image is False
    for mode in ("mlm", "supcon", "distill", "gradcam"):
        with pytest.raises(SystemExit):
            train.parse_args([mode, "--group_by_image"])
