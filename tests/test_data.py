"""CPU tests of the data layer (mmvqa_amd.data): the ROCO / VQA-Med tables as the reference reads them, the collate
packing, the text tensors, and determinism of the host batches (worker count, reruns, DDP shards)."""
import os
import random

import numpy as np
import pytest
import torch

from feeder_helpers import CAPTIONS, MED_VOCAB, make_roco_tree, make_vqa_tree, tokenizer
from mmvqa_amd import data as D
from mmvqa_amd import text


@pytest.fixture(scope="module")
def roco(tmp_path_factory):
    return make_roco_tree(str(tmp_path_factory.mktemp("roco")))


@pytest.fixture(scope="module")
def vqa(tmp_path_factory):
    return make_vqa_tree(str(tmp_path_factory.mktemp("vqa")))


def test_roco_table_drops_missing_images_and_keeps_captions(roco):
    rows = D.roco_table(roco, "train")
    names = [os.path.basename(p) for p, _ in rows]
    assert names == [f"PMC{1000 + i}_train.jpg" for i in range(18) if i not in (3, 11)]     # order kept
    assert all(os.path.exists(p) for p, _ in rows)
    caps = {c.strip() for c in CAPTIONS}
    assert all(c in caps for _, c in rows)
    assert "MRI of the brain: \"large\" lesion, no edema" in [c for _, c in rows]          # commas and quotes intact
    assert "Axial CT of the chest, showing a mass in the left upper lobe." in [c for _, c in rows]   # stripped
    assert len(D.roco_table(roco, "validation")) == 6
    kw = D.load_keywords(roco)
    assert set(text.get_keywords(MED_VOCAB)) == set(kw) and "lung" in kw


def test_vqa_tables(vqa):
    cols, tabs, idx2ans = D.vqa_tables(vqa)
    assert cols == ["img_id", "question", "answer", "category", "mode"]
    assert [len(tabs[k]) for k in ("train", "val", "test")] == [10, 5, 7]
    seen = []
    for k in ("train", "val", "test"):
        for r in tabs[k]:
            a = idx2ans[r[2]]
            if a not in seen:
                seen.append(a)
            assert a == a.lower() and r[3] == r[3].lower()
    assert [idx2ans[i] for i in range(len(idx2ans))] == seen                   # first-seen order over train+val+test
    assert "liver" in seen and "LIVER" not in seen and "ct" in seen
    p = tabs["test"][2][0]
    assert p == os.path.join(vqa, "Test", "images", "synpictest2.jpg") and os.path.exists(p)
    assert tabs["val"][0][0] == os.path.join(vqa, "Val", "images", "synpicval0.jpg")


def test_collate_round_trip():
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((5, 7), (1, 1), (9, 3))]
    items = [(a, torch.full((4,), n), torch.zeros(4, dtype=torch.long), torch.ones(4, dtype=torch.long),
              torch.tensor(n), 10 + n) for n, a in enumerate(imgs)]
    b = D.collate(items)
    assert b["pixels"].dtype == torch.uint8 and b["pixels"].numel() == sum(a.size for a in imgs)
    assert b["shapes"].tolist() == [[5, 7], [1, 1], [9, 3]] and b["index"].tolist() == [10, 11, 12]
    assert D.offsets(b["shapes"]) == [0, 105, 108]
    for a, u in zip(imgs, D.unpack(b)):
        assert np.array_equal(a, u)
    assert b["ids"].shape == (3, 4) and b["target"].tolist() == [0, 1, 2]


def test_text_tensors_match_text_py(roco, vqa):
    tok, kw = tokenizer(), D.load_keywords(roco)
    rows = D.roco_table(roco, "train")
    ds = D.RocoDataset(rows, tok, kw, num_vis=5, max_position_embeddings=24, mlm_prob=0.5, seed=7)
    for idx in (0, 4, 9):
        _img, ids, seg, mask, tgt, i = ds[(3, idx)]
        ref = text.roco_text_batch([rows[idx][1]], tok, kw, 5, 24, 0.5, rng=D.sample_rng(7, 3, idx))
        for a, r in zip((ids, seg, mask, tgt), ref):
            assert torch.equal(a, r[0])
        assert i == idx
    assert any(int((ds[(0, k)][4] > 0).sum()) > 0 for k in range(len(rows)))   # some keyword was masked
    _c, tabs, _i = D.vqa_tables(vqa)
    vd = D.VqaDataset(tabs["val"], tok, 20)
    for idx in range(3):
        _img, ids, seg, mask, ans, _ = vd[(0, idx)]
        ref = text.vqa_text_batch([tabs["val"][idx][1]], tok, 20)
        for a, r in zip((ids, seg, mask), ref):
            assert torch.equal(a, r[0])
        assert int(ans) == tabs["val"][idx][2]


def _epoch(loader, epoch):
    loader.set_epoch(epoch)
    return [(b, p, m) for b, p, m in loader]


def _same(a, b):
    assert len(a) == len(b)
    for (x, px, mx), (y, py, my) in zip(a, b):
        assert mx == my and px == py
        for k in x:
            assert torch.equal(x[k], y[k]), k


def test_host_batches_are_deterministic(roco):
    tok, kw = tokenizer(), D.load_keywords(roco)
    ds = D.RocoDataset(D.roco_table(roco, "train"), tok, kw, 5, 24, 0.3, seed=11)
    runs = []
    for workers in (0, 2, 2):
        ld = D.HostLoader(ds, 5, shuffle=True, seed=11, num_workers=workers, aug=D.VQA_AUG, size=224, pin_memory=False)
        runs.append([_epoch(ld, 0), _epoch(ld, 1)])
        del ld
    for r in runs[1:]:
        for e in range(2):
            _same(runs[0][e], r[e])
    e0, e1 = runs[0]
    assert [len(b[0]["index"]) for b in e0] == [5, 5, 5, 1]                         # 16 rows: partial last batch kept
    assert sorted(sum((b[0]["index"].tolist() for b in e0), [])) == list(range(16))
    assert [b[0]["index"].tolist() for b in e0] != [b[0]["index"].tolist() for b in e1]   # a new order each epoch
    assert e0[0][1] != e1[0][1] and len(e0[3][1]) == 1                            # params per (epoch, batch)


def test_ddp_shards_are_disjoint_and_cover_the_epoch():
    for n in (16, 17):
        shards = []
        for rank in range(2):
            s = D.EpochBatchSampler(n, 3, True, seed=5, rank=rank, world=2)
            s.epoch = 4
            shards.append([i for b in s for (_e, i) in b])
            assert len(list(iter(s))) == len(s)
        assert len(shards[0]) == len(shards[1]) == -(-n // 2)
        if n % 2 == 0:
            assert not set(shards[0]) & set(shards[1])
        assert set(shards[0]) | set(shards[1]) == set(range(n))
        g = torch.Generator().manual_seed(5 + 4)
        perm = torch.randperm(n, generator=g).tolist()
        perm += perm[:(-n) % 2]
        assert shards[0] == perm[0::2] and shards[1] == perm[1::2]                 # DistributedSampler semantics
    v = D.EpochBatchSampler(7, 3, False)
    assert [[i for _e, i in b] for b in v] == [[0, 1, 2], [3, 4, 5], [6]]


def test_feeder_refuses_cpu():
    ds = D.VqaDataset([], None)
    ld = D.HostLoader(ds, 2, num_workers=0, pin_memory=False)
    with pytest.raises(RuntimeError, match="GPU only"):
        D.DeviceFeeder(ld, "cpu")
