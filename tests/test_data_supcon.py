"""CPU tests of the SupCon data layer (mmvqa_amd.data): the train table with back-translations as
pretrain/roco_supcon_train.py reads it, an item's rng order (supcon_utils.py:218-232), the process_tensors layout of a
collated batch, and the host batches' two-view parameters and determinism."""
import os

import pytest
import torch

from feeder_helpers import make_roco_tree, tokenizer
from mmvqa_amd import augment as AU
from mmvqa_amd import data as D
from mmvqa_amd import text
from supcon_helpers import DROPPED, make_supcon_tree

T = 24


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return make_supcon_tree(str(tmp_path_factory.mktemp("supcon")))


def _dataset(root, seed=5):
    return D.RocoSupConDataset(D.roco_supcon_table(root), tokenizer(), D.load_keywords(root), 5, T, 0.3, seed=seed)


def test_table_drops_missing_images_and_the_three_names(tree):
    root, kept = tree
    rows = D.roco_supcon_table(root)
    assert [os.path.basename(p) for p, _, _ in rows] == [k[0] for k in kept]          # file order
    assert all(os.path.exists(p) for p, _, _ in rows)
    assert not set(DROPPED) & {os.path.basename(p) for p, _, _ in rows}
    assert set(DROPPED) <= set(os.listdir(os.path.join(root, "train", "radiology", "images")))   # dropped by name
    assert [(c, t) for _, c, t in rows] == [(k[1], k[2]) for k in kept]               # columns 3-5 by position, stripped
    assert all(t[0].startswith("fr ") and t[1].startswith("de ") and t[2].startswith("es ") for _, _, t in rows)
    assert len(D.roco_table(root, "train")) == len(rows) + len(DROPPED)              # the mlm table keeps them


def test_table_refuses_short_rows_and_empty_translations(tmp_path):
    root, _ = make_supcon_tree(str(tmp_path / "short"), short_row=1)
    with pytest.raises(ValueError, match=r"traindata\.csv: row 3 .*5 fields"):         # row 3: a dropped name precedes it
        D.roco_supcon_table(root)
    root, _ = make_supcon_tree(str(tmp_path / "empty"), empty_cell=(4, 5))
    with pytest.raises(ValueError, match=r"traindata\.csv: row 7 .*empty translation in column 5"):
        D.roco_supcon_table(root)
    root, _ = make_supcon_tree(str(tmp_path / "missing"), short_row=3)                 # row 3 has no image: never read
    assert len(D.roco_supcon_table(root)) == 7


def test_item_draws_one_rng_in_the_reference_order(tree):
    root, _ = tree
    ds = _dataset(root)
    tok, kw = tokenizer(), D.load_keywords(root)
    picked = set()
    for epoch in (0, 3, 4, 9):
        for idx in range(len(ds)):
            img, ids, aug_ids, seg, mask, tgt, aug_tgt, i = ds[(epoch, idx)]
            _path, caption, trans = ds.rows[idx]
            rng = D.sample_rng(5, epoch, idx)
            r_ids, r_seg, r_mask, r_tgt = text.encode_text(caption, tok, kw, 5, T, 0.3, rng)
            col = rng.randint(3, 5)
            a_ids, _s, _m, a_tgt = text.encode_text(trans[col - 3], tok, kw, 5, T, 0.3, rng)
            picked.add(col)
            assert i == idx and img.dtype.name == "uint8" and img.ndim == 3
            for a, b in ((ids, r_ids), (seg, r_seg), (mask, r_mask), (tgt, r_tgt), (aug_ids, a_ids), (aug_tgt, a_tgt)):
                assert torch.equal(a, b), (epoch, idx)
    assert picked == {3, 4, 5}


def test_collate_is_process_tensors_layout(tree):
    root, _ = tree
    ds = _dataset(root)
    items = [ds[(1, i)] for i in (4, 0, 2)]
    b = D.collate_supcon(items)
    assert b["shapes"].tolist() == [list(it[0].shape[:2]) for it in items]
    assert b["pixels"].numel() == sum(it[0].size for it in items) and b["index"].tolist() == [4, 0, 2]
    assert [tuple(b[k].shape) for k in ("ids", "seg", "mask", "target")] == [(6, T)] * 4
    st = lambda j: torch.stack([it[j] for it in items])   # noqa: E731
    assert torch.equal(b["ids"], torch.cat([st(1), st(2)])) and torch.equal(b["target"], torch.cat([st(5), st(6)]))
    # the caption's seg / mask for both halves (supcon_utils.py:256), even where the translation is longer or shorter
    assert torch.equal(b["seg"], torch.cat([st(3), st(3)])) and torch.equal(b["mask"], torch.cat([st(4), st(4)]))
    assert D.unpack(b)[1].shape == items[1][0].shape
    # the other datasets keep collate
    rd = D.RocoDataset(D.roco_table(root, "validation"), tokenizer(), D.load_keywords(root), 5, T, 0.3)
    assert getattr(rd, "collate", None) is None and D.RocoSupConDataset.collate is D.collate_supcon


def test_host_loader_draws_two_views_per_image(tree):
    root, _ = tree
    host = D.HostLoader(_dataset(root), 3, shuffle=True, seed=11, rank=0, num_workers=0, aug=D.ROCO_AUG, size=224,
                        pin_memory=False, views=2)
    host.set_epoch(2)
    got = list(host)
    assert [b["shapes"].shape[0] for b, _, _ in got] == [3, 3, 1]                      # drop_last=False: a one-pair tail
    for b, params, meta in got:
        n = b["shapes"].shape[0]
        assert b["ids"].shape[0] == 2 * n and len(params) == 2 * n
        ref = AU.sample_params(2 * n, 224, generator=D.batch_generator(11, 2, meta["batch"], 0), **D.ROCO_AUG)
        assert params == ref
    with pytest.raises(ValueError):
        D.HostLoader(_dataset(root), 3, views=0)


def _flat(host, epoch):
    host.set_epoch(epoch)
    return [({k: v.clone() for k, v in b.items()}, p, m) for b, p, m in host]


def test_batches_do_not_depend_on_workers(tree):
    root, _ = tree
    mk = lambda w: D.HostLoader(_dataset(root), 2, shuffle=True, seed=3, num_workers=w, aug=D.ROCO_AUG,   # noqa: E731
                                size=224, pin_memory=False, views=2)
    a, b = _flat(mk(0), 1), _flat(mk(2), 1)
    assert len(a) == len(b) == 4
    for (ba, pa, ma), (bb, pb, mb) in zip(a, b):
        assert ma == mb and pa == pb
        assert all(torch.equal(ba[k], bb[k]) for k in ba)


def test_mlm_tree_without_translations_is_refused(tmp_path):
    root = make_roco_tree(str(tmp_path / "roco"))
    with pytest.raises(ValueError, match=r"traindata\.csv: row 1 .*3 fields"):
        D.roco_supcon_table(root)
