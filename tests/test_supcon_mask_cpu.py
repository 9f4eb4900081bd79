"""CPU tests of SupCon with caption-similarity positives: the masked oracle restatement against the reference's
fixture, the host word-set CSR against the reference's Jaccard matrix (bit-equal), argument handling of supcon_loss and
of `train supcon --supcon_mask`, the dataset's aug_col report, and the global mask / masked loss over two gloo ranks."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import mmvqa_amd
from feeder_helpers import tokenizer
from mmvqa_amd import data as D
from mmvqa_amd import train
from supcon_helpers import make_supcon_tree
from supcon_mask_helpers import fixture, fixture_texts, jaccard_strings, labels_mask, soft_mask, supcon_masked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_helper_equals_the_reference_fixture(tag):
    g = fixture()
    for kind in ("mask", "labels"):
        f = torch.from_numpy(g[f"{tag}_feat"]).requires_grad_(True)
        m = torch.from_numpy(g[f"{tag}_mask"]) if kind == "mask" else labels_mask(torch.from_numpy(g[f"{tag}_labels"]))
        l = supcon_masked(f, m)
        l.backward()
        lerr = abs(float(l.detach()) - float(g[f"{tag}_loss_{kind}"]))
        gerr = float((f.grad - torch.from_numpy(g[f"{tag}_dfeat_{kind}"])).abs().max())
        print(f"{tag} {kind}: loss err {lerr:.2e} grad err {gerr:.2e}")
        assert lerr < 1e-6 and gerr < 1e-5
    m = torch.from_numpy(g[f"{tag}_mask"])
    assert not torch.equal(m, m.T) and bool((m.diagonal() == 1).all()) and bool(((m > 0) & (m < 1)).any())


def test_word_sets_give_the_reference_jaccard_matrix_bit_equal():
    caps, augs, rows = fixture_texts()
    ref = fixture()["jaccard"]
    assert ref.dtype == np.float32 and ref[4, 5] == 0.0 and ref[1, 2] == 1.0       # empty union; identical off-diagonal
    assert np.array_equal(jaccard_strings(caps, augs), ref)
    ws = D.WordSets.from_texts(rows)
    assert ws.offsets.dtype == torch.int32 and ws.ids.dtype == torch.int32 and ws.offsets.numel() == 4 * len(rows) + 1
    idx = list(range(len(rows)))
    for cols in ([1] * 6, [1, 2, 3, 1, 2, 3], [3, 3, 2, 2, 1, 1]):
        got = ws.jaccard_host(idx, [0] * 6, idx, cols)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), cols
    # sets are sorted, unique, lower-cased; ids are exact (one per distinct word of the table)
    w = ws.word_ids(2, 0)
    assert list(w) == sorted(set(w)) and len(w) == len(set(caps[2].lower().split())) == 6
    assert len(ws.vocab) == len({x for r in rows for t in r for x in t.lower().split()})
    assert ws.word_ids(4, 0).size == 0
    with pytest.raises(ValueError):
        D.WordSets.from_texts([("a", "b", "c")])
    perm = [3, 0, 5, 1]                                    # a batch is any (row, col) selection, diagonal by position
    got = ws.jaccard_host(perm, [0] * 4, perm, [2] * 4)
    assert np.array_equal(got, jaccard_strings([caps[i] for i in perm], [augs[i] for i in perm]))


def test_supcon_loss_argument_handling():
    f = torch.zeros(4, 2, 8)
    with pytest.raises(ValueError, match="Cannot define both `labels` and `mask`"):
        mmvqa_amd.supcon_loss(f, labels=torch.zeros(4, dtype=torch.long), mask=torch.eye(4))
    with pytest.raises(ValueError, match="mask"):
        mmvqa_amd.supcon_loss(f, mask=torch.eye(5))
    with pytest.raises(ValueError, match="mask"):
        mmvqa_amd.supcon_loss(f, mask=torch.ones(4))
    with pytest.raises(ValueError, match="labels"):
        mmvqa_amd.supcon_loss(f, labels=torch.zeros(3, dtype=torch.long))
    with pytest.raises(mmvqa_amd.MMVQAError):              # no CPU fallback on either path
        mmvqa_amd.supcon_loss(f, mask=torch.eye(4))
    with pytest.raises(mmvqa_amd.MMVQAError):
        mmvqa_amd.supcon_loss(f)


def test_masked_entry_points_refuse_bad_arguments_on_the_host():
    from mmvqa_amd import _lib as L
    lib = L.lib()
    p = 0x1000                                              # never dereferenced: every call is refused first
    for args in ((None, p, p, p, p, 4, 8), (p, None, p, p, p, 4, 8), (p, p, None, p, p, 4, 8), (p, p, p, p, None, 4, 8),
                 (p, p, p, p, p, 0, 8), (p, p, p, p, p, -3, 8), (p, p, p, p, p, 4, 257), (p, p, p, p, p, 4, 0)):
        assert lib.mmvqa_supcon_loss_masked(None, *args, 0.07, 0.07, 1.0) == -1, args
        assert b"supcon_masked" in lib.mmvqa_last_error()
    for args in ((None, p, p, p, p, p, p, 4, 9), (p, None, p, p, p, p, p, 4, 9), (p, p, None, p, p, p, p, 4, 9),
                 (p, p, p, p, p, None, p, 4, 9), (p, p, p, p, p, p, None, 4, 9), (p, p, p, p, p, p, p, 0, 9),
                 (p, p, p, p, p, p, p, 4, 0)):
        assert lib.mmvqa_jaccard_mask(None, *args) == -1, args
        assert b"jaccard_mask" in lib.mmvqa_last_error()


def test_train_supcon_mask_arguments(capsys):
    for bad, msg in ((["supcon", "--supcon_mask", "jaccard"], "needs --data_dir"),
                     (["supcon", "--supcon_mask", "jaccard", "--data_dir", "x", "--con_task", "simclr"], "contradicts"),
                     (["supcon", "--supcon_mask", "cosine", "--data_dir", "x"], "invalid choice")):
        with pytest.raises(SystemExit) as e:
            train.parse_args(bad)
        assert e.value.code == 2 and msg in capsys.readouterr().err, bad
    mode, a = train.parse_args(["supcon", "--similarity", "jaccard", "--con_task", "supcon"])
    assert mode == "supcon" and a.supcon_mask == "none" and a.similarity == "jaccard"      # the unmasked path, as before
    mode, a = train.parse_args(["supcon", "--supcon_mask", "jaccard", "--data_dir", "x"])
    assert a.supcon_mask == "jaccard"
    with pytest.raises(SystemExit):
        train.parse_args(["mlm", "--supcon_mask", "jaccard", "--data_dir", "x"])          # a supcon option only


def test_dataset_reports_the_drawn_column_only_when_asked(tmp_path):
    root, _ = make_supcon_tree(str(tmp_path / "t"))
    table, tok, kw = D.roco_supcon_table(root), tokenizer(), D.load_keywords(root)
    off = D.RocoSupConDataset(table, tok, kw, 5, 24, 0.3, seed=5)
    on = D.RocoSupConDataset(table, tok, kw, 5, 24, 0.3, seed=5, report_aug_col=True)
    assert off.collate is D.collate_supcon and on.collate is D.collate_supcon_cols
    keys = {"pixels", "shapes", "ids", "seg", "mask", "target", "index"}
    picked = set()
    for epoch in (0, 2, 7):
        items_off = [off[(epoch, i)] for i in range(len(off))]
        items_on = [on[(epoch, i)] for i in range(len(on))]
        assert all(len(it) == 8 for it in items_off) and all(len(it) == 9 for it in items_on)
        assert len(on.encode(epoch, 0)) == 6
        b_off, b_on = off.collate(items_off), on.collate(items_on)
        assert set(b_off) == keys and set(b_on) == keys | {"aug_col", "row"}
        assert all(torch.equal(b_off[k], b_on[k]) for k in keys)
        assert b_on["aug_col"].dtype == torch.int32 and b_on["row"].dtype == torch.int32
        assert b_on["row"].tolist() == b_on["index"].tolist()
        for i, it in enumerate(items_on):
            rng = D.sample_rng(5, epoch, i)                 # documented order: caption masking, column, translation masking
            D.text.encode_text(table[i][1], tok, kw, 5, 24, 0.3, rng)
            col = rng.randint(3, 5)
            assert it[8] == col - 2 == b_on["aug_col"][i].item()
            a_ids = D.text.encode_text(table[i][2][col - 3], tok, kw, 5, 24, 0.3, rng)[0]
            assert torch.equal(it[2], a_ids)
            picked.add(it[8])
    assert picked == {1, 2, 3}
    ws = D.WordSets.from_table(table)                       # column c of the word sets is the text column c drew from
    assert ws.rows == len(table)
    for r in (0, 3):
        for c in (1, 2, 3):
            assert len(ws.word_ids(r, c)) == len(set(table[r][2][c - 1].lower().split()))
        assert len(ws.word_ids(r, 0)) == len(set(table[r][1].lower().split()))


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mmvqa_amd.ddp import global_supcon_pairs, global_supcon_views
        from supcon_mask_helpers import random_word_sets, supcon_masked as oracle
        n, Dm = 3, 16
        ws, _ = random_word_sets(20, [5, 9, 0, 12, 7], 24, seed=3)
        g = torch.Generator().manual_seed(11)
        rows_all = torch.randperm(20, generator=g)[:n * world].to(torch.int32)
        cols_all = torch.randint(1, 4, (n * world,), generator=g).to(torch.int32)
        full = torch.nn.functional.normalize(torch.randn(n * world, 2, Dm, generator=g), dim=2)
        sl = slice(rank * n, (rank + 1) * n)
        rows, cols = global_supcon_pairs(rows_all[sl].clone(), cols_all[sl].clone())
        ok_pairs = torch.equal(rows, rows_all) and torch.equal(cols, cols_all) and rows.dtype == torch.int32
        mask = ws.jaccard_host(rows.tolist(), [0] * (n * world), rows.tolist(), cols.tolist())
        single = ws.jaccard_host(rows_all.tolist(), [0] * (n * world), rows_all.tolist(), cols_all.tolist())
        local = torch.cat([full[sl, 0], full[sl, 1]], 0).requires_grad_(True)
        feats = global_supcon_views(local, n)
        loss = oracle(feats, torch.from_numpy(mask))
        loss.backward()
        ref_in = full.clone().requires_grad_(True)
        ref = oracle(ref_in, torch.from_numpy(single))
        ref.backward()
        gref = torch.cat([ref_in.grad[sl, 0], ref_in.grad[sl, 1]], 0)
        ok_loss = abs(float(loss.detach()) - float(ref.detach())) < 1e-6 and torch.allclose(local.grad, gref * world, atol=1e-5)
        q.put((rank, ok_pairs, mask.tobytes(), bool(np.array_equal(mask, single)), float(loss.detach()), ok_loss,
               bool(((mask > 0) & (mask < 1)).any())))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_global_mask_and_masked_loss():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 27500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, ok_pairs, _mb, same, _loss, ok_loss, soft in res:
        assert ok_pairs, f"rank {rank}: gathered (row, col) pairs are not the rank-major global batch"
        assert same, f"rank {rank}: global mask differs from the single-process mask of the concatenated batch"
        assert soft, "the generated word sets give no fractional overlap: the test would not see a wrong weight"
        assert ok_loss, f"rank {rank}: masked loss / gradient slice"
    assert res[0][2] == res[1][2] and res[0][4] == res[1][4]       # same matrix, same loss on both ranks
