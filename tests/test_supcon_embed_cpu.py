"""CPU tests of the SupCon mask from caption sentence embeddings: data.CaptionEmbeddings.cosine_host against the
reference's fixture, the .npz round trip and its refusals, the host-side argument checks of the two entry points, the
`train supcon --supcon_mask embeddings` options, and the global mask / masked loss over two gloo ranks."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import mmvqa_amd
from mmvqa_amd import data as D
from mmvqa_amd import train
from supcon_embed_helpers import FIXTURE_DIMS, FIXTURE_DRAWS, bound, fixture, signed_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("Dm", FIXTURE_DIMS)
def test_cosine_host_equals_the_reference_fixture(Dm):
    g = fixture()
    emb = g[f"emb_{Dm}"]
    assert emb.dtype == np.float32 and emb.shape == (6, 4, Dm) and not emb[2, 0].any() and (emb < 0).any()
    ce = D.CaptionEmbeddings.from_array(emb)
    assert ce.rows == 6 and ce.dim == Dm and ce.table.dtype == torch.float32 and not ce.normalised
    idx = list(range(6))
    for k in range(FIXTURE_DRAWS):
        cols, ref = g[f"cols_{Dm}_{k}"].tolist(), g[f"ref_{Dm}_{k}"]
        got = ce.cosine_host(idx, [0] * 6, idx, cols)
        err = float(np.abs(got - ref).max())
        print(f"D={Dm} draw {k}: cosine_host vs the reference's fp32 matrix {err:.2e} (bound {bound(Dm):.2e})")
        assert got.dtype == np.float64 and err <= bound(Dm)
        assert (np.diag(got) == 1.0).all() and (np.diag(ref) == 1.0).all()
        off = ~np.eye(6, dtype=bool)
        assert (got[2][off[2]] == 0.0).all() and np.isfinite(got).all()        # the all-zero caption: zeros, no NaN
        assert abs(got[1, 4] - 1.0) <= bound(Dm) and abs(ref[1, 4] - 1.0) <= bound(Dm)   # parallel texts off the diagonal
        assert (got[off] < 0).any() and ((got[off] > 0) & (got[off] < 1)).any()          # signed, soft
    perm = [3, 0, 5, 1]                                    # a batch is any (row, col) selection, diagonal by position
    got = ce.cosine_host(perm, [0] * 4, perm, [2] * 4)
    full = ce.cosine_host(idx, [0] * 6, idx, [2] * 6)
    off = ~np.eye(4, dtype=bool)
    assert np.allclose(got[off], full[np.ix_(perm, perm)][off], rtol=0, atol=1e-13) and (np.diag(got) == 1.0).all()


def _table(names):
    return [(os.path.join("some", "tree", "images", n), "caption", ("a", "b", "c")) for n in names]


def test_from_array_and_from_file_round_trip(tmp_path):
    emb = signed_table(9, 7, seed=1, dtype=np.float64)
    names = np.array([f"PMC{i}_x.jpg" for i in range(9)])
    kept = [4, 0, 7, 2]                                    # the table keeps four rows, in its own order
    table = _table([names[i] for i in kept])
    order = np.random.default_rng(0).permutation(9)        # the file: a shuffled superset
    tables = {}
    for dt in (np.float16, np.float32, np.float64):
        p = str(tmp_path / f"e_{np.dtype(dt).name}.npz")
        np.savez(p, names=names[order], emb=emb[order].astype(dt))
        ce = D.CaptionEmbeddings.from_file(p, table)
        assert ce.rows == 4 and ce.dim == 7 and ce.table.dtype == torch.float32 and ce.table.is_contiguous()
        assert np.array_equal(ce.table.numpy(), emb[kept].astype(dt).astype(np.float32))     # the cast, nothing else
        tables[dt] = ce.table.numpy()
    assert np.abs(tables[np.float16] - tables[np.float32]).max() <= 2.0 ** -11 * np.abs(tables[np.float32]).max()
    for dt in (np.float16, np.float32, np.float64):
        a = D.CaptionEmbeddings.from_array(emb.astype(dt))
        assert a.table.dtype == torch.float32 and np.array_equal(a.table.numpy(), emb.astype(dt).astype(np.float32))
    assert D.CaptionEmbeddings.from_array(torch.from_numpy(emb)).table.dtype == torch.float32
    with pytest.raises(mmvqa_amd.MMVQAError):              # the table is normalised by a kernel: no CPU fallback
        D.CaptionEmbeddings.from_array(emb).to("cpu")


def test_from_file_refusals(tmp_path):
    emb = signed_table(8, 5, seed=2)
    names = np.array([f"n{i}.jpg" for i in range(8)])
    table = _table(names[:6])
    p = str(tmp_path / "e.npz")

    def refused(match, **arrs):
        np.savez(p, **arrs)
        with pytest.raises(ValueError, match=match):
            D.CaptionEmbeddings.from_file(p, table)

    refused("no embeddings for 2 of the table's 6 rows: n1.jpg, n4.jpg", names=names[[0, 2, 3, 5, 6, 7]],
            emb=emb[[0, 2, 3, 5, 6, 7]])
    dup = names.copy()
    dup[7] = "n2.jpg"
    refused("n2.jpg.*more than once", names=dup, emb=emb)
    refused(r"emb must be \[8, 4, D\]", names=names, emb=emb[:, 0])                 # rank 2
    refused(r"emb must be \[8, 4, D\]", names=names, emb=emb[:, :3])                # three texts per row
    refused(r"emb must be \[8, 4, D\]", names=names, emb=emb[:7])                   # one row short of the names
    refused("float16, float32 or float64", names=names, emb=(emb * 100).astype(np.int32))
    for bad in (np.nan, np.inf):
        e = emb.copy()
        e[4, 2, 1] = bad
        refused("non-finite", names=names, emb=e)
    refused("unicode", names=np.arange(8), emb=emb)
    refused("no array 'names'", emb=emb)
    np.savez(p, names=names.astype(object), emb=emb)                                # a pickled array is not loaded
    with pytest.raises(ValueError):
        D.CaptionEmbeddings.from_file(p, table)
    for bad in (emb[:, 0], emb[:, :3], (emb * 100).astype(np.int64), np.full_like(emb, np.nan), emb[:, :, :0]):
        with pytest.raises(ValueError):
            D.CaptionEmbeddings.from_array(bad)


def test_entry_points_refuse_bad_arguments_on_the_host():
    from mmvqa_amd import _lib as L
    lib = L.lib()
    p = 0x1000                                              # never dereferenced: every call is refused first
    for args in ((None, 4, 8), (p, 0, 8), (p, -2, 8), (p, 4, 0), (p, 4, 4097)):
        assert lib.mmvqa_normalize_rows(None, *args, 1e-8) == -1, args
        assert b"normalize_rows" in lib.mmvqa_last_error()
    good = [p, p, p, p, p, p, 4, 8, 9]
    cases = [good[:k] + [None] + good[k + 1:] for k in range(6)]
    cases += [good[:6] + tail for tail in ([0, 8, 9], [-1, 8, 9], [4, 0, 9], [4, 4097, 9], [4, 8, 0], [4, 8, -5])]
    for args in cases:
        assert lib.mmvqa_cosine_mask(None, *args) == -1, args
        assert b"cosine_mask" in lib.mmvqa_last_error()
    assert mmvqa_amd.embedding_mask is mmvqa_amd.functional.embedding_mask and "embedding_mask" in mmvqa_amd.__all__
    ce = D.CaptionEmbeddings.from_array(signed_table(8, 5, seed=3))
    t = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(mmvqa_amd.MMVQAError):              # a table left on the host: no CPU fallback
        mmvqa_amd.embedding_mask(ce, t, t, t, t)
    with pytest.raises(ValueError):
        mmvqa_amd.embedding_mask(ce, t, t)


def test_train_embeddings_mask_arguments(capsys):
    ok = ["supcon", "--supcon_mask", "embeddings", "--caption_embeddings", "e.npz", "--data_dir", "x"]
    for bad, msg in ((["supcon", "--supcon_mask", "embeddings", "--data_dir", "x"], "needs --caption_embeddings"),
                     (["supcon", "--caption_embeddings", "e.npz", "--data_dir", "x"], "--supcon_mask embeddings only"),
                     (["supcon", "--supcon_mask", "jaccard", "--caption_embeddings", "e.npz", "--data_dir", "x"],
                      "--supcon_mask embeddings only"),
                     (ok[:-2], "needs --data_dir"),
                     (ok + ["--con_task", "simclr"], "contradicts"),
                     (["mlm"] + ok[1:], "unrecognized arguments")):
        with pytest.raises(SystemExit) as e:
            train.parse_args(bad)
        assert e.value.code == 2 and msg in capsys.readouterr().err, bad
    mode, a = train.parse_args(ok)
    assert mode == "supcon" and a.supcon_mask == "embeddings" and a.caption_embeddings == "e.npz"
    assert a.similarity == "sentence_transformers"                                    # still accepted, still unread
    mode, a = train.parse_args(["supcon"])
    assert a.supcon_mask == "none" and a.caption_embeddings is None                   # the default path, as before


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mmvqa_amd.ddp import global_supcon_pairs, global_supcon_views
        from supcon_embed_helpers import positive_table
        from supcon_mask_helpers import supcon_masked as oracle
        n, Dm = 3, 16
        ce = D.CaptionEmbeddings.from_array(positive_table(20, 24, seed=3))
        g = torch.Generator().manual_seed(11)
        rows_all = torch.randperm(20, generator=g)[:n * world].to(torch.int32)
        cols_all = torch.randint(1, 4, (n * world,), generator=g).to(torch.int32)
        full = torch.nn.functional.normalize(torch.randn(n * world, 2, Dm, generator=g), dim=2)
        sl = slice(rank * n, (rank + 1) * n)
        rows, cols = global_supcon_pairs(rows_all[sl].clone(), cols_all[sl].clone())
        ok_pairs = torch.equal(rows, rows_all) and torch.equal(cols, cols_all) and rows.dtype == torch.int32
        mask = ce.cosine_host(rows.tolist(), [0] * (n * world), rows.tolist(), cols.tolist())
        single = ce.cosine_host(rows_all.tolist(), [0] * (n * world), rows_all.tolist(), cols_all.tolist())
        local = torch.cat([full[sl, 0], full[sl, 1]], 0).requires_grad_(True)
        feats = global_supcon_views(local, n)
        loss = oracle(feats, torch.from_numpy(mask))
        loss.backward()
        ref_in = full.clone().requires_grad_(True)
        ref = oracle(ref_in, torch.from_numpy(single))
        ref.backward()
        gref = torch.cat([ref_in.grad[sl, 0], ref_in.grad[sl, 1]], 0)
        ok_loss = abs(float(loss.detach()) - float(ref.detach())) < 1e-6 and torch.allclose(local.grad, gref * world, atol=1e-5)
        q.put((rank, ok_pairs, mask.tobytes(), bool(np.array_equal(mask.view(np.uint64), single.view(np.uint64))),
               float(loss.detach()), ok_loss, bool(((mask > 0) & (mask < 1)).any())))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_global_embedding_mask_and_masked_loss():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
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
        assert soft, "the generated embeddings give no fractional cosine: the test would not see a wrong weight"
        assert ok_loss, f"rank {rank}: masked loss / gradient slice"
    assert res[0][2] == res[1][2] and res[0][4] == res[1][4]       # same matrix, same loss on both ranks
