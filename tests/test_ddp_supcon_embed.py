"""SupCon with the caption-embedding mask under data parallelism on the GPU with two processes: the (row, column) pairs
of both ranks are gathered, every rank builds the global cosine mask on the device from its resident, normalised copy of
the embedding table, and the masked HIP loss over the gathered features gives each rank the gradient of its own rows of
the single-process global loss.  Both ranks share cuda:0 and talk over gloo, as in test_ddp_supcon_mask.py."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import numpy as np
        import mmvqa_amd
        from mmvqa_amd import data as D
        from mmvqa_amd.ddp import global_supcon_pairs, global_supcon_views
        from supcon_embed_helpers import bound, positive_table
        from supcon_mask_helpers import supcon_masked
        dev = torch.device("cuda", 0)
        n, Df, De = 64, 128, 64                         # 2n*world = 256 rows = BASELINE configs[3] on 8 GPUs
        host = D.CaptionEmbeddings.from_array(positive_table(300, De, seed=5))
        emb = host.to(dev)
        g = torch.Generator().manual_seed(7)
        full = torch.nn.functional.normalize(torch.randn(n * world, 2, Df, generator=g), dim=2)
        rows_all = torch.randperm(300, generator=g)[:n * world].to(torch.int32)
        cols_all = torch.randint(1, 4, (n * world,), generator=g).to(torch.int32)
        sl = slice(rank * n, (rank + 1) * n)
        local = torch.cat([full[sl, 0], full[sl, 1]], 0).to(dev).requires_grad_(True)    # model output order
        feats = global_supcon_views(local, n)
        rows, cols = global_supcon_pairs(rows_all[sl].to(dev), cols_all[sl].to(dev))
        mask = mmvqa_amd.embedding_mask(emb, rows, torch.zeros_like(cols), rows, cols)
        loss = mmvqa_amd.supcon_loss(feats, mask=mask)
        loss.backward()
        torch.cuda.synchronize()
        m = mask.cpu().numpy()
        ref_mask = host.cosine_host(rows_all.tolist(), [0] * (n * world), rows_all.tolist(), cols_all.tolist())
        merr = float(np.abs(m - ref_mask).max())
        ref_in = full.double().requires_grad_(True)
        ref = supcon_masked(ref_in, torch.from_numpy(m))          # the oracle on the device's mask: no tolerances stack
        ref.backward()
        gr = ref_in.grad[sl]
        gref = torch.cat([gr[:, 0], gr[:, 1]], 0) * world     # every rank back-propagates the same global loss
        err = float((local.grad.cpu().double() - gref).abs().max() / gref.abs().max())
        off = ~np.eye(n * world, dtype=bool)
        lv, lr = float(loss.detach()), float(ref.detach())
        q.put((rank, m.tobytes(), merr, bound(De), abs(lv - lr) / abs(lr), err,
               bool(((m[off] > 0) & (m[off] < 1)).all()), bool((np.diag(m) == 1.0).all())))
    finally:
        dist.destroy_process_group()


def test_two_rank_global_embedding_mask_and_masked_supcon_on_gpu():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 37500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][1] == res[1][1], "the global mask differs between the ranks"
    for rank, _mb, merr, lim, lerr, gerr, soft, diag in res:
        print(f"rank {rank}: mask vs fp64 host {merr:.2e} (bound {lim:.2e}) loss rel err {lerr:.2e} grad rel-to-max {gerr:.2e}")
        assert merr <= lim, f"rank {rank}: device mask is not the host mask of the concatenated batch: {merr:.2e}"
        assert soft and diag
        assert lerr <= 2e-5, f"rank {rank}: global masked SupCon loss differs from the oracle: {lerr:.2e}"
        assert gerr <= 1e-4, f"rank {rank}: feature gradient differs from the slice of the global one: {gerr:.2e}"
