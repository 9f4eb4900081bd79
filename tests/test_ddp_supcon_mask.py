"""Masked SupCon under data parallelism on the GPU with two processes: the (row, column) pairs of both ranks are
gathered, every rank builds the global Jaccard mask on the device from its resident word sets, and the masked HIP loss
over the gathered features gives each rank the gradient of its own rows of the single-process global loss.  Both ranks
share cuda:0 and talk over gloo, as in test_ddp_gpu.py."""
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
        from mmvqa_amd.ddp import global_supcon_pairs, global_supcon_views
        from supcon_mask_helpers import random_word_sets, supcon_masked
        dev = torch.device("cuda", 0)
        n, D = 64, 128                                  # 2n*world = 256 rows = BASELINE configs[3] on 8 GPUs
        ws, _ = random_word_sets(300, [12, 30, 7, 0, 19, 25], 60, seed=5)
        words = ws.to(dev)
        g = torch.Generator().manual_seed(7)
        full = torch.nn.functional.normalize(torch.randn(n * world, 2, D, generator=g), dim=2)
        rows_all = torch.randperm(300, generator=g)[:n * world].to(torch.int32)
        cols_all = torch.randint(1, 4, (n * world,), generator=g).to(torch.int32)
        sl = slice(rank * n, (rank + 1) * n)
        local = torch.cat([full[sl, 0], full[sl, 1]], 0).to(dev).requires_grad_(True)    # model output order
        feats = global_supcon_views(local, n)
        rows, cols = global_supcon_pairs(rows_all[sl].to(dev), cols_all[sl].to(dev))
        mask = mmvqa_amd.jaccard_mask(words, rows, torch.zeros_like(cols), rows, cols)
        loss = mmvqa_amd.supcon_loss(feats, mask=mask)
        loss.backward()
        torch.cuda.synchronize()
        ref_mask = ws.jaccard_host(rows_all.tolist(), [0] * (n * world), rows_all.tolist(), cols_all.tolist())
        ref_in = full.double().requires_grad_(True)
        ref = supcon_masked(ref_in, torch.from_numpy(ref_mask))
        ref.backward()
        gr = ref_in.grad[sl]
        gref = torch.cat([gr[:, 0], gr[:, 1]], 0) * world     # every rank back-propagates the same global loss
        err = float((local.grad.cpu().double() - gref).abs().max() / gref.abs().max())
        m = mask.cpu().numpy()
        q.put((rank, m.tobytes(), bool(np.array_equal(m.view(np.uint32), ref_mask.view(np.uint32))),
               abs(float(loss) - float(ref)) / abs(float(ref)), err, bool(((m > 0) & (m < 1)).any())))
    finally:
        dist.destroy_process_group()


def test_two_rank_global_jaccard_mask_and_masked_supcon_on_gpu():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][1] == res[1][1], "the global mask differs between the ranks"
    for rank, _mb, same, lerr, gerr, soft in res:
        print(f"rank {rank}: loss rel err {lerr:.2e} grad rel-to-max {gerr:.2e}")
        assert same, f"rank {rank}: device mask is not the numpy mask of the concatenated batch"
        assert soft
        assert lerr <= 2e-5, f"rank {rank}: global masked SupCon loss differs from the oracle: {lerr:.2e}"
        assert gerr <= 1e-4, f"rank {rank}: feature gradient differs from the slice of the global one: {gerr:.2e}"
