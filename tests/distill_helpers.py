"""Shared pieces of the distillation tests: the oracle's side of the task (OracleModel does not know it: the model's
output is its transformer's, models/mmbert.py:159-161, and the loss nn.MSELoss, pretrain/roco_train.py:94-95), the dense
target from (table, start, count) written independently of mmvqa_amd.data, and the fixtures."""
import os

import numpy as np
import torch
import torch.nn.functional as F


def load(golden_dir, name):
    return dict(np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False))


def dense_target(table, start, count, T, first):
    """roco_utils.py:196-197: zeros(first) | states[:n] | zeros(1) | zeros(n_pad), n = min(count, T - first - 1)"""
    out = torch.zeros(len(start), T, table.shape[1], dtype=table.dtype, device=table.device)
    for b in range(len(start)):
        n = min(int(count[b]), T - first - 1)
        out[b, first:first + n] = table[int(start[b]):int(start[b]) + n]
    return out


def oracle_h(orc, img, ids, seg, mask):
    return orc.transformer(img, ids, seg, mask)


def oracle_loss(orc, img, ids, seg, mask, target):
    h = oracle_h(orc, img, ids, seg, mask)
    return h, F.mse_loss(h, target.to(h.dtype))


def write_teacher_file(path, names, captions_ids, states, order=None, extra=(), dtype=np.float32, **scalars):
    """an .npz in TeacherStates' file format: entries `extra` (name, ids, states) are mixed in and everything is stored in
    `order` (a permutation of the entries)"""
    entries = [(n, np.asarray(i, dtype=np.int64), np.asarray(s)) for n, i, s in zip(names, captions_ids, states)] + list(extra)
    order = list(range(len(entries))) if order is None else list(order)
    entries = [entries[k] for k in order]
    offs = np.concatenate([[0], np.cumsum([len(e[1]) for e in entries])]).astype(np.int64)
    Dm = entries[0][2].shape[1]
    np.savez(path, names=np.array([e[0] for e in entries]), offsets=offs,
             ids=np.concatenate([e[1] for e in entries]).astype(np.int64),
             states=np.concatenate([np.asarray(e[2]).reshape(-1, Dm) for e in entries]).astype(dtype), **scalars)
    return path


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ddp_worker(rank, world, port, q):
    """one rank of test_hip_distill_model.test_two_rank_distillation_step_on_gpu (a spawned process: imports inside)"""
    import sys
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import mmvqa_amd
        from mmvqa_amd import synth
        from mmvqa_amd.ddp import GradReducer
        from oracle import mmbert_oracle as O
        d = torch.device("cuda", 0)
        args = O.make_args(resnet_layers=(1, 1, 1, 1), resnet_width=16, hidden_size=96, n_layers=2, heads=12, vocab_size=64,
                           emb_vocab=64, bert_max_pos=32, hidden_dropout_prob=0.0, emb_dropout_prob=0.0, rf_dropout_prob=0.0,
                           task="distillation", transformer_model="realformer")
        torch.manual_seed(0)                       # identical replicas
        model = mmvqa_amd.Model(args).to(d).train()
        batches = [synth.distill_batch(3, 12, 32, vocab=64, D=96, seed=60 + r, device=d) for r in range(world)]

        def fwd_bwd(b):
            (img, ids, seg, mask, start, count), table = b
            mmvqa_amd.distill_loss(model(img, ids, seg, mask), table, start, count, 5).backward()

        red = GradReducer(model.flat_grads, bucket_mb=0.02)
        calls = []
        model.set_grad_ready_hook(lambda lo, hi: (calls.append((lo, hi)), red.start(lo, hi)))
        fwd_bwd(batches[rank])
        red.allreduce()
        torch.cuda.synchronize()
        got = model.flat_grads.clone() / world     # the averaged gradient Adam receives (grad_scale = 1 / world)
        model.set_grad_ready_hook(None)
        ref = torch.zeros_like(got)
        for r in range(world):
            model.flat_grads.zero_()
            fwd_bwd(batches[r])
            torch.cuda.synchronize()
            ref += model.flat_grads / world
        err = float((got - ref).abs().max() / ref.abs().max())
        lo_sorted = sorted(calls)
        partition = lo_sorted[0][0] == 0 and lo_sorted[-1][1] == got.numel() and all(a[1] == b[0] for a, b in zip(lo_sorted, lo_sorted[1:]))
        q.put((rank, err, len(calls), partition))
    finally:
        dist.destroy_process_group()
