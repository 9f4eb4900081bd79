"""The consumers of the BERTScore mask on the GPU: `train supcon --supcon_mask bert_score` on a generated tree, and the
global mask of two ranks (both on cuda:0, talking over gloo, as in test_ddp_supcon_embed.py)."""
import math
import os
import sys
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from mmvqa_amd import train  # noqa: E402
import bertscore_helpers as BH  # noqa: E402
import teacher_helpers as TH  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, "tests", "golden", "text_vocab.txt")

MINI = ["--resnet_layers", "1", "1", "1", "1", "--resnet_width", "8", "--n_layers", "1", "--vocab_size", "256", "--emb_vocab", "256",
        "--image_size", "32", "--max_position_embeddings", "16", "--hidden_dropout_prob", "0.1", "--lr", "1e-3", "--epochs", "1",
        "--num_workers", "0"]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return TH.load(golden_dir)


def _teacher_files(fx, tmp_path):
    w = tmp_path / "teacher.pt"
    torch.save({"bert." + k: v for k, v in TH.fixture_state_dict(fx).items()}, w)
    return ["--teacher_weights", str(w), "--teacher_vocab_file", VOCAB, "--max_token_length", "64"]


def one_layer(sd):
    return {k: v for k, v in sd.items() if not k.startswith("encoder.layer.1.")}


def test_train_supcon_with_the_bert_score_mask(fx, tmp_path, monkeypatch, capsys):
    """two steps of the loop with a 2-layer x 128 teacher scored at layer 1: the mask the loss receives is
    teacher_bertscore_mask's, and the first one is the float64 restatement's for the batch the feeder drew"""
    from supcon_helpers import make_supcon_tree
    tree = make_supcon_tree(str(tmp_path / "tree"))[0]
    made, used = [], []
    real_mask, real_loss = train.teacher_bertscore_mask, train.supcon_loss

    def spy_mask(teacher, rows, layer, baseline, teacher_T=None):
        m = real_mask(teacher, rows, layer, baseline, teacher_T)
        made.append(dict(rows=rows.clone(), layer=layer, baseline=baseline, T=teacher_T, mask=m))
        return m

    def spy_loss(feat, mask=None, **kw):
        used.append(mask)
        return real_loss(feat, mask=mask, **kw)

    monkeypatch.setattr(train, "teacher_bertscore_mask", spy_mask)
    monkeypatch.setattr(train, "supcon_loss", spy_loss)
    files = _teacher_files(fx, tmp_path)
    best = train.main(["supcon", "--data_dir", tree, "--supcon_mask", "bert_score", "--bert_score_layer", "1",
                       "--bert_score_baseline", "0.1", "--hidden_size", "96", "--vocab_file", VOCAB, "--batch_size", "8",
                       "--save_dir", str(tmp_path / "sc")] + MINI + files)
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("Epoch ")]
    assert len(lines) == 1 and math.isfinite(best) and len(made) == 2 and len(used) == 2, (lines, len(made), len(used))
    assert all(u is m["mask"] for u, m in zip(used, made))            # the loss got that very tensor
    c = made[0]
    rows = c["rows"].cpu()
    n, Tp = rows.shape[0] // 2, int(rows[:, 0].max())
    assert c["T"] == Tp and n == 4 and rows.shape[1] == 65 and c["layer"] == 1 and c["baseline"] == 0.1
    sd = one_layer(TH.fixture_state_dict(fx))
    lens = rows[:, 0].to(torch.int32)
    with torch.no_grad():
        h64 = TH.bert_forward(sd, rows[:, 1:1 + Tp], lens, eps=float(fx["eps"]), dtype=torch.float64)
        h32 = TH.bert_forward(sd, rows[:, 1:1 + Tp], lens, eps=float(fx["eps"]), dtype=torch.float32)
    ref = BH.bertscore(h64[:n], lens[:n], h64[n:], lens[n:], 0.1, torch.float64)[2]
    e = float((BH.bertscore(h32[:n], lens[:n], h32[n:], lens[n:], 0.1, torch.float32)[2].double() - ref).abs().max())
    mask = c["mask"].cpu()
    err = float((mask.double() - ref).abs().max())
    print(f"first step's mask vs float64: {err:.3e} (fp32 CPU pipeline {e:.3e}, bound {BH.bound(e):.3e})")
    assert err <= BH.bound(e) and torch.equal(torch.diagonal(mask), torch.ones(n)) and float(ref.min()) < 0.999
    # the default layer 8 is deeper than this checkpoint: refused when the teacher is loaded, before any feeder exists
    _, args = train.parse_args(["supcon", "--data_dir", tree, "--supcon_mask", "bert_score", "--vocab_file", VOCAB] + MINI + files)
    assert args.bert_score_layer == 8
    with pytest.raises(ValueError, match="--bert_score_layer 8 is outside 1..2"):
        train.roco_supcon_feeders(args, types.SimpleNamespace(dev=torch.device("cuda:0")), 4)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import bertscore_helpers as BH2
        import teacher_helpers as TH2
        from mmvqa_amd import train as tr
        from mmvqa_amd.teacher import BertTeacher as BT
        dev = torch.device("cuda", 0)
        fx = TH2.load(os.path.join(ROOT, "tests", "golden"))
        sd = TH2.fixture_state_dict(fx)
        teacher = BT.from_state_dict(sd, eps=float(fx["eps"])).to(dev)
        cids, clens = torch.from_numpy(fx["c_ids"]), torch.from_numpy(fx["c_lens"])
        N, Lmax = cids.shape[0] // 2, int(fx["max_pos"])
        n = N // world
        allrows = torch.zeros(2 * N, 1 + Lmax, dtype=torch.int64)
        allrows[:, 0] = clens
        allrows[:, 1:1 + cids.shape[1]] = cids
        mine = torch.cat([allrows[rank * n:(rank + 1) * n], allrows[N + rank * n:N + (rank + 1) * n]])
        Tp = int(mine[:, 0].max())
        mask = tr.teacher_bertscore_mask(teacher, mine.to(dev), 1, 0.0, Tp)
        torch.cuda.synchronize()
        one = {k: v for k, v in sd.items() if not k.startswith("encoder.layer.1.")}
        with torch.no_grad():
            h64 = TH2.bert_forward(one, cids, clens, eps=float(fx["eps"]), dtype=torch.float64)
            h32 = TH2.bert_forward(one, cids, clens, eps=float(fx["eps"]), dtype=torch.float32)
        ref = BH2.bertscore(h64[:N], clens[:N], h64[N:], clens[N:], 0.0, torch.float64)[2]
        e = float((BH2.bertscore(h32[:N], clens[:N], h32[N:], clens[N:], 0.0, torch.float32)[2].double() - ref).abs().max())
        m = mask.cpu()
        q.put((rank, m.numpy().tobytes(), tuple(m.shape), float((m.double() - ref).abs().max()), e,
               bool(torch.equal(torch.diagonal(m), torch.ones(N))), Tp))
    finally:
        dist.destroy_process_group()


def test_two_rank_global_bert_score_mask_on_gpu():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 39500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][1] == res[1][1], "the global mask differs between the ranks"
    assert res[0][6] != res[1][6]                       # the ranks' own batches really have different longest lengths
    for rank, _mb, shape, err, e, diag, Tp in res:
        print(f"rank {rank}: mask {shape}, longest text {Tp}, vs float64 {err:.3e} (fp32 CPU pipeline {e:.3e}, bound {BH.bound(e):.3e})")
        assert shape == (8, 8) and diag
        assert err <= BH.bound(e), f"rank {rank}: the gathered mask is not the mask of the concatenated batch"
