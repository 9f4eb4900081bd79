"""The consumers of the BERT teacher on the GPU: online distillation against the resident-table path, the cosine SupCon
mask against the reference's bert_embedd (fixture (c) of tests/golden/teacher.npz), the two `train` modes on generated
trees, and the gathered mask of two ranks."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

import mmvqa_amd  # noqa: E402
from mmvqa_amd import data as D  # noqa: E402
from mmvqa_amd import train  # noqa: E402
from mmvqa_amd.ddp import GradReducer  # noqa: E402
from mmvqa_amd.teacher import BertTeacher  # noqa: E402
from oracle import mmbert_oracle as O  # noqa: E402
import teacher_helpers as TH  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, "tests", "golden", "text_vocab.txt")
MASK_FLOOR = 2.0 ** -22          # four roundings of a value near 1


@pytest.fixture(scope="module")
def fx(golden_dir):
    return TH.load(golden_dir)


@pytest.fixture(scope="module")
def small(fx):
    return BertTeacher.from_state_dict(TH.fixture_state_dict(fx), eps=float(fx["eps"])).to("cuda:0")


def test_online_distillation_equals_the_resident_table(fx, small, monkeypatch):
    """the teacher run per batch, then its states copied into a TeacherStates table: train.distill_step takes both, and
    on the same h the two give the same loss and the same dh, bit for bit; the states are the reference's
    distillation() output"""
    dev = torch.device("cuda:0")
    tok = D.text.BertWordPiece(VOCAB, do_lower_case=False)
    caps = [str(c) for c in fx["b_captions"]]
    T, Lmax = 24, int(fx["max_pos"])
    ds = D.OnlineDistillDataset([("img%d.jpg" % i, c) for i, c in enumerate(caps)], tok, 5, T, Lmax)
    enc = [ds.encode(i) for i in range(len(caps))]
    ids, seg, mask, rows = (torch.stack([e[k] for e in enc]).to(dev) for k in range(4))
    Tp = int(rows[:, 0].max())
    assert Tp == Lmax
    args = O.make_args(resnet_layers=(1, 1, 1, 1), resnet_width=16, hidden_size=128, n_layers=1, heads=2, vocab_size=64,
                       emb_vocab=256, bert_max_pos=32, hidden_dropout_prob=0.0, emb_dropout_prob=0.0, task="distillation")
    torch.manual_seed(3)
    model = mmvqa_amd.Model(args).to(dev).eval()          # eval: no batch statistics, no dropout
    opt, red = mmvqa_amd.FusedAdam(model, lr=0.0), GradReducer(model.flat_grads)
    img = torch.randn(len(caps), 3, 32, 32, generator=torch.Generator().manual_seed(4)).to(dev)
    seen = []
    real = train.distill_loss

    def spy(h, teacher, start, count, num_vis=5):
        h.retain_grad()
        seen.append(dict(h=h, table=teacher, start=start.clone(), count=count.clone()))
        return real(h, teacher, start, count, num_vis)

    monkeypatch.setattr(train, "distill_loss", spy)
    loss_on = train.distill_step(model, opt, red, 1, (img, ids, seg, mask, rows), small, teacher_T=Tp)
    on = seen[0]
    states = on["table"]
    assert tuple(states.shape) == (len(caps) * Tp, 128) and on["count"].tolist() == [len(fx[f"b_ids{c}"]) for c in range(len(caps))]
    # fixture (b): the reference ran each caption alone, unpadded
    e0 = float(fx["e0"])
    for c in range(len(caps)):
        n = len(fx[f"b_ids{c}"])
        got = states[c * Tp + 1:c * Tp + 1 + n].cpu()
        err = float((got - torch.from_numpy(fx[f"b_states{c}"])).abs().max()) if n else 0.0
        print(f"caption {c} ({n} pieces): states vs distillation() {err:.3e}, ratio to e0 {err / e0:.2f}")
        assert err <= 4.0 * e0
    # the same states as a resident table
    lens = [len(fx[f"b_ids{c}"]) for c in range(len(caps))]
    offs = np.concatenate([[0], np.cumsum(lens)])
    table = torch.cat([states[c * Tp + 1:c * Tp + 1 + n] for c, n in enumerate(lens)]).cpu()
    ts = D.TeacherStates.from_arrays(offs, np.concatenate([fx[f"b_ids{c}"] for c in range(len(caps))]), table,
                                     int(fx["cls_id"]), int(fx["sep_id"]))
    sids, sseg, smask, start, count = ts.batch(range(len(caps)), T, 5)
    assert torch.equal(sids, ids.cpu()) and torch.equal(sseg, seg.cpu()) and torch.equal(smask, mask.cpu())
    resident = ts.to(dev)
    loss_off = train.distill_step(model, opt, red, 1, (img, ids, seg, mask, start.to(dev), count.to(dev)), resident)
    off = seen[1]
    print(f"online loss {float(loss_on):.6f} offline {float(loss_off):.6f}")
    assert float(loss_on) > 0 and math.isfinite(float(loss_on))
    # two forward passes of the model are not bit-equal on the GPU (torch.equal of the two h fails), so the two steps
    # are compared within 1e-5 and the bit-equality is shown on ONE h: what each step handed to distill_loss
    assert abs(float(loss_on) - float(loss_off)) <= 1e-5 * float(loss_on)
    assert float((on["h"].grad - off["h"].grad).abs().max()) <= 1e-5 * float(on["h"].grad.abs().max()) and float(on["h"].grad.abs().max()) > 0
    h1 = on["h"].detach().clone().requires_grad_(True)
    h2 = on["h"].detach().clone().requires_grad_(True)
    l1 = real(h1, on["table"], on["start"], on["count"], 5)
    l2 = real(h2, resident, off["start"], off["count"], 5)
    l1.backward()
    l2.backward()
    assert torch.equal(l1, l2) and torch.equal(l1, loss_on.detach()) and torch.equal(h1.grad, h2.grad)
    assert torch.equal(h1.grad, on["h"].grad)
    # without the host-side length the step reads it from the device: the same table
    train.distill_step(model, opt, red, 1, (img, ids, seg, mask, rows), small)
    assert torch.equal(seen[2]["table"], on["table"]) and torch.equal(seen[2]["start"], on["start"])


def test_cosine_mask_against_bert_embedd(fx, small):
    dev = torch.device("cuda:0")
    cids, clens = torch.from_numpy(fx["c_ids"]), torch.from_numpy(fx["c_lens"])
    n, Tp, Lmax = cids.shape[0] // 2, cids.shape[1], int(fx["max_pos"])
    rows = torch.zeros(2 * n, 1 + Lmax, dtype=torch.int64)
    rows[:, 0] = clens
    rows[:, 1:1 + Tp] = cids
    mask = train.teacher_cosine_mask(small, rows.to(dev), Tp).cpu()
    assert tuple(mask.shape) == (n, n) and torch.equal(torch.diagonal(mask), torch.ones(n))
    bound = max(4.0 * float(fx["e_mask"]), MASK_FLOOR)
    err = float((mask.double() - torch.from_numpy(fx["c_f64"])).abs().max())
    err_ref = float((mask - torch.from_numpy(fx["c_ref"])).abs().max())
    print(f"cosine mask: vs float64 {err:.3e} (bound {bound:.3e}), vs bert_embedd's fp32 {err_ref:.3e}")
    assert err <= bound
    # the quirk, pinned: the mean runs over the padded rows too, so the mask depends on the batch's longest text
    longer = train.teacher_cosine_mask(small, rows.to(dev), Tp + 6).cpu()
    assert float((longer - mask).abs().max()) > 1e-3


def _teacher_files(fx, tmp_path):
    w = tmp_path / "teacher.pt"
    torch.save({"bert." + k: v for k, v in TH.fixture_state_dict(fx).items()}, w)
    return ["--teacher_weights", str(w), "--teacher_vocab_file", VOCAB, "--max_token_length", "64"]


MINI = ["--resnet_layers", "1", "1", "1", "1", "--resnet_width", "8", "--n_layers", "1", "--vocab_size", "256", "--emb_vocab", "256",
        "--image_size", "32", "--max_position_embeddings", "16", "--hidden_dropout_prob", "0.1", "--lr", "1e-3", "--epochs", "1",
        "--num_workers", "0"]


def test_train_distill_with_the_teacher_on_the_gpu(fx, tmp_path, monkeypatch, capsys):
    """`train distill --data_dir <tree> --teacher_weights f --teacher_vocab_file v`: two steps, and the first step's
    table is the teacher's output for the captions the feeder logged"""
    from feeder_helpers import make_roco_tree
    tree = make_roco_tree(str(tmp_path / "tree"), n_train=8, n_val=4, missing=())
    seen = {}
    real_feeders, real_loss = train.online_distill_feeders, train.distill_loss

    def spy_feeders(args, ctx):
        out = real_feeders(args, ctx)
        seen["fd"], seen["teacher"] = out[0], out[2]
        return out

    def spy_loss(h, teacher, start, count, num_vis=5):
        if "table" not in seen:
            seen.update(table=teacher.clone(), start=start.clone(), count=count.clone(), T=seen["fd"].log[-1]["teacher_T"],
                        rows=list(seen["fd"].log[-1]["index"]))
        seen["calls"] = seen.get("calls", 0) + 1
        return real_loss(h, teacher, start, count, num_vis)

    monkeypatch.setattr(train, "online_distill_feeders", spy_feeders)
    monkeypatch.setattr(train, "distill_loss", spy_loss)
    best = train.main(["distill", "--data_dir", tree, "--hidden_size", "128", "--heads", "2", "--batch_size", "4", "--save_dir",
                       str(tmp_path / "out")] + MINI + _teacher_files(fx, tmp_path))
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("Epoch ")]
    assert len(lines) == 1 and math.isfinite(best) and seen["calls"] == 3            # two train steps, one validation batch
    assert isinstance(seen["teacher"], BertTeacher) and seen["teacher"].flat.is_cuda
    tok = D.text.BertWordPiece(VOCAB, do_lower_case=False)
    table = D.roco_table(tree, "train")
    rows = torch.stack([D.teacher_row(tok, table[i][1], 64) for i in seen["rows"]])
    Tp = int(rows[:, 0].max())
    assert seen["T"] == Tp and tuple(seen["table"].shape) == (4 * Tp, 128)
    assert seen["start"].tolist() == [b * Tp + 1 for b in range(4)] and seen["count"].tolist() == (rows[:, 0] - 2).tolist()
    ref = TH.bert_forward(TH.fixture_state_dict(fx), rows[:, 1:1 + Tp], rows[:, 0].to(torch.int32), dtype=torch.float64)
    err = float((seen["table"].cpu().double().view(4, Tp, 128) - ref).abs().max())
    print(f"first step's teacher states vs float64: {err:.3e}")
    assert err <= 4.0 * float(fx["e0"])
    # synthetic batches: a seeded random teacher of N layers
    best = train.main(["distill", "--teacher_layers", "1", "--hidden_size", "64", "--heads", "1", "--batch_size", "4",
                       "--steps_per_epoch", "2", "--val_steps", "1", "--save_dir", str(tmp_path / "syn")] + MINI)
    assert math.isfinite(best)


def test_train_supcon_with_the_cosine_mask(fx, tmp_path, monkeypatch, capsys):
    """`train supcon --supcon_mask cosine`: two steps; the first step's mask is bert_embedd's of the captions and the
    translations the batch drew, padded to that batch's longest text"""
    from supcon_helpers import make_supcon_tree
    tree = make_supcon_tree(str(tmp_path / "tree"))[0]
    calls = []
    real = train.teacher_cosine_mask

    def spy(teacher, rows, teacher_T=None):
        m = real(teacher, rows, teacher_T)
        calls.append(dict(rows=rows.clone(), T=teacher_T, mask=m.clone()))
        return m

    monkeypatch.setattr(train, "teacher_cosine_mask", spy)
    best = train.main(["supcon", "--data_dir", tree, "--supcon_mask", "cosine", "--hidden_size", "96", "--vocab_file", VOCAB,
                       "--batch_size", "8", "--save_dir", str(tmp_path / "sc")] + MINI + _teacher_files(fx, tmp_path))
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("Epoch ")]
    assert len(lines) == 1 and math.isfinite(best) and len(calls) == 2, (lines, len(calls))
    c = calls[0]
    rows = c["rows"].cpu()
    n = rows.shape[0] // 2
    Tp = int(rows[:, 0].max())
    assert c["T"] == Tp and n == 4 and rows.shape[1] == 65
    h = TH.bert_forward(TH.fixture_state_dict(fx), rows[:, 1:1 + Tp], rows[:, 0].to(torch.int32), dtype=torch.float64)
    f = h.mean(1)
    f = f / f.norm(dim=1, keepdim=True).clamp_min(1e-8)
    ref = (f[:n] @ f[n:].T).fill_diagonal_(1.0)
    err = float((c["mask"].cpu().double() - ref).abs().max())
    print(f"first step's mask vs float64: {err:.3e}")
    assert err <= max(4.0 * float(fx["e_mask"]), MASK_FLOOR) and float(ref.min()) < 0.999


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import teacher_helpers as TH2
        from mmvqa_amd import train as tr
        from mmvqa_amd.teacher import BertTeacher as BT, cosine_mask_from_means
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

        def rank_rows(r):      # captions r*n .. r*n+n-1, then their translations
            return torch.cat([allrows[r * n:(r + 1) * n], allrows[N + r * n:N + (r + 1) * n]])

        mine = rank_rows(rank)
        Tp = int(mine[:, 0].max())
        mask = tr.teacher_cosine_mask(teacher, mine.to(dev), Tp)
        # one rank, the concatenated batch, each rank's half padded to that rank's longest text
        means, means64, Ts = [], [], []
        for r in range(world):
            rr = rank_rows(r)
            t = int(rr[:, 0].max())
            Ts.append(t)
            ids, lens, _ = tr.teacher_inputs(rr.to(dev), t)
            means.append(teacher.sentence_means(ids, lens))
            means64.append(TH2.bert_forward(sd, rr[:, 1:1 + t], rr[:, 0].to(torch.int32), dtype=torch.float64).mean(1))
        cat = lambda ms: torch.cat([m[:n] for m in ms] + [m[n:] for m in ms])   # noqa: E731
        one = cosine_mask_from_means(cat(means))
        f = cat(means64)
        f = f / f.norm(dim=1, keepdim=True).clamp_min(1e-8)
        ref = (f[:N] @ f[N:].T).fill_diagonal_(1.0)
        torch.cuda.synchronize()
        q.put((rank, mask.cpu().numpy().tobytes(), bool(torch.equal(mask, one)), float((mask.cpu().double() - ref).abs().max()),
               float(fx["e_mask"]), tuple(mask.shape), Ts))
    finally:
        dist.destroy_process_group()


def test_two_rank_gathered_cosine_mask_on_gpu():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 38500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][1] == res[1][1], "the global mask differs between the ranks"
    for rank, _mb, same, err, e_mask, shape, Ts in res:
        print(f"rank {rank}: mask {shape}, per-rank lengths {Ts}, equals the one-rank mask: {same}, vs float64 {err:.3e}")
        assert shape == (8, 8) and Ts[0] != Ts[1]            # the ranks really pad differently
        assert same, f"rank {rank}: the gathered mask is not the one-rank mask of the concatenated batch"
        assert err <= max(4.0 * e_mask, MASK_FLOOR)
