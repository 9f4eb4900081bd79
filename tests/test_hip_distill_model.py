"""The distillation task on the GPU: the headless model (engine head kind 2: the output is the encoder's h,
models/mmbert.py:159-161) with mmvqa_amd.distill_loss against the CPU oracle's transformer + nn.MSELoss, the replay of
the reference's own train_one_epoch (tests/golden/make_golden_distill.py), the `train distill` sub-command on synthetic
batches and on a generated tree, and the data-parallel step."""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import mmvqa_amd  # noqa: E402
from mmvqa_amd import data as D  # noqa: E402
from mmvqa_amd import synth, train  # noqa: E402
from mmvqa_amd.ddp import GradReducer  # noqa: E402
from oracle import mmbert_oracle as O  # noqa: E402
from hip_helpers import dev, relerr  # noqa: E402
from dropout_helpers import engine_seed  # noqa: E402
from distill_helpers import ddp_worker, dense_target, load, write_teacher_file  # noqa: E402
from test_hip_model import DROPOUT, TOL, build_pair, compare_grads, mini_args  # noqa: E402
from test_hip_amp_model import emulate_f16  # noqa: E402
from test_hip_loops import _check_after  # noqa: E402
from test_oracle_golden import model_case_args  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = ("fc1.", "classifier.", "head.")


def batch_and_target(B, T, hw, V, H, seed=5):
    (img, ids, seg, mask, start, count), table = synth.distill_batch(B, T, hw, vocab=V, D=H, seed=seed)
    return (img, ids, seg, mask, start, count), table, dense_target(table, start, count, T, 7)


def run_distill_case(args, B=3, T=12, hw=32, seed=0, stat_tol=1e-4, tune=False, dropout_seed=None):
    """test_hip_model.run_case for the headless model: h and the loss within TOL of the oracle, every gradient by
    compare_grads (whose rule also asserts that the head parameters, which the oracle's loss never touches, have no
    gradient), BatchNorm running statistics by run_case's rule"""
    orc, hip = build_pair(args, seed, dropout_seed)
    assert hip._desc.head_kind == 2
    H = args.hidden_size
    (img, ids, seg, mask, start, count), table, tgt = batch_and_target(B, T, hw, args.emb_vocab, H)
    orc64 = copy.deepcopy(orc).double().train()
    orc.train()
    h_ref = orc.transformer(img, ids, seg, mask)
    loss_ref = F.mse_loss(h_ref, tgt)
    loss_ref.backward()
    F.mse_loss(orc64.transformer(img.double(), ids, seg, mask), tgt.double()).backward()
    assert all(p.grad is None for n, p in orc.named_parameters() if n.startswith(HEADS))
    osd = orc.state_dict()
    dimg, dids, dseg, dmask, dstart, dcount, dtable = (t.to(dev()) for t in (img, ids, seg, mask, start, count, table))
    hip.train()
    if tune:
        assert hip.tune(dimg, dids, dseg, dmask) > 20
    if dropout_seed is not None:
        hip.set_seed(dropout_seed)
    h = hip(dimg, dids, dseg, dmask)
    if dropout_seed is not None:
        assert hip._seed_ctr == engine_seed(dropout_seed)
    assert isinstance(h, torch.Tensor) and tuple(h.shape) == (B, T, H)
    e = relerr(h, h_ref)
    assert e <= TOL, f"h rel err {e:.2e}"
    loss = mmvqa_amd.distill_loss(h, dtable, dstart, dcount, 5)
    assert abs(float(loss.detach()) - float(loss_ref.detach())) <= TOL * abs(float(loss_ref.detach())), (float(loss.detach()), float(loss_ref.detach()))
    loss.backward()
    compare_grads(orc, hip, orc64)
    for n, p in hip.named_parameters():
        if n.startswith(HEADS):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
    hsd = hip.state_dict()
    for k, v in osd.items():
        if "running_" in k:
            assert relerr(hsd[k], v) <= stat_tol, f"{k}: {relerr(hsd[k], v):.2e}"
        if k.endswith("num_batches_tracked"):
            assert int(hsd[k]) == int(v), k
    return orc, hip


@pytest.mark.parametrize("tm", ["transformer", "realformer"])
def test_headless_step_mini(tm):
    run_distill_case(mini_args(task="distillation", transformer_model=tm))


def test_headless_step_effnet():
    run_distill_case(mini_args(task="distillation", transformer_model="realformer", cnn_encoder="tf_efficientnetv2_m",
                               effnet_depth_div=8))


def test_headless_step_dropout():
    run_distill_case(mini_args(task="distillation", **DROPOUT), dropout_seed=15)


def test_headless_step_tuned():
    run_distill_case(mini_args(task="distillation", transformer_model="realformer"), tune=True)


def test_headless_step_mixed_precision():
    """the forward under fp16 autocast (f16 operand mode of the ResNet and the encoder), the loss in fp32: against the
    operand-rounding oracle in fp64 by test_hip_amp_model.run_mixed_case's rule, max(1e-3, 5 x the fp32 emulating
    oracle's own distance from fp64)"""
    args = mini_args(task="distillation")
    B, T, hw, H = 3, 12, 32, args.hidden_size
    orc, hip = build_pair(args, 31)
    orc.train()
    o64 = emulate_f16(copy.deepcopy(orc).double().train())
    emulate_f16(orc)
    (img, ids, seg, mask, start, count), table, tgt = batch_and_target(B, T, hw, args.emb_vocab, H, seed=8)
    ref = orc.transformer(img, ids, seg, mask)
    loss_ref = F.mse_loss(ref, tgt)
    loss_ref.backward()
    ref64 = o64.transformer(img.double(), ids, seg, mask)
    loss64 = F.mse_loss(ref64, tgt.double())
    loss64.backward()

    def check(name, got, r32, r64):
        tol = max(1e-3, 5 * relerr(r32, r64))
        e = relerr(got, r64)
        assert e <= tol, f"{name}: {e:.2e} > {tol:.2e}"

    dimg, dids, dseg, dmask, dstart, dcount, dtable = (t.to(dev()) for t in (img, ids, seg, mask, start, count, table))
    hip.train()
    with torch.autocast("cuda", dtype=torch.float16):
        h = hip(dimg, dids, dseg, dmask)
        loss = mmvqa_amd.distill_loss(h, dtable, dstart, dcount, 5)
    assert h.dtype == torch.float32 and loss.dtype == torch.float32
    check("h", h, ref, ref64)
    check("loss", loss.detach().reshape(1), loss_ref.detach().reshape(1), loss64.detach().reshape(1))
    loss.backward()
    hp, p64 = dict(hip.named_parameters()), dict(o64.named_parameters())
    n = 0
    for name, p in orc.named_parameters():
        if p.grad is None:
            continue
        check(name, hp[name].grad, p.grad, p64[name].grad)
        n += 1
    assert n > 30
    hb, b64 = dict(hip.named_buffers()), dict(o64.named_buffers())
    for name, b in orc.named_buffers():
        if name.endswith("running_mean") or name.endswith("running_var"):
            check(name, hb[name], b, b64[name])
    # the fp32 forward of the same model differs: the autocast forward really ran with fp16 operands
    h32 = hip(dimg, dids, dseg, dmask)
    assert not torch.equal(h32, h)


@pytest.mark.parametrize("tm", ["transformer", "realformer"])
def test_reference_distillation_loop_replays(golden_dir, tm):
    """the reference's own train_one_epoch with task='distillation' and nn.MSELoss, two Adam steps: per-step losses
    within 1e-3, parameters by test_hip_loops._check_after's rule (at most 3 % of the sampled elements further than
    0.5 lr), the head parameters bit-equal to their start"""
    g = load(golden_dir, "loop_distill")
    assert bool(g["total_acc_is_none"])
    B, T, hw, V = [int(v) for v in g["dims"]]
    lr = float(g["lr"])
    args = O.make_args(**model_case_args(tm, "roco", False, "resnet152", False, V, emb_dropout_prob=0.0, rf_dropout_prob=0.0,
                                         emb_vocab=V, task="distillation"))
    torch.manual_seed(int(g["seed"]))
    orc = O.OracleModel(args)
    hip = mmvqa_amd.Model(args)
    hip.load_state_dict(orc.state_dict())
    hip.to(dev()).train()
    before = {k: v.detach().clone() for k, v in hip.state_dict().items() if k in ("fc1.weight", "classifier.2.weight")}
    opt, red = mmvqa_amd.FusedAdam(hip, lr=lr), GradReducer(hip.flat_grads)
    tg = lambda k: torch.from_numpy(g[k]).to(dev())   # noqa: E731
    losses = []
    for i in range(2):
        batch = tuple(tg(f"{n}{i}") for n in ("img", "ids", "seg", "mask", "start", "count"))
        loss = train.distill_step(hip, opt, red, 1, batch, tg(f"table{i}"))
        want = float(g[f"{tm}_losses"][i])
        losses.append(float(loss))
        print(f"{tm} step {i}: loss {float(loss):.6f} reference {want:.6f}")
        assert abs(float(loss) - want) <= 1e-3 * abs(want), (i, float(loss), want)
    assert abs(float(np.mean(losses)) - float(g[f"{tm}_mean_loss"])) <= 1e-3 * float(g[f"{tm}_mean_loss"])
    gg = {k[len(tm) + 1:]: v for k, v in g.items() if k.startswith(tm + "_p_") or k.startswith(tm + "_b_")}
    _check_after(hip, gg, lr)
    sd = hip.state_dict()
    for k, v in before.items():
        assert torch.equal(sd[k], v), f"{k} moved: the headless model must not update its head"
        assert torch.equal(sd[k].flatten().cpu()[:: max(1, v.numel() // 4096)][:4096], torch.from_numpy(gg["p_" + k.replace(".", "__")]))


MINI = ["--resnet_layers", "1", "1", "1", "1", "--resnet_width", "8", "--hidden_size", "96", "--n_layers", "2",
        "--vocab_size", "64", "--image_size", "32", "--max_position_embeddings", "16", "--hidden_dropout_prob", "0.1",
        "--lr", "1e-3", "--batch_size", "4"]


def test_train_distill_synthetic(tmp_path, capsys):
    """three synthetic steps per epoch with validation; the best model lands in save_dir/distillation/run.pt; the epoch
    line is roco_train.py:190 without an accuracy; a recorder of another loop is refused"""
    base = MINI + ["--emb_vocab", "64", "--steps_per_epoch", "3", "--val_steps", "2"]
    best = train.main(["distill", "--epochs", "5", "--save_dir", str(tmp_path)] + base)
    out = capsys.readouterr().out
    lines = [x for x in out.splitlines() if x.startswith("Epoch ")]
    assert len(lines) == 5 and math.isfinite(best) and "acc" not in lines[0] and "Val loss: " in lines[0], out
    tl = [float(x.split("Train loss: ")[1].split(",")[0]) for x in lines]
    assert tl[-1] < tl[0]                                           # it learns
    sd = torch.load(tmp_path / "distillation" / "run.pt")
    assert "fc1.weight" in sd and "classifier.2.weight" in sd
    rec = torch.load(tmp_path / "recorder_2.pt", weights_only=False)
    assert rec["mode"] == "distill" and rec["epoch"] == 4 and rec["best"]["best"] == pytest.approx(best)
    # --resume refuses the recorder of another loop
    other = tmp_path / "other"
    other.mkdir()
    torch.save(dict(rec, mode="mlm"), other / "recorder_2.pt")
    with pytest.raises(RuntimeError, match="written by the 'mlm' loop, this is 'distill'"):
        train.main(["distill", "--resume", "--epochs", "6", "--save_dir", str(other)] + base)
    # ... and resumes from its own: one more epoch
    assert math.isfinite(train.main(["distill", "--resume", "--epochs", "6", "--save_dir", str(tmp_path)] + base))
    assert len([x for x in capsys.readouterr().out.splitlines() if x.startswith("Epoch ")]) == 1
    # mixed precision: autocast forward, fp32 loss, GradScaler
    assert math.isfinite(train.main(["distill", "--epochs", "1", "--mixed_precision", "--save_dir", str(tmp_path / "amp")] + base))


def test_train_distill_from_files(tmp_path, monkeypatch, capsys):
    """`train distill --data_dir <tree> --teacher_states f.npz --val_teacher_states g.npz` on 8 + 4 generated JPEGs: it
    runs, and the first batch's target -- a dense gather of the DEVICE table by the (start, count) the loss received --
    equals TeacherStates.target_host of the rows the feeder logged"""
    from feeder_helpers import make_roco_tree
    tree = make_roco_tree(str(tmp_path / "tree"), n_train=8, n_val=4, missing=())
    rng = np.random.default_rng(12)
    T, Hd = 16, 96
    files = {}
    for split, lens in (("train", [0, 1, 8, 9, 3, 12, 5, 2]), ("validation", [4, 0, 11, 6])):
        rows = D.roco_table(tree, split)
        names = [os.path.basename(r[0]) for r in rows] + ["PMC_extra.jpg"]
        lens = lens + [3]
        ids = [rng.integers(5, 200, size=n) for n in lens]
        states = [rng.standard_normal((n, Hd)).astype(np.float32) for n in lens]
        files[split] = write_teacher_file(str(tmp_path / f"{split}.npz"), names[:-1], ids[:-1], states[:-1],
                                          order=rng.permutation(len(names)), extra=[(names[-1], ids[-1], states[-1])],
                                          dtype=np.float16 if split == "train" else np.float32, cls_id=2, sep_id=3)
    seen = {}
    real_feeders, real_loss = train.distill_feeders, train.distill_loss

    def spy_feeders(args, ctx):
        out = real_feeders(args, ctx)
        seen["fd"], seen["teacher"] = out[0], out[2]
        return out

    def spy_loss(h, teacher, start, count, num_vis=5):
        if "start" not in seen:
            seen.update(start=start.clone(), count=count.clone(), table=teacher.states, ids_shape=tuple(h.shape))
        return real_loss(h, teacher, start, count, num_vis)

    monkeypatch.setattr(train, "distill_feeders", spy_feeders)
    monkeypatch.setattr(train, "distill_loss", spy_loss)
    argv = ["distill", "--data_dir", tree, "--teacher_states", files["train"], "--val_teacher_states", files["validation"],
            "--emb_vocab", "256", "--epochs", "2", "--num_workers", "0", "--save_dir", str(tmp_path / "out")] + MINI
    best = train.main(argv)
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("Epoch ")]
    assert len(lines) == 2 and math.isfinite(best)
    assert (tmp_path / "out" / "distillation" / "run.pt").exists()
    rows = seen["fd"].log[0]["index"]
    assert len(rows) == 4 and seen["ids_shape"] == (4, T, Hd)
    assert seen["table"].dtype == torch.float16 and seen["table"].is_cuda          # float16 stays float16 on the device
    host = D.TeacherStates.from_file(files["train"], D.roco_table(tree, "train"))
    want = host.target_host(rows, T, 5)
    got = dense_target(seen["table"].float(), seen["start"].tolist(), seen["count"].tolist(), T, 7)
    assert torch.equal(got.cpu().double(), want) and float(want.abs().sum()) > 0
    # an id beyond the embedding table is refused where the loop knows emb_vocab; so is a table of another width
    with pytest.raises(ValueError, match="outside the embedding table"):
        train.main([a if a != "256" else "100" for a in argv])
    with pytest.raises(ValueError, match="--hidden_size is 192"):
        train.main([a if a != "96" else "192" for a in argv])


def test_two_rank_distillation_step_on_gpu():
    """two processes on cuda:0 over gloo, in the manner of test_ddp_gpu.py: the all-reduced gradient, averaged, equals
    the mean of the per-rank gradients computed one after the other in a single process (that file's rule, 1e-5), and
    the gradient-ready ranges still partition the flat buffer although the head's ranges receive nothing"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, err, n_calls, partition in res:
        assert n_calls >= 3 and partition, f"rank {rank}: {n_calls} announcements, partition {partition}"
        assert err <= 1e-5, f"rank {rank}: averaged gradients differ from the single-process ones: {err:.2e}"
