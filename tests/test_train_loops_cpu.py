"""The epoch loops of train.py on scripted numbers, without a GPU: Ctx, build, the step functions, the losses, the savers
and synth are replaced, so what is checked is the loops' own sequence -- which batches, train / eval mode, the scheduler
stepped on the validation loss, the rank mean calls, the epoch lines byte for byte, the best-model and recorder saves, the
early stop and the resumed trackers.  Every scripted value is exactly representable, so the lines are exact strings."""
import warnings

import torch
from torch.optim import lr_scheduler

from mmvqa_amd import train

VAL = [3.0, 2.5, 2.75, 2.0, 2.25, 2.125]
LR = ["0.0010000", "0.0010000", "0.0001000", "0.0001000", "0.0000100", "0.0000010"]   # patience 0, factor 0.1 on VAL
COMMON = ["--epochs", "6", "--steps_per_epoch", "3", "--val_steps", "2", "--patience", "0", "--lr", "1e-3"]
SAVES = [("model", ""), ("model", ""), ("model", "")]                                 # epochs 1, 2 and 4


class Stats:
    """what mlm_loss / the MLM steps return third: {loss, #target>0, #correct}, read with tolist()"""

    def __init__(self, values):
        self.values, self.reads = values, 0

    def tolist(self):
        self.reads += 1
        return list(self.values)


class FakeModel:
    def __init__(self):
        self.calls = []

    def train(self):
        self.calls.append("train")

    def eval(self):
        self.calls.append("eval")

    def state_dict(self):
        return {}

    def __call__(self, *a):
        return torch.zeros(2, 3), None, None


class FakeCtx:
    world, rank, dev = 1, 0, torch.device("cpu")

    def __init__(self):
        self.means = []

    def mean(self, x):
        self.means.append(x)
        return x


class FakeOpt:
    def __init__(self, lr):
        self.param_groups = [{"lr": lr}]

    def state_dict(self):
        return {}


class FakeFeeder:
    def __init__(self, batches):
        self.batches, self.epochs = batches, []

    def set_epoch(self, epoch):
        self.epochs.append(epoch)

    def __iter__(self):
        return iter(self.batches)


class World:
    """the fakes of one run; `first` is the epoch the run starts at (validation values are indexed by epoch)"""

    def __init__(self, monkeypatch, first=0):
        self.ctx, self.model, self.log = FakeCtx(), FakeModel(), []
        self.train_steps, self.val_batches, self.train_stats = 0, 2 * first, []
        monkeypatch.setattr(train, "Ctx", lambda args: self.ctx)
        monkeypatch.setattr(train, "build", self.build)
        monkeypatch.setattr(train, "save_model", lambda args, model, suffix="": self.log.append(("model", suffix)))
        monkeypatch.setattr(train, "save_recorder",
                            lambda args, epoch, model, opt, sched, mode, best=None: self.log.append(("rec", epoch, mode, best)))
        z = torch.zeros(2, 1)
        monkeypatch.setattr(train.synth, "roco_batch", lambda *a, **k: (z, z, z, z, z))
        monkeypatch.setattr(train.synth, "distill_batch", lambda *a, **k: ((1, 2, 3, 4, 5, 6), "table"))
        monkeypatch.setattr(train.synth, "vqa_batch", lambda *a, **k: (0, 0, 0, 0, torch.tensor([0, 1])))

    def build(self, args, ctx, n_classes=None):
        opt = FakeOpt(args.lr)
        sched = lr_scheduler.ReduceLROnPlateau(train._SchedShim(opt), patience=args.patience, factor=args.factor)
        return self.model, opt, sched, None

    def train_loss(self):
        self.train_steps += 1
        return 4.0 - 0.25 * ((self.train_steps - 1) // 3)

    def val_loss(self):
        self.val_batches += 1
        return VAL[(self.val_batches - 1) // 2]

    # ---- what the patched step and loss functions return
    def mlm_step(self, *a, **k):
        loss = self.train_loss()
        return torch.tensor(loss), None, Stats([loss, 8, 2])

    def mlm_loss(self, logits, tgt):
        v = self.val_loss()
        return torch.tensor(v), None, Stats([v, 8, 1])

    def supcon_step(self, *a, **k):
        loss = self.train_loss()
        self.train_stats.append(Stats([loss, 8, 2]))
        return torch.tensor(loss), None, self.train_stats[-1]


def run(mode, argv, capsys):
    _, args = train.parse_args([mode] + COMMON + argv)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # torch.autocast("cuda") without a GPU warns
        best = getattr(train, "run_" + mode)(args)
    return best, capsys.readouterr().out.splitlines()


def mlm_lines(first=0):
    return [f"Epoch {e + 1}/6 Learning rate: {LR[e - first]}, Train loss: {4.0 - 0.25 * (e - first):.4f}, "
            f"Train acc: 25.0000 ,Val loss: {VAL[e]:.4f}, Val acc: 12.5000" for e in range(first, 6)]


def test_mlm_loop(monkeypatch, capsys):
    w = World(monkeypatch)
    monkeypatch.setattr(train, "mlm_step", w.mlm_step)
    monkeypatch.setattr(train, "mlm_loss", w.mlm_loss)
    best, lines = run("mlm", [], capsys)
    assert lines == mlm_lines()
    assert w.log == SAVES + [("rec", 4, "mlm", {"best": 2.0})]
    assert best == 2.0
    assert len(w.ctx.means) == 12
    assert w.model.calls == ["train", "eval"] * 6


def test_distill_loop(monkeypatch, capsys):
    w = World(monkeypatch)
    monkeypatch.setattr(train, "distill_step", lambda *a, **k: torch.tensor(w.train_loss()))
    monkeypatch.setattr(train, "distill_loss", lambda *a, **k: torch.tensor(w.val_loss()))
    best, lines = run("distill", [], capsys)
    assert lines == [f"Epoch {e + 1}/6 Learning rate: {LR[e]}, Train loss: {4.0 - 0.25 * e:.4f}, Val loss: {VAL[e]:.4f}"
                     for e in range(6)]
    assert w.log == SAVES + [("rec", 4, "distill", {"best": 2.0})]
    assert best == 2.0
    assert len(w.ctx.means) == 12
    assert w.model.calls == ["train", "eval"] * 6


def test_supcon_loop_synthetic(monkeypatch, capsys):
    """without --data_dir: the train loss is not averaged over ranks, no train accuracy, `stats` never read on the host"""
    w = World(monkeypatch)
    monkeypatch.setattr(train, "supcon_step", w.supcon_step)
    monkeypatch.setattr(train, "mlm_loss", w.mlm_loss)
    best, lines = run("supcon", ["--batch_size", "4"], capsys)
    assert lines == [f"Epoch {e + 1}/6 Learning rate: {LR[e]}, Train loss: {4.0 - 0.25 * e:.4f}, Val loss: {VAL[e]:.4f}, "
                     f"Val acc: 12.5000" for e in range(6)]
    assert w.log == SAVES + [("rec", 4, "supcon", {"best": 2.0})]
    assert best == 2.0
    assert w.ctx.means == [float(v) for v in VAL]          # validation only
    assert len(w.train_stats) == 18 and not any(s.reads for s in w.train_stats)
    assert w.model.calls == ["train", "eval"] * 6


def test_supcon_loop_fed(monkeypatch, capsys):
    w = World(monkeypatch)
    z = torch.zeros(2, 1)
    tr, va = FakeFeeder([(z, z, z, z, z)] * 3), FakeFeeder([(z, z, z, z, z)] * 2)
    monkeypatch.setattr(train, "roco_supcon_feeders", lambda args, ctx, pairs: (tr, va, None))
    monkeypatch.setattr(train, "supcon_step", w.supcon_step)
    monkeypatch.setattr(train, "mlm_loss", w.mlm_loss)
    best, lines = run("supcon", ["--batch_size", "4", "--data_dir", "x", "--vocab_file", "v"], capsys)
    assert lines == mlm_lines()
    assert w.log == SAVES + [("rec", 4, "supcon", {"best": 2.0})]
    assert best == 2.0
    assert len(w.ctx.means) == 12
    assert tr.epochs == va.epochs == list(range(6))
    assert all(s.reads == 1 for s in w.train_stats)


def test_vqa_loop(monkeypatch, capsys):
    """the early stop: accuracy stays at 50 %, so the counter passes --counter 2 in epoch 4, before the first recorder"""
    w = World(monkeypatch)
    monkeypatch.setattr(train, "vqa_step", lambda *a, **k: (torch.tensor(w.train_loss()), None))
    monkeypatch.setattr(train, "vqa_criterion", lambda args, ctx, train_rows=None: lambda lg, t: torch.tensor(w.val_loss()))
    best, lines = run("vqa", ["--counter", "2"], capsys)
    assert lines == [f"Epoch {e + 1}/6 lr {LR[e]} train_loss {4.0 - 0.25 * e:.4f} val_loss {VAL[e]:.4f} val_total_acc 50.00"
                     for e in range(4)] + ["Counter expired, finishing."]
    assert w.log == [("model", "_loss"), ("model", ""), ("model", "_loss"), ("model", "_loss")]
    assert best == 2.0
    assert w.ctx.means == [float(v) for v in VAL[:4]]
    assert w.model.calls == ["train", "eval"] * 4


def test_resumed_trackers(monkeypatch, capsys):
    """epoch 6 alone, under a best of 1.0 kept from the interrupted run: nothing is saved, the best stays"""
    w = World(monkeypatch, first=5)
    monkeypatch.setattr(train, "maybe_resume", lambda args, model, opt, sched, mode: (5, {"best": 1.0}))
    monkeypatch.setattr(train, "mlm_step", w.mlm_step)
    monkeypatch.setattr(train, "mlm_loss", w.mlm_loss)
    best, lines = run("mlm", [], capsys)
    assert lines == mlm_lines(first=5)
    assert w.log == []
    assert best == 1.0

