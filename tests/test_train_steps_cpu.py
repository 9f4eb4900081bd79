"""What the four step functions of train.py do after they have their loss, as an event log, without a GPU: one recorder
plays model, optimizer and gradient reducer, the losses are replaced, and the log must read zero_grad -> forward ->
(scale) -> backward with the expected incoming gradient -> all-reduce -> opt.step or scaler.step + update, with the
averaging / clip factor as grad_scale."""
import warnings

import pytest
import torch

from mmvqa_amd import train

WORLD = 2
CLIPPED = 0.5 * min(1.0, 1.0 / (4 * 0.5 + 1e-6))        # |flat_grads| = 4, averaged over two ranks: ~ 0.24999987500006


class Recorder:
    """model, optimizer and reducer in one.  Calling it logs 'forward' and returns shape(scalar), the scalar built from a
    leaf tensor with a hook that logs the gradient arriving at it."""

    def __init__(self, shape=lambda s: s):
        self.log, self.shape = [], shape
        self.flat_grads = torch.full((4,), 2.0)

    def __call__(self, *a):
        self.log.append("forward")
        out = torch.zeros((), requires_grad=True) * 1.0
        out.register_hook(lambda g: self.log.append(("backward", float(g))))
        return self.shape(out)

    def zero_grad(self):
        self.log.append("zero_grad")

    def step(self, **kw):
        self.log.append(("opt.step", kw))

    def allreduce(self):
        self.log.append("allreduce")


class Scaler:
    def __init__(self, log):
        self.log = log

    def scale(self, x):
        self.log.append("scale")
        return x * 8

    def step(self, opt, **kw):
        self.log.append(("scaler.step", kw))

    def update(self):
        self.log.append("update")


def plain(grad_scale=0.5):
    return ["zero_grad", "forward", ("backward", 1.0), "allreduce", ("opt.step", {"grad_scale": grad_scale, "zero_grad": True})]


def scaled(incoming, grad_scale=0.5):
    return ["zero_grad", "forward", "scale", ("backward", incoming), "allreduce",
            ("scaler.step", {"grad_scale": grad_scale, "zero_grad": True}), "update"]


def call(step, r, *args, amp=False, **kw):
    if amp:
        kw["scaler"] = Scaler(r.log)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # torch.autocast("cuda") without a GPU warns
        return step(r, r, r, WORLD, *args, **kw)


Z = torch.zeros(2, 1)


@pytest.mark.parametrize("amp", [False, True])
def test_mlm_step(monkeypatch, amp):
    monkeypatch.setattr(train, "mlm_loss", lambda logits, tgt: (logits, "pred", "stats"))
    r = Recorder()
    loss, pred, stats = call(train.mlm_step, r, (Z, Z, Z, Z, Z), amp=amp)
    assert r.log == (scaled(8.0) if amp else plain())
    assert (pred, stats) == ("pred", "stats") and float(loss.detach()) == 0.0


@pytest.mark.parametrize("amp", [False, True])
def test_distill_step(monkeypatch, amp):
    seen = []
    monkeypatch.setattr(train, "distill_loss", lambda h, *a: seen.append(a) or h)
    r = Recorder()
    start, count = torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    loss = call(train.distill_step, r, (Z, Z, Z, Z, start, count), "table", amp=amp, num_vis=7)
    assert r.log == (scaled(8.0) if amp else plain())
    (teacher, s, c, num_vis), = seen
    assert float(loss.detach()) == 0.0 and teacher == "table" and s is start and c is count and num_vis == 7


def test_supcon_step(monkeypatch):
    monkeypatch.setattr(train, "mlm_loss", lambda logits, tgt: (logits, "pred", "stats"))
    monkeypatch.setattr(train, "supcon_loss", lambda feat: 0.0)
    monkeypatch.setattr(train, "global_supcon_views", lambda feat, bsz: feat)
    r = Recorder(lambda s: (s, s))
    loss, pred, stats = call(train.supcon_step, r, (Z, Z, Z, Z, Z), words=None)
    assert r.log == plain()
    assert (pred, stats) == ("pred", "stats")


def logits_of(s):
    return s.reshape(1, 1).expand(2, 3), None, None


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("amp", [False, True])
def test_vqa_step(amp, clip):
    """with a scaler the scaled loss is computed and thrown away: the backward stays unscaled"""
    r = Recorder(logits_of)
    loss, pred = call(train.vqa_step, r, (Z, Z, Z, Z, Z), lambda lg, t: lg[0, 0], amp=amp, clip=clip)
    want = CLIPPED if clip else 0.5
    assert r.log == (scaled(1.0, want) if amp else plain(want))
    assert want == 0.5 or abs(want - 0.24999987500006) < 1e-14
    assert pred.tolist() == [0, 0]


def test_vqa_step_passes_the_category(monkeypatch):
    seen = []
    r = Recorder(logits_of)
    cat = torch.tensor([3, 4])
    call(train.vqa_step, r, (Z, Z, Z, Z, Z, cat), lambda lg, t, c: seen.append((t, c)) or lg[0, 0])
    assert len(seen) == 1 and seen[0][0] is Z and seen[0][1] is cat
    assert r.log == plain()
