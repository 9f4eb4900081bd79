"""mmvqa_amd.watch on the GPU: TensorStats over a whole mini model by name, the table rebuilt after classifier[2]
surgery, the lines `train mlm --watch` writes, the overflow report of a skipped step, and the watcher's being read-only."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mmvqa_amd  # noqa: E402
from mmvqa_amd import synth, train  # noqa: E402
from mmvqa_amd.amp import GradScaler  # noqa: E402
from mmvqa_amd.watch import TensorStats, Watcher  # noqa: E402
from tensor_stats_helpers import assert_record, restate  # noqa: E402
from test_hip_model import build_pair, mini_args  # noqa: E402

MINI = ["--resnet_layers", "1", "1", "1", "1", "--resnet_width", "8", "--hidden_size", "96", "--n_layers", "2",
        "--vocab_size", "64", "--emb_vocab", "64", "--image_size", "32", "--val_steps", "1", "--max_position_embeddings", "16",
        "--hidden_dropout_prob", "0.0", "--batch_size", "4", "--lr", "1e-3"]


def host(t):
    return np.zeros(0, np.float32) if t is None else t.detach().cpu().contiguous().numpy()


def roco(seed, dev="cuda"):
    return synth.roco_batch(2, 16, 32, vocab=50, seed=seed, device=dev, mlm_prob=0.4)


def test_whole_model_by_name():
    _, hip = build_pair(mini_args(), seed=1)
    hip.train()
    img, ids, seg, mask, tgt = roco(3)
    mmvqa_amd.mlm_loss(hip(img, ids, seg, mask), tgt)[0].backward()
    ts = TensorStats(hip)
    hg, hp = ts.grads(), ts.params()            # both in flight before either is read
    g, p = hg.result(), hp.result()
    assert hg.ready() and hp.ready()
    named = dict(hip.named_parameters())
    assert sorted(g) == sorted(p) == sorted(named) and len(g) == len(named) > 40
    with_grad = 0
    for name, prm in named.items():
        assert_record(p[name], restate(host(prm)), "param " + name)
        grad = host(prm.grad) if prm.grad is not None else np.zeros(prm.numel(), np.float32)   # never-used tensors: zeros
        assert_record(g[name], restate(grad), "grad " + name)
        assert int(g[name]["hist"].sum()) == prm.numel()
        with_grad += prm.grad is not None and bool(g[name]["max"] > g[name]["min"])
    assert with_grad > 20


def test_flat_pair_is_one_unnamed_tensor():
    class Flat:
        flat_params = torch.linspace(-1, 1, 20001, device="cuda")
        flat_grads = torch.full((20001,), 0.25, device="cuda")

    ts = TensorStats(Flat())
    p, g = ts.params().result(), ts.grads(moments_only=True).result()
    assert list(p) == list(g) == [""]
    assert_record(p[""], restate(host(Flat.flat_params)))
    assert g[""]["hist"] is None and g[""]["n_finite"] == 20001 and g[""]["min"] == g[""]["max"] == 0.25


def test_table_is_rebuilt_after_rehead():
    _, hip = build_pair(mini_args(dataset="VQA-Med", vocab_size=23), seed=2)
    ts = TensorStats(hip)
    before = ts.params().result()
    assert before["classifier.2.weight"]["n_finite"] == 23 * 96
    hip.classifier[2] = torch.nn.Linear(96, 7)
    after = ts.params().result()
    assert after["classifier.2.weight"]["n_finite"] == 7 * 96 and after["classifier.2.bias"]["n_finite"] == 7
    named = dict(hip.named_parameters())
    assert sorted(after) == sorted(named)
    for name, prm in named.items():
        assert_record(after[name], restate(host(prm)), name)


def read_lines(path):
    with open(path) as f:
        return [json.loads(ln) for ln in f]


def test_mlm_loop_writes_the_expected_lines(tmp_path):
    train.main(["mlm", "--watch", "all", "--watch_freq", "2", "--steps_per_epoch", "4", "--epochs", "2",
                "--save_dir", str(tmp_path)] + MINI)
    lines = read_lines(os.path.join(tmp_path, "watch_mlm.jsonl"))
    assert [(d["step"], d["epoch"]) for d in lines] == [(2, 0), (4, 0), (6, 1), (8, 1)]
    for d in lines:
        assert d["loop"] == "mlm" and d["grad_scale"] == 1.0 and d["loss_scale"] is None and "skipped" not in d
        assert len(d["tensors"]) > 40
        for name, t in d["tensors"].items():
            assert "frozen" not in t
            for kind in ("grad", "param"):
                r = t[kind]
                assert len(r["hist"]) == 64 and sum(r["hist"]) == t["numel"] == r["n_finite"], (name, kind)
                assert r["edges"][0] <= r["edges"][1]
    # the parameters move between logged steps
    w = "transformer.bert_embedding.word_embeddings.weight" if "transformer.bert_embedding.word_embeddings.weight" in lines[0]["tensors"] \
        else next(iter(lines[0]["tensors"]))
    assert lines[0]["tensors"][w]["param"]["sum"] != lines[-1]["tensors"][w]["param"]["sum"]


def test_frozen_backbone_is_marked(tmp_path):
    train.main(["mlm", "--watch", "gradients", "--watch_freq", "1", "--steps_per_epoch", "1", "--epochs", "1",
                "--freeze_backbone", "--save_dir", str(tmp_path)] + MINI)
    (d,) = read_lines(os.path.join(tmp_path, "watch_mlm.jsonl"))
    frozen = [n for n, t in d["tensors"].items() if t.get("frozen")]
    assert frozen and all(n.startswith("transformer.trans.model.") for n in frozen)
    for n, t in d["tensors"].items():
        assert ("grad" in t) == (n not in frozen) and "param" not in t


class Inject:
    """stands where the gradient reducer stands: writes `value` into one element of the flat gradients after backward"""

    def __init__(self, model, index, value):
        self.model, self.index, self.value = model, index, value

    def allreduce(self):
        self.model.flat_grads[self.index] = self.value


def test_skipped_step_names_the_tensor_that_overflowed(tmp_path, capsys):
    _, hip = build_pair(mini_args(), seed=4)
    hip.train()
    opt = mmvqa_amd.FusedAdam(hip, lr=1e-3)
    name, _, lo, _ = hip._param_ranges()[7]
    path = os.path.join(tmp_path, "watch_mlm.jsonl")
    w = Watcher(hip, "gradients", 1000, path, "mlm")       # not a logged step: only the report is written
    scaler = GradScaler(init_scale=1024.0)
    p0 = hip.flat_params.clone()
    train.mlm_step(hip, opt, Inject(hip, lo + 1, float("inf")), 1, roco(5), scaler=scaler, watch=w)
    w.close()
    assert torch.equal(p0, hip.flat_params) and opt.step_count == 0 and scaler.get_scale() == 512.0
    (d,) = read_lines(path)
    assert d["skipped"] is True and d["step"] == 1 and d["loss_scale"] == 1024.0 and d["nonfinite"] == {name: [0, 1, 0]}
    assert f"step 1 skipped: the gradient of {name} holds 0 nan, 1 +inf and 0 -inf values" in capsys.readouterr().out


class Record:
    def __init__(self, model):
        self.model, self.grads = model, []

    def allreduce(self):
        self.grads.append(self.model.flat_grads.clone())


class Replay:
    def __init__(self, model, grads):
        self.model, self.grads = model, list(grads)

    def allreduce(self):
        self.model.flat_grads.copy_(self.grads.pop(0))


@pytest.mark.parametrize("amp", [False, True])
def test_watcher_reads_only(tmp_path, amp):
    """Three steps with --watch all at every step and three without end with bit-equal parameters and Adam moments.
    Two backward passes of the model are not bit-equal on the GPU (the order of its floating-point atomics), so the
    run without the watcher takes each step's gradient from the watched run as it stood at the all-reduce point, before
    the watcher's hook: whatever the hook did to the gradients or the parameters would part the two runs."""
    args = mini_args()
    _, a = build_pair(args, seed=6)
    _, b = build_pair(args, seed=6)
    a.train(); b.train()
    opt_a, opt_b = mmvqa_amd.FusedAdam(a, lr=1e-3), mmvqa_amd.FusedAdam(b, lr=1e-3)
    sa, sb = (GradScaler(init_scale=256.0), GradScaler(init_scale=256.0)) if amp else (None, None)
    path = os.path.join(tmp_path, "watch_mlm.jsonl")
    w = Watcher(a, "all", 1, path, "mlm")
    rec = Record(a)
    for step in range(3):
        train.mlm_step(a, opt_a, rec, 1, roco(20 + step), scaler=sa, watch=w)
    w.close()
    play = Replay(b, rec.grads)
    for step in range(3):
        train.mlm_step(b, opt_b, play, 1, roco(20 + step), scaler=sb)
    torch.cuda.synchronize()
    assert opt_a.step_count == opt_b.step_count == 3
    assert torch.equal(a.flat_params, b.flat_params) and torch.equal(opt_a.m, opt_b.m) and torch.equal(opt_a.v, opt_b.v)
    lines = read_lines(path)
    assert [d["step"] for d in lines] == [1, 2, 3]
    assert [d["loss_scale"] for d in lines] == ([256.0] * 3 if amp else [None] * 3)
