"""`train vqa --group_by_image` and `train eval --group_by_image` end to end: synthetic batches, a tiny
on-disk VQA-Med tree whose images have 4, 3 and 1 questions, and the two result files of a grouped test-set run against
the plain one's."""
import csv
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmvqa_amd import checkpoint, data as D, text, train  # noqa: E402
from oracle import mmbert_oracle as O  # noqa: E402
from feeder_helpers import QUESTIONS, SIZES, VOCAB, rebuild_images, tokenizer, write_jpeg  # noqa: E402
from test_augment import synth_image  # noqa: E402
from test_hip_model import TOL, build_oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MINI = ["--resnet_layers", "1", "1", "1", "1", "--resnet_width", "8", "--hidden_size", "96", "--n_layers", "2",
        "--image_size", "32", "--max_position_embeddings", "16", "--hidden_dropout_prob", "0.1", "--epochs", "2",
        "--lr", "1e-3", "--seed", "7"]
SYNTH = ["--vocab_size", "64", "--emb_vocab", "64", "--steps_per_epoch", "3", "--val_steps", "1", "--num_classes", "11",
         "--batch_size", "8"]
# the vocabulary of the generated tree has 213 pieces: the embedding must cover it
DATA = ["--vocab_size", "256", "--emb_vocab", "256", "--batch_size", "4", "--num_workers", "0", "--vocab_file", VOCAB]

# questions per image, the rows of an image spread over the table (row r of the split belongs to image r % len(counts)
# while that image still has questions left): grouped order and table order differ
COUNTS = {"train": (4, 3, 4), "val": (3, 1, 4), "test": (4, 1, 3, 4)}


def make_grouped_vqa_tree(root, seed=2, all_counts=COUNTS):
    rng = np.random.default_rng(seed)
    for (split, folder, fname) in (("train", "Train", "traindf.csv"), ("val", "Val", "valdf.csv"), ("test", "Test", "testdf.csv")):
        counts = list(all_counts[split])
        os.makedirs(os.path.join(root, folder, "images"))
        for i in range(len(counts)):
            h, wd = SIZES[(i * 3 + len(split)) % len(SIZES)]
            write_jpeg(os.path.join(root, folder, "images", f"synpic{split}{i}.jpg"), synth_image(rng, h, wd))
        with open(os.path.join(root, fname), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["img_id", "question", "answer", "category", "mode"])
            left, r = counts[:], 0
            while any(left):
                for i in range(len(counts)):
                    if left[i]:
                        q, a, c = QUESTIONS[(r + i) % len(QUESTIONS)]
                        w.writerow([f"synpic{split}{i}", q, a, c, split])
                        left[i] -= 1
                        r += 1
    return root


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return make_grouped_vqa_tree(str(tmp_path_factory.mktemp("vqa_grouped")))


@pytest.fixture
def step_losses(monkeypatch):
    """the loss of every training step the loop runs, and whether the step was a grouped one"""
    seen = []
    inner = train.vqa_step

    def recording(model, opt, red, world, batch, crit, **kw):
        loss, pred = inner(model, opt, red, world, batch, crit, **kw)
        seen.append((float(loss.detach()), kw.get("group") is not None, batch[0].shape[0], batch[1].shape[0]))
        return loss, pred
    monkeypatch.setattr(train, "vqa_step", recording)
    return seen


def check_run(seen, save_dir, steps, decreasing):
    losses = [s[0] for s in seen]
    print("step losses:", " ".join(f"{v:.4f}" for v in losses))
    assert len(seen) == steps and all(s[1] for s in seen)
    assert all(math.isfinite(v) for v in losses)
    if decreasing:
        assert losses[-1] < losses[0], losses
    assert any(s[2] < s[3] for s in seen)                      # fewer images than questions: the batches really are grouped
    sd = checkpoint.read_state_dict(os.path.join(save_dir, "MLM", "run_loss.pt"))
    assert "transformer.trans.conv2.weight" in sd and all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())
    return sd


def test_vqa_grouped_synthetic(tmp_path, step_losses):
    """2 epochs x 3 steps on synthetic batches: every step is a grouped one, its loss finite, the checkpoint loads.  (Every
    synthetic step draws fresh images, questions and uniformly random answers, so the loss stays around ln(11) = 2.40 --
    measured 2.39 1.76 3.14 2.99 2.62 2.66 -- and has nothing to decrease on; the fed runs below repeat a table.)"""
    best = train.main(["vqa", "--group_by_image", "--save_dir", str(tmp_path)] + MINI + SYNTH)
    assert math.isfinite(best)
    check_run(step_losses, str(tmp_path), 6, decreasing=False)
    assert all((s[2], s[3]) == (2, 8) for s in step_losses)   # --batch_size counts questions: 8 of them on 2 images


@pytest.mark.parametrize("extra", [[], ["--smoothing", "0.1", "--clip"], ["--mixed_precision", "--freeze_backbone"]],
                         ids=["plain", "smoothing-clip", "amp-frozen"])
def test_vqa_grouped_from_files(tmp_path, tree, step_losses, extra):
    best = train.main(["vqa", "--group_by_image", "--data_dir", tree, "--save_dir", str(tmp_path)] + MINI + DATA + extra)
    assert math.isfinite(best)
    # (4, 3, 4) questions at --batch_size 4: three steps an epoch; the loss of the last step is below the first's
    sd = check_run(step_losses, str(tmp_path), 6, decreasing=True)
    assert all(s[3] <= 4 for s in step_losses)
    assert sd["classifier.2.weight"].shape[0] == len(D.vqa_tables(tree)[2])


def test_two_ranks_stay_in_step_on_uneven_counts(tmp_path):
    """Two data-parallel ranks (gloo, both on the one GPU) through `vqa --group_by_image` on a table whose images have
    4, 1, 4, 3, 2, 2, 1 questions: whole batches are dealt to the ranks, so both run the same number of steps and of
    gradient all-reduces, and both processes end.  (Ranks that packed their own image shards could differ in their step
    counts -- test_group_cpu.test_every_rank_runs_the_same_number_of_steps -- and the rank with a step more would wait in
    its all-reduce for good.)"""
    counts = (4, 1, 4, 3, 2, 2, 1)
    tree = make_grouped_vqa_tree(str(tmp_path / "tree"), all_counts=dict(COUNTS, train=counts))
    per_rank = []
    for r in range(2):
        s = D.GroupedBatchSampler(counts, 4, True, seed=7, rank=r, world=2)
        per_rank.append([len(s) for s.epoch in (0, 1)])
    assert per_rank[0] == per_rank[1]
    port = str(33700 + os.getpid() % 2000)
    argv = [sys.executable, "-m", "mmvqa_amd.train", "vqa", "--group_by_image", "--data_dir", tree, "--save_dir",
            str(tmp_path / "out")] + MINI + DATA
    procs = [subprocess.Popen(argv, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                              env=dict(os.environ, PYTHONPATH=ROOT, WORLD_SIZE="2", RANK=str(r), LOCAL_RANK=str(r),
                                       MASTER_PORT=port, MMVQA_REHEARSE_GLOO="1")) for r in range(2)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=240)[0])      # a guard only: the run itself is seconds
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert [p.returncode for p in procs] == [0, 0], outs[0][-2000:] + outs[1][-2000:]
    assert "Epoch 2/2" in outs[0]


def test_eval_grouped_synthetic(tmp_path):
    """without --data_dir the synthetic test table has an image of its own per question: the grouped step runs with the
    identity map (nothing is shared) and writes one line per row, in the table's order"""
    loss, _acc, _bleu = train.main(["eval", "--group_by_image", "--test_samples", "10", "--save_dir", str(tmp_path)] + MINI + SYNTH)
    assert math.isfinite(float(loss))
    table = list(csv.reader(open(tmp_path / "run_preds.csv")))
    assert len(table) == 11 and [r[1] for r in table[1:]] == [f"what is shown in image {i}?" for i in range(10)]
    assert len(open(tmp_path / "run_res.txt").read().splitlines()) == 10


def oracle_logits(tree, sd, rows, C, T=16, size=32):
    """the CPU oracle's eval-mode logits of the test table under the checkpoint: val transform of every row's image, the
    tokenizer's rows"""
    args = O.make_args(resnet_layers=(1, 1, 1, 1), resnet_width=8, hidden_size=96, n_layers=2, heads=12, vocab_size=C,
                       emb_vocab=256, dataset="VQA-Med")
    orc = O.OracleModel(args)
    orc.load_state_dict(sd)
    orc.eval()
    _, img = rebuild_images([r[0] for r in rows], None, size)
    tok = tokenizer()
    enc = [text.encode_text_vqa(r[1], tok, T) for r in rows]
    ids, seg, mask = (torch.tensor([e[k] for e in enc]) for k in range(3))
    with torch.no_grad():
        return orc(img, ids, seg, mask)[0]


# picked on the CPU among seeds 0..39: the margin condition below holds (0.0376 against 0.0057 needed) and the oracle's
# predictions differ between rows, so a question answered from another image's tokens would show
CKPT_SEED = 9


def test_eval_grouped_writes_the_plain_files(tmp_path, tree):
    """Condition of the comparison: under the seeded checkpoint the oracle's top-two logit margin of every test row is at
    least ten times the parity tolerance (TOL relative to the largest logit), so neither the grouped nor the plain run can
    flip an argmax inside its tolerance.  Given that, the two runs write equal files, in the table's row order."""
    cols, tabs, idx2ans = D.vqa_tables(tree)
    rows, C = tabs["test"], len(idx2ans)
    args = O.make_args(resnet_layers=(1, 1, 1, 1), resnet_width=8, hidden_size=96, n_layers=2, heads=12, vocab_size=C,
                       emb_vocab=256, dataset="VQA-Med")
    orc = build_oracle(args, CKPT_SEED)                         # seeded weights, randomised BatchNorm / LayerNorm affine
    ck = str(tmp_path / "seeded.pt")
    torch.save(orc.state_dict(), ck)
    logits = oracle_logits(tree, checkpoint.read_state_dict(ck), rows, C)
    top = logits.topk(2, dim=1).values
    margin, need = float((top[:, 0] - top[:, 1]).min()), 10 * TOL * float(logits.abs().max())
    print(f"top-two margin {margin:.4f}, needed {need:.4f}")
    assert margin >= need, (margin, need)
    out = {}
    for name, flag in (("plain", []), ("grouped", ["--group_by_image"])):
        d = tmp_path / name
        train.main(["eval", "--data_dir", tree, "--model_dir", ck, "--save_dir", str(d)] + flag + MINI + DATA)
        out[name] = (open(d / "seeded.pt_preds.csv").read(), open(d / "seeded.pt_res.txt").read())
    assert out["grouped"] == out["plain"]
    table = list(csv.reader(out["grouped"][0].splitlines()))
    assert [r[0] for r in table[1:]] == [r[0] for r in rows] and [r[1] for r in table[1:]] == [r[1] for r in rows]
    assert [int(r[5]) for r in table[1:]] == logits.argmax(1).tolist()
    assert len(set(logits.argmax(1).tolist())) > 1
