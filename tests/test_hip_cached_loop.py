"""`train vqa --cache_tokens` end to end on the mini model: the run finishes with finite losses, the
backbone, the taps and every BatchNorm buffer of the saved checkpoint are the initial ones bit for bit while the encoder
moved, a second run prints the same epoch lines, and the validation logits computed from the cache are those of a plain
forward on the same images."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from mmvqa_amd import checkpoint, synth, train  # noqa: E402
from hip_helpers import relerr  # noqa: E402
from test_hip_model import TOL  # noqa: E402

B, T, S, C, VOCAB = 8, 16, 32, 11, 64
ARGV = ["vqa", "--cache_tokens", "--cache_views", "2", "--cache_images", "12", "--weight_decay", "0.01", "--ema_decay", "0.9",
        "--clip", "--epochs", "2", "--steps_per_epoch", "4", "--val_steps", "2", "--batch_size", str(B),
        "--resnet_layers", "1", "1", "1", "1", "--resnet_width", "8", "--hidden_size", "96", "--n_layers", "2",
        "--image_size", str(S), "--max_position_embeddings", str(T), "--hidden_dropout_prob", "0.1", "--lr", "1e-3",
        "--seed", "7", "--vocab_size", str(VOCAB), "--emb_vocab", str(VOCAB), "--num_classes", str(C)]
VISUAL = "transformer.trans."


def run(tmp_path, monkeypatch, capsys, check_validation):
    """one run of the loop -> (initial state_dict, step losses, views used, epoch lines, worst validation difference)"""
    init, losses, views, val_err = {}, [], set(), []
    inner_build, inner_step, inner_forward = train.build, train.vqa_step, train.vqa_forward

    def build(args, ctx, n_classes=None):
        out = inner_build(args, ctx, n_classes=n_classes)
        init.update({k: v.detach().clone().cpu() for k, v in out[0].state_dict().items()})
        return out

    def step(model, opt, red, world, batch, crit, **kw):
        assert kw.get("cache") is not None and not isinstance(batch[0], torch.Tensor)     # no image reaches a step
        views.update(batch[0][1].tolist())
        loss, pred = inner_step(model, opt, red, world, batch, crit, **kw)
        losses.append(float(loss.detach()))
        return loss, pred

    def forward(model, batch, group=None, cache=None):
        logits = inner_forward(model, batch, group, cache)
        if check_validation and cache is not None and not model.training:
            index, view = batch[0]
            assert view.tolist() == [0] * B and index.tolist() == list(range(int(index[0]), int(index[0]) + B))
            seed = list(train.val_seeds(type("A", (), {"val_steps": 2})))[int(index[0]) // B]
            img = synth.vqa_batch(B, T, S, VOCAB, C, seed=seed, device=logits.device)[0]   # the images behind these rows
            ctr = model._seed_ctr                       # every forward advances the dropout counter: the check must not
            with torch.no_grad():                       # change the stream of the epochs that follow
                val_err.append(relerr(logits, model(img, *batch[1:4])[0]))
            model._seed_ctr = ctr
        return logits

    monkeypatch.setattr(train, "build", build)
    monkeypatch.setattr(train, "vqa_step", step)
    monkeypatch.setattr(train, "vqa_forward", forward)
    capsys.readouterr()
    best = train.main(ARGV + ["--save_dir", str(tmp_path)])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Epoch ")]
    assert math.isfinite(best)
    return init, losses, views, lines, val_err


def test_cached_loop(tmp_path, monkeypatch, capsys):
    init, losses, views, lines, val_err = run(tmp_path / "a", monkeypatch, capsys, check_validation=True)
    print("step losses:", " ".join(f"{v:.4f}" for v in losses), "\n" + "\n".join(lines))
    assert len(losses) == 8 and all(math.isfinite(v) for v in losses) and len(lines) == 2
    assert views == {0, 1}                                        # both views of the train cache are drawn
    # validation from the cache = the plain forward on the same images (4 batches: 2 epochs x 2 validation steps)
    print("validation logits, cache vs forward:", " ".join(f"{e:.2e}" for e in val_err))
    assert len(val_err) == 4 and max(val_err) <= TOL
    saved = sorted(os.listdir(os.path.join(str(tmp_path / "a"), "MLM")))
    assert "run_loss.pt" in saved                                 # (run.pt too once an epoch's accuracy is above zero)
    for name in saved:
        sd = checkpoint.read_state_dict(os.path.join(str(tmp_path / "a"), "MLM", name))
        frozen = [k for k in sd if k.startswith(VISUAL)]
        assert len(frozen) > 60 and any("running_var" in k for k in frozen) and any(k.endswith("conv2.weight") for k in frozen)
        for k in frozen:                                          # parameters and buffers, weight decay and EMA notwithstanding
            assert torch.equal(sd[k].cpu(), init[k]), f"{name}: {k} is not its initial value"
        moved = [k for k in sd if not k.startswith(VISUAL) and sd[k].is_floating_point() and not torch.equal(sd[k].cpu(), init[k])]
        assert any(k.startswith("transformer.blocks.") or k.startswith("transformer.mains.") for k in moved), moved[:5]
        assert any(k.startswith("classifier.") for k in moved) and any("embeddings" in k for k in moved)
    # the same seed prints the same epoch lines (4 decimals)
    monkeypatch.undo()
    _, _, _, lines2, _ = run(tmp_path / "b", monkeypatch, capsys, check_validation=False)
    assert lines2 == lines, (lines, lines2)


# ----------------------------------------------------------------------------- from files (--data_dir)
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from test_hip_group_loop import make_grouped_vqa_tree
    return make_grouped_vqa_tree(str(tmp_path_factory.mktemp("vqa_cached")))


def test_cached_loop_from_files(tree, tmp_path, monkeypatch, capsys):
    """`train vqa --cache_tokens --cache_views 2 --data_dir` on a tiny VQA-Med tree (3 train images with 4 + 3 + 4
    questions, 3 validation images with 3 + 1 + 4): every image is decoded once per view during the fill and never
    again, the steps carry cache rows instead of images, validation from the cache agrees with a plain forward on the
    evaluation transform of the same files, the frozen range of the checkpoint is the initial one."""
    from feeder_helpers import VOCAB as VOCAB_FILE
    from mmvqa_amd import data as D
    from mmvqa_amd.augment import DeviceAugment
    _cols, tabs, idx2ans = D.vqa_tables(tree)
    decoded, state = [], {}
    inner_decode, inner_build, inner_step, inner_forward = D.decode, train.build, train.vqa_step, train.vqa_forward

    def decode(path):
        decoded.append((path, len(state.get("steps", []))))
        return inner_decode(path)

    def build(args, ctx, n_classes=None):
        out = inner_build(args, ctx, n_classes=n_classes)
        state["init"] = {k: v.detach().clone().cpu() for k, v in out[0].state_dict().items()}
        return out

    def step(model, opt, red, world, batch, crit, **kw):
        cache = kw.get("cache")
        assert cache is not None and tuple(cache.tokens.shape[:2]) == (3, 2) and not isinstance(batch[0], torch.Tensor)
        index, view = batch[0]
        state.setdefault("views", set()).update(view.tolist())
        state.setdefault("rows", []).extend(index.tolist())
        state.setdefault("cache", cache)
        loss, pred = inner_step(model, opt, red, world, batch, crit, **kw)
        state.setdefault("steps", []).append(float(loss.detach()))
        return loss, pred

    val_paths, val_image_of = D.image_of_rows(tabs["val"])

    def forward(model, batch, group=None, cache=None):
        logits = inner_forward(model, batch, group, cache)
        if cache is not None and not model.training:
            index, view = batch[0]
            assert view.tolist() == [0] * len(index) and tuple(cache.tokens.shape[:2]) == (3, 1)
            n_before = len(decoded)
            imgs = DeviceAugment(size=32, train=False, device=logits.device)([inner_decode(p) for p in val_paths])
            assert len(decoded) == n_before
            ctr = model._seed_ctr
            with torch.no_grad():
                state.setdefault("val_err", []).append(relerr(logits, model(imgs[index.to(logits.device)], *batch[1:4])[0]))
            model._seed_ctr = ctr
            state.setdefault("val_rows", []).extend(index.tolist())
        return logits

    monkeypatch.setattr(D, "decode", decode)
    monkeypatch.setattr(train, "build", build)
    monkeypatch.setattr(train, "vqa_step", step)
    monkeypatch.setattr(train, "vqa_forward", forward)
    best = train.main(["vqa", "--cache_tokens", "--cache_views", "2", "--data_dir", tree, "--vocab_file", VOCAB_FILE,
                       "--num_workers", "0", "--batch_size", "4", "--vocab_size", "256", "--emb_vocab", "256",
                       "--weight_decay", "0.01", "--ema_decay", "0.9", "--clip", "--smoothing", "0.1", "--epochs", "2",
                       "--resnet_layers", "1", "1", "1", "1", "--resnet_width", "8", "--hidden_size", "96", "--n_layers", "2",
                       "--image_size", "32", "--max_position_embeddings", "16", "--hidden_dropout_prob", "0.1", "--lr", "1e-3",
                       "--seed", "7", "--save_dir", str(tmp_path)])
    assert math.isfinite(best)
    losses = state["steps"]
    print("step losses:", " ".join(f"{v:.4f}" for v in losses), "validation:", " ".join(f"{e:.2e}" for e in state["val_err"]))
    # 11 questions in batches of 4: 3 steps an epoch; every question of the table once an epoch, on its own image's row
    assert len(losses) == 6 and all(math.isfinite(v) for v in losses)
    train_image_of = D.image_of_rows(tabs["train"])[1]
    assert sorted(state["rows"]) == sorted(train_image_of * 2) and state["views"] <= {0, 1}
    assert sorted(state["val_rows"]) == sorted(val_image_of * 2)
    # the fill decodes 3 train images x 2 views + 3 validation images, all before the first step; nothing after it
    assert len(decoded) == 3 * 2 + 3 and all(n_steps == 0 for _, n_steps in decoded), decoded
    assert max(state["val_err"]) <= TOL
    tokens = state["cache"].tokens
    assert float(tokens.abs().max()) > 0 and not torch.equal(tokens[:, 0], tokens[:, 1])     # view 1 is another view
    sd = checkpoint.read_state_dict(os.path.join(str(tmp_path), "MLM", "run_loss.pt"))
    frozen = [k for k in sd if k.startswith(VISUAL)]
    assert len(frozen) > 60 and all(torch.equal(sd[k].cpu(), state["init"][k]) for k in frozen)
    assert not torch.equal(sd["classifier.2.weight"].cpu(), state["init"]["classifier.2.weight"])
