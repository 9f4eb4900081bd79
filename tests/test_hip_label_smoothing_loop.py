"""Label smoothing by question category through the loops on the GPU: the VQA step against the oracle loop restated with
the reference's three-argument criterion (vqamed2019/utils.py:633-673 with args.smoothing), one mixed-precision step,
validation through the criterion's eval branch, the feeder's category ids, and the CLI."""
import math

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

import mmvqa_amd  # noqa: E402
from mmvqa_amd import data as D  # noqa: E402
from mmvqa_amd import evaluate, synth, train  # noqa: E402
from mmvqa_amd.amp import GradScaler  # noqa: E402
from mmvqa_amd.ddp import GradReducer  # noqa: E402
from hip_helpers import dev  # noqa: E402
from test_hip_loops import LR, check_param_deltas, to_dev  # noqa: E402
from test_hip_model import build_pair, mini_args  # noqa: E402
import label_smoothing_helpers as H  # noqa: E402

SM, NC = 0.1, 23


def vqa_train_one_epoch_smoothing(loader, model, optimizer, criterion, clip=False):
    """oracle.loops_oracle.vqa_train_one_epoch (vqamed2019/utils.py:625-688) with args.smoothing set: the loader item
    carries the category and the loss is criterion(logits, target, category) (:648-649)"""
    model.train()
    losses, PREDS = [], []
    for img, question_token, segment_ids, attention_mask, target, category in loader:
        optimizer.zero_grad()
        logits, _, _ = model(img, question_token, segment_ids, attention_mask)
        loss = criterion(logits, target, category)
        loss.backward()
        if clip:
            nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        optimizer.step()
        PREDS.append(logits.softmax(1).argmax(1).detach())
        losses.append(loss.detach().cpu().numpy())
    return losses, PREDS


def loader6(n=2):
    return [synth.vqa_batch(4, 10, 32, vocab=50, n_classes=NC, seed=50 + i) + (synth.vqa_categories(4, NC, seed=50 + i),)
            for i in range(n)]


@pytest.mark.parametrize("clip", [False, True])
def test_vqa_loop_with_smoothing_matches_oracle_loop(clip):
    args = mini_args(transformer_model="realformer", dataset="VQA-Med", vocab_size=NC)
    orc, hip = build_pair(args, seed=23)
    before = {k: v.detach().clone() for k, v in orc.named_parameters()}
    loader = loader6()
    crit = mmvqa_amd.CategorySmoothing(synth.vqa_category_rows(NC), NC, SM).to(dev())
    names, table_ref = H.category_table(synth.vqa_category_rows(NC), NC, SM)      # the oracle's own table, not crit's
    assert names == crit.categories
    crit_ref = lambda lg, t, c: H.soft_ce(lg, H.soft_targets(H.CATEGORY, t, NC, SM, table_ref, c, lg.dtype))   # noqa: E731
    opt_ref = torch.optim.Adam(orc.parameters(), lr=LR)
    ref_losses, ref_preds = vqa_train_one_epoch_smoothing(loader, orc, opt_ref, crit_ref, clip=clip)
    hip.train()
    opt = mmvqa_amd.FusedAdam(hip, lr=LR)
    red = GradReducer(hip.flat_grads)
    for i, b in enumerate(loader):
        loss, pred = train.vqa_step(hip, opt, red, 1, to_dev(b), crit, clip=clip)
        print(f"step {i}: loss {float(loss):.6f} oracle {float(ref_losses[i]):.6f}")
        assert abs(float(loss) - float(ref_losses[i])) <= 1e-3 * abs(float(ref_losses[i])), (i, float(loss), float(ref_losses[i]))
        assert torch.equal(pred.cpu(), ref_preds[i])
    check_param_deltas(orc, hip, before)


def test_five_tuple_batches_still_step_with_two_argument_criteria():
    args = mini_args(dataset="VQA-Med", vocab_size=NC)
    _, hip = build_pair(args, seed=4)
    hip.train()
    opt, red = mmvqa_amd.FusedAdam(hip, lr=LR), GradReducer(hip.flat_grads)
    b = to_dev(loader6(1)[0])
    loss, _ = train.vqa_step(hip, opt, red, 1, b[:5], lambda lg, t: mmvqa_amd.mlm_loss(lg, t)[0])
    assert math.isfinite(float(loss))
    with pytest.raises(ValueError, match="category ids"):
        train.vqa_step(hip, opt, red, 1, b[:5], mmvqa_amd.CategorySmoothing(synth.vqa_category_rows(NC), NC, SM).to(dev()))


def test_one_mixed_precision_step_is_finite():
    args = mini_args(dataset="VQA-Med", vocab_size=NC)
    _, hip = build_pair(args, seed=5)
    hip.train()
    opt, red = mmvqa_amd.FusedAdam(hip, lr=LR), GradReducer(hip.flat_grads)
    crit = mmvqa_amd.CategorySmoothing(synth.vqa_category_rows(NC), NC, SM).to(dev())
    before = [p.detach().clone() for p in hip.parameters()]
    loss, pred = train.vqa_step(hip, opt, red, 1, to_dev(loader6(1)[0]), crit, scaler=GradScaler())
    torch.cuda.synchronize()
    assert math.isfinite(float(loss)) and pred.shape == (4,)
    assert all(bool(torch.isfinite(p).all()) for p in hip.parameters())
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, hip.parameters()))   # the step was not skipped


def test_validate_uses_the_eval_branch():
    args = mini_args(dataset="VQA-Med", vocab_size=NC)
    _, hip = build_pair(args, seed=6)
    loader = [to_dev(b[:5]) for b in loader6(2)]
    cats = [synth.VQA_CATEGORIES[int(c)] for b in loader6(2) for c in b[5]]
    idx2ans = {i: f"answer {i}" for i in range(NC)}
    crit = mmvqa_amd.CategorySmoothing(synth.vqa_category_rows(NC), NC, SM).to(dev())
    assert crit.training
    vl, preds, _acc, _bleu = evaluate.validate(loader, hip, crit, cats, idx2ans)
    assert not crit.training                                            # utils.py:693
    vl_ce, preds_ce, _a, _b = evaluate.validate(loader, hip, lambda lg, t: mmvqa_amd.mlm_loss(lg, t)[0], cats, idx2ans)
    assert float(vl) == float(vl_ce) and np.array_equal(preds, preds_ce)
    tl, _p, _a, _b = evaluate.test(loader, hip, mmvqa_amd.LabelSmoothing(SM), cats, idx2ans)
    assert float(tl) == float(vl_ce)


def test_feeder_hands_out_category_ids(tmp_path):
    from feeder_helpers import make_vqa_tree, tokenizer
    root = make_vqa_tree(str(tmp_path / "vqa"))
    _cols, tabs, idx2ans = D.vqa_tables(root)
    rows = tabs["train"]
    crit = mmvqa_amd.CategorySmoothing(rows, len(idx2ans), SM)
    assert crit.cat2idx == D.category_ids(rows) and len(crit.categories) == 5
    tok = tokenizer()
    host = D.HostLoader(D.VqaDataset(rows, tok, 16, categories=crit.cat2idx), 4, shuffle=True, seed=3, num_workers=0,
                        aug=D.VQA_AUG, size=32)
    fd = D.DeviceFeeder(host, "cuda", category=True)
    seen = []
    for epoch in range(2):
        fd.set_epoch(epoch)
        got = [tuple(t.clone() for t in b) for b in fd]
        torch.cuda.synchronize()
        log = fd.log[-len(got):]
        assert [len(e["index"]) for e in log] == [4, 4, 2]
        for b, e in zip(got, log):
            assert len(b) == 6 and b[5].dtype == torch.int64 and b[5].is_cuda
            want = [crit.cat2idx[rows[i][3]] for i in e["index"]]
            assert b[5].cpu().tolist() == want == e["category"]
            assert b[4].cpu().tolist() == [rows[i][2] for i in e["index"]]
        seen.append([e["index"] for e in log])
    assert seen[0] != seen[1]                                            # the two epochs are different permutations
    plain = D.DeviceFeeder(D.HostLoader(D.VqaDataset(rows, tok, 16), 4, shuffle=True, seed=3, num_workers=0,
                                        aug=D.VQA_AUG, size=32), "cuda")
    plain.set_epoch(1)
    base = [tuple(t.clone() for t in b) for b in plain]
    torch.cuda.synchronize()
    assert all(len(b) == 5 for b in base)                                # the default batch is the 5-tuple, unchanged:
    assert all(torch.equal(x, y) for a, b in zip(base, got) for x, y in zip(a, b[:5]))   # same tensors as with the ids
    with pytest.raises(ValueError, match="carry no `category`"):
        next(iter(D.DeviceFeeder(plain.host, "cuda", category=True)))


MINI = ["--resnet_layers", "1", "1", "1", "1", "--resnet_width", "8", "--hidden_size", "96", "--n_layers", "2",
        "--vocab_size", "64", "--emb_vocab", "64", "--image_size", "32", "--steps_per_epoch", "2", "--val_steps", "1",
        "--epochs", "1", "--max_position_embeddings", "16", "--hidden_dropout_prob", "0.1"]


def test_cli_trains_with_smoothing(tmp_path, capsys):
    best = train.main(["vqa", "--lr", "1e-3", "--batch_size", "8", "--smoothing", "0.1", "--loss", "ASLSingleLabel",
                       "--num_classes", "11", "--save_dir", str(tmp_path)] + MINI)
    assert math.isfinite(best) and best < 10.0
    assert "train_loss" in capsys.readouterr().out
    assert (tmp_path / "MLM" / "run_loss.pt").exists()
    sd = torch.load(tmp_path / "MLM" / "run_loss.pt", weights_only=False)
    assert not any("smooth" in k or "table" in k for k in sd)           # nothing new goes into checkpoints
