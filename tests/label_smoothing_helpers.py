"""Oracle of the label-smoothing criteria, beside the tests (oracle/ is frozen): a restatement of
vqamed2019/utils.py:1234-1300 (LabelSmoothByCategory) and :178-200 (LabelSmoothing) as one soft-target cross entropy.
It is itself pinned to the reference by tests/golden/label_smoothing.npz (test_label_smoothing_cpu.py).  Runs in the
dtype of the logits: float64 logits give the truth run.  The soft targets are the fp32 numbers the reference holds (the
table entries and the confidence are rounded to fp32 when they are stored into its float tensors), widened exactly."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HARD, UNIFORM, CATEGORY = 0, 1, 2
ORDER = ["plane", "modality", "binary", "organ", "abnormality"]      # utils.py:1292-1293


def fixture():
    return dict(np.load(os.path.join(GOLDEN, "label_smoothing.npz")))


def fixture_rows(g, C):
    """the fixture's train frame in the row layout of data.vqa_tables (path, question, answer index, category, mode)"""
    return [(f"img{i}.jpg", "q", int(a), str(c), "train")
            for i, (c, a) in enumerate(zip(g[f"c{C}_train_category"], g[f"c{C}_train_answer"]))]


def category_table(rows, num_classes, smoothing):
    """computeCategoryTensors (:1266-1293) for any categories -> (names in first-appearance order, fp32 [n_cat, C])"""
    names = []
    for r in rows:
        if r[3] not in names:
            names.append(r[3])
    table = torch.zeros(len(names), num_classes)
    for i, c in enumerate(names):
        idx = torch.tensor(sorted({int(r[2]) for r in rows if r[3] == c}), dtype=torch.long)
        table[i, idx] = smoothing / len(idx)
    return names, table


def soft_targets(mode, target, C, smoothing=0.0, table=None, category=None, dtype=torch.float64):
    """[rows, C] soft targets: HARD one-hot; UNIFORM smoothing / C + confidence one-hot (:190-195 folded into one
    target); CATEGORY table[category] with the target entry OVERWRITTEN by the confidence (:1249-1256)"""
    rows = target.shape[0]
    conf = torch.tensor(1.0 if mode == HARD else 1.0 - smoothing, dtype=torch.float32).to(dtype)
    r = torch.arange(rows)
    if mode == CATEGORY:
        soft = table.float()[category.long()].clone().to(dtype)
        soft[r, target.long()] = conf
        return soft
    base = torch.tensor(smoothing / C if mode == UNIFORM else 0.0, dtype=torch.float32).to(dtype)
    soft = torch.full((rows, C), 1.0, dtype=dtype) * base
    soft[r, target.long()] += conf
    return soft


def soft_ce(logits, soft):
    """mean_rows(sum_j -soft_j log_softmax(x)_j) (:1296-1300), differentiable in the logits"""
    return -(soft * torch.log_softmax(logits, dim=1)).sum(1).mean()


def loss_and_grad(logits, soft):
    x = logits.clone().requires_grad_(True)
    loss = soft_ce(x, soft)
    loss.backward()
    return loss.detach(), x.grad


def closed_form_grad(logits, soft):
    """(S p - soft) / rows with S the row sum of the soft target"""
    return (soft.sum(1, keepdim=True) * torch.softmax(logits, dim=1) - soft) / logits.shape[0]


def case(rows, C, scale, seed, n_cat=5):
    """seeded logits (|x| ~ scale), targets, categories and a category table with sets of different sizes: category k
    owns the classes c with c % n_cat == k below 0.9 C (the top tenth is in no set), a category k >= 0.9 C is left EMPTY
    (C = 3: categories 2, 3, 4)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) * scale
    tgt = torch.randint(0, C, (rows,), generator=g)
    cat = torch.randint(0, n_cat, (rows,), generator=g)
    table = torch.zeros(n_cat, C)
    lim = max(1, int(0.9 * C))
    for k in range(n_cat):
        if k < lim:
            idx = torch.arange(k, lim, n_cat)
            table[k, idx] = 0.1 / idx.numel()
    return x, tgt, cat, table
