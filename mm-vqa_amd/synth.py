"""Synthetic inputs with the layout of the reference's data layer.

ROCO / MLM (pretrain/roco_utils.py:162-199): tokens [CLS] + 5 visual slots (id 0) + [SEP] + caption +
[SEP] + padding; segment ids 0*7, 1*(n+1), 0*pad; mask 1*(8+n); labels = original id at [MASK]ed caption
positions, 0 elsewhere.  VQA-Med (vqamed2019/utils.py:156-170): same token layout, one class id per sample.
"""
from __future__ import annotations

import torch


def roco_batch(B, T=32, hw=224, vocab=30522, seed=1234, device="cpu", mlm_prob=0.15):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(B, 3, hw, hw, generator=g) * 2 - 1
    ids = torch.zeros(B, T, dtype=torch.long)
    seg = torch.zeros(B, T, dtype=torch.long)
    mask = torch.zeros(B, T, dtype=torch.long)
    tgt = torch.zeros(B, T, dtype=torch.long)
    lo = min(1000, max(1, vocab // 2))
    for b in range(B):
        n_max = T - 8                      # [CLS] + 5 visual slots + 2x[SEP] are always present
        n = int(torch.randint(min(4, n_max), n_max + 1, (1,), generator=g))
        cap = torch.randint(lo, vocab, (n,), generator=g)
        m = torch.rand(n, generator=g) < mlm_prob
        ids[b, 0] = 101 % vocab
        ids[b, 6] = 102 % vocab
        ids[b, 7:7 + n] = torch.where(m, torch.full_like(cap, 103 % vocab), cap)
        ids[b, 7 + n] = 102 % vocab
        tgt[b, 7:7 + n] = torch.where(m, cap, torch.zeros_like(cap))
        seg[b, 7:8 + n] = 1
        mask[b, :8 + n] = 1
    return tuple(t.to(device) for t in (img, ids, seg, mask, tgt))


def vqa_batch(B, T=32, hw=224, vocab=30522, n_classes=1552, seed=1234, device="cpu"):
    img, ids, seg, mask, _ = roco_batch(B, T, hw, vocab, seed, "cpu", mlm_prob=0.0)
    g = torch.Generator().manual_seed(seed + 77)
    tgt = torch.randint(0, n_classes, (B,), generator=g)
    return tuple(t.to(device) for t in (img, ids, seg, mask, tgt))


def vqa_grouped_batch(NI, counts, T=32, hw=224, vocab=30522, n_classes=1552, seed=1234, device="cpu"):
    """A grouped VQA batch (Model.forward_grouped): NI images, counts[i] questions of image i, B = sum(counts) rows.
    -> (img [NI,3,hw,hw], group [B] int64 on the HOST, ids, seg, mask [B,T], tgt [B]).  The text rows and targets are
    those of vqa_batch(B, ...) at the same seed, the images its first NI."""
    counts = [int(c) for c in counts]
    if len(counts) != NI or min(counts, default=0) < 1:
        raise ValueError(f"counts must name at least one question for each of the {NI} images, not {counts}")
    B = sum(counts)
    img, ids, seg, mask, tgt = vqa_batch(B, T, hw, vocab, n_classes, seed, "cpu")
    group = torch.repeat_interleave(torch.arange(NI), torch.tensor(counts))
    img = img[:NI].contiguous()
    return (img.to(device), group) + tuple(t.to(device) for t in (ids, seg, mask, tgt))


def distill_batch(B, T=32, hw=224, vocab=28996, D=768, seed=1234, device="cpu", num_vis=5):
    """A batch of the distillation task (pretrain/roco_utils.py:162-199, task 'distillation') and a small seeded teacher
    table: ((img, ids, seg, mask, start, count), table).  table [total, D] fp32 holds the per-token states of the batch's
    captions back to back; start int64 [B] / count int32 [B] name each caption's rows.  Caption lengths include 0 and one
    above T - num_vis - 3 (the surplus token is cut from ids, as encode_text cuts it; count keeps it), the rest are drawn."""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(B, 3, hw, hw, generator=g) * 2 - 1
    ids = torch.zeros(B, T, dtype=torch.long)
    seg = torch.zeros(B, T, dtype=torch.long)
    mask = torch.zeros(B, T, dtype=torch.long)
    n_max, first = T - (num_vis + 3), num_vis + 2
    lo = min(1000, max(1, vocab // 2))
    lens = [(0, n_max + 1)[b] if b < 2 else int(torch.randint(0, n_max + 1, (1,), generator=g)) for b in range(B)]
    start = torch.tensor([sum(lens[:b]) for b in range(B)], dtype=torch.int64)
    count = torch.tensor(lens, dtype=torch.int32)
    table = torch.randn(max(sum(lens), 1), D, generator=g) * 0.5
    for b, n_all in enumerate(lens):
        n = min(n_all, n_max)
        ids[b, 0] = 101 % vocab
        ids[b, first - 1] = 102 % vocab
        ids[b, first:first + n] = torch.randint(lo, vocab, (n_all,), generator=g)[:n]
        ids[b, first + n] = 102 % vocab
        seg[b, first:first + n + 1] = 1
        mask[b, :first + n + 1] = 1
    return tuple(t.to(device) for t in (img, ids, seg, mask, start, count)), table.to(device)


VQA_CATEGORIES = ("modality", "plane", "organ", "abnormality", "binary")   # the five question types of VQA-Med-2019


def vqa_category_rows(n_classes):
    """A synthetic train table for label smoothing by category: one row per class, class c in category
    VQA_CATEGORIES[c % 5], in the row layout of data.vqa_tables (image path, question, answer index, category, mode).
    In first-appearance order category id i is VQA_CATEGORIES[i]."""
    return [(f"synpic{c}.jpg", f"what is shown in image {c}?", c, VQA_CATEGORIES[c % len(VQA_CATEGORIES)], "train")
            for c in range(n_classes)]


def vqa_categories(B, n_classes=1552, seed=1234, device="cpu"):
    """category ids [B] (int64) of vqa_batch(B, ..., n_classes, seed): the batch's targets are drawn again from the
    batch seed and sample b gets the category of its class, target_b % 5 -- the partition of vqa_category_rows, so
    every target lies in its category's answer set"""
    g = torch.Generator().manual_seed(seed + 77)
    tgt = torch.randint(0, n_classes, (B,), generator=g)
    return (tgt % len(VQA_CATEGORIES)).to(device)


def vqa_test_table(n, n_classes, seed=1234, data_dir="../ImageClef-2019-VQA-Med"):
    """A synthetic stand-in for the test split's table as vqamed2019/utils.py:51-79 (load_data) + eval.py:84-97 leave
    it: columns (img_id, question, answer, category, mode) with img_id a path under <data_dir>/Test/images, answer the
    class id.  Returns (columns, rows, idx2ans)."""
    g = torch.Generator().manual_seed(seed + 4242)
    ans = torch.randint(0, n_classes, (n,), generator=g).tolist()
    cat = torch.randint(0, len(VQA_CATEGORIES), (n,), generator=g).tolist()
    cols = ["img_id", "question", "answer", "category", "mode"]
    rows = [(f"{data_dir}/Test/images/synpic{10000 + i}.jpg", f"what is shown in image {i}?", ans[i], VQA_CATEGORIES[cat[i]], "test")
            for i in range(n)]
    idx2ans = {i: f"answer {i}" if i % 3 else f"finding, type {i}" for i in range(n_classes)}
    return cols, rows, idx2ans
