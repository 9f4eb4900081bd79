"""Oracle of SupCon with a positive mask, beside the tests (oracle/ is frozen): a restatement of
models/SupConLoss/loss.py:21-98 (contrast_mode 'all', two views) in the closed form the HIP kernels implement.  It is
itself pinned to the reference by tests/golden/supcon_mask.npz (test_supcon_mask_cpu.py).  Runs in the dtype of the
features: float64 features give the truth run (feed it a mask that fp32 represents exactly -- the reference rounds the
mask to fp32 before use)."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def supcon_masked(features, mask, temperature=0.07, base_temperature=0.07):
    """features [N, 2, D], mask [N, N] -> loss (differentiable in the features)"""
    R = 2 * features.shape[0]
    f = torch.cat(torch.unbind(features, dim=1), dim=0)
    z = f @ f.T / temperature
    logits = z - z.max(dim=1, keepdim=True)[0].detach()             # row max over all columns, the diagonal included
    eye = torch.eye(R, dtype=torch.bool, device=f.device)
    mt = mask.float().to(f.dtype).repeat(2, 2).masked_fill(eye, 0.0)
    lse = torch.log(torch.exp(logits).masked_fill(eye, 0.0).sum(1, keepdim=True))
    row = (mt * (logits - lse)).sum(1) / mt.sum(1)
    return -(temperature / base_temperature) * row.mean()


def labels_mask(labels):
    y = labels.view(-1, 1)
    return torch.eq(y, y.T).float()


def soft_mask(n, seed, density=0.6):
    """asymmetric soft mask with unit diagonal, fp32"""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(n, n, generator=g) * (torch.rand(n, n, generator=g) < density).float()
    return m.fill_diagonal_(1.0)


def fixture():
    return dict(np.load(os.path.join(GOLDEN, "supcon_mask.npz")))


def fixture_texts():
    """(captions, augs) of the fixture's Jaccard matrix, and rows of four texts that hold them: (caption i, aug i and
    two respellings of it with the same word set), so columns 1..3 all name B_i"""
    with open(os.path.join(GOLDEN, "supcon_mask_texts.json")) as fh:
        t = json.load(fh)
    rows = [(c, a, a.upper(), "\t " + a.replace(" ", "  ") + "\n") for c, a in zip(t["captions"], t["augs"])]
    return t["captions"], t["augs"], rows


def jaccard_strings(captions, augs):
    """the definition, straight from the strings (supcon_utils.py:110-138), fp32"""
    n = len(captions)
    out = np.zeros((n, n), dtype=np.float32)
    for i in range(n):
        for j in range(n):
            if i == j:
                out[i, j] = 1.0
                continue
            a, b = set(captions[i].lower().split()), set(augs[j].lower().split())
            u = len(a | b)
            out[i, j] = np.float32(float(len(a & b)) / u) if u else 0.0
    return out


def random_word_sets(n_rows, lengths, vocab, seed):
    """a data.WordSets over generated texts: text (row, col) has lengths[(row * 4 + col) % len(lengths)] distinct words
    drawn from `vocab` words (small vocab => large overlaps); returns (WordSets, texts)"""
    from mmvqa_amd import data as D
    rng = np.random.default_rng(seed)
    texts = []
    for r in range(n_rows):
        row = []
        for c in range(4):
            k = lengths[(r * 4 + c) % len(lengths)]
            row.append(" ".join(f"w{v}" for v in rng.choice(vocab, size=k, replace=False)))
        texts.append(tuple(row))
    return D.WordSets.from_texts(texts), texts
