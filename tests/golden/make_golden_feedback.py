#!/usr/bin/env python3
"""Golden vectors that pin tests/feedback_helpers.FeedbackBlock to the reference's FeedbackTransformer.

Run ONCE where a checkout of the reference (DannielSilva/MM-VQA) is at hand, from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_feedback.py <path of the reference checkout>

It imports the reference's own class from that checkout on CPU (needs einops), gives it the weights
feedback_helpers.seeded_weights draws from numpy.random.RandomState(seed), runs it in eval mode on a seeded input, and
stores the input, the output, the output gradient it was given, the gradients of the input and of every parameter that
receives one, the reference's state_dict key list, and the distance of this fp32 run from the same run in fp64.
Weights are not stored: the test draws them again.  Only data is written -- no reference source text.

Two files, each under the 1 MB limit for a committed file: feedback.npz (T 12 and T 2), feedback_odd.npz (T 11).
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "models")):
    sys.exit("usage: make_golden_feedback.py <path of the reference checkout>")
sys.path.insert(0, os.path.abspath(sys.argv[1]))
sys.dont_write_bytecode = True

from models.feedback_transformer_pytorch import FeedbackTransformer  # noqa: E402
import feedback_helpers as FH  # noqa: E402

NUM_TOKENS = 16
# (tag, file, dim, depth, B, T, seed)
CASES = (("d2_t12", "feedback.npz", 32, 2, 3, 12, 11), ("d1_t2", "feedback.npz", 32, 1, 3, 2, 12),
         ("d2_t11", "feedback_odd.npz", 32, 2, 3, 11, 13))


def relerr(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def run(model, x, dy):
    x = x.clone().requires_grad_(True)
    model.zero_grad()
    out = model(x)
    out.backward(dy)
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    return out.detach(), x.grad.clone(), grads


def main():
    files = {}
    for tag, fname, dim, depth, B, T, seed in CASES:
        ref = FeedbackTransformer(num_tokens=NUM_TOKENS, dim=dim, depth=depth, seq_len=2, mem_len=256, dim_head=64, heads=8,
                                  attn_dropout=0.1, ff_dropout=0.1).eval()
        FH.seeded_weights(ref, seed)
        rs = np.random.RandomState(seed + 1000)
        x = torch.from_numpy(rs.standard_normal((B, T, dim))).float()
        dy = torch.from_numpy(rs.standard_normal((B, T, dim))).float()
        out, dx, grads = run(ref, x, dy)
        out64, dx64, grads64 = run(copy.deepcopy(ref).double(), x.double(), dy.double())
        assert set(grads) == set(grads64)
        dist = max([relerr(out, out64), relerr(dx, dx64)] + [relerr(grads[n], grads64[n]) for n in grads])
        d = files.setdefault(fname, {})
        d[f"{tag}/cfg"] = np.array([dim, depth, B, T, seed, NUM_TOKENS], dtype=np.int64)
        d[f"{tag}/x"], d[f"{tag}/dy"], d[f"{tag}/out"], d[f"{tag}/dx"] = x.numpy(), dy.numpy(), out.numpy(), dx.numpy()
        d[f"{tag}/fp64_dist"] = np.array(dist)
        d[f"{tag}/keys"] = np.array(list(ref.state_dict().keys()))
        d[f"{tag}/param_names"] = np.array([n for n, _ in ref.named_parameters()])
        for n, g in grads.items():
            d[f"{tag}/grad/{n}"] = g.numpy()
        print(f"{tag}: fp32 vs fp64 {dist:.2e}, {len(grads)} gradients, layer_weight grad "
              f"{'present' if 'layer_weight' in grads else 'absent'}")
    for fname, d in files.items():
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **d)
        print(fname, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
