#!/usr/bin/env python3
"""Label smoothing by category (train.py vqa --smoothing) against the cross-entropy path, on the GPU.

1. The loss launch alone, at config 5's shape (B 64, C 1552): forward + backward of mmvqa_amd.soft_ce_loss (category
   mode: one launch + the one-workgroup mean) next to mlm_loss (statistics, reduce and the gradient launch) and asl_loss,
   alternating in one process on an idle device; device events around each forward + backward, median of 20.
2. The whole config-5 step (bench.py --config 5's model and batch: tf_efficientnetv2_m + realformer, B 64, 224^2, T 28)
   with the smoothing criterion against the cross-entropy criterion, in alternating blocks of one process; a host clock
   around each block, which ends in a device synchronise.  The step is train.vqa_step with the launcher's default tiles,
   as train.py runs it; --tune selects tiles per shape first, as bench.py does, for a figure next to bench.py --config 5.

    python tools/label_smoothing_bench.py --out profiles/label_smoothing_cfg5.json
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, T, HW, VOCAB, C = 64, 28, 224, 30522, 1552


def loss_launches(dev, reps=20):
    import mmvqa_amd
    from mmvqa_amd import synth
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(B, C, generator=g) * 2).to(dev).requires_grad_(True)
    tgt = torch.randint(0, C, (B,), generator=g).to(dev)
    cat = (tgt % 5).to(dev)
    crit = mmvqa_amd.CategorySmoothing(synth.vqa_category_rows(C), C, 0.1).to(dev)
    forms = {"soft_ce_category": lambda: crit(x, tgt, cat),
             "mlm_loss": lambda: mmvqa_amd.mlm_loss(x, tgt)[0],
             "asl_loss": lambda: mmvqa_amd.asl_loss(x, tgt)}
    ms = {k: [] for k in forms}
    for it in range(reps + 5):                      # 5 warm-up rounds; the forms alternate inside every round
        for k, fn in forms.items():
            x.grad = None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn().backward()
            e1.record()
            torch.cuda.synchronize()
            if it >= 5:
                ms[k].append(e0.elapsed_time(e1))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ms.items()}


def whole_step(dev, blocks, steps, warmup, tune):
    import mmvqa_amd
    from mmvqa_amd import synth, train
    from mmvqa_amd.ddp import GradReducer
    args = SimpleNamespace(task="VQA", dataset="VQA-Med", transformer_model="realformer", cnn_encoder="tf_efficientnetv2_m",
                           num_vis=5, hidden_size=768, n_layers=4, heads=12, hidden_dropout_prob=0.3, vocab_size=C,
                           emb_vocab=VOCAB, use_relu=False, max_position_embeddings=T)
    torch.manual_seed(1234)
    model = mmvqa_amd.Model(args)
    model.to(dev).train()
    model.set_seed(1234)
    opt = mmvqa_amd.FusedAdam(model, lr=2e-5)
    red = GradReducer(model.flat_grads)
    batch = synth.vqa_batch(B, T, HW, VOCAB, C, seed=1234, device=dev)
    batch6 = batch + (synth.vqa_categories(B, C, seed=1234, device=dev),)
    smooth = mmvqa_amd.CategorySmoothing(synth.vqa_category_rows(C), C, 0.1).to(dev)
    forms = {"cross_entropy": (batch, lambda lg, t: mmvqa_amd.mlm_loss(lg, t)[0]), "smoothing_0.1": (batch6, smooth)}
    if tune:                                        # per-shape tile / split-K selection, as bench.py makes it
        model.tune(*batch[:4])
    for _ in range(warmup):
        for b, crit in forms.values():
            train.vqa_step(model, opt, red, 1, b, crit)
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(blocks):
        for k, (b, crit) in forms.items():
            t0 = time.perf_counter()
            for _s in range(steps):
                train.vqa_step(model, opt, red, 1, b, crit)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps)
    out = {k: dict(blocks_ms_per_step=v, median_ms_per_step=statistics.median(v)) for k, v in ms.items()}
    out["tuned"] = bool(tune)
    ce = ms["cross_entropy"]
    out["difference_ms"] = out["smoothing_0.1"]["median_ms_per_step"] - out["cross_entropy"]["median_ms_per_step"]
    out["cross_entropy_block_spread_ms"] = max(ce) - min(ce)
    out["difference_inside_spread"] = abs(out["difference_ms"]) <= out["cross_entropy_block_spread_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8, help="steps per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip_step", action="store_true", help="the loss launches only")
    ap.add_argument("--tune", action="store_true", help="Model.tune() before the step, as bench.py does (train.py does not)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("label_smoothing_bench.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    res = dict(shape=dict(B=B, C=C, T=T, image=HW), loss_launch=loss_launches(dev))
    print(json.dumps(res["loss_launch"]), flush=True)
    if not a.skip_step:
        res["config5_step"] = whole_step(dev, a.blocks, a.steps, a.warmup, a.tune)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
