#!/usr/bin/env python3
"""The distillation task (train.py distill) on the GPU.

1. The loss launch pair alone at (B T, H) = (1200, 768) (B 16, T 75, the reference's --max_position_embeddings): forward +
   backward of mmvqa_amd.distill_loss (one launch for the rows' distances and dh, the one-workgroup mean, the multiply by
   the upstream gradient) from an fp32 and an fp16 table, next to the unfused route in torch alone: a materialised
   [B, T, H] target (zeros + one slice copy per sample, from sizes known on the host) and F.mse_loss with autograd.  The
   forms alternate in one process on an idle device; device events around each forward + backward, median of 20.
2. The whole config-2 step (bench.py's model and batch: resnet152 + transformer, B 16, 224^2, T 32) of train.distill_step
   (headless model) against train.mlm_step (heads + the 30522-wide MLM loss), two models in one process, alternating
   blocks; a host clock around each block, which ends in a device synchronise.  Default launch choices, as train.py runs.

    python tools/distill_bench.py --out profiles/distill_cfg2.json
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
import torch.nn.functional as F  # noqa: E402

B, T, HW, VOCAB, H = 16, 32, 224, 30522, 768


def loss_launches(dev, reps=20, Bl=16, Tl=75):
    import mmvqa_amd
    from mmvqa_amd import synth
    (_img, _ids, _seg, _mask, start, count), table = synth.distill_batch(Bl, Tl, 8, vocab=VOCAB, D=H, seed=3, device=dev)
    g = torch.Generator().manual_seed(3)
    h = torch.randn(Bl, Tl, H, generator=g).to(dev).requires_grad_(True)
    t16 = table.half()
    st, ct = start.tolist(), [min(c, Tl - 8) for c in count.tolist()]          # the unfused route's sizes, on the host

    def unfused():
        tgt = torch.zeros(Bl, Tl, H, dtype=torch.float32, device=dev)
        for b in range(Bl):
            tgt[b, 7:7 + ct[b]] = table[st[b]:st[b] + ct[b]]
        return F.mse_loss(h, tgt)

    forms = {"distill_loss_fp32_table": lambda: mmvqa_amd.distill_loss(h, table, start, count, 5),
             "distill_loss_fp16_table": lambda: mmvqa_amd.distill_loss(h, t16, start, count, 5),
             "unfused_torch": unfused}
    ms = {k: [] for k in forms}
    for it in range(reps + 5):                      # 5 warm-up rounds; the forms alternate inside every round
        for k, fn in forms.items():
            h.grad = None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn().backward()
            e1.record()
            torch.cuda.synchronize()
            if it >= 5:
                ms[k].append(e0.elapsed_time(e1))
    out = {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ms.items()}
    out["rows"], out["H"], out["reps"] = Bl * Tl, H, reps
    return out


def whole_step(dev, blocks, steps, warmup):
    import mmvqa_amd
    from mmvqa_amd import synth, train
    from mmvqa_amd.ddp import GradReducer
    forms = {}
    for task in ("MLM", "distillation"):
        args = SimpleNamespace(task=task, dataset="roco", transformer_model="transformer", cnn_encoder="resnet152", num_vis=5,
                               hidden_size=H, n_layers=4, heads=12, hidden_dropout_prob=0.3, vocab_size=VOCAB, use_relu=False,
                               max_position_embeddings=T)
        torch.manual_seed(1234)
        model = mmvqa_amd.Model(args)
        model.to(dev).train()
        model.set_seed(1234)
        opt, red = mmvqa_amd.FusedAdam(model, lr=2e-5), GradReducer(model.flat_grads)
        if task == "MLM":
            batch = synth.roco_batch(B, T, HW, VOCAB, seed=1234, device=dev)
            forms["mlm"] = (lambda m=model, o=opt, r=red, b=batch: train.mlm_step(m, o, r, 1, b))
        else:
            batch, table = synth.distill_batch(B, T, HW, vocab=VOCAB, D=H, seed=1234, device=dev)
            forms["distill"] = (lambda m=model, o=opt, r=red, b=batch, t=table: train.distill_step(m, o, r, 1, b, t))
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(blocks):
        for k, fn in forms.items():
            t0 = time.perf_counter()
            for _s in range(steps):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps)
    out = {k: dict(blocks_ms_per_step=v, median_ms_per_step=statistics.median(v)) for k, v in ms.items()}
    out["difference_ms"] = out["distill"]["median_ms_per_step"] - out["mlm"]["median_ms_per_step"]
    out["mlm_block_spread_ms"] = max(ms["mlm"]) - min(ms["mlm"])
    out["blocks"], out["steps_per_block"], out["warmup_steps"] = blocks, steps, warmup
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8, help="steps per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip_step", action="store_true", help="the loss launches only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("distill_bench.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), shape=dict(B=B, T=T, H=H, image=HW), loss_launch=loss_launches(dev))
    print(json.dumps(res["loss_launch"]), flush=True)
    if not a.skip_step:
        res["config2_step"] = whole_step(dev, a.blocks, a.steps, a.warmup)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
