#!/usr/bin/env python3
"""The BERT teacher (mmvqa_amd.teacher, csrc/bertattn.hip + csrc/teacher.cpp) on the GPU.

1. The attention launch alone at B 16, 12 heads, T 128, head dimension 64, q / k / v inside one fused [B T][3 hidden]
   buffer: mmvqa_attention_len_fwd (run-time key loop, online softmax, nothing saved; all lengths = T) against
   mmvqa_attention's forward (compile-time key tiles, writes the probabilities its backward needs; mask of ones, no
   dropout).  The two alternate in one process on an idle device; device events around each launch, median of 20.
2. The forward of a 12-layer, 768-wide teacher (BERT-base geometry, random weights) at B 16 and T in {32, 64, 128, 512},
   every length = T: device events around BertTeacher.forward, median of 20, the shapes alternating.
3. The whole config-2 step (bench.py's model and batch: resnet152 + transformer, B 16, 224^2, T 32) of
   train.distill_step with the teacher run per batch (teacher rows of 26 tokens: [CLS], the 24 caption ids the student
   can hold, [SEP]) against the same step from a resident table of states; two models in one process, alternating
   blocks, a host clock around each block, which ends in a device synchronise (the method of tools/distill_bench.py).

    python tools/teacher_bench.py --out profiles/teacher_cfg2.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, T, HW, VOCAB, H, HEADS = 16, 32, 224, 30522, 768, 12


def _timed(forms, reps, warm=5):
    ms = {k: [] for k in forms}
    for it in range(reps + warm):                   # the forms alternate inside every round
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warm:
                ms[k].append(e0.elapsed_time(e1))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ms.items()}


def attention_alone(dev, reps=20, Ta=128):
    from mmvqa_amd import _lib as L
    from mmvqa_amd.teacher import attention_len_fwd
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(B, Ta, 3 * H, generator=g).to(dev)
    q, k, v = (qkv[:, :, i * H:(i + 1) * H].view(B, Ta, HEADS, 64) for i in range(3))
    lens = torch.full((B,), Ta, dtype=torch.int32, device=dev)
    out = torch.empty(B, Ta, HEADS, 64, device=dev)
    mask = torch.ones(B, Ta, dtype=torch.int64, device=dev)
    probs = torch.empty(B, HEADS, Ta, Ta, device=dev)
    out2 = torch.empty(B * Ta, H, device=dev)
    d = L.AttnDesc()
    d.q, d.k, d.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    d.row_stride, d.head_stride = 3 * H, 64
    d.out, d.out_row_stride, d.out_head_stride = out2.data_ptr(), H, 64
    d.mask, d.probs = mask.data_ptr(), probs.data_ptr()
    d.B, d.T, d.heads, d.sqrt_d = B, Ta, HEADS, 8.0
    lib = L.lib()
    forms = {"attention_len_fwd": lambda: attention_len_fwd(q, k, v, lens, out=out),
             "attention_fwd_T128": lambda: L.check(lib.mmvqa_attention(C.byref(d), 64, 0, L.stream_ptr()))}
    res = _timed(forms, reps)
    err = float((out.view(B * Ta, H) - out2).abs().max())
    res.update(B=B, T=Ta, heads=HEADS, reps=reps, max_abs_difference=err,
               ratio_len_over_T128=res["attention_len_fwd"]["median_ms"] / res["attention_fwd_T128"]["median_ms"])
    return res


def teacher_forward(dev, reps=20):
    from mmvqa_amd.teacher import BertTeacher
    teacher = BertTeacher.random(12, H, 4 * H, VOCAB, 512, seed=2).to(dev)
    g = torch.Generator().manual_seed(3)
    forms = {}
    for Tt in (32, 64, 128, 512):
        ids = torch.randint(1, VOCAB, (B, Tt), generator=g).to(dev)
        lens = torch.full((B,), Tt, dtype=torch.int32, device=dev)
        forms[f"T{Tt}"] = (lambda i=ids, n=lens: teacher(i, n))
    res = _timed(forms, reps)
    for Tt in (32, 64, 128, 512):
        M = B * Tt
        flops = 12 * (2.0 * M * H * (3 * H + H + 8 * H) + 4.0 * B * HEADS * Tt * Tt * 64)
        r = res[f"T{Tt}"]
        r["gflop"] = flops / 1e9
        r["tflops"] = flops / (r["median_ms"] * 1e-3) / 1e12
    res.update(B=B, layers=12, hidden=H, reps=reps)
    return res


def whole_step(dev, blocks, steps, warmup):
    import mmvqa_amd
    from mmvqa_amd import synth, train
    from mmvqa_amd.ddp import GradReducer
    from mmvqa_amd.teacher import BertTeacher
    teacher = BertTeacher.random(12, H, 4 * H, VOCAB, 512, seed=2).to(dev)
    forms = {}
    for form in ("resident_table", "online_teacher"):
        args = SimpleNamespace(task="distillation", dataset="roco", transformer_model="transformer", cnn_encoder="resnet152",
                               num_vis=5, hidden_size=H, n_layers=4, heads=12, hidden_dropout_prob=0.3, vocab_size=VOCAB,
                               use_relu=False, max_position_embeddings=T)
        torch.manual_seed(1234)
        model = mmvqa_amd.Model(args)
        model.to(dev).train()
        model.set_seed(1234)
        opt, red = mmvqa_amd.FusedAdam(model, lr=2e-5), GradReducer(model.flat_grads)
        batch, table = synth.distill_batch(B, T, HW, vocab=VOCAB, D=H, seed=1234, device=dev)
        if form == "resident_table":
            forms[form] = (lambda m=model, o=opt, r=red, b=batch, t=table: train.distill_step(m, o, r, 1, b, t))
        else:
            rows = train.synthetic_teacher_rows(batch, 5)
            ob = batch[:4] + (rows,)
            forms[form] = (lambda m=model, o=opt, r=red, b=ob, L=rows.shape[1] - 1: train.distill_step(m, o, r, 1, b, teacher, teacher_T=L))
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
    out["difference_ms"] = out["online_teacher"]["median_ms_per_step"] - out["resident_table"]["median_ms_per_step"]
    out["resident_block_spread_ms"] = max(ms["resident_table"]) - min(ms["resident_table"])
    out["teacher_T"] = T - 6
    out["blocks"], out["steps_per_block"], out["warmup_steps"] = blocks, steps, warmup
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8, help="steps per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip_step", action="store_true", help="the attention launch and the teacher's forward only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("teacher_bench.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), attention=attention_alone(dev))
    print(json.dumps(res["attention"]), flush=True)
    res["teacher_forward"] = teacher_forward(dev)
    print(json.dumps(res["teacher_forward"]), flush=True)
    if not a.skip_step:
        res["config2_distill_step"] = whole_step(dev, a.blocks, a.steps, a.warmup)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
