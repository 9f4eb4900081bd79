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

With --bertscore, instead (csrc/bertscore.hip):
4. mmvqa_bertscore_mask alone on resident unit-length states at (n, T, D) = (16, 64, 768), (128, 64, 768) and
   (16, 512, 768), lengths uniform in [T/2, T], against the plain-torch form on the GPU (einsum to [n, n, T, T], masked
   amax, means) with that form's peak memory; the two alternate, device events, median of 20.
5. The whole config-4 step (tf_efficientnetv2_m + realformer + SupCon head, 16 samples x 2 views) of train.supcon_step
   with no mask, with the cosine mask and with the BERTScore mask of a 12 x 768 teacher at layer 8; one model, the forms
   alternating in blocks, a host clock around each block; and the two masks alone with device events.

    python tools/teacher_bench.py --bertscore --out profiles/bertscore_cfg4.json
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


def _torch_bertscore(xa, la, xb, lb):
    """the plain-torch form on the GPU -- what the feature would be without the kernel: every cosine of every pair as one
    [n, n, T, T] tensor, then masked maxima and means"""
    n, Tt, _ = xa.shape
    S = torch.einsum("itd,jud->ijtu", xa, xb)
    pos = torch.arange(Tt, device=xa.device)
    va, vb = pos[None, :] < la[:, None], pos[None, :] < lb[:, None]                          # valid positions
    wa, wb = (pos[None, :] >= 1) & (pos[None, :] < la[:, None] - 1), (pos[None, :] >= 1) & (pos[None, :] < lb[:, None] - 1)
    rowmax = S.masked_fill(~vb[None, :, None, :], float("-inf")).amax(3)                    # [n, n, T]
    colmax = S.masked_fill(~va[:, None, :, None], float("-inf")).amax(2)                    # [n, n, T]
    P = (rowmax * wa[:, None, :]).nan_to_num(0.0, 0.0, 0.0).sum(2) / (la[:, None] - 2)
    R = (colmax * wb[None, :, :]).nan_to_num(0.0, 0.0, 0.0).sum(2) / (lb[None, :] - 2)
    F = (2 * P * R / (P + R)).nan_to_num(0.0)
    return F.fill_diagonal_(1.0)


def bertscore_kernel(dev, reps=20):
    """mmvqa_bertscore_mask alone (unit-length states resident) against the plain-torch form; the forms alternate in one
    process, device events around each, median of `reps`.  Lengths are drawn from [T/2, T]; the flop count is the
    algorithmic one over the valid positions, sum_ij la_i lb_j D 2 (the diagonal is not computed)."""
    from mmvqa_amd.teacher import bertscore_mask_unit, normalize_states_
    out = {}
    for n, Tt, D, torch_form in ((16, 64, 768, True), (128, 64, 768, True), (16, 512, 768, True)):
        g = torch.Generator().manual_seed(n + Tt)
        xa = normalize_states_((0.5 + torch.randn(n, Tt, D, generator=g)).to(dev))
        xb = normalize_states_((0.5 + torch.randn(n, Tt, D, generator=g)).to(dev))
        la = torch.randint(Tt // 2, Tt + 1, (n,), generator=g).to(torch.int32).to(dev)
        lb = torch.randint(Tt // 2, Tt + 1, (n,), generator=g).to(torch.int32).to(dev)
        forms = {"kernel": lambda: bertscore_mask_unit(xa, la, xb, lb)}
        key = f"n{n}_T{Tt}_D{D}"
        r = dict(n=n, T=Tt, D=D, reps=reps, score_tensor_bytes=4 * n * n * Tt * Tt)
        if torch_form:
            try:
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                ref = _torch_bertscore(xa, la, xb, lb)
                torch.cuda.synchronize()
                r["torch_peak_bytes"] = torch.cuda.max_memory_allocated() - base
                r["max_abs_difference"] = float((bertscore_mask_unit(xa, la, xb, lb) - ref).abs().max())
                forms["torch"] = lambda: _torch_bertscore(xa, la, xb, lb)
            except torch.cuda.OutOfMemoryError as e:
                r["torch"] = f"skipped: {str(e)[:80]}"
        r.update(_timed(forms, reps))
        lf, lbf = la.double().cpu(), lb.double().cpu()
        flops = 2.0 * D * float(lf.sum() * lbf.sum() - (lf * lbf).sum())
        r["gflop_valid"] = flops / 1e9
        r["gflop_full"] = 2.0 * D * (n * Tt) ** 2 / 1e9
        r["kernel"]["tflops"] = flops / (r["kernel"]["median_ms"] * 1e-3) / 1e12
        if "torch" in forms:
            r["torch"]["tflops_valid"] = flops / (r["torch"]["median_ms"] * 1e-3) / 1e12
            r["kernel_over_torch"] = r["kernel"]["median_ms"] / r["torch"]["median_ms"]
        out[key] = r
        print(json.dumps({key: r}), flush=True)
    return out


def supcon_mask_step(dev, blocks, steps, warmup, Tt=64):
    """the whole config-4 step (bench.py's model and batch: tf_efficientnetv2_m + realformer + SupCon head, 16 samples x
    2 views, 224^2, T 32) of train.supcon_step with no mask, with --supcon_mask cosine and with --supcon_mask bert_score
    (layer 8), a 12 x 768 teacher over 32 texts of 20..64 tokens cut at 64; ONE model, the forms alternating in blocks,
    a host clock around each block, which ends in a device synchronise"""
    import mmvqa_amd
    from mmvqa_amd import synth, train
    from mmvqa_amd.ddp import GradReducer
    from mmvqa_amd.teacher import BertTeacher
    teacher = BertTeacher.random(12, H, 4 * H, VOCAB, 512, seed=2).to(dev)
    args = SimpleNamespace(task="MLM", dataset="roco", transformer_model="realformer", cnn_encoder="tf_efficientnetv2_m",
                           num_vis=5, hidden_size=H, n_layers=4, heads=12, hidden_dropout_prob=0.3, vocab_size=VOCAB,
                           use_relu=False, max_position_embeddings=T, supcon=True)
    torch.manual_seed(1234)
    model = mmvqa_amd.Model(args)
    model.to(dev).train()
    model.set_seed(1234)
    opt, red = mmvqa_amd.FusedAdam(model, lr=2e-5), GradReducer(model.flat_grads)
    va = synth.roco_batch(B, T, HW, VOCAB, seed=1234, device=dev)
    vb = synth.roco_batch(B, T, HW, VOCAB, seed=4321, device=dev)
    batch = tuple(train.process_tensors((va[0], vb[0]), va[1], vb[1], va[2], va[3], va[4], vb[4]))
    g = torch.Generator().manual_seed(5)
    rows = torch.zeros(2 * B, 1 + Tt, dtype=torch.int64)
    rows[:, 0] = torch.randint(20, Tt + 1, (2 * B,), generator=g)
    rows[0, 0] = Tt
    for b in range(2 * B):
        rows[b, 1:1 + int(rows[b, 0])] = torch.randint(1, VOCAB, (int(rows[b, 0]),), generator=g)
    b6 = batch[:5] + (rows.to(dev),)
    forms = {"no_mask": lambda: train.supcon_step(model, opt, red, 1, batch),
             "cosine": lambda: train.supcon_step(model, opt, red, 1, b6, words=teacher, teacher_T=Tt),
             "bert_score": lambda: train.supcon_step(model, opt, red, 1, b6, words=teacher, teacher_T=Tt, bert_score=(8, 0.0))}
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
    out["no_mask_block_spread_ms"] = max(ms["no_mask"]) - min(ms["no_mask"])
    out.update(teacher="12 x 768", texts=2 * B, teacher_T=Tt, layer=8, blocks=blocks, steps_per_block=steps, warmup_steps=warmup)
    # the mask alone (teacher forward + mask kernels), device events
    out["mask_alone"] = _timed({"cosine": lambda: train.teacher_cosine_mask(teacher, b6[5], Tt),
                                "bert_score": lambda: train.teacher_bertscore_mask(teacher, b6[5], 8, 0.0, Tt)}, 20)
    return out


def main_bertscore(a, dev):
    res = dict(device=torch.cuda.get_device_name(0), bertscore_kernel=bertscore_kernel(dev))
    if not a.skip_step:
        res["config4_supcon_step"] = supcon_mask_step(dev, a.blocks, a.steps, a.warmup)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bertscore", action="store_true",
                    help="measure the BERTScore mask instead: mmvqa_bertscore_mask against the plain-torch form at three "
                         "shapes, and the config-4 SupCon step with no mask / the cosine mask / the BERTScore mask "
                         "(python tools/teacher_bench.py --bertscore --out profiles/bertscore_cfg4.json)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8, help="steps per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip_step", action="store_true", help="the attention launch and the teacher's forward only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("teacher_bench.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    if a.bertscore:
        res = main_bertscore(a, dev)
    else:
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
