#!/usr/bin/env python3
"""The weight average kept inside the Adam launch against keeping it in a pass of its own, on config 2's flat buffer
(ResNet-152 MMBERT), one launch (or pair) each of
  adam       mmvqa_adam                                   32 B of HBM traffic per parameter
  fused      mmvqa_adam_ema                               40 B
  separate   mmvqa_adam, then ema.lerp_(p, 1 - d)         32 B + 12 B and a second launch
and the same three over the segment table FusedAdam(weight_decay=0.01, groups=[no_decay without decay]) builds for
config 2 (mmvqa_adam_groups / mmvqa_adam_groups_ema), alternating in one process, a device-event pair around every
form's launches; median and min / max over the rounds.

Then the config-2 training step (bench.py's flagship) with FusedAdam(ema_decay=None) and FusedAdam(ema_decay=0.999) on
one model, alternating, RUNS timed runs of STEPS steps each (host clock around work that ends in a synchronise).

    python tools/ema_bench.py [--rounds 30] [--out profiles/ema_cfg2.json] [--no-step]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DECAY = 0.999
STEPS, RUNS = int(os.environ.get("EMA_BENCH_STEPS", "10")), int(os.environ.get("EMA_BENCH_RUNS", "5"))


def summary(ms, n, nbytes):
    med = statistics.median(ms)
    return dict(median_ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                bytes_per_parameter=nbytes, tb_per_s=round(n * nbytes / med / 1e9, 3))


def launches(a):
    import torch
    import bench
    import mmvqa_amd
    from mmvqa_amd import _lib as L
    from mmvqa_amd.optim import merge_segments, no_decay
    bench.CONFIG = 2
    model = mmvqa_amd.Model(bench.make_args())            # on the host: only its tensor table is used
    n = model.flat_params.numel()
    rows = merge_segments([(lo, hi, 2e-5, 0.0 if no_decay(name) else 0.01, L.ADAM_DECOUPLED)
                           for name, _, lo, hi in model._param_ranges()])
    dev = torch.device("cuda:0")
    p, g, m, v, e = (torch.randn(n, device=dev) for _ in range(5))
    v.abs_()
    host = (L.AdamSeg * len(rows))()
    for h, (lo, hi, lr, wd, mode) in zip(host, rows):
        h.begin, h.end, h.lr, h.weight_decay, h.mode = lo, hi, lr, wd, mode
    devt = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)
    lib, hp = L.lib(), C.cast(host, C.c_void_p)
    P = L.ptr

    def go(form, step):
        s = L.stream_ptr()
        table = form.startswith("groups_")
        kind = form[len("groups_"):] if table else form
        if table and kind == "fused":
            L.check(lib.mmvqa_adam_groups_ema(s, P(p), P(g), P(m), P(v), P(e), 0, n, hp, P(devt), len(rows), 0.9, 0.999,
                                              1e-8, step, 1.0, 0, DECAY))
        elif table:
            L.check(lib.mmvqa_adam_groups(s, P(p), P(g), P(m), P(v), 0, n, hp, P(devt), len(rows), 0.9, 0.999, 1e-8, step, 1.0, 0))
        elif kind == "fused":
            L.check(lib.mmvqa_adam_ema(s, P(p), P(g), P(m), P(v), P(e), n, 2e-5, 0.9, 0.999, 1e-8, step, 1.0, 0, DECAY))
        else:
            L.check(lib.mmvqa_adam(s, P(p), P(g), P(m), P(v), n, 2e-5, 0.9, 0.999, 1e-8, step, 1.0, 0))
        if kind == "separate":
            e.lerp_(p, 1.0 - DECAY)

    forms = ("adam", "fused", "separate", "groups_adam", "groups_fused", "groups_separate")
    nbytes = dict(adam=32, fused=40, separate=44, groups_adam=32, groups_fused=40, groups_separate=44)
    for f in forms:
        for k in range(3):
            go(f, k + 1)
    torch.cuda.synchronize()
    ms = {f: [] for f in forms}
    step = 4
    for r in range(a.rounds):
        evs = []
        for f in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            go(f, step)
            e1.record()
            evs.append((f, e0, e1))
            step += 1
        torch.cuda.synchronize()
        for f, e0, e1 in evs:
            ms[f].append(e0.elapsed_time(e1))
    res = dict(parameters=n, rounds=a.rounds, ema_decay=DECAY, segments=len(rows),
               forms={f: summary(ms[f], n, nbytes[f]) for f in forms})
    for pre in ("", "groups_"):
        base = res["forms"][pre + "adam"]["median_ms"]
        res[pre + "fused_over_adam"] = round(res["forms"][pre + "fused"]["median_ms"] / base, 4)
        res[pre + "separate_over_adam"] = round(res["forms"][pre + "separate"]["median_ms"] / base, 4)
    del p, g, m, v, e
    torch.cuda.empty_cache()
    return res


def training_step():
    import torch
    import bench
    import mmvqa_amd
    from mmvqa_amd import synth
    from mmvqa_amd import train as TR
    from mmvqa_amd.ddp import GradReducer
    bench.CONFIG = 2
    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)
    model = mmvqa_amd.Model(bench.make_args()).to(dev).train()
    model.set_seed(1234)
    opts = {"plain": mmvqa_amd.FusedAdam(model, lr=2e-5), "ema": mmvqa_amd.FusedAdam(model, lr=2e-5, ema_decay=DECAY)}
    red = GradReducer(model.flat_grads)
    batch = synth.roco_batch(bench.B_PER_GPU, bench.T, bench.HW, bench.VOCAB, seed=1234, device=dev)
    model.tune(*batch[:4])
    for k in opts:
        for _ in range(3):
            TR.mlm_step(model, opts[k], red, 1, batch)
    torch.cuda.synchronize()
    ms = {k: [] for k in opts}
    for _ in range(RUNS):
        for k in opts:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                TR.mlm_step(model, opts[k], red, 1, batch)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / STEPS)
    med = {k: statistics.median(v) for k, v in ms.items()}
    return dict(config=2, batch=bench.B_PER_GPU, steps_per_run=STEPS, runs=RUNS, step_ms=ms, median_ms=med,
                ema_over_plain=round(med["ema"] / med["plain"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--no-step", action="store_true", help="the launches only, without the training step")
    a = ap.parse_args()
    res = dict(launches=launches(a))
    if not a.no_step:
        res["training_step"] = training_step()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
