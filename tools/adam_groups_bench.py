#!/usr/bin/env python3
"""mmvqa_adam_groups against mmvqa_adam on config 2's flat buffer (ResNet-152 MMBERT, 32 B of HBM traffic per
parameter either way): one launch each of
  adam          mmvqa_adam
  one_segment   mmvqa_adam_groups, one segment over the whole buffer
  no_decay      mmvqa_adam_groups, the table FusedAdam(weight_decay=0.01, groups=[no_decay without decay]) builds for
                config 2 (convolutions alternating with their BatchNorm scale and shift)
alternating in one process, a device-event pair around every launch; median and min / max of the launches of a form.
    python tools/adam_groups_bench.py [--rounds 30] [--out profiles/adam_groups.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    import bench
    import mmvqa_amd
    from mmvqa_amd import _lib as L
    from mmvqa_amd.optim import merge_segments, no_decay
    bench.CONFIG = 2
    model = mmvqa_amd.Model(bench.make_args())            # on the host: only its tensor table is used
    ranges = model._param_ranges()
    n = model.flat_params.numel()
    rows = merge_segments([(lo, hi, 2e-5, 0.0 if no_decay(name) else 0.01, L.ADAM_DECOUPLED) for name, _, lo, hi in ranges])
    tables = {"one_segment": [(0, n, 2e-5, 0.0, L.ADAM_L2)], "no_decay": rows}
    dev = torch.device("cuda:0")
    p, g, m, v = (torch.randn(n, device=dev) for _ in range(4))
    v.abs_()
    tabs = {}
    for k, segs in tables.items():
        host = (L.AdamSeg * len(segs))()
        for h, (lo, hi, lr, wd, mode) in zip(host, segs):
            h.begin, h.end, h.lr, h.weight_decay, h.mode = lo, hi, lr, wd, mode
        tabs[k] = (host, torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev), len(segs))

    def go(form, step):
        if form == "adam":
            L.check(L.lib().mmvqa_adam(L.stream_ptr(), L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, 2e-5, 0.9, 0.999, 1e-8, step, 1.0, 0))
        else:
            host, devt, nseg = tabs[form]
            L.check(L.lib().mmvqa_adam_groups(L.stream_ptr(), L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), 0, n, C.cast(host, C.c_void_p),
                                              L.ptr(devt), nseg, 0.9, 0.999, 1e-8, step, 1.0, 0))

    forms = ("adam", "one_segment", "no_decay")
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
    res = dict(parameters=n, bytes_per_parameter=32, rounds=a.rounds, segments={k: len(s) for k, s in tables.items()}, forms={})
    for f in forms:
        med = statistics.median(ms[f])
        res["forms"][f] = dict(median_ms=round(med, 4), min_ms=round(min(ms[f]), 4), max_ms=round(max(ms[f]), 4),
                               tb_per_s=round(n * 32 / med / 1e9, 3))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
