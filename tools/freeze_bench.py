#!/usr/bin/env python3
"""Step time of bench.py's config 2 or 5 with the backbone unfrozen, frozen (Model.freeze_backbone()) and frozen on running
BatchNorm statistics (bn_stats="running"): the three forms alternate in one process, `--steps` steps per visit behind one
untimed step (the optimizer's table changes with the form), a device-event pair around each visit; median and min / max of
the per-step time over the visits.  Beside it the time the frozen form can save at most: the backbone's backward pass of the
unfrozen step, from the profile regions (backbone + bn_coef + tap) of a serialized forward + backward minus those of a
forward under no_grad -- every launch alone on the chip, so an upper estimate of what overlapped execution takes.
    python tools/freeze_bench.py --config 2 [--rounds 8] [--steps 5] [--out profiles/freeze_cfg2.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2, choices=[2, 5])
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    import bench
    import mmvqa_amd
    from mmvqa_amd import synth
    bench.CONFIG = a.config
    Bn, T = (64, 28) if a.config == 5 else (16, 32)
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    model = mmvqa_amd.Model(bench.make_args())
    model.to(dev).train()
    model.set_seed(1234)
    opt = mmvqa_amd.FusedAdam(model, lr=2e-5)
    if a.config == 5:
        img, ids, seg, mask, tgt = synth.vqa_batch(Bn, T, bench.HW, bench.VOCAB, bench.N_CLASSES, seed=1234, device=dev)
        loss_of = lambda out: mmvqa_amd.asl_loss(out[0], tgt)
    else:
        img, ids, seg, mask, tgt = synth.roco_batch(Bn, T, bench.HW, bench.VOCAB, seed=1234, device=dev)
        loss_of = lambda out: mmvqa_amd.mlm_loss(out, tgt)[0]

    def step():
        loss_of(model(img, ids, seg, mask)).backward()
        opt.step()

    def set_form(f):
        if f == "unfrozen":
            model.unfreeze_backbone()
        else:
            model.freeze_backbone("running" if f == "frozen_running_stats" else "batch")

    model.tune(img, ids, seg, mask)
    forms = ("unfrozen", "frozen", "frozen_running_stats")
    for f in forms:
        set_form(f)
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    ms = {f: [] for f in forms}
    for r in range(a.rounds):
        for f in forms:
            set_form(f)
            step()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            ms[f].append(e0.elapsed_time(e1) / a.steps)

    def regions(fn):
        model.profile(True, serialized=True)
        fn()
        torch.cuda.synchronize()
        r = model.profile_read_regions()
        model.profile(False)
        return {reg: dict(ms=sum(c["ms"] for c in cls.values()), launches=sum(c["launches"] for c in cls.values())) for reg, cls in r.items()}

    def fwd_only():
        with torch.no_grad():
            model(img, ids, seg, mask)

    prof = {}
    for f in ("unfrozen", "frozen"):
        set_form(f)
        step()
        prof[f] = regions(lambda: loss_of(model(img, ids, seg, mask)).backward())
    set_form("unfrozen")
    prof["forward"] = regions(fwd_only)
    model.flat_grads.zero_()
    below = ("backbone", "bn_coef", "tap")
    bwd = {f: sum(prof[f][r]["ms"] - prof["forward"][r]["ms"] for r in below) for f in ("unfrozen", "frozen")}
    res = dict(config=a.config, batch=Bn, rounds=a.rounds, steps_per_visit=a.steps, step_ms={}, profile_serialized=prof,
               backbone_backward_ms_serialized=dict(unfrozen=round(bwd["unfrozen"], 3), frozen=round(bwd["frozen"], 3)))
    for f in forms:
        res["step_ms"][f] = dict(median=round(statistics.median(ms[f]), 3), min=round(min(ms[f]), 3), max=round(max(ms[f]), 3))
    saved = res["step_ms"]["unfrozen"]["median"] - res["step_ms"]["frozen"]["median"]
    res["saved_ms"] = round(saved, 3)
    res["saved_over_serialized_backbone_backward"] = round(saved / (bwd["unfrozen"] - bwd["frozen"]), 3)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
