#!/usr/bin/env python3
"""Step time of a VQA fine-tuning step with every question carrying its own copy of the image (Model.forward) against the
grouped step (Model.forward_grouped), same questions, four per image:
    config5   bench.py's config 5 (tf_efficientnetv2_m + RealFormer, VQA head, T 28): 64 questions, 64 images vs 16
    resnet152 ResNet-152 + transformer under the VQA head (T 32):                     16 questions, 16 images vs 4
The two arms alternate in one process, `--steps` steps per visit behind one untimed step, a device-event pair around each
visit; median and min / max of the per-step time over the visits.  Beside it: the two new launches (mmvqa_vis_expand,
mmvqa_dvis_group_sum) timed alone at the step's shape, and the backbone's share of the ungrouped step -- the profile
regions backbone + bn_coef + tap of a serialized forward + backward, every launch alone on the chip -- which bounds what
grouping can save: at four questions an image at most 3/4 of that share.
    python tools/grouped_bench.py [--rounds 8] [--steps 5] [--out profiles/grouped_cfg5.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(name, a):
    import torch
    import bench
    import mmvqa_amd
    from mmvqa_amd import _lib as L, synth
    from mmvqa_amd.model import group_maps
    bench.CONFIG = 5
    args = bench.make_args()
    B, T, per = 64, 28, 4
    if name == "resnet152":
        args.cnn_encoder, args.transformer_model, B, T = "resnet152", "transformer", 16, 32
    NI = B // per
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    model = mmvqa_amd.Model(args)
    model.to(dev).train()
    model.set_seed(1234)
    opt = mmvqa_amd.FusedAdam(model, lr=2e-5)
    img, group, ids, seg, mask, tgt = synth.vqa_grouped_batch(NI, [per] * NI, T, bench.HW, bench.VOCAB, bench.N_CLASSES,
                                                              seed=1234, device=dev)
    dup = img[group.to(dev)].contiguous()                 # the ungrouped arm's batch: every question with its image

    def step_ungrouped():
        mmvqa_amd.asl_loss(model(dup, ids, seg, mask)[0], tgt).backward()
        opt.step()

    def step_grouped():
        mmvqa_amd.asl_loss(model.forward_grouped(img, group, ids, seg, mask)[0], tgt).backward()
        opt.step()

    arms = (("ungrouped", step_ungrouped), ("grouped", step_grouped))
    model.tune(dup, ids, seg, mask)                        # Model.tune is not extended: the grouped step takes these
    for _, step in arms:                                   # entries where its shapes match, the defaults elsewhere
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    ms = {n: [] for n, _ in arms}
    for _ in range(a.rounds):
        for n, step in arms:
            step()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            ms[n].append(e0.elapsed_time(e1) / a.steps)

    # the two new launches alone, at the step's shape
    H, lib = args.hidden_size, L.lib()
    maps = group_maps(group, NI, B).to(dev)
    vi, vq = torch.randn(5, NI, H, device=dev), torch.empty(5, B, H, device=dev)

    def launches(fn, n=200):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n               # microseconds per launch, back to back

    import ctypes as C
    offs = C.c_void_p(maps.data_ptr() + 4 * B)
    us_expand = launches(lambda: L.check(lib.mmvqa_vis_expand(L.stream_ptr(), L.ptr(vi), L.ptr(maps), L.ptr(vq), NI, B, H, 5)))
    us_sum = launches(lambda: L.check(lib.mmvqa_dvis_group_sum(L.stream_ptr(), L.ptr(vq), offs, L.ptr(vi), NI, B, H, 5)))

    # the backbone's share of the ungrouped step, serialized
    step_ungrouped()
    model.profile(True, serialized=True)
    mmvqa_amd.asl_loss(model(dup, ids, seg, mask)[0], tgt).backward()
    torch.cuda.synchronize()
    reg = model.profile_read_regions()
    model.profile(False)
    model.flat_grads.zero_()
    reg_ms = {r: sum(c["ms"] for c in cls.values()) for r, cls in reg.items()}
    below = sum(reg_ms.get(r, 0.0) for r in ("backbone", "bn_coef", "tap"))
    share = below / max(sum(reg_ms.values()), 1e-9)

    res = dict(shape=name, cnn=args.cnn_encoder, encoder=args.transformer_model, questions=B, images_grouped=NI,
               questions_per_image=per, T=T, rounds=a.rounds, steps_per_visit=a.steps, step_ms={}, questions_per_s={},
               new_launches_us=dict(vis_expand=round(us_expand, 2), dvis_group_sum=round(us_sum, 2)),
               regions_ms_serialized={r: round(v, 3) for r, v in reg_ms.items()},
               backbone_share_of_ungrouped_step_serialized=round(share, 4))
    for n, _ in arms:
        med = statistics.median(ms[n])
        res["step_ms"][n] = dict(median=round(med, 3), min=round(min(ms[n]), 3), max=round(max(ms[n]), 3))
        res["questions_per_s"][n] = round(B / (med * 1e-3), 1)
    res["speedup"] = round(res["step_ms"]["ungrouped"]["median"] / res["step_ms"]["grouped"]["median"], 3)
    # all of the backbone's (serialized) time shrinking by 1 - 1/per and nothing else moving
    res["speedup_bound_from_share"] = round(1.0 / (1.0 - share * (1.0 - 1.0 / per)), 3)
    del model, opt
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--shapes", type=str, nargs="+", default=["config5", "resnet152"], choices=["config5", "resnet152"])
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    res = dict(shapes=[measure(n, a) for n in a.shapes])
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
