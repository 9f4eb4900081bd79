#!/usr/bin/env python3
"""Config-2 training step (bench.py's flagship: ResNet-152, 16 x 224^2 images, T 32, hidden 768, 4 layers) with the
Feedback-Transformer fusion encoder beside the same step with `transformer`, alternating on the same device, RUNS timed runs
of STEPS steps each; both models are tuned first.  Writes profiles/feedback_cfg2.json (or argv[1]).

Per encoder: ms/step; from the engine's profiler on a serialized step (one stream, every launch has the chip to itself) the
encoder's launches and time (regions qkv + attention + qkv_attention_fused + encoder_rest), and for the feedback encoder the
launches and time of the weight-gradient block that follows its time loop."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import mmvqa_amd  # noqa: E402
from mmvqa_amd import synth  # noqa: E402
from mmvqa_amd import train as TR  # noqa: E402
from mmvqa_amd.ddp import GradReducer  # noqa: E402

STEPS, RUNS = int(os.environ.get("FB_BENCH_STEPS", "8")), int(os.environ.get("FB_BENCH_RUNS", "5"))
ENCODERS = ("transformer", "feedback-transformer")
ENC_REGIONS = ("qkv", "attention", "qkv_attention_fused", "encoder_rest")


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "feedback_cfg2.json")
    dev = torch.device("cuda", 0)
    batch = synth.roco_batch(bench.B_PER_GPU, bench.T, bench.HW, bench.VOCAB, seed=1234, device=dev)
    forms = {}
    for tm in ENCODERS:
        args = bench.make_args()
        args.transformer_model = tm
        torch.manual_seed(1234)
        model = mmvqa_amd.Model(args).to(dev).train()
        model.set_seed(1234)
        opt = mmvqa_amd.FusedAdam(model, lr=2e-5)
        red = GradReducer(model.flat_grads)
        model.tune(*batch[:4])
        forms[tm] = (model, lambda m=model, o=opt, r=red: TR.mlm_step(m, o, r, 1, batch))
    for _, step in forms.values():
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    ms = {tm: [] for tm in ENCODERS}
    for _ in range(RUNS):
        for tm in ENCODERS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                forms[tm][1]()
            torch.cuda.synchronize()
            ms[tm].append((time.perf_counter() - t0) * 1e3 / STEPS)
    prof = {}
    for tm in ENCODERS:
        model, step = forms[tm]
        model.profile(True, serialized=True)
        step()
        torch.cuda.synchronize()
        regs = model.profile_read_regions()
        hbm = model.profile_read_hbm()
        model.profile(False)
        enc = {r: {"launches": sum(c["launches"] for c in regs[r].values()), "ms": sum(c["ms"] for c in regs[r].values())}
               for r in ENC_REGIONS}
        prof[tm] = {"encoder_launches": sum(v["launches"] for v in enc.values()), "encoder_ms": sum(v["ms"] for v in enc.values()),
                    "by_region": enc, "step_launches": sum(c["launches"] for r in regs.values() for c in r.values()),
                    "step_ms_serialized": sum(c["ms"] for r in regs.values() for c in r.values())}
        if "fb_weight_gradients" in hbm:
            prof[tm]["weight_gradient_block"] = {k: hbm["fb_weight_gradients"][k] for k in ("launches", "ms")}
    res = {"config": 2, "steps_per_run": STEPS, "runs": RUNS, "step_ms": ms,
           "median_ms": {k: sorted(v)[len(v) // 2] for k, v in ms.items()}, "serialized_profile": prof}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
