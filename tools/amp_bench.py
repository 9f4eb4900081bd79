#!/usr/bin/env python3
"""Config-2 training step (bench.py's flagship: ResNet-152 + BERT-style encoder, 16 x 224^2 images, T 32) in fp32 and in
the mixed-precision mode (fp16 autocast + mmvqa_amd.amp.GradScaler), alternating on the same device, RUNS timed runs of
STEPS steps each; both forms are tuned first.  Writes profiles/amp_cfg2.json (or argv[1]).

The implicit-GEMM time of both families (all launches of one step, and per region of the step) comes from the engine's
profiler on a serialized step.  Per-shape times: run the script under
  MMVQA_IGEMM_LOG=1 rocprofv3 --kernel-trace --stats -d out -- python tools/amp_bench.py
the log lines carry `prec f32` / `prec f16` per launch and the kernel statistics separate the two instantiation
families (template argument PREC)."""
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
from mmvqa_amd.amp import GradScaler  # noqa: E402
from mmvqa_amd.ddp import GradReducer  # noqa: E402

STEPS, RUNS = int(os.environ.get("AMP_BENCH_STEPS", "10")), int(os.environ.get("AMP_BENCH_RUNS", "5"))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "amp_cfg2.json")
    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)
    model = mmvqa_amd.Model(bench.make_args()).to(dev).train()
    model.set_seed(1234)
    opt = mmvqa_amd.FusedAdam(model, lr=2e-5)
    red = GradReducer(model.flat_grads)
    scaler = GradScaler()
    img, ids, seg, mask, tgt = synth.roco_batch(bench.B_PER_GPU, bench.T, bench.HW, bench.VOCAB, seed=1234, device=dev)
    from mmvqa_amd import train as TR

    def step(mixed):
        TR.mlm_step(model, opt, red, 1, (img, ids, seg, mask, tgt), scaler=scaler if mixed else None)

    model.tune(img, ids, seg, mask)
    with torch.autocast("cuda", dtype=torch.float16):
        model.tune(img, ids, seg, mask)
    for mixed in (False, True):
        for _ in range(3):
            step(mixed)
    torch.cuda.synchronize()
    ms = {"fp32": [], "mixed": []}
    for _ in range(RUNS):
        for mixed in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                step(mixed)
            torch.cuda.synchronize()
            ms["mixed" if mixed else "fp32"].append((time.perf_counter() - t0) * 1e3 / STEPS)
    # implicit-GEMM time of each family: the engine's per-launch HIP-event profile of one step on ONE stream (every
    # launch has the chip to itself), split by region of the step; achieved rate against the family's MFMA peak
    # (MI355X_MICROARCH matrix-core table: fp32-input 157 TF, fp16 2.5 PF dense)
    peak = {"fp32": 157e12, "mixed": 2.5e15}
    gemm = {}
    for mixed in (False, True):
        key = "mixed" if mixed else "fp32"
        model.profile(True, serialized=True)
        step(mixed)
        torch.cuda.synchronize()
        g = model.profile_read()["igemm"]
        regs = model.profile_read_regions()
        model.profile(False)
        rate = g["flops"] / (g["ms"] * 1e-3) if g["ms"] > 0 else 0.0
        gemm[key] = {"launches": g["launches"], "ms": g["ms"], "tflops": rate / 1e12, "fraction_of_peak": rate / peak[key],
                     "by_region_ms": {r: v["igemm"]["ms"] for r, v in regs.items() if v["igemm"]["launches"]}}
    res = {"config": 2, "steps_per_run": STEPS, "runs": RUNS, "step_ms": ms, "igemm_serialized": gemm,
           "median_ms": {k: sorted(v)[len(v) // 2] for k, v in ms.items()}, "final_scale": scaler.get_scale()}
    res["speedup"] = res["median_ms"]["fp32"] / res["median_ms"]["mixed"]
    print(json.dumps(res))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
