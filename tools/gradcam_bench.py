#!/usr/bin/env python3
"""Attribution pass at full size, one phase per timed loop: eval forward, feature backward (data gradients to the deepest
feature map), the CAM launches, and for scale the full training backward after a training forward at the same batch.

    python tools/gradcam_bench.py --config 5 --out profiles/gradcam_cfg5.json     # EfficientNetV2-M + RealFormer, VQA head
    python tools/gradcam_bench.py --config 2 --out profiles/gradcam_cfg2.json     # ResNet-152 + transformer, VQA head, B 16

Per batch at 224 x 224: median of RUNS runs of PASSES passes after warm-up; a run is synchronise, wall clock over the
passes, synchronise (as tools/amp_bench.py times a step).  MMVQA_GRADCAM_FUSED=1 times the one-launch form of the CAM."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import mmvqa_amd  # noqa: E402
from mmvqa_amd import _lib as L  # noqa: E402
from mmvqa_amd import gradcam as G  # noqa: E402
from mmvqa_amd import synth  # noqa: E402

RUNS, PASSES = 5, 8


def timed(fn):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(PASSES):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / PASSES)
    return sorted(ms)[len(ms) // 2], ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=5, choices=[2, 5])
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    bench.CONFIG = 5
    args = bench.make_args()
    B, T = 64, 28
    if a.config == 2:                      # config 2's backbone and encoder under the VQA head
        args.cnn_encoder, args.transformer_model, B, T = "resnet152", "transformer", 16, 32
    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)
    model = mmvqa_amd.Model(args).to(dev)
    img, ids, seg, mask, tgt = synth.vqa_batch(B, T, bench.HW, bench.VOCAB, bench.N_CLASSES, seed=1234, device=dev)
    model.train()
    model.tune(img, ids, seg, mask)
    lib = L.lib()
    state = {}

    def eval_forward():
        model.eval()
        with torch.no_grad():
            state["logits"] = model._engine_forward(img, ids, seg, mask)

    def feature_backward():                # after eval_forward: the same one-hot rows every pass
        lib_rc = lib.mmvqa_engine_backward_feature(model._handle, L.stream_ptr(), L.ptr(state["g"]), state["ld"], L.ptr(state["dA"]))
        L.check(lib_rc)

    def cam_launches():
        state["cam"] = G.cam_from_maps(state["A"], state["dA"], (bench.HW, bench.HW), state["u8"])

    def train_forward():
        model.train()
        state["out"] = model._engine_forward(img, ids, seg, mask)

    def full_backward():                   # after train_forward
        model._engine_backward(state["dl"])

    def whole_pass():
        G.grad_cam(model, img, ids, seg, mask, image_u8=state["u8"])

    res = {"config": a.config, "batch": B, "T": T, "runs": RUNS, "passes_per_run": PASSES, "ms": {}, "runs_ms": {},
           "cam_form": "one launch" if os.environ.get("MMVQA_GRADCAM_FUSED") else "two launches"}
    state["u8"] = G.image_u8_from_normalised(img)
    logits, A, dA, target = model.feature_gradient(img, ids, seg, mask)
    ld = (bench.N_CLASSES + 3) & ~3
    g = torch.zeros(B, ld, device=dev)
    g.scatter_(1, target.view(B, 1), 1.0)
    state.update(A=A, dA=dA, g=g, ld=ld)
    for name, fn, pre in (("eval_forward", eval_forward, None), ("feature_backward", feature_backward, eval_forward),
                          ("cam", cam_launches, None), ("attribution_pass", whole_pass, None),
                          ("train_forward", train_forward, None), ("full_backward", full_backward, train_forward)):
        if pre is not None:
            pre()
        if name == "full_backward":
            state["dl"] = torch.zeros_like(state["out"]).index_put_((torch.arange(B, device=dev), target), torch.ones(B, device=dev))
        res["ms"][name], res["runs_ms"][name] = timed(fn)
    model.flat_grads.zero_()
    res["images_per_s"] = B / (res["ms"]["attribution_pass"] * 1e-3)
    res["feature_backward_below_full_backward"] = res["ms"]["feature_backward"] < res["ms"]["full_backward"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
