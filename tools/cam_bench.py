#!/usr/bin/env python3
"""Attribution methods at full size: time per pass of every method beside the Grad-CAM pass of the
same run, forward_tokens at four questions per image against four full eval forwards, how the token forward scales with
its batch, and Ablation-CAM's split into the token launches, the encoder / head forwards and the rest.

    python tools/cam_bench.py --config 5 --out profiles/cam_methods_cfg5.json     # EfficientNetV2-M + RealFormer, B 64
    python tools/cam_bench.py --config 2 --out profiles/cam_methods_cfg2.json     # ResNet-152 + transformer, B 16

Per entry at 224 x 224: median of RUNS runs of PASSES passes after warm-up, the entries of a group alternating inside
every run (a run is synchronise, wall clock over the passes, synchronise, as tools/gradcam_bench.py times).  Ablation-CAM
runs hundreds of forwards per pass: its entries take ABL_PASSES passes per run."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import mmvqa_amd  # noqa: E402
from mmvqa_amd import gradcam as G  # noqa: E402
from mmvqa_amd import synth  # noqa: E402

RUNS, PASSES, ABL_PASSES = 5, 8, 1


def timed_group(fns, passes=PASSES, warm=2):
    """{name: fn} -> ({name: median ms per pass}, {name: runs}); the entries alternate inside every run"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    runs = {k: [] for k in fns}
    for _ in range(RUNS):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(passes):
                fn()
            torch.cuda.synchronize()
            runs[k].append((time.perf_counter() - t0) * 1e3 / passes)
    return {k: sorted(v)[len(v) // 2] for k, v in runs.items()}, runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=5, choices=[2, 5])
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--skip_ablation", action="store_true")
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
    model.eval()
    u8 = G.image_u8_from_normalised(img)
    res = {"config": a.config, "batch": B, "T": T, "runs": RUNS, "passes_per_run": PASSES, "ablation_passes_per_run": ABL_PASSES,
           "ablation_variants_per_forward": G.ABLATION_VARIANTS, "ms": {}, "runs_ms": {}}

    def put(ms_runs):
        res["ms"].update(ms_runs[0])
        res["runs_ms"].update(ms_runs[1])

    # ---- the one-backward methods and Eigen-CAM beside Grad-CAM
    fns = {"gradcam_pass": lambda: G.grad_cam(model, img, ids, seg, mask, image_u8=u8)}
    for m in ("gradcam", "gradcam++", "xgradcam", "eigencam"):
        fns[f"attribute_{m}"] = (lambda m=m: G.attribute(model, img, ids, seg, mask, method=m, image_u8=u8))
    put(timed_group(fns))
    logits, A, dA, target = model.feature_gradient(img, ids, seg, mask)
    raw = G.eigencam_raw(A)[0]
    put(timed_group({"kernel_weights_gradcam++": lambda: G.cam_weights(A, dA, "gradcam++"),
                     "kernel_weights_xgradcam": lambda: G.cam_weights(A, dA, "xgradcam"),
                     "kernel_eigencam_raw": lambda: G.eigencam_raw(A),
                     "kernel_cam_from_weights": lambda: G.cam_from_weights(A, (bench.HW, bench.HW), raw=raw, image_u8=u8)}))

    # ---- token reuse: four questions per image
    qs = [synth.vqa_batch(B, T, bench.HW, bench.VOCAB, bench.N_CLASSES, seed=2000 + q, device=dev)[1:4] for q in range(4)]

    def four_full():
        with torch.no_grad():
            for q in qs:
                model(img, *q)

    def tokens_then_four():
        vis = model.visual_tokens(img)
        for q in qs:
            model.forward_tokens(vis, *q)

    vis = model.visual_tokens(img)
    put(timed_group({"four_full_eval_forwards": four_full, "visual_tokens_plus_four_forward_tokens": tokens_then_four,
                     "visual_tokens": lambda: model.visual_tokens(img),
                     "forward_tokens": lambda: model.forward_tokens(vis, *qs[0])}))
    res["token_reuse_speedup_q4"] = res["ms"]["four_full_eval_forwards"] / res["ms"]["visual_tokens_plus_four_forward_tokens"]

    # ---- how the token forward scales with its batch (the evidence behind ABLATION_VARIANTS)
    scale = {}
    for n in (64, 256, 1024):
        rep = lambda t: t[:1].expand(n, *t.shape[1:]).contiguous()
        v, q = rep(vis), [rep(t) for t in qs[0]]
        ms, _ = timed_group({"f": lambda: model.forward_tokens(v, *q)})
        scale[str(n)] = {"ms_per_forward": ms["f"], "us_per_row": ms["f"] * 1e3 / n}
    res["forward_tokens_scaling"] = scale

    # ---- Ablation-CAM and its split
    if not a.skip_ablation:
        Cc = A.shape[3]
        Wt, k, act = model.deepest_tap()
        nc = max(1, min(Cc, G.ABLATION_VARIANTS // B))
        rep = lambda t: t.repeat_interleave(nc, dim=0)
        v_fixed = vis[:, None].repeat(1, nc, 1, 1).view(B * nc, *vis.shape[1:])
        q_fixed = [rep(t) for t in (ids, seg, mask)]
        n_chunks = (Cc + nc - 1) // nc

        def token_launches():
            u = None
            for lo in range(0, Cc, nc):
                _, u = G.ablated_tokens(A, Wt, act, min(lo, Cc - nc), nc, u)

        def token_forwards():
            for _ in range(n_chunks):
                model.forward_tokens(v_fixed, *q_fixed)

        put(timed_group({"attribute_ablationcam": lambda: G.attribute(model, img, ids, seg, mask, method="ablationcam", image_u8=u8),
                         "ablation_token_launches": token_launches, "ablation_token_forwards": token_forwards},
                        passes=ABL_PASSES, warm=1))
        res["ablation"] = {"channels": Cc, "chunk": nc, "forwards_per_pass": n_chunks, "rows_per_forward": B * nc,
                           "rest_ms": res["ms"]["attribute_ablationcam"] - res["ms"]["ablation_token_launches"]
                           - res["ms"]["ablation_token_forwards"]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
