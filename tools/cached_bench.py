#!/usr/bin/env python3
"""Step time of VQA fine-tuning from cached visual tokens (Model.forward_cached) against the frozen
full step it replaces, per shape:
    config5   bench.py's config 5 (tf_efficientnetv2_m + RealFormer, VQA head): B 64, T 28  -> profiles/cached_cfg5.json
    resnet152 ResNet-152 + transformer under the VQA head:                      B 16, T 32  -> profiles/cached_cfg2.json
Three entries, ms per step:
    (a) frozen_full   the step of --freeze_backbone --freeze_bn_stats: forward, loss, backward, Adam
    (b) cached        the same step through forward_cached (the cache holds 8 x B images, 2 views)
    (c) above_tokens  what (a) spends above the visual tokens: the profile regions qkv + attention + encoder_rest + heads +
                      embed (+ the fused qkv/attention launch) of a serialized forward + backward of (a), every launch
                      alone on the chip, summed; one figure per visit, so it has a spread of its own
(a) and (b) alternate in one process, `--steps` steps per visit behind one untimed step, one device-event pair around a
visit; (b) is also timed without loss and optimizer (forward + backward only), which is what (c) covers.  Beside them: the
gather alone at the step's shape, the host time of validating and uploading index / view, the cache fill in images/s
against Model.visual_tokens alone, and the cache's bytes.
    python tools/cached_bench.py [--rounds 8] [--steps 5] [--shapes config5 resnet152]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ABOVE = ("qkv", "attention", "encoder_rest", "heads", "embed", "qkv_attention_fused")
OUT = {"config5": "profiles/cached_cfg5.json", "resnet152": "profiles/cached_cfg2.json"}


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def measure(name, a):
    import torch
    import bench
    import mmvqa_amd
    from mmvqa_amd import _lib as L, synth
    from mmvqa_amd.model import cached_maps
    from mmvqa_amd.tokens import TokenCache
    bench.CONFIG = 5
    args = bench.make_args()
    B, T = 64, 28
    if name == "resnet152":
        args.cnn_encoder, args.transformer_model, B, T = "resnet152", "transformer", 16, 32
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    model = mmvqa_amd.Model(args)
    model.to(dev).train()
    model.set_seed(1234)
    model.freeze_backbone("running")
    opt = mmvqa_amd.FusedAdam(model, lr=2e-5)
    img, ids, seg, mask, tgt = synth.vqa_batch(B, T, bench.HW, bench.VOCAB, bench.N_CLASSES, seed=1234, device=dev)
    N, K = 8 * B, 2
    cache = TokenCache(model, N, views=K)
    model.tune(img, ids, seg, mask)

    # ---- cache fill against visual_tokens alone (the fill adds the fingerprint once, then a scatter per call)
    def timed_host(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    rows = [list(range(lo, lo + B)) for lo in range(0, N, B)]
    cache.fill(rows[0], img, 0)
    model.visual_tokens(img)
    t_fill = timed_host(lambda: [cache.fill(r, img, v) for v in range(K) for r in rows], 1) / (K * len(rows))
    t_vis = timed_host(lambda: model.visual_tokens(img), K * len(rows))
    g = torch.Generator().manual_seed(1)
    index, view = torch.randint(0, N, (B,), generator=g), torch.randint(0, K, (B,), generator=g)

    def as_full():                   # (a): the step of --freeze_backbone --freeze_bn_stats, the five taps train
        model.unfreeze_visual()
        model.freeze_backbone("running")

    def as_cached():                 # (b): the taps frozen too (what a cache needs); the optimizer's table follows
        model.freeze_visual()

    def step_full():
        mmvqa_amd.asl_loss(model(img, ids, seg, mask)[0], tgt).backward()
        opt.step()

    def step_cached():
        mmvqa_amd.asl_loss(model.forward_cached(cache, index, view, ids, seg, mask)[0], tgt).backward()
        opt.step()

    dl = torch.zeros(B, bench.N_CLASSES, device=dev)

    def fb_cached():                 # forward + backward only: what (c) covers
        model.forward_cached(cache, index, view, ids, seg, mask)[0].backward(dl)

    def above_tokens():              # (c): one serialized, profiled forward + backward of (a)
        model.profile(True, serialized=True)
        model(img, ids, seg, mask)[0].backward(dl)
        torch.cuda.synchronize()
        reg = model.profile_read_regions()
        model.profile(False)
        ms = {r: sum(c["ms"] for c in cls.values()) for r, cls in reg.items()}
        return sum(ms[r] for r in ABOVE), ms

    arms = (("frozen_full", step_full, as_full), ("cached", step_cached, as_cached),
            ("cached_forward_backward", fb_cached, as_cached))
    for _, step, mode in arms:
        mode()
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    ms = {n: [] for n, _, _ in arms}
    above, regions = [], None
    for _ in range(a.rounds):
        for n, step, mode in arms:
            mode()                   # (taken up by the untimed step below: the optimizer re-reads requires_grad there)
            step()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            ms[n].append(e0.elapsed_time(e1) / a.steps)
        as_full()
        c, regions = above_tokens()
        above.append(c)
    model.flat_grads.zero_()

    # ---- the pieces a cached step adds: the gather alone, and the host side of index / view
    H, lib = args.hidden_size, L.lib()
    maps = cached_maps(index, view, N, K, B).to(dev)
    out = torch.empty(5, B, H, device=dev)
    import ctypes as C
    vw = C.c_void_p(maps.data_ptr() + 4 * B)

    def gather():
        L.check(lib.mmvqa_tokens_gather(L.stream_ptr(), L.ptr(cache.tokens), N, K, L.ptr(maps), vw, L.ptr(out), B, H, 5))

    for _ in range(10):
        gather()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200):
        gather()
    e1.record()
    torch.cuda.synchronize()
    us_gather = e0.elapsed_time(e1) * 1e3 / 200

    def upload():
        m = cached_maps(index, view, N, K, B)
        p = torch.empty(m.numel(), dtype=torch.int32, pin_memory=True)
        p.copy_(m)
        p.to(dev, non_blocking=True)

    us_upload = timed_host(upload, 200) * 1e6

    res = dict(shape=name, cnn=args.cnn_encoder, encoder=args.transformer_model, B=B, T=T, rounds=a.rounds,
               steps_per_visit=a.steps, step_ms={n: spread(v) for n, v in ms.items()},
               above_tokens_ms_serialized=spread(above),
               regions_ms_serialized={r: round(v, 3) for r, v in regions.items()},
               gather_us=round(us_gather, 2), index_view_host_us=round(us_upload, 1),
               cache=dict(images=N, views=K, bytes=cache.nbytes),
               fill=dict(images_per_s=round(B / t_fill, 1), visual_tokens_images_per_s=round(B / t_vis, 1)))
    b, c = res["step_ms"]["cached_forward_backward"]["median"], res["above_tokens_ms_serialized"]["median"]
    res["cached_forward_backward_minus_above_tokens_ms"] = round(b - c, 3)
    res["above_tokens_spread_ms"] = round(max(above) - min(above), 3)
    res["speedup_cached_over_frozen_full"] = round(res["step_ms"]["frozen_full"]["median"] / res["step_ms"]["cached"]["median"], 2)
    del model, opt, cache
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--shapes", type=str, nargs="+", default=["config5", "resnet152"], choices=["config5", "resnet152"])
    ap.add_argument("--out_dir", type=str, default=ROOT, help="the files go to <out_dir>/profiles/cached_cfg{5,2}.json")
    a = ap.parse_args()
    for n in a.shapes:
        res = measure(n, a)
        print(json.dumps(res))
        path = os.path.join(a.out_dir, OUT[n])
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
