#!/usr/bin/env python3
"""Config-2 training step (resnet152 + transformer, ROCO MLM, B 16, 224^2, T 32) fed synthetically vs by the
DeviceFeeder from JPEG files, in one process, in alternating blocks; plus the augment's GPU time per batch, fused
(3 launches) vs fused=False (the multi-launch chain).

--config 4: the SupCon step of bench.py --config 4 (tf_efficientnetv2_m + realformer + SupCon head, 16 pairs = 32
views, 224^2, T 32) fed by a RocoSupConDataset feeder (two views per image, run_packed(views=2)); the augment's GPU
time for three forms: the views launch, the one-view fused launch on the 32 images duplicated, the multi-launch chain.

A local ROCO-like tree is generated first (sides 400-1200 px, mixed aspect, baseline JPEG; with --config 4 also the
three translation columns): no dataset is needed.  Host cores used = CPU time of this process and of the decode
workers over the wall time of the fed blocks.

    python tools/feeder_bench.py --out profiles/feeder_cfg2.json
    python tools/feeder_bench.py --config 4 --out profiles/feeder_cfg4.json

--config 4 --supcon_mask jaccard: the fed config-4 step with the Jaccard positive mask (train.py --supcon_mask jaccard:
the feeder hands out the (row, column) pairs, mmvqa_jaccard_mask builds the mask, mmvqa_supcon_loss_masked replaces the
unmasked loss) against the same fed step without it, alternating blocks in one process; plus the GPU time of the mask
launch and of the masked loss (forward + gradient) next to the unmasked loss, alone on an idle device.

    python tools/feeder_bench.py --config 4 --supcon_mask jaccard --out profiles/supcon_mask_cfg4.json

--config 4 --supcon_mask embeddings: the same with a third kind of block, the step under the caption-embedding mask
(train.py --supcon_mask embeddings: mmvqa_cosine_mask over a resident table of random non-negative 768-wide embeddings
for the generated table), alternating unmasked / jaccard / embeddings blocks in one process; the cosine launch alone at
(n, D) = (16, 768) and (128, 768) next to the Jaccard launch; and the one-off upload + normalisation of a
65 536-row x 768 table.

    python tools/feeder_bench.py --config 4 --supcon_mask embeddings --out profiles/supcon_embed_cfg4.json
"""
import argparse
import json
import os
import pickle
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, T, HW, VOCAB = 16, 32, 224, 30522
WORDS = ("axial ct of the chest showing a mass in the left upper lobe , mri of the brain with lesion and edema "
         "bilateral pleural effusion on chest x - ray normal liver kidney fracture nodule").split()


def make_tree(root, n, seed=0, translations=False):
    from PIL import Image
    rng = np.random.default_rng(seed)
    d = os.path.join(root, "train", "radiology")
    os.makedirs(os.path.join(d, "images"))
    with open(os.path.join(d, "traindata.csv"), "w") as f:
        f.write("id,name,caption" + (",fr,de,es" if translations else "") + "\n")
        for i in range(n):
            h, w = (int(v) for v in rng.integers(400, 1201, 2))
            yy, xx = np.mgrid[0:h, 0:w]
            img = np.stack([127 + 120 * np.sin(xx / (5 + i % 7) + yy / 17.0), 127 + 120 * np.cos(xx / 13.0 - yy / 7.0),
                            (xx * 3 + yy * 5 + i) % 256], -1) + rng.normal(0, 20, (h, w, 3))
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(d, "images", f"{i}.jpg"), quality=90)
            cap = " ".join(rng.choice(WORDS, int(rng.integers(8, 30))))
            tr = "".join(f",\"{' '.join(rng.choice(WORDS, int(rng.integers(8, 30))))}\"" for _ in range(3)) if translations else ""
            f.write(f"ROCO_{i},{i}.jpg,\"{cap}\"{tr}\n")
    os.makedirs(os.path.join(root, "vocab"))
    with open(os.path.join(root, "vocab", "med_vocab.pkl"), "wb") as f:
        pickle.dump({"organ": ["chest", "brain", "liver", "kidney"], "finding": ["mass", "lesion", "fracture"]}, f)


def cpu_seconds(pid):
    try:
        v = open(f"/proc/{pid}/stat").read().rsplit(")", 1)[1].split()
        return (int(v[11]) + int(v[12])) / os.sysconf("SC_CLK_TCK")
    except OSError:
        return 0.0


def mask_bench(a, dev, tmp, model, opt, red, tok, fd, T_):
    """fed config-4 step with / without the Jaccard mask (and, with --supcon_mask embeddings, under the
    caption-embedding mask), and the mask / loss launches alone"""
    import mmvqa_amd
    from mmvqa_amd import _lib as L
    from mmvqa_amd import data as D
    from mmvqa_amd.train import supcon_step
    table = D.roco_supcon_table(tmp)
    t0 = time.perf_counter()
    host_words = D.WordSets.from_table(table)
    words_ms = 1e3 * (time.perf_counter() - t0)
    words = host_words.to(dev)
    ds = D.RocoSupConDataset(table, tok, D.load_keywords(tmp), 5, T_, 0.15, seed=1, report_aug_col=True)
    host = D.HostLoader(ds, B, shuffle=True, seed=1, num_workers=a.workers, aug=D.ROCO_AUG, size=HW, views=2)
    fdm = D.DeviceFeeder(host, dev, depth=2, pairs=True)

    def batches(feeder):
        epoch = 0
        while True:
            feeder.set_epoch(epoch)
            for b in feeder:
                if b[0].shape[0] == 2 * B:
                    yield b
            epoch += 1

    gens = {"unmasked": (batches(fd), None), "masked": (batches(fdm), words)}
    embed = a.supcon_mask == "embeddings"
    De = 768                                     # all-mpnet-base-v2, the reference's default encoder
    if embed:                                    # a second feeder with pairs: every kind of block draws its own batches
        erng = np.random.default_rng(2)
        host_emb = D.CaptionEmbeddings.from_array((np.abs(erng.standard_normal((len(table), 4, De))) + 0.25).astype(np.float32))
        emb = host_emb.to(dev)
        hoste = D.HostLoader(ds, B, shuffle=True, seed=1, num_workers=a.workers, aug=D.ROCO_AUG, size=HW, views=2)
        gens["embeddings"] = (batches(D.DeviceFeeder(hoste, dev, depth=2, pairs=True)), emb)

    def run(n, kind):
        g, w = gens[kind]
        for _ in range(n):
            _, _, stats = supcon_step(model, opt, red, 1, next(g), words=w)
            stats.tolist()                       # the per-step host sync of train.py
    for kind in gens:
        run(a.warmup, kind)
    torch.cuda.synchronize()
    res = {k: [] for k in gens}
    for _ in range(a.blocks):
        for kind in gens:
            t0 = time.perf_counter()
            run(a.steps, kind)
            torch.cuda.synchronize()
            res[kind].append(1e3 * (time.perf_counter() - t0) / a.steps)
            print(f"{kind:9s} {res[kind][-1]:.2f} ms/step", flush=True)

    # the launches alone: the stream is held behind a ~20 ms matmul block so that the host side of the calls is done
    # before the GPU reaches e0 (the method of augment_gpu_ms_per_batch)
    s = torch.cuda.Stream()
    m = torch.randn(4096, 4096, device=dev)
    mo = torch.empty_like(m)
    lib, Dm = L.lib(), 128
    alone = {}
    for n in (16, 128):                          # one GPU's 16 pairs; the gathered set of 8 GPUs
        g = torch.Generator().manual_seed(n)
        f = torch.nn.functional.normalize(torch.randn(2 * n, Dm, generator=g), dim=1).to(dev)
        rows = torch.randint(0, len(table), (n,), generator=g).to(torch.int32).to(dev)
        cols = torch.randint(1, 4, (n,), generator=g).to(torch.int32).to(dev)
        zero = torch.zeros_like(cols)
        mask = torch.empty(n, n, device=dev)
        loss, df, ws = torch.empty(1, device=dev), torch.empty_like(f), torch.empty(6 * n, device=dev)
        sp = s.cuda_stream
        calls = {
            "jaccard_mask": lambda: lib.mmvqa_jaccard_mask(sp, L.ptr(words.offsets), L.ptr(words.ids), L.ptr(rows), L.ptr(zero),
                                                           L.ptr(rows), L.ptr(cols), L.ptr(mask), n, words.rows),
            "masked_loss_fwd_bwd": lambda: lib.mmvqa_supcon_loss_masked(sp, L.ptr(f), L.ptr(mask), L.ptr(loss), L.ptr(df),
                                                                        L.ptr(ws), n, Dm, 0.07, 0.07, 1.0),
            "unmasked_loss_fwd_bwd": lambda: lib.mmvqa_supcon_loss(sp, L.ptr(f), L.ptr(loss), L.ptr(df), L.ptr(ws), n, Dm,
                                                                   0.07, 0.07, 1.0),
        }
        if embed:
            calls[f"cosine_mask_D{De}"] = lambda: lib.mmvqa_cosine_mask(sp, L.ptr(emb.table), L.ptr(rows), L.ptr(zero),
                                                                        L.ptr(rows), L.ptr(cols), L.ptr(mask), n, De, emb.rows)
        for key, call in calls.items():
            ts = []
            for r in range(a.aug_reps + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(s):
                    for _ in range(12):
                        torch.mm(m, m, out=mo)
                e0.record(s)
                L.check(call())
                e1.record(s)
                e1.synchronize()
                if r >= 3:
                    ts.append(e0.elapsed_time(e1))
            alone[f"{key}_n{n}"] = round(statistics.median(ts), 4)
    un, ma = statistics.median(res["unmasked"]), statistics.median(res["masked"])
    spread = max(res["unmasked"]) - min(res["unmasked"])
    extra = {}
    if embed:
        em = statistics.median(res["embeddings"])
        # the one-off cost of a ROCO-sized table: 65 536 rows x 4 texts x 768 floats = 0.8 GB, upload + normalise
        big = D.CaptionEmbeddings(torch.rand(65536, 4, De).pin_memory())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        big_dev = big.to(dev)
        torch.cuda.synchronize()
        to_ms = 1e3 * (time.perf_counter() - t0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(L.lib().mmvqa_normalize_rows(L.stream_ptr(), L.ptr(big_dev.table), big.rows * 4, De, 1e-8))
        e1.record()
        e1.synchronize()
        extra = dict(embeddings_ms_per_step=round(em, 3), embeddings_minus_unmasked_ms=round(em - un, 3),
                     embeddings_minus_jaccard_ms=round(em - ma, 3), embeddings_within_unmasked_spread=bool(em - un <= spread),
                     caption_embeddings=dict(table_rows=host_emb.rows, D=De, mbytes=round(host_emb.table.numel() * 4 / 2 ** 20, 2),
                                             roco_sized_table_rows=65536, roco_sized_table_mbytes=round(65536 * 4 * De * 4 / 2 ** 20, 1),
                                             roco_sized_to_device_ms=round(to_ms, 1),
                                             roco_sized_normalize_rows_ms=round(e0.elapsed_time(e1), 3),
                                             note="to_device = CaptionEmbeddings.to(device) from pinned host memory, upload "
                                                  "+ mmvqa_normalize_rows, wall time to completion, once; normalize_rows = "
                                                  "the kernel alone on that table (events)"))
        del big, big_dev
    out = dict(
        workload="config 4 (tf_efficientnetv2_m + realformer + SupCon head, ROCO MLM + SupCon), 16 pairs = 32 views, 224^2, "
                 f"T 32, one GPU, fed by a DeviceFeeder (depth 2, views 2) over {a.images} generated JPEGs; unmasked = "
                 "supcon_step as train.py runs it without --supcon_mask (the launches of the default path); masked = "
                 "--supcon_mask jaccard: feeder with pairs, mmvqa_jaccard_mask, mmvqa_supcon_loss_masked"
                 + ("; embeddings = --supcon_mask embeddings: feeder with pairs, mmvqa_cosine_mask over a resident "
                    f"[{len(table)}, 4, {De}] table of random non-negative embeddings, mmvqa_supcon_loss_masked" if embed else ""),
        unmasked_ms_per_step=round(un, 3), masked_ms_per_step=round(ma, 3), ratio=round(ma / un, 4),
        unmasked_block_spread_ms=round(spread, 3), masked_minus_unmasked_ms=round(ma - un, 3),
        within_unmasked_spread=bool(ma - un <= spread), **extra,
        blocks={k: [round(x, 3) for x in v] for k, v in res.items()}, steps_per_block=a.steps, workers=host.num_workers,
        word_sets=dict(table_rows=host_words.rows, ids=int(host_words.ids.numel()), words=len(host_words.vocab),
                       host_build_ms=round(words_ms, 3)),
        gpu_ms_alone=dict(alone, D=Dm,
                          method="cuda events around the launches of one C-ABI call, the stream held behind a ~20 ms matmul "
                                 f"block so that the host side is done first; otherwise idle device, median of {a.aug_reps}; "
                                 "the loss calls are forward + gradient + reduce (2N rows, D 128)"))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2, choices=[2, 4])
    ap.add_argument("--images", type=int, default=384)
    ap.add_argument("--blocks", type=int, default=4, help="block pairs (synthetic, fed)")
    ap.add_argument("--steps", type=int, default=12, help="steps per block")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--aug_reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--supcon_mask", type=str, default="none", choices=["none", "jaccard", "embeddings"],
                    help="jaccard (with --config 4): time the fed step with the Jaccard mask against the one without; "
                         "embeddings: also the step with the caption-embedding mask, and the cosine launch")
    a = ap.parse_args()
    if a.supcon_mask != "none" and a.config != 4:
        ap.error("--supcon_mask needs --config 4 (the SupCon step)")

    import mmvqa_amd
    from mmvqa_amd import data as D
    from mmvqa_amd import synth, text
    from mmvqa_amd.ddp import GradReducer
    from mmvqa_amd.train import mlm_step, process_tensors, supcon_step
    from types import SimpleNamespace

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.set_num_threads(min(D.usable_host_threads(), 16))
    tmp = tempfile.mkdtemp(prefix="feeder_bench_")
    t0 = time.perf_counter()
    cfg4 = a.config == 4
    make_tree(tmp, a.images, translations=cfg4)
    print(f"generated {a.images} JPEGs in {time.perf_counter() - t0:.1f} s", flush=True)

    torch.manual_seed(1234)
    if cfg4:            # bench.py --config 4
        args = SimpleNamespace(task="MLM", dataset="roco", transformer_model="realformer", cnn_encoder="tf_efficientnetv2_m",
                               num_vis=5, hidden_size=768, n_layers=4, heads=12, hidden_dropout_prob=0.3,
                               vocab_size=VOCAB, use_relu=False, max_position_embeddings=T, supcon=True)
    else:
        args = SimpleNamespace(task="MLM", dataset="roco", transformer_model="transformer", cnn_encoder="resnet152",
                               num_vis=5, hidden_size=768, n_layers=4, heads=12, hidden_dropout_prob=0.3,
                               vocab_size=VOCAB, use_relu=False, max_position_embeddings=T)
    model = mmvqa_amd.Model(args).to(dev).train()
    model.set_seed(1234)
    opt = mmvqa_amd.FusedAdam(model, lr=2e-5)
    red = GradReducer(model.flat_grads, bucket_mb=64.0)
    if cfg4:            # 16 pairs = 32 views, as bench.py --config 4 builds them
        va = synth.roco_batch(B, T, HW, VOCAB, seed=1234, device=dev)
        vb = synth.roco_batch(B, T, HW, VOCAB, seed=4321, device=dev)
        syn = process_tensors((va[0], vb[0]), va[1], vb[1], va[2], va[3], va[4], vb[4])
    else:
        syn = synth.roco_batch(B, T, HW, VOCAB, seed=1234, device=dev)
    model.tune(*syn[:4])
    step_fn = supcon_step if cfg4 else mlm_step
    views = 2 if cfg4 else 1

    tok = text.BertWordPiece(os.path.join(ROOT, "tests", "golden", "text_vocab.txt"))
    if cfg4:
        ds = D.RocoSupConDataset(D.roco_supcon_table(tmp), tok, D.load_keywords(tmp), 5, T, 0.15, seed=1)
    else:
        ds = D.RocoDataset(D.roco_table(tmp, "train"), tok, D.load_keywords(tmp), 5, T, 0.15, seed=1)
    host = D.HostLoader(ds, B, shuffle=True, seed=1, num_workers=a.workers, aug=D.ROCO_AUG, size=HW, views=views)
    fd = D.DeviceFeeder(host, dev, depth=2)
    if a.supcon_mask != "none":
        return mask_bench(a, dev, tmp, model, opt, red, tok, fd, T)

    def fed_batches():
        epoch = 0
        while True:
            fd.set_epoch(epoch)
            for b in fd:
                if b[0].shape[0] == views * B:
                    yield b
            epoch += 1

    fed = fed_batches()
    next_ms = []

    def run(n, feed):
        for _ in range(n):
            if feed:
                t = time.perf_counter()
                b = next(fed)                    # host time between step n's sync and step n + 1's first launch
                next_ms.append(1e3 * (time.perf_counter() - t))
            else:
                b = syn
            _, _, stats = step_fn(model, opt, red, 1, b)
            stats.tolist()                       # the per-step host sync of train.py
    run(a.warmup, False)
    run(a.warmup, True)
    torch.cuda.synchronize()
    next_ms.clear()
    workers = [w.pid for w in fd.host.loader._iterator._workers]
    res = {"synthetic": [], "fed": []}
    cpu_fed, wall_fed = 0.0, 0.0
    for _ in range(a.blocks):
        for kind in ("synthetic", "fed"):
            c0 = time.process_time() + sum(cpu_seconds(p) for p in workers)
            t0 = time.perf_counter()
            run(a.steps, kind == "fed")
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res[kind].append(1e3 * dt / a.steps)
            if kind == "fed":
                cpu_fed += time.process_time() + sum(cpu_seconds(p) for p in workers) - c0
                wall_fed += dt
            print(f"{kind:9s} {res[kind][-1]:.2f} ms/step", flush=True)

    # the augment alone: one ROCO-like batch.  A bounded ~20 ms matmul block goes first on the stream, so the GPU
    # reaches e0 only after run_packed has finished its host-side packing: e0 -> e1 spans the blob upload and the
    # launches alone (GPU time), not the Python work before them.
    rows = D.roco_table(tmp, "train")[:B]
    imgs = [D.decode(p) for p, _ in rows]
    src = torch.from_numpy(np.concatenate([x.reshape(-1) for x in imgs])).to(dev)
    offs = np.cumsum([0] + [x.size for x in imgs])[:-1].tolist()
    shapes = [x.shape[:2] for x in imgs]
    aug = mmvqa_amd.augment.DeviceAugment(train=True, **D.ROCO_AUG)
    params = mmvqa_amd.augment.sample_params(views * B, HW, generator=torch.Generator().manual_seed(3), **D.ROCO_AUG)
    if cfg4:            # (key, run_packed arguments): the same 32 views three ways
        rows = [params[n * 2 + v] for v in range(2) for n in range(B)]
        forms = [("views", (src, offs, shapes, params), dict(fused=True, views=2)),
                 ("one_view_fused_duplicated", (src, offs + offs, shapes + shapes, rows), dict(fused=True)),
                 ("multi_launch", (src, offs, shapes, params), dict(fused=False, views=2))]
    else:
        forms = [("fused", (src, offs, shapes, params), dict(fused=True)),
                 ("multi_launch", (src, offs, shapes, params), dict(fused=False))]
    s = torch.cuda.Stream()
    m = torch.randn(4096, 4096, device=dev)
    mo = torch.empty_like(m)
    aug_ms, host_ms, margins = {}, {}, []
    for key, pos, kw in forms:
        ts, hs = [], []
        for r in range(a.aug_reps + 3):
            ep, e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            ep.record(s)
            with torch.cuda.stream(s):
                for _ in range(12):
                    torch.mm(m, m, out=mo)
            e0.record(s)
            t = time.perf_counter()
            aug.run_packed(*pos, stream=s, **kw)
            h = 1e3 * (time.perf_counter() - t)
            e1.record(s)
            e1.synchronize()
            if r >= 3:
                ts.append(e0.elapsed_time(e1))
                hs.append(h)
                margins.append(ep.elapsed_time(e0) - h)   # > 0: the packing was done before the GPU reached e0
        aug_ms[key], host_ms[key] = statistics.median(ts), statistics.median(hs)
    syn_ms, fed_ms = statistics.median(res["synthetic"]), statistics.median(res["fed"])
    if cfg4:
        head = dict(workload="config 4 (tf_efficientnetv2_m + realformer + SupCon head, ROCO MLM + SupCon), 16 pairs = "
                             "32 views, 224^2, T 32, one GPU; fed = DeviceFeeder (depth 2, views 2) over a "
                             f"RocoSupConDataset of {a.images} generated JPEGs, sides 400-1200 px",
                    synthetic_ms_per_step=round(syn_ms, 3), fed_ms_per_step=round(fed_ms, 3),
                    ratio=round(fed_ms / syn_ms, 4))
    else:
        head = dict(workload="config 2 (resnet152 + transformer, ROCO MLM), B 16, 224^2, T 32, one GPU; fed = DeviceFeeder "
                             f"(depth 2) over {a.images} generated JPEGs, sides 400-1200 px",
                    synthetic_ms_per_step=round(syn_ms, 3), fed_ms_per_step=round(fed_ms, 3),
                    ratio=round(fed_ms / syn_ms, 4), target_ratio=1.03, target_met=fed_ms / syn_ms <= 1.03)
    out = dict(
        **head,
        blocks=dict(synthetic=[round(x, 3) for x in res["synthetic"]], fed=[round(x, 3) for x in res["fed"]]),
        steps_per_block=a.steps, workers=host.num_workers, usable_host_threads=D.usable_host_threads(),
        host_cores_used_fed=round(cpu_fed / wall_fed, 3),
        augment_gpu_ms_per_batch=dict({k: round(v, 4) for k, v in aug_ms.items()},
                                      method="cuda events around the upload + launches of run_packed, the stream held "
                                             "behind a ~20 ms matmul block so that host packing is done first; "
                                             f"otherwise idle device, median of {a.aug_reps}"),
        augment_timing_min_margin_ms=round(min(margins), 3),
        **(dict(augment_forms=dict(
            views="run_packed(views=2): Resize+CenterCrop of the 16 images, then mmvqa_aug_train_fused_views on 32 rows",
            one_view_fused_duplicated="run_packed on the 16 images listed twice (32 offsets): Resize+CenterCrop of 32, "
                                      "then mmvqa_aug_train_fused in place on 32 rows",
            multi_launch="run_packed(views=2, fused=False): Resize+CenterCrop of 16, then the stage launches on 32 rows"))
           if cfg4 else {}),
        augment_host_ms_per_batch={k: round(v, 3) for k, v in host_ms.items()},
        feeder_next_host_ms=dict(median=round(statistics.median(next_ms), 3), mean=round(statistics.mean(next_ms), 3),
                                 max=round(max(next_ms), 3),
                                 note="host time of DeviceFeeder.__next__ in the fed blocks (refill: DataLoader get + "
                                      "run_packed packing), spent after the step's sync while the GPU has no step work"),
        feeder_stream_priority=fd.priority,
        fused_launch_used=bool(fd.aug.last_fused))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
