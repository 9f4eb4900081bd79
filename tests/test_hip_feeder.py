"""GPU tests of the device input pipeline for training: the one-launch train chain (mmvqa_aug_train_fused) against the
multi-launch stages and Pillow, its refusal when the image does not fit LDS, the DeviceFeeder end to end against a
CPU rebuild of every batch, slot reuse under a slow consumer, and the CLI on generated ROCO / VQA-Med trees."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from feeder_helpers import ROOT, VOCAB, make_roco_tree, make_vqa_tree, rebuild_images, tokenizer
from mmvqa_amd import _lib as L
from mmvqa_amd import augment as AU
from mmvqa_amd import data as D
from mmvqa_amd import text
from oracle import augment_oracle as AO
from test_augment import synth_image

pytestmark = pytest.mark.gpu

SRC_SIZES = [(224, 224), (100, 120), (37, 900), (900, 37), (1500, 1200), (301, 257)]


def _upload(imgs):
    host = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs]))
    offs = np.cumsum([0] + [a.size for a in imgs])[:-1].tolist()
    return host.cuda(), offs, [a.shape[:2] for a in imgs]


def _cases(S=224):
    """>= 64 images (not a power of two) and their params: random ROCO and VQA draws, angle 0, the fallback box,
    jitter factors 1.0 / on the `inside` bounds, negative hue, all-0 and all-255 images"""
    rng = np.random.default_rng(3)
    imgs = []
    for n in range(66):
        h, w = SRC_SIZES[n % len(SRC_SIZES)]
        a = synth_image(rng, h, w)
        if n == 7:
            a[:] = 0
        if n == 8:
            a[:] = 255
        imgs.append(a)
    g = torch.Generator().manual_seed(9)
    params = AU.sample_params(33, S, generator=g, **D.ROCO_AUG) + AU.sample_params(33, S, generator=g, **D.VQA_AUG)
    params[1]["angle"] = 0.0
    params[2]["box"] = (0, 0, S, S)                                   # RandomResizedCrop's fallback (central) box
    params[3].update(brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0)
    params[4].update(brightness=0.0, contrast=1.0, saturation=0.0)    # factors on the `inside` bounds
    params[5].update(hue=-0.3, order=[3, 1, 0, 2])                    # negative hue: wraps as uint8
    params[6].update(contrast=0.0, order=[1, 1, 1, 1])                # the same op in every round (contrast x4)
    params[7].update(hue=0.4)
    params[9]["box"] = (S - 1, S - 1, 1, 1)                           # a one-pixel box
    params[10]["box"] = (0, 3, S, S - 3)
    return imgs, params


def test_fused_equals_multi_launch_bit_for_bit():
    imgs, params = _cases()
    src, offs, shapes = _upload(imgs)
    aug = AU.DeviceAugment(train=True)
    s = torch.cuda.current_stream()
    ref = aug.run_packed(src, offs, shapes, params, s, fused=False)
    ref_u8 = aug.last_uint8.clone()
    assert aug.last_fused is False
    got = aug.run_packed(src, offs, shapes, params, s, fused=True)
    assert aug.last_fused is True
    got_u8 = aug.last_uint8.clone()
    torch.cuda.synchronize()
    bad = [n for n in range(len(imgs)) if not torch.equal(got_u8[n], ref_u8[n])]
    assert not bad, f"uint8 differs on images {bad}: {[(int((got_u8[n] != ref_u8[n]).sum())) for n in bad[:5]]}"
    assert torch.equal(got, ref)
    # the multi-launch chain of run_packed is today's __call__ chain on the same images and params
    old = aug(imgs[:9], params=params[:9])
    torch.cuda.synchronize()
    assert torch.equal(old, ref[:9]) and torch.equal(aug.last_uint8, ref_u8[:9])


def test_fused_equals_pillow():
    imgs, params = _cases()
    pick = [0, 1, 2, 4, 5, 8, 33, 40]
    imgs, params = [imgs[i] for i in pick], [params[i] for i in pick]
    src, offs, shapes = _upload(imgs)
    aug = AU.DeviceAugment(train=True)
    out = aug.run_packed(src, offs, shapes, params)
    torch.cuda.synchronize()
    assert aug.last_fused
    for n, (a, p) in enumerate(zip(imgs, params)):
        ref_u8, ref_f = AO.train_transform(a, p)
        assert np.array_equal(aug.last_uint8[n].cpu().numpy(), ref_u8), f"image {n} {a.shape}"
        assert torch.equal(out[n].cpu(), ref_f)


def test_too_large_for_lds_is_refused_and_falls_back():
    lib = L.lib()
    S = 256                                                           # 196 608 B > 160 KiB of LDS
    dummy = torch.zeros(64, dtype=torch.uint8, device="cuda")
    f = torch.zeros(16, device="cuda")
    m = (C.c_float * 3)(0.5, 0.5, 0.5)
    rc = lib.mmvqa_aug_train_fused(L.stream_ptr(), L.ptr(dummy), L.ptr(f), L.ptr(dummy), L.ptr(dummy), 1, S, m, m)
    assert rc == -1 and b"LDS" in lib.mmvqa_last_error()
    assert lib.mmvqa_aug_train_fused_fits(224) == 1 and lib.mmvqa_aug_train_fused_fits(S) == 0
    assert lib.mmvqa_aug_train_fused(L.stream_ptr(), None, L.ptr(f), L.ptr(dummy), L.ptr(dummy), 1, 224, m, m) == -1
    rng = np.random.default_rng(4)
    imgs = [synth_image(rng, h, w) for h, w in SRC_SIZES[:5]]
    g = torch.Generator().manual_seed(2)
    params = AU.sample_params(5, 240, generator=g, **D.VQA_AUG)
    src, offs, shapes = _upload(imgs)
    aug = AU.DeviceAugment(size=240, train=True, **D.VQA_AUG)
    got = aug.run_packed(src, offs, shapes, params, fused=True)
    assert aug.last_fused is False                                    # 240 * 240 * 3 B do not fit: multi-launch
    got_u8 = aug.last_uint8.clone()
    ref = aug.run_packed(src, offs, shapes, params, fused=False)
    torch.cuda.synchronize()
    assert torch.equal(got, ref) and torch.equal(got_u8, aug.last_uint8)


def _rebuild_check(batch, entry, ds_rows, tok, kw, seed, T, S=224, train=True):
    img, ids, seg, mask, tgt = batch
    paths = [ds_rows[i][0] for i in entry["index"]]
    _u8, ref_f = rebuild_images(paths, entry["params"] if train else None, S)
    assert torch.equal(img.cpu(), ref_f), f"epoch {entry['epoch']} batch {entry['batch']}: image differs"
    for n, i in enumerate(entry["index"]):
        r = text.roco_text_batch([ds_rows[i][1]], tok, kw, 5, T, 0.3, rng=D.sample_rng(seed, entry["epoch"], i))
        for a, b in zip((ids[n], seg[n], mask[n], tgt[n]), r):
            assert torch.equal(a.cpu(), b[0])


@pytest.fixture(scope="module")
def roco_tree(tmp_path_factory):
    return make_roco_tree(str(tmp_path_factory.mktemp("roco")), n_train=19, n_val=5)   # 17 rows: 4 x 4 + 1


def _feeder(root, workers=2, depth=2, seed=21, T=24):
    tok, kw = tokenizer(), D.load_keywords(root)
    rows = D.roco_table(root, "train")
    ds = D.RocoDataset(rows, tok, kw, 5, T, 0.3, seed=seed)
    host = D.HostLoader(ds, 4, shuffle=True, seed=seed, num_workers=workers, aug=D.VQA_AUG, size=224)
    return D.DeviceFeeder(host, "cuda", depth=depth), rows, tok, kw, seed, T


def test_feeder_stream_has_the_least_priority(roco_tree):
    fd = _feeder(roco_tree, workers=0)[0]
    lib = L.lib()
    got, normal = C.c_int(), C.c_int()
    L.check(lib.mmvqa_stream_priority(C.c_void_p(fd.stream.cuda_stream), C.byref(got)))
    L.check(lib.mmvqa_stream_priority(L.stream_ptr(), C.byref(normal)))
    assert got.value == fd.priority and got.value > normal.value          # HIP: a larger number is a lower priority
    assert D.DeviceFeeder(fd.host, "cuda").stream.cuda_stream == fd.stream.cuda_stream   # one per device


def test_feeder_end_to_end(roco_tree):
    fd, rows, tok, kw, seed, T = _feeder(roco_tree)
    with pytest.raises(RuntimeError, match="GPU only"):
        D.DeviceFeeder(fd.host, "cpu")
    for epoch in range(2):
        fd.set_epoch(epoch)
        got = [tuple(t.clone() for t in b) for b in fd]
        torch.cuda.synchronize()
        log = fd.log[-len(got):]
        assert [len(e["index"]) for e in log] == [4, 4, 4, 4, 1]
        assert sorted(sum((e["index"] for e in log), [])) == list(range(17))
        for b, e in zip(got, log):
            assert e["epoch"] == epoch
            _rebuild_check(b, e, rows, tok, kw, seed, T)
    assert fd.aug.last_fused


def test_feeder_slot_reuse_under_a_slow_consumer(roco_tree):
    """the consumer enqueues tens of ms of work on its stream before it reads each batch: a feeder that refilled a
    slot before the consumer's stream had passed it would overwrite the batch before the clone reads it.  Also across
    an epoch left early (break) and the next one started at once."""
    fd, rows, tok, kw, seed, T = _feeder(roco_tree, workers=1)
    a = torch.randn(4096, 4096, device="cuda")
    c = torch.empty_like(a)
    waits = []

    def slow_read(batch):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(24):                                            # bounded: 24 x 137 GFLOP on the caller's stream
            torch.mm(a, a, out=c)
        e1.record()
        waits.append((e0, e1))
        return tuple(t.clone() for t in batch)

    fd.set_epoch(0)
    clones, entries = [], []
    for batch in fd:                                                   # leave epoch 0 after its first batch
        clones.append(slow_read(batch))
        entries.append(fd.log[-1])
        break
    fd.set_epoch(1)
    for batch in fd:
        clones.append(slow_read(batch))
        entries.append(fd.log[-1])
    torch.cuda.synchronize()
    assert len(clones) == 6 and [e["epoch"] for e in entries] == [0, 1, 1, 1, 1, 1]
    ms = [e0.elapsed_time(e1) for e0, e1 in waits]
    assert min(ms) >= 10.0, ms                                         # the margin the test relies on, measured
    for b, e in zip(clones, entries):
        _rebuild_check(b, e, rows, tok, kw, seed, T)


MINI = ["--resnet_layers", "1", "1", "1", "1", "--resnet_width", "8", "--hidden_size", "96", "--n_layers", "2",
        "--vocab_size", "64", "--emb_vocab", "64", "--image_size", "32", "--steps_per_epoch", "6", "--val_steps", "2",
        "--epochs", "5", "--max_position_embeddings", "16", "--hidden_dropout_prob", "0.1"]
# the vocabulary of the generated trees has 213 pieces: the embedding must cover it
DATA = ["--vocab_size", "256", "--emb_vocab", "256", "--epochs", "2", "--batch_size", "4", "--num_workers", "2",
        "--vocab_file", VOCAB]


def _cli(args, timeout=900):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "mmvqa_amd.train"] + args, cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _losses(out, pat):
    v = [float(x) for x in re.findall(pat, out)]
    assert v and all(math.isfinite(x) for x in v), out
    return v


def test_cli_trains_from_files(tmp_path, roco_tree):
    out = _cli(["mlm", "--data_dir", roco_tree, "--lr", "1e-3", "--save_dir", str(tmp_path / "mlm")] + MINI + DATA)
    assert len(_losses(out, r"Train loss: (\S+),")) == 2 and _losses(out, r"Val loss: (\S+),")
    assert (tmp_path / "mlm" / "MLM" / "run.pt").exists()
    vq = make_vqa_tree(str(tmp_path / "vqa"))
    out = _cli(["vqa", "--data_dir", vq, "--lr", "1e-3", "--save_dir", str(tmp_path / "ft")] + MINI + DATA)
    assert len(_losses(out, r"train_loss (\S+) ")) == 2 and _losses(out, r"val_loss (\S+) ")
    ck = tmp_path / "ft" / "MLM" / "run_loss.pt"
    assert ck.exists()
    out = _cli(["eval", "--data_dir", vq, "--model_dir", str(ck), "--save_dir", str(tmp_path / "ev")] + MINI + DATA)
    _losses(out, r"test_loss (\S+)")
    _cols, tabs, _idx2ans = D.vqa_tables(vq)
    import csv
    rows = list(csv.reader(open(tmp_path / "ev" / "run_loss.pt_preds.csv")))
    assert [r[0] for r in rows[1:]] == [t[0] for t in tabs["test"]]              # the real image paths, file order
    res = open(tmp_path / "ev" / "run_loss.pt_res.txt").read().splitlines()
    assert len(res) == len(tabs["test"]) and res[0].startswith("synpictest0|")
