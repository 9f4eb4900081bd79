"""GPU tests of SupCon's two-view input pipeline: mmvqa_aug_train_fused_views (V views of each image in one launch,
the resized image only read) against the one-view fused launch, the multi-launch chain and Pillow; its refusals; the
LDS fallback of run_packed(views=2); the DeviceFeeder over a RocoSupConDataset against a CPU rebuild of every batch;
and `train supcon --data_dir` on generated trees."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from feeder_helpers import ROOT, rebuild_images, tokenizer
from mmvqa_amd import _lib as L
from mmvqa_amd import augment as AU
from mmvqa_amd import data as D
from oracle import augment_oracle as AO
from supcon_helpers import make_supcon_tree
from test_augment import synth_image
from test_hip_feeder import DATA, MINI, SRC_SIZES, _cases, _losses, _upload

pytestmark = pytest.mark.gpu


def _row_params(params, B, V):
    """params in draw order (params[n * V + v]) -> output-row order (row v * B + n)"""
    return [params[n * V + v] for v in range(V) for n in range(B)]


@pytest.mark.parametrize("V", [2, 3])
def test_views_equal_one_view_launch_multi_launch_and_pillow(V):
    imgs, params = _cases()
    B = len(params) // V                                              # 33 x 2 or 22 x 3: the edge cases spread over views
    imgs = imgs[:B]
    src, offs, shapes = _upload(imgs)
    aug = AU.DeviceAugment(train=True)
    s = torch.cuda.current_stream()
    got = aug.run_packed(src, offs, shapes, params, s, fused=True, views=V)
    assert aug.last_fused is True and got.shape == (V * B, 3, 224, 224)
    got_u8 = aug.last_uint8.clone()
    assert got_u8.shape == (V * B, 224, 224, 3)
    multi = aug.run_packed(src, offs, shapes, params, s, fused=False, views=V)
    assert aug.last_fused is False
    multi_u8 = aug.last_uint8.clone()
    rows = _row_params(params, B, V)                                  # the one-view launch on the images repeated per row
    one = aug.run_packed(src, [offs[r % B] for r in range(V * B)], [shapes[r % B] for r in range(V * B)], rows, s,
                         fused=True)
    assert aug.last_fused is True
    one_u8 = aug.last_uint8.clone()
    torch.cuda.synchronize()
    for name, ref, ref_u8 in (("one-view fused", one, one_u8), ("multi-launch", multi, multi_u8)):
        bad = [r for r in range(V * B) if not torch.equal(got_u8[r], ref_u8[r])]
        assert not bad, f"{name}: uint8 differs on rows {bad}"
        assert torch.equal(got, ref), name
    for r in range(V * B):
        ref_u8, ref_f = AO.train_transform(imgs[r % B], rows[r])
        assert np.array_equal(got_u8[r].cpu().numpy(), ref_u8), f"row {r} (view {r // B} of image {r % B})"
        assert torch.equal(got[r].cpu(), ref_f), f"row {r}"


def test_views_source_is_read_only():
    imgs, params = _cases()
    imgs, params = imgs[:12], params[:24]
    src, offs, shapes = _upload(imgs)
    val = AU.DeviceAugment(train=False)
    resized = val.run_packed(src, offs, shapes)
    resized_u8 = val.last_uint8.clone()
    aug = AU.DeviceAugment(train=True)
    aug.run_packed(src, offs, shapes, params, fused=True, views=2)
    torch.cuda.synchronize()
    assert aug.last_fused and aug.last_resized.data_ptr() != aug.last_uint8.data_ptr()
    assert torch.equal(aug.last_resized, resized_u8)                 # src_u8 after the views launch: unchanged
    assert resized.shape == (12, 3, 224, 224)


def test_views_refusals():
    lib = L.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    f = torch.zeros(16, device="cuda")
    m = (C.c_float * 3)(0.5, 0.5, 0.5)
    st = L.stream_ptr()
    p, q = L.ptr(buf), C.c_void_p(buf.data_ptr() + 2048)             # (never launched on: every call below is refused)

    def call(src, scr, out, recs, tabs, B, V, S, mean=m, std=m):
        return lib.mmvqa_aug_train_fused_views(st, src, scr, out, recs, tabs, B, V, S, mean, std)

    def refused(rc, what):
        assert rc == -1, what
        assert what.encode() in lib.mmvqa_last_error(), (what, lib.mmvqa_last_error())

    for args in ((None, q, L.ptr(f), p, p), (p, None, L.ptr(f), p, p), (p, q, None, p, p), (p, q, L.ptr(f), None, p),
                 (p, q, L.ptr(f), p, None)):
        refused(call(*args, 1, 2, 224), "bad arguments")
    refused(call(p, q, L.ptr(f), p, p, 1, 2, 224, None, m), "bad arguments")
    refused(call(p, q, L.ptr(f), p, p, 1, 2, 224, m, None), "bad arguments")
    for B, V, S in ((0, 2, 224), (1, 0, 224), (1, 2, 0), (-1, 2, 224), (1, -2, 224), (1, 2, -3)):
        refused(call(p, q, L.ptr(f), p, p, B, V, S), "bad arguments")
    # overlapping ranges (compared, never touched): src_u8 is B * S * S * 3 bytes, scratch_u8 V times that
    img = 224 * 224 * 3
    at = lambda off: C.c_void_p(buf.data_ptr() + off)   # noqa: E731
    refused(call(p, at(1), L.ptr(f), p, p, 1, 2, 224), "overlap")                  # scratch starts inside src
    refused(call(p, at(img - 1), L.ptr(f), p, p, 1, 2, 224), "overlap")            # ... at src's last byte
    refused(call(at(2 * img - 1), p, L.ptr(f), p, p, 1, 2, 224), "overlap")        # src starts at scratch's last byte
    refused(call(p, p, L.ptr(f), p, p, 1, 1, 224), "overlap")
    assert lib.mmvqa_aug_train_fused_fits(256) == 0                   # 196 608 B > the device's LDS: refused below
    refused(call(p, at(1 << 30), L.ptr(f), p, p, 1, 2, 256), "LDS")


def test_views_lds_fallback():
    rng = np.random.default_rng(4)
    imgs = [synth_image(rng, h, w) for h, w in SRC_SIZES[:5]]
    params = AU.sample_params(10, 240, generator=torch.Generator().manual_seed(2), **D.VQA_AUG)
    src, offs, shapes = _upload(imgs)
    aug = AU.DeviceAugment(size=240, train=True, **D.VQA_AUG)
    got = aug.run_packed(src, offs, shapes, params, fused=True, views=2)
    assert aug.last_fused is False and got.shape == (10, 3, 240, 240)  # 240 * 240 * 3 B do not fit: multi-launch
    got_u8 = aug.last_uint8.clone()
    ref = aug.run_packed(src, offs, shapes, params, fused=False, views=2)
    torch.cuda.synchronize()
    assert torch.equal(got, ref) and torch.equal(got_u8, aug.last_uint8)
    rows = _row_params(params, 5, 2)
    for r in (0, 4, 5, 9):
        ref_u8, _ = AO.train_transform(imgs[r % 5], rows[r], 240)
        assert np.array_equal(got_u8[r].cpu().numpy(), ref_u8)
    with pytest.raises(ValueError):
        aug.run_packed(src, offs, shapes, params[:9], views=2)        # V * B parameter sets
    with pytest.raises(ValueError):
        AU.DeviceAugment(train=False).run_packed(src, offs, shapes, views=2)


@pytest.fixture(scope="module")
def supcon_tree(tmp_path_factory):
    return make_supcon_tree(str(tmp_path_factory.mktemp("supcon")))[0]     # 7 rows: 3 + 3 + 1 pairs, 2 + 2 + 2 + 1


def _check(batch, entry, ds, S=224):
    img, ids, seg, mask, tgt = batch
    n = len(entry["index"])
    assert img.shape[0] == 2 * n and ids.shape[0] == 2 * n and len(entry["params"]) == 2 * n
    paths = [ds.rows[entry["index"][r % n]][0] for r in range(2 * n)]
    _u8, ref_f = rebuild_images(paths, _row_params(entry["params"], n, 2), S)
    assert torch.equal(img.cpu(), ref_f), f"epoch {entry['epoch']} batch {entry['batch']}: image differs"
    txt = [ds.encode(entry["epoch"], i) for i in entry["index"]]
    col = lambda j: torch.stack([t[j] for t in txt])   # noqa: E731
    for got, ref in ((ids, torch.cat([col(0), col(1)])), (seg, torch.cat([col(2), col(2)])),
                     (mask, torch.cat([col(3), col(3)])), (tgt, torch.cat([col(4), col(5)]))):
        assert torch.equal(got.cpu(), ref), f"epoch {entry['epoch']} batch {entry['batch']}: text differs"


def test_feeder_two_views_end_to_end(supcon_tree):
    ds = D.RocoSupConDataset(D.roco_supcon_table(supcon_tree), tokenizer(), D.load_keywords(supcon_tree), 5, 24, 0.3,
                             seed=17)
    host = D.HostLoader(ds, 3, shuffle=True, seed=17, num_workers=2, aug=D.ROCO_AUG, size=224, views=2)
    fd = D.DeviceFeeder(host, "cuda", depth=2)
    got = []
    fd.set_epoch(0)
    for b in fd:                                                      # leave epoch 0 after its first batch
        got.append((tuple(t.clone() for t in b), fd.log[-1]))
        break
    for epoch in (1, 2):
        fd.set_epoch(epoch)
        for b in fd:
            got.append((tuple(t.clone() for t in b), fd.log[-1]))
    torch.cuda.synchronize()
    assert [(e["epoch"], len(e["index"])) for _, e in got] == [(0, 3), (1, 3), (1, 3), (1, 1), (2, 3), (2, 3), (2, 1)]
    assert fd.aug.last_fused
    for b, e in got:
        _check(b, e, ds)
    p0 = [p for _, e in got[1:4] for p in e["params"]]
    assert p0 == [p for b in range(3) for p in AU.sample_params(2 * len(got[1 + b][1]["index"]), 224,
                                                                  generator=D.batch_generator(17, 1, b, 0), **D.ROCO_AUG)]


def _run(args, timeout=900):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "mmvqa_amd.train"] + args, cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=timeout)


def test_cli_supcon_from_files(tmp_path, supcon_tree):
    r = _run(["supcon", "--data_dir", supcon_tree, "--lr", "1e-3", "--save_dir", str(tmp_path / "sc")] + MINI + DATA)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("Epoch ")]
    assert len(lines) == 2 and all("Train acc: " in x for x in lines), r.stdout
    assert len(_losses(r.stdout, r"Train loss: (\S+),")) == 2 and len(_losses(r.stdout, r"Train acc: (\S+) ,")) == 2
    assert len(_losses(r.stdout, r"Val loss: (\S+),")) == 2
    assert (tmp_path / "sc" / "MLM" / "run.pt").exists()
    short, _ = make_supcon_tree(str(tmp_path / "short"), short_row=1)
    r = _run(["supcon", "--data_dir", short, "--save_dir", str(tmp_path / "sc2")] + MINI + DATA)
    assert r.returncode != 0 and "Epoch " not in r.stdout
    assert os.path.join(short, "train", "radiology", "traindata.csv") + ": row 3 " in r.stderr, r.stderr[-3000:]
