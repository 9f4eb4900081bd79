"""Grad-CAM on the GPU: the data-only backward to the deepest feature map against autograd on the CPU oracle, the CAM
kernel against the fp64 restatement of the formula, batching, the promise that nothing else moves, refusals, the
resize / overlay stage through the op entry, one full-size pass and the sub-command.

Tolerance of every oracle comparison: max(1e-3, 5 x relerr(fp32 oracle, fp64 oracle)) against the fp64 oracle (the rule
of the parity tests, test_hip_amp_model.run_mixed_case)."""
import csv

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mmvqa_amd  # noqa: E402
from mmvqa_amd import _lib as L  # noqa: E402
from mmvqa_amd import gradcam as G  # noqa: E402
from mmvqa_amd import synth  # noqa: E402
from oracle import mmbert_oracle as O  # noqa: E402
from hip_helpers import dev, relerr  # noqa: E402
from test_hip_model import build_pair, mini_args  # noqa: E402

import gradcam_helpers as GH  # noqa: E402

C = 23
EFF = dict(cnn_encoder="tf_efficientnetv2_m", effnet_depth_div=8)
DROP = dict(hidden_dropout_prob=0.3, emb_dropout_prob=0.1, rf_dropout_prob=0.1)   # eval mode must switch these off
# (name, args, image size, seed, given targets?, re-head)
CASES = [
    ("resnet_transformer", dict(transformer_model="transformer", **DROP), 64, 51, True, False),
    ("resnet_realformer", dict(transformer_model="realformer"), 64, 12, False, False),
    ("effnet_transformer_relu", dict(transformer_model="transformer", use_relu=True, **EFF), 64, 73, False, False),
    ("effnet_realformer", dict(transformer_model="realformer", **EFF, **DROP), 64, 74, True, False),
    ("resnet_rehead", dict(transformer_model="transformer"), 64, 35, False, True),
]


def make_case(kw, hw, seed, rehead, B=3, T=10):
    args = mini_args(dataset="VQA-Med", vocab_size=C, **kw)
    orc, hip = build_pair(args, seed)
    n_cls = C
    if rehead:                                                     # vqamed2019/train.py:137
        torch.manual_seed(seed + 100)
        lin = torch.nn.Linear(args.hidden_size, 17)
        orc.classifier[2] = lin
        hip.classifier[2] = lin
        n_cls = 17
    img, ids, seg, mask, tgt = synth.vqa_batch(B, T, hw, vocab=args.emb_vocab, n_classes=n_cls, seed=seed)
    return orc, hip, (img, ids, seg, mask, tgt)


def check(name, got, r32, r64):
    tol = max(1e-3, 5 * relerr(r32, r64))
    e = relerr(got, r64)
    print(f"{name}: relerr {e:.3e} tol {tol:.3e}")
    assert e <= tol, f"{name}: {e:.2e} > {tol:.2e}"


@pytest.mark.parametrize("name,kw,hw,seed,given,rehead", CASES, ids=[c[0] for c in CASES])
def test_feature_gradient_and_cam_against_autograd(name, kw, hw, seed, given, rehead):
    orc, hip, (img, ids, seg, mask, tgt) = make_case(kw, hw, seed, rehead)
    target = tgt if given else None
    l32, A32, dA32, t32 = GH.oracle_feature_gradient(orc, img, ids, seg, mask, target)
    l64, A64, dA64, t64 = GH.oracle_feature_gradient(orc, img, ids, seg, mask, t32, double=True)
    # precondition on the oracle alone: positive evidence, and a maximum that normalisation does not turn into noise
    raw = GH.raw_cam(A64, dA64).flatten(1)
    assert bool((raw.max(1).values > 0).all()), raw.max(1).values
    assert bool((raw.max(1).values >= 1e-2 * raw.abs().max(1).values).all())
    hip.train()                                                    # the call must run in eval mode and put this back
    d = [t.to(dev()) for t in (img, ids, seg, mask)]
    res_t = None if target is None else target.to(dev())
    logits, A, dA, t = hip.feature_gradient(*d, target=res_t)
    assert hip.training
    assert torch.equal(t.cpu(), t32), "target (argmax) differs from the oracle's"
    assert A.shape == A64.shape and dA.shape == dA64.shape
    check("logits", logits, l32, l64)
    check("A", A, A32, A64)
    check("dA", dA, dA32, dA64)
    res = G.grad_cam(hip, *d, target=res_t)
    cam32, _ = GH.reference_cam(A32, dA32)
    cam64, v64 = GH.reference_cam(A64, dA64)
    check("cam", res.cam, cam32, cam64)
    assert res.valid.cpu().tolist() == [1] * 3 and res.overlay is None
    assert res.heatmap.shape == (3, hw, hw)


def test_batched_equals_single():
    orc, hip, (img, ids, seg, mask, tgt) = make_case(dict(transformer_model="realformer", **EFF), 64, 21, False, B=4)
    d = [t.to(dev()) for t in (img, ids, seg, mask, tgt)]

    def run(sl):
        _, _, dA, _ = hip.feature_gradient(*(t[sl] for t in d[:4]), target=d[4][sl])
        r = G.grad_cam(hip, *(t[sl] for t in d[:4]), target=d[4][sl])
        return dA.clone(), r.cam.clone()

    dA1, cam1 = run(slice(0, 4))
    dA2, cam2 = run(slice(0, 4))
    floor_dA, floor_cam = max(1e-5, 5 * relerr(dA1, dA2)), max(1e-5, 5 * relerr(cam1, cam2))
    for b in range(4):
        dAs, cams = run(slice(b, b + 1))
        e1, e2 = relerr(dAs[0], dA1[b]), relerr(cams[0], cam1[b])
        print(f"sample {b}: dA {e1:.2e} (floor {floor_dA:.1e}) cam {e2:.2e} (floor {floor_cam:.1e})")
        assert e1 <= floor_dA and e2 <= floor_cam, (b, e1, e2)


def test_nothing_else_moves():
    args = mini_args(dataset="VQA-Med", vocab_size=C, transformer_model="transformer")
    _, a = build_pair(args, seed=31)
    _, b = build_pair(args, seed=31)
    img, ids, seg, mask, tgt = (t.to(dev()) for t in synth.vqa_batch(4, 10, 64, vocab=50, n_classes=C, seed=32))

    def step(m):
        m.train()
        loss = mmvqa_amd.asl_loss(m(img, ids, seg, mask)[0], tgt)
        loss.backward()
        return loss.detach().clone()

    for m in (a, b):
        m.set_seed(7)
        step(m)
    assert float(a.flat_grads.abs().max()) > 0
    snap = [t.clone() for t in (a.flat_grads, a.flat_params, a._flat[1], a._flat[2])]
    res = G.grad_cam(a, img, ids, seg, mask, image_u8=G.image_u8_from_normalised(img))
    torch.cuda.synchronize()
    assert a.training and res.overlay.shape == (4, 64, 64, 3)
    for before, after in zip(snap, (a.flat_grads, a.flat_params, a._flat[1], a._flat[2])):
        assert torch.equal(before, after)
    # a following training step equals the twin's that never ran grad_cam (run-to-run rule of the fp32 repeat check)
    b._seed_ctr = a._seed_ctr = 99
    la, lb = step(a), step(b)
    assert relerr(la.reshape(1), lb.reshape(1)) < 1e-5, (float(la), float(lb))
    assert relerr(a.flat_grads, b.flat_grads) < 1e-4


def test_refusals():
    args = mini_args(dataset="VQA-Med", vocab_size=C)
    _, hip = build_pair(args, seed=41)
    img, ids, seg, mask, tgt = (t.to(dev()) for t in synth.vqa_batch(2, 10, 64, vocab=50, n_classes=C, seed=42))
    hip.train()
    out = hip(img, ids, seg, mask)[0]                              # a training-mode forward
    dA = torch.empty(2, 2, 2, 256, device=dev())
    g = torch.zeros(2, 24, device=dev())
    rc = L.lib().mmvqa_engine_backward_feature(hip._handle, L.stream_ptr(), L.ptr(g), 24, L.ptr(dA))
    assert rc == -3 and b"training" in L.lib().mmvqa_last_error()
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError, match="autocast"):
            with torch.autocast("cuda", dtype=dt):
                G.grad_cam(hip, img, ids, seg, mask)
    mmvqa_amd.asl_loss(out, tgt).backward()                        # the model still trains
    torch.cuda.synchronize()
    assert float(hip.flat_grads.abs().max()) > 0 and bool(torch.isfinite(hip.flat_grads).all())
    mlm = mmvqa_amd.Model(mini_args()).to(dev())
    with pytest.raises(NotImplementedError, match="VQA head"):
        mlm.feature_gradient(img, ids, seg, mask)


def test_no_positive_evidence_gives_zeros_and_the_plain_image():
    g = torch.Generator().manual_seed(5)
    A = torch.randn(2, 7, 7, 512, generator=g).abs().to(dev())
    dA = (-torch.randn(2, 7, 7, 512, generator=g).abs()).to(dev())
    image = torch.randint(0, 256, (2, 32, 32, 3), generator=g, dtype=torch.uint8).to(dev())
    cam, up, overlay, valid = G.cam_from_maps(A, dA, (32, 32), image)
    assert valid.cpu().tolist() == [0, 0]
    assert float(cam.abs().max()) == 0.0 and float(up.abs().max()) == 0.0
    assert torch.equal(overlay, image)                             # byte for byte


@pytest.mark.parametrize("H,W,Cc,IH,IW", [(7, 7, 512, 224, 224), (7, 7, 2048, 224, 224), (5, 9, 48, 50, 63)])
def test_resize_and_overlay(H, W, Cc, IH, IW):
    g = torch.Generator().manual_seed(H * W + Cc)
    A = torch.randn(3, H, W, Cc, generator=g).abs()
    dA = torch.randn(3, H, W, Cc, generator=g) + 0.05
    image = torch.randint(0, 256, (3, IH, IW, 3), generator=g, dtype=torch.uint8)
    cam64, v = GH.reference_cam(A, dA)
    assert bool(v.all())
    cam, up, overlay, valid = G.cam_from_maps(A.to(dev()), dA.to(dev()), (IH, IW), image.to(dev()))
    assert valid.cpu().tolist() == [1, 1, 1]
    assert relerr(cam, cam64) <= 1e-5
    e = relerr(up, GH.bilinear_resize(cam.cpu(), IH, IW))          # the kernel's own cam, resized in fp64
    print(f"up relerr {e:.2e}")
    assert e <= 1e-5
    want = GH.overlay_formula(up.cpu().numpy(), image.numpy(), G.jet_table(), 0.4)
    assert np.array_equal(overlay.cpu().numpy(), want)
    _, up2, none, _ = G.cam_from_maps(A.to(dev()), dA.to(dev()), (IH, IW))
    assert none is None and torch.equal(up2, up)


def test_full_size_config5():
    """tf_efficientnetv2_m at full depth + RealFormer + VQA head, 224 x 224, B = 2: shapes, finiteness, valid"""
    args = O.make_args(cnn_encoder="tf_efficientnetv2_m", transformer_model="realformer", heads=8, dataset="VQA-Med",
                       vocab_size=1552, emb_vocab=30522)
    torch.manual_seed(3)
    hip = mmvqa_amd.Model(args).to(dev()).eval()
    img, ids, seg, mask, _ = (t.to(dev()) for t in synth.vqa_batch(2, 28, 224, vocab=30522, n_classes=1552, seed=9))
    logits, A, dA, t = hip.feature_gradient(img, ids, seg, mask)
    assert A.shape == (2, 7, 7, 512) and dA.shape == (2, 7, 7, 512)
    assert torch.equal(t, logits.argmax(1))
    res = G.grad_cam(hip, img, ids, seg, mask, image_u8=G.image_u8_from_normalised(img))
    for x in (dA, res.cam, res.heatmap):
        assert bool(torch.isfinite(x).all())
    assert float(dA.abs().max()) > 0
    assert res.valid.cpu().tolist() == [1, 1] and res.overlay.shape == (2, 224, 224, 3)
    assert float(res.cam.flatten(1).max(1).values.min()) == 1.0


def test_gradcam_subcommand(tmp_path):
    from PIL import Image
    from mmvqa_amd import train
    mini = ["--resnet_layers", "1", "1", "1", "1", "--resnet_width", "8", "--hidden_size", "96", "--n_layers", "2",
            "--emb_vocab", "64", "--max_position_embeddings", "16", "--num_classes", "11", "--batch_size", "4"]
    out = tmp_path / "cam"
    index = train.main(["gradcam", "--test_samples", "10", "--limit", "6", "--target", "predicted", "--save_dir", str(out)] + mini)
    rows = list(csv.reader(open(out / "gradcam_index.csv")))
    assert rows[0] == ["image", "category", "question_index", "target", "predicted", "valid"]
    assert len(rows) == 7 and len(index) == 6
    _, table, _ = synth.vqa_test_table(10, 11, seed=1234)
    for i, r in enumerate(rows[1:]):
        assert r[0] == f"{table[i][3]}_synpic{10000 + i}.png" and r[1] == table[i][3] and int(r[2]) == i
        assert r[3] == r[4] and r[5] in ("0", "1")                 # --target predicted
        with Image.open(out / r[0]) as im:
            assert im.size == (224, 224) and im.mode == "RGB"
    assert len(list(out.glob("*.png"))) == 6
    index = train.main(["gradcam", "--test_samples", "4", "--save_dir", str(tmp_path / "ans")] + mini)
    _, table, _ = synth.vqa_test_table(4, 11, seed=1234)
    assert [r[3] for r in index] == [t[2] for t in table]          # --target answer (the default)
