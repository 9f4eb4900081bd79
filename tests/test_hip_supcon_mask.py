"""GPU tests of SupCon with a positive mask: mmvqa_supcon_loss_masked against the reference's fixture and the fp64
oracle restatement (tests/supcon_mask_helpers.py), its tie to the unmasked entry point, the labels path, the NaN rule;
mmvqa_jaccard_mask against the reference's matrix and numpy (bit-equal); the DeviceFeeder's (row, col) pairs; a whole
MLM + masked-SupCon step against the oracle model; `train supcon --supcon_mask jaccard` on a generated tree."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import mmvqa_amd  # noqa: E402
from mmvqa_amd import _lib as L  # noqa: E402
from mmvqa_amd import data as D  # noqa: E402
from mmvqa_amd import synth, train  # noqa: E402
from oracle import mmbert_oracle as O  # noqa: E402
from feeder_helpers import tokenizer  # noqa: E402
from hip_helpers import assert_close, dev, relerr  # noqa: E402
from supcon_helpers import make_supcon_tree  # noqa: E402
from supcon_mask_helpers import (fixture, fixture_texts, labels_mask, random_word_sets, soft_mask,  # noqa: E402
                                 supcon_masked)
from test_hip_feeder import DATA, MINI  # noqa: E402
from test_hip_model import build_pair, compare_grads, mini_args  # noqa: E402

TOL = 1e-4          # tests/test_hip_ops.py's bound for the unmasked kernel (rel-to-max); unnormalised features 2e-4


def hip_masked(f, m=None, labels=None):
    fd = f.detach().float().to(dev()).requires_grad_(True)
    kw = dict(mask=m.to(dev())) if m is not None else dict(labels=labels.to(dev()))
    l = mmvqa_amd.supcon_loss(fd, **kw)
    l.backward()
    return l.detach().cpu(), fd.grad.cpu()


def truth(f, m):
    f64 = f.detach().double().requires_grad_(True)
    l = supcon_masked(f64, m)
    l.backward()
    return l.detach(), f64.grad


@pytest.mark.parametrize("tag", ["a", "b"])
def test_masked_loss_equals_the_reference_fixture(tag):
    g = fixture()
    f = torch.from_numpy(g[f"{tag}_feat"])
    l, df = hip_masked(f, torch.from_numpy(g[f"{tag}_mask"]))
    ref = float(g[f"{tag}_loss_mask"])
    print(f"{tag} mask: loss {float(l):.7f} ref {ref:.7f} grad err {relerr(df, torch.from_numpy(g[f'{tag}_dfeat_mask'])):.2e}")
    assert abs(float(l) - ref) <= TOL * abs(ref)
    assert_close(df, torch.from_numpy(g[f"{tag}_dfeat_mask"]), TOL, "masked grad")
    l, df = hip_masked(f, labels=torch.from_numpy(g[f"{tag}_labels"]))
    ref = float(g[f"{tag}_loss_labels"])
    assert abs(float(l) - ref) <= TOL * abs(ref)
    assert_close(df, torch.from_numpy(g[f"{tag}_dfeat_labels"]), TOL, "labels grad")


@pytest.mark.parametrize("D_", [16, 128, 256])
@pytest.mark.parametrize("N", [1, 5, 16, 100, 128, 300])
def test_masked_loss_sizes(N, D_):
    """row-block and column-tile edges (N = 128: the gathered set of 8 GPUs x 16 pairs), against the fp64 oracle:
    an asymmetric soft mask with unit diagonal; a 0/1 mask in which some rows keep only their diagonal (the other view
    is their one positive); un-normalised features"""
    torch.manual_seed(40 + N + D_)
    f = F.normalize(torch.randn(N, 2, D_), dim=2)
    hard = (torch.rand(N, N) < 0.3).float()
    hard[::3] = 0.0
    hard.fill_diagonal_(1.0)
    for what, feats, m, tol in (("soft", f, soft_mask(N, 7 + N), TOL), ("hard", f, hard, TOL),
                                ("unnormalised", torch.randn(N, 2, D_) * 0.1, soft_mask(N, 9 + N), 2e-4)):
        lt, gt = truth(feats, m)
        l, df = hip_masked(feats, m)
        if N == 1:
            # one sample: the other view is the only contrast, so the loss and its gradient are identically zero and a
            # relative error has no denominator; what the kernel subtracts are scores, so measure against their size
            ff = torch.cat(torch.unbind(feats, 1)).double()
            zmax = float((ff @ ff.T).abs().max()) / 0.07
            print(f"N=1 D={D_} {what}: loss {float(l):.2e} grad max {float(df.abs().max()):.2e} (scores up to {zmax:.1f})")
            assert abs(float(lt)) < 1e-12 and float(gt.abs().max()) < 1e-12
            assert abs(float(l)) <= tol * zmax and float(df.abs().max()) <= tol * zmax
            continue
        lerr = abs(float(l) - float(lt)) / abs(float(lt))
        print(f"N={N} D={D_} {what}: loss rel err {lerr:.2e} grad rel-to-max {relerr(df, gt):.2e}")
        assert lerr <= tol, (what, float(l), float(lt))
        assert_close(df, gt, tol, f"masked grad {what} N={N} D={D_}")


@pytest.mark.parametrize("N,D_", [(5, 16), (64, 128), (128, 128), (300, 96)])
def test_identity_mask_ties_to_the_unmasked_entry_point(N, D_):
    """two kernels, each within TOL of the same truth: 2 x TOL apart at most (not bit-equal: summation orders differ)"""
    torch.manual_seed(3 + N)
    f = F.normalize(torch.randn(N, 2, D_), dim=2)
    l, df = hip_masked(f, torch.eye(N))
    fd = f.to(dev()).requires_grad_(True)
    lu = mmvqa_amd.supcon_loss(fd)
    lu.backward()
    lerr = abs(float(l) - float(lu)) / abs(float(lu))
    print(f"N={N} D={D_}: identity mask vs unmasked: loss {lerr:.2e} grad {relerr(df, fd.grad):.2e}")
    assert lerr <= 2 * TOL
    assert_close(df, fd.grad, 2 * TOL, "identity-mask grad vs unmasked")


def test_labels_path_is_the_mask_path_bit_equal():
    torch.manual_seed(2)
    f = F.normalize(torch.randn(37, 2, 128), dim=2)
    y = torch.randint(0, 5, (37,))
    l1, g1 = hip_masked(f, labels=y)
    l2, g2 = hip_masked(f, labels_mask(y))
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    l3, g3 = hip_masked(f, labels_mask(y).bool())              # any dtype: cast to fp32 as the reference does
    assert torch.equal(l1, l3) and torch.equal(g1, g3)


def test_zero_weight_row_gives_nan_as_the_reference():
    torch.manual_seed(4)
    f = F.normalize(torch.randn(6, 2, 16), dim=2)
    m = soft_mask(6, 1)
    m[2] = 0.0                                                  # also the diagonal: the tiled row has no positive left
    assert math.isnan(float(supcon_masked(f, m)))               # the restated reference divides 0 by 0
    l, _ = hip_masked(f, m)
    assert math.isnan(float(l))


def test_mask_gets_no_gradient_and_scales_upstream():
    torch.manual_seed(5)
    f = F.normalize(torch.randn(9, 2, 32), dim=2)
    m = soft_mask(9, 2).to(dev()).requires_grad_(True)
    fd = f.to(dev()).requires_grad_(True)
    (3.0 * mmvqa_amd.supcon_loss(fd, mask=m)).backward()
    assert m.grad is None
    _, g1 = hip_masked(f, m.detach().cpu())
    assert_close(fd.grad.cpu(), 3.0 * g1, 1e-6, "upstream scale")


# ----------------------------------------------------------------------------------------------- Jaccard mask
def _device_mask(ws, rows_a, cols_a, rows_b, cols_b):
    t = lambda v: torch.tensor(v, dtype=torch.int32, device=dev())   # noqa: E731
    m = mmvqa_amd.jaccard_mask(ws.to(dev()), t(rows_a), t(cols_a), t(rows_b), t(cols_b))
    torch.cuda.synchronize()
    return m.cpu().numpy()


def test_jaccard_mask_equals_the_reference_fixture_bit_equal():
    _caps, _augs, rows = fixture_texts()
    ref = fixture()["jaccard"]
    ws = D.WordSets.from_texts(rows)
    idx = list(range(6))
    for cols in ([1] * 6, [1, 2, 3, 1, 2, 3]):
        got = _device_mask(ws, idx, [0] * 6, idx, cols)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (cols, got, ref)


@pytest.mark.parametrize("n", [1, 16, 128])
def test_jaccard_mask_equals_numpy_on_generated_sets(n):
    """set sizes 0, 1, 63, 64, 65 (the wave width and its neighbours) and 700 (beyond the LDS-resident length: searched
    in global memory), a vocabulary small enough that every pair overlaps"""
    ws, _ = random_word_sets(40, [0, 1, 63, 64, 65, 700, 5, 31], 900, seed=n)
    g = np.random.default_rng(n)
    rows_a, rows_b = g.integers(0, 40, n).tolist(), g.integers(0, 40, n).tolist()
    cols_a, cols_b = g.integers(0, 4, n).tolist(), g.integers(0, 4, n).tolist()
    ref = ws.jaccard_host(rows_a, cols_a, rows_b, cols_b)
    got = _device_mask(ws, rows_a, cols_a, rows_b, cols_b)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    if n > 1:
        lens = {len(ws.word_ids(r, c)) for r, c in zip(rows_a, cols_a)}
        assert {0, 700} <= lens or n < 128
        assert ((ref > 0) & (ref < 1)).any()


def test_jaccard_mask_refusals_and_out_of_table_indices():
    ws, _ = random_word_sets(4, [3, 5], 10, seed=0)
    wd = ws.to(dev())
    t = lambda v, dt=torch.int32: torch.tensor(v, dtype=dt, device=dev())   # noqa: E731
    with pytest.raises(ValueError):
        mmvqa_amd.jaccard_mask(wd, t([0, 1]), t([0, 0]), t([0, 1]), t([1, 1], torch.int64))
    with pytest.raises(ValueError):
        mmvqa_amd.jaccard_mask(wd, t([0, 1]), t([0, 0]), t([0, 1]), t([1]))
    with pytest.raises(ValueError):
        mmvqa_amd.jaccard_mask(wd, t([0, 1]), t([0, 0]))
    with pytest.raises(mmvqa_amd.MMVQAError):
        mmvqa_amd.jaccard_mask(ws, t([0, 1]), t([0, 0]), t([0, 1]), t([1, 1]))
    lib, p = L.lib(), wd.offsets.data_ptr()
    assert lib.mmvqa_jaccard_mask(L.stream_ptr(), p, p, p, p, p, p, p, 0, 4) == -1
    assert lib.mmvqa_jaccard_mask(L.stream_ptr(), p, p, p, p, p, p, None, 2, 4) == -1
    # a (row, col) outside the table is never read: its entries are NaN, the rest of the matrix is right
    got = mmvqa_amd.jaccard_mask(wd, t([0, 4, 2]), t([0, 0, 0]), t([0, 1, 2]), t([1, 4, 2])).cpu().numpy()
    ref = ws.jaccard_host([0, 0, 2], [0, 0, 0], [0, 0, 2], [1, 1, 2])
    assert np.isnan(got[1]).all() and np.isnan(got[:, 1]).all()
    assert np.array_equal(got[[0, 2]][:, [0, 2]], ref[[0, 2]][:, [0, 2]])


# ----------------------------------------------------------------------------------------------- feeder, step, loop
@pytest.fixture(scope="module")
def supcon_tree(tmp_path_factory):
    return make_supcon_tree(str(tmp_path_factory.mktemp("supcon_mask")))[0]


def test_feeder_hands_out_the_pairs_only_when_asked(supcon_tree):
    table, tok, kw = D.roco_supcon_table(supcon_tree), tokenizer(), D.load_keywords(supcon_tree)
    ds = D.RocoSupConDataset(table, tok, kw, 5, 24, 0.3, seed=17, report_aug_col=True)
    host = D.HostLoader(ds, 3, shuffle=True, seed=17, num_workers=2, aug=D.ROCO_AUG, size=64, views=2)
    fd = D.DeviceFeeder(host, "cuda", depth=2, pairs=True)
    seen = 0
    for epoch in (0, 1):
        fd.set_epoch(epoch)
        for b in fd:
            assert len(b) == 6
            rows, cols = b[5]
            e = fd.log[-1]
            assert rows.dtype == torch.int32 and cols.dtype == torch.int32 and rows.is_cuda and cols.is_cuda
            assert rows.tolist() == e["index"] and cols.tolist() == e["aug_col"]
            assert cols.tolist() == [ds.encode_col(epoch, i)[1] for i in e["index"]]
            ref = torch.cat([torch.stack([ds.encode(epoch, i)[0] for i in e["index"]]),
                             torch.stack([ds.encode(epoch, i)[1] for i in e["index"]])])
            assert torch.equal(b[1].cpu(), ref)
            seen += 1
    assert seen == 6
    plain = D.RocoSupConDataset(table, tok, kw, 5, 24, 0.3, seed=17)
    fd = D.DeviceFeeder(D.HostLoader(plain, 3, shuffle=True, seed=17, num_workers=0, aug=D.ROCO_AUG, size=64, views=2),
                        "cuda")
    fd.set_epoch(0)
    assert all(len(b) == 5 for b in fd) and "aug_col" not in fd.log[-1]
    fd = D.DeviceFeeder(D.HostLoader(plain, 3, shuffle=True, seed=17, num_workers=0, aug=D.ROCO_AUG, size=64, views=2),
                        "cuda", pairs=True)
    with pytest.raises(ValueError, match="report_aug_col"):
        next(iter(fd))


def test_whole_step_mlm_plus_masked_supcon_against_the_oracle():
    """mini EfficientNetV2 + RealFormer with the SupCon head: MLM + masked SupCon, loss and every gradient against the
    oracle model + the masked restatement, under test_hip_model's parity rule (1e-3, fp64 truth where fp32 is noisy)"""
    import copy
    args = mini_args(cnn_encoder="tf_efficientnetv2_m", effnet_depth_div=8, transformer_model="realformer", supcon=True)
    orc, hip = build_pair(args)
    B, T, hw = 8, 12, 64
    img, ids, seg, mask, tgt = synth.roco_batch(B, T, hw, vocab=args.vocab_size, seed=5, mlm_prob=0.3)
    pos = soft_mask(B // 2, 21)
    orc64 = copy.deepcopy(orc).double().train()
    orc.train()

    def oracle_loss(out):
        return O.mlm_loss(out[0], tgt)[0] + supcon_masked(O.split_feat(out[1], B // 2), pos)

    loss_ref = oracle_loss(orc(img, ids, seg, mask))
    loss_ref.backward()
    oracle_loss(orc64(img.double(), ids, seg, mask)).backward()
    hip.train()
    d = lambda t: t.to(dev())   # noqa: E731
    logits, feat = hip(d(img), d(ids), d(seg), d(mask))
    loss = mmvqa_amd.mlm_loss(logits, d(tgt))[0] + mmvqa_amd.supcon_loss(mmvqa_amd.split_feat(feat, B // 2), mask=d(pos))
    print(f"whole step: loss {float(loss):.6f} oracle {float(loss_ref):.6f}")
    assert abs(float(loss) - float(loss_ref)) <= 1e-3 * abs(float(loss_ref))
    loss.backward()
    compare_grads(orc, hip, orc64)


def test_train_supcon_with_the_jaccard_mask(tmp_path, supcon_tree, monkeypatch, capsys):
    """a few steps of `train supcon --data_dir <tree> --supcon_mask jaccard`: runs, losses finite, and the first step's
    SupCon term is the oracle's value on that batch's features and the numpy Jaccard mask of its (row, column) pairs"""
    calls = []
    real_loss, real_mask = train.supcon_loss, train.jaccard_mask

    def spy_mask(words, rows_a, cols_a, rows_b, cols_b):
        m = real_mask(words, rows_a, cols_a, rows_b, cols_b)
        if not calls:
            calls.append(dict(rows=rows_a.tolist(), cols_a=cols_a.tolist(), cols=cols_b.tolist(), mask=m.clone()))
        return m

    def spy_loss(feat, **kw):
        l = real_loss(feat, **kw)
        if len(calls) == 1 and "feat" not in calls[0]:
            calls[0].update(feat=feat.detach().clone(), loss=l.detach().clone(), kw=sorted(kw))
        return l

    monkeypatch.setattr(train, "jaccard_mask", spy_mask)
    monkeypatch.setattr(train, "supcon_loss", spy_loss)
    best = train.main(["supcon", "--data_dir", supcon_tree, "--supcon_mask", "jaccard", "--lr", "1e-3", "--save_dir",
                       str(tmp_path / "sc")] + MINI + DATA + ["--num_workers", "0"])
    out = capsys.readouterr().out
    lines = [x for x in out.splitlines() if x.startswith("Epoch ")]
    assert len(lines) == 2 and math.isfinite(best), out
    assert all(math.isfinite(float(x.split("Train loss: ")[1].split(",")[0])) for x in lines)
    c = calls[0]
    assert c["kw"] == ["mask"] and c["cols_a"] == [0] * len(c["rows"]) and set(c["cols"]) <= {1, 2, 3}
    ws = D.WordSets.from_table(D.roco_supcon_table(supcon_tree))
    ref_mask = ws.jaccard_host(c["rows"], c["cols_a"], c["rows"], c["cols"])
    assert np.array_equal(c["mask"].cpu().numpy().view(np.uint32), ref_mask.view(np.uint32))
    assert ((ref_mask > 0) & (ref_mask < 1)).any()             # the tree's captions share words: a real soft mask
    ref = float(supcon_masked(c["feat"].cpu().double(), torch.from_numpy(ref_mask)))
    print(f"first step SupCon term {float(c['loss']):.6f} oracle {ref:.6f}")
    assert abs(float(c["loss"]) - ref) <= 1e-4 * abs(ref)
