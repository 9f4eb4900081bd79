"""GPU tests of the SupCon mask from caption sentence embeddings: mmvqa_normalize_rows + mmvqa_cosine_mask against the
reference's fixture (SimilarityCalculator.bert_embedd) and the fp64 host matrix within the derived bound
(2 D + 8) 2^-24, bit-exact diagonal and repeatability, a float16-sourced table, refusals and out-of-table indices; a
whole MLM + masked-SupCon step against the oracle model; `train supcon --supcon_mask embeddings` on a generated tree."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mmvqa_amd  # noqa: E402
from mmvqa_amd import _lib as L  # noqa: E402
from mmvqa_amd import data as D  # noqa: E402
from mmvqa_amd import synth, train  # noqa: E402
from oracle import mmbert_oracle as O  # noqa: E402
from hip_helpers import dev  # noqa: E402
from supcon_embed_helpers import FIXTURE_DIMS, FIXTURE_DRAWS, bound, fixture, positive_table, signed_table  # noqa: E402
from supcon_helpers import make_supcon_tree  # noqa: E402
from supcon_mask_helpers import supcon_masked  # noqa: E402
from test_hip_feeder import DATA, MINI  # noqa: E402
from test_hip_model import build_pair, compare_grads, mini_args  # noqa: E402


def t32(v, dt=torch.int32):
    return torch.tensor(v, dtype=dt, device=dev())


def device_mask(ce, rows_a, cols_a, rows_b, cols_b):
    m = mmvqa_amd.embedding_mask(ce, t32(rows_a), t32(cols_a), t32(rows_b), t32(cols_b))
    torch.cuda.synchronize()
    return m.cpu().numpy()


@pytest.mark.parametrize("Dm", FIXTURE_DIMS)
def test_embedding_mask_equals_the_reference_fixture(Dm):
    """two fp32 computations (the reference's and the kernel's) of the same cosine: 2 x bound apart at most; the whole
    batch of the fixture and its leading 5 x 5 and 1 x 1 batches"""
    g = fixture()
    host = D.CaptionEmbeddings.from_array(g[f"emb_{Dm}"])
    ce = host.to(dev())
    assert ce.normalised and ce.table.is_cuda and ce.table.dtype == torch.float32 and not host.normalised
    worst = 0.0
    for k in range(FIXTURE_DRAWS):
        cols, ref = g[f"cols_{Dm}_{k}"].tolist(), g[f"ref_{Dm}_{k}"]
        for n in (6, 5, 1):
            idx = list(range(n))
            got = device_mask(ce, idx, [0] * n, idx, cols[:n])
            assert got.dtype == np.float32 and (np.diag(got) == 1.0).all()
            worst = max(worst, float(np.abs(got.astype(np.float64) - ref[:n, :n]).max()))
            if n > 2:
                assert (np.delete(got[2], 2) == 0.0).all()                # the all-zero caption: zeros, no NaN
    print(f"D={Dm}: device mask vs the reference's matrix {worst:.2e} (2 x bound {2 * bound(Dm):.2e})")
    assert worst <= 2 * bound(Dm)


@pytest.fixture(scope="module")
def tables():
    """D -> (host embeddings, the same on the device): 12 texts rows, signed, built once for the size grid"""
    out = {}
    for Dm in (5, 64, 384, 1000):
        host = D.CaptionEmbeddings.from_array(signed_table(12, Dm, seed=Dm))
        out[Dm] = (host, host.to(dev()))
    return out


@pytest.mark.parametrize("Dm", [5, 64, 384, 1000])
@pytest.mark.parametrize("n", [1, 5, 37])
def test_embedding_mask_equals_the_host_matrix(tables, n, Dm):
    """scalar loads (D = 5) and 16-byte loads, D below / not a multiple of / above the wave's stride, more columns than
    waves (n = 5, 37), one column (n = 1); any column on the anchor's side, repeated (row, column) pairs"""
    host, ce = tables[Dm]
    g = np.random.default_rng(100 * n + Dm)
    rows_a, rows_b = g.integers(0, 12, n), g.integers(0, 12, n)
    cols_a, cols_b = g.integers(0, 4, n), g.integers(0, 4, n)
    if n >= 5:
        rows_a[:5], cols_a[:5] = [1, 9, 3, 7, 7], [0, 2, 0, 1, 3]
        rows_b[:5], cols_b[:5] = [2, 5, 8, 2, 7], [1, 2, 3, 1, 1]
    else:
        rows_a[0], cols_a[0], rows_b[0], cols_b[0] = 1, 2, 6, 3                  # different texts on the diagonal
    ref = host.cosine_host(rows_a, cols_a, rows_b, cols_b)
    got = device_mask(ce, rows_a.tolist(), cols_a.tolist(), rows_b.tolist(), cols_b.tolist())
    again = device_mask(ce, rows_a.tolist(), cols_a.tolist(), rows_b.tolist(), cols_b.tolist())
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"n={n} D={Dm}: device mask vs fp64 host {err:.2e} (bound {bound(Dm):.2e})")
    assert got.shape == (n, n) and err <= bound(Dm)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))          # same inputs, same bits
    assert np.array_equal(np.diag(got).view(np.uint32), np.ones(n, np.float32).view(np.uint32))
    if n >= 5:
        assert abs(got[0, 1] - 1.0) <= bound(Dm)          # text (5, 2) is a positive multiple of caption 1
        assert abs(got[3, 4] - 1.0) <= bound(Dm)          # the same text (7, 1) on both sides, off the diagonal
        assert (np.delete(got[2], 2) == 0.0).all()        # caption 3 is all zero
        assert (rows_a[4], cols_a[4]) != (rows_b[4], cols_b[4])   # ... and the diagonal is 1 where the two texts differ
        off = ~np.eye(n, dtype=bool)
        assert (got[off] < 0).any() and (got[off] > 0).any()
    if n == 37:
        pairs = list(zip(rows_b.tolist(), cols_b.tolist()))
        assert len(set(pairs)) < n                         # repeated (row, column) pairs


def test_normalize_rows_on_the_device():
    """x / max(|x|, eps) in place: unit rows, a zero row stays zero, a row shorter than eps is divided by eps"""
    torch.manual_seed(0)
    for rows, Dm in ((1, 1), (7, 5), (9, 64), (5, 1000), (3, 4096)):
        x = torch.randn(rows, Dm, dtype=torch.float64) * torch.rand(rows, 1, dtype=torch.float64) * 3
        if rows > 2:
            x[1] = 0.0
            x[2] = 1e-12
        xd = x.float().to(dev())
        L.check(L.lib().mmvqa_normalize_rows(L.stream_ptr(), L.ptr(xd), rows, Dm, 1e-8))
        x32 = x.float().double()
        ref = x32 / x32.norm(dim=1, keepdim=True).clamp_min(1e-8)
        err = float((xd.cpu().double() - ref).abs().max())
        print(f"normalize_rows {rows} x {Dm}: {err:.2e}")
        assert err <= (Dm / 2 + 4) * 2.0 ** -24             # the norm (sum of D squares, a root) and one division
        if rows > 2:
            assert not xd[1].any()


def test_float16_sourced_table_gives_the_mask_of_its_cast_bit_equal():
    e16 = signed_table(12, 64, seed=5, dtype=np.float16)
    a = D.CaptionEmbeddings.from_array(e16).to(dev())
    b = D.CaptionEmbeddings.from_array(e16.astype(np.float32)).to(dev())
    assert torch.equal(a.table, b.table)
    g = np.random.default_rng(5)
    rows, cols = g.integers(0, 12, 9).tolist(), g.integers(1, 4, 9).tolist()
    ma, mb = device_mask(a, rows, [0] * 9, rows, cols), device_mask(b, rows, [0] * 9, rows, cols)
    assert np.array_equal(ma.view(np.uint32), mb.view(np.uint32))
    ref = D.CaptionEmbeddings.from_array(e16).cosine_host(rows, [0] * 9, rows, cols)
    assert float(np.abs(ma - ref).max()) <= bound(64)


@pytest.mark.parametrize("Dm", [6, 8])                     # the scalar and the 16-byte kernel
def test_embedding_mask_refusals_and_out_of_table_indices(Dm):
    host = D.CaptionEmbeddings.from_array(signed_table(8, Dm, seed=0)[:4])
    ce = host.to(dev())
    with pytest.raises(ValueError):
        mmvqa_amd.embedding_mask(ce, t32([0, 1]), t32([0, 0]), t32([0, 1]), t32([1, 1], torch.int64))
    with pytest.raises(ValueError):
        mmvqa_amd.embedding_mask(ce, t32([0, 1]), t32([0, 0]), t32([0, 1]), t32([1]))
    with pytest.raises(ValueError):
        mmvqa_amd.embedding_mask(ce, t32([0, 1]), t32([0, 0]))
    with pytest.raises(ValueError):
        mmvqa_amd.embedding_mask(ce, t32([0, 1]), t32([0, 0]), torch.tensor([0, 1], dtype=torch.int32), t32([1, 1]))
    with pytest.raises(mmvqa_amd.MMVQAError):              # a table left on the host
        mmvqa_amd.embedding_mask(host, t32([0, 1]), t32([0, 0]), t32([0, 1]), t32([1, 1]))
    lib, p = L.lib(), ce.table.data_ptr()
    assert lib.mmvqa_cosine_mask(L.stream_ptr(), p, p, p, p, p, p, 0, Dm, 4) == -1
    assert lib.mmvqa_cosine_mask(L.stream_ptr(), p, p, p, p, p, None, 2, Dm, 4) == -1
    assert lib.mmvqa_cosine_mask(L.stream_ptr(), p, p, p, p, p, p, 2, 4097, 4) == -1
    # a (row, col) outside the table is never read: its entries are NaN, the rest of the matrix is right
    for rows_a, cols_b in (([0, 4, 2], [1, 4, 2]), ([0, -1, 2], [1, -1, 2])):
        got = device_mask(ce, rows_a, [0, 0, 0], [0, 1, 2], cols_b)
        ref = host.cosine_host([0, 0, 2], [0, 0, 0], [0, 0, 2], [1, 1, 2])
        assert np.isnan(got[1]).all() and np.isnan(got[:, 1]).all()
        keep = got[[0, 2]][:, [0, 2]]
        assert np.isfinite(keep).all() and float(np.abs(keep - ref[[0, 2]][:, [0, 2]]).max()) <= bound(Dm)


def test_whole_step_mlm_plus_embedding_masked_supcon_against_the_oracle():
    """mini EfficientNetV2 + RealFormer with the SupCon head: MLM + SupCon under the mask embedding_mask builds from a
    12-row table of non-negative embeddings, loss and every gradient against the oracle model + the masked
    restatement evaluated on the device's mask (the mask has its own tests above: no tolerances stack), under
    test_hip_model's parity rule"""
    import copy
    args = mini_args(cnn_encoder="tf_efficientnetv2_m", effnet_depth_div=8, transformer_model="realformer", supcon=True)
    orc, hip = build_pair(args)
    B, T, hw = 8, 12, 64
    img, ids, seg, mask, tgt = synth.roco_batch(B, T, hw, vocab=args.vocab_size, seed=5, mlm_prob=0.3)
    host = D.CaptionEmbeddings.from_array(positive_table(12, 32, seed=21))
    rows, cols = t32([3, 7, 0, 10]), t32([2, 1, 3, 1])
    pos_dev = mmvqa_amd.embedding_mask(host.to(dev()), rows, torch.zeros_like(cols), rows, cols)
    pos = pos_dev.cpu()
    ref_pos = host.cosine_host(rows.tolist(), [0] * 4, rows.tolist(), cols.tolist())
    off = ~np.eye(4, dtype=bool)
    assert float(np.abs(pos.numpy() - ref_pos).max()) <= bound(32)
    assert 0.3 < ref_pos[off].min() and ref_pos[off].max() < 0.99             # soft, and far from a zero row sum
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
    loss = mmvqa_amd.mlm_loss(logits, d(tgt))[0] + mmvqa_amd.supcon_loss(mmvqa_amd.split_feat(feat, B // 2), mask=pos_dev)
    lv, lr = float(loss.detach()), float(loss_ref.detach())
    print(f"whole step: loss {lv:.6f} oracle {lr:.6f}")
    assert abs(lv - lr) <= 1e-3 * abs(lr)
    loss.backward()
    compare_grads(orc, hip, orc64)


def test_train_supcon_with_the_embeddings_mask(tmp_path, monkeypatch, capsys):
    """two epochs of `train supcon --data_dir <tree> --supcon_mask embeddings --caption_embeddings f.npz`: runs, losses
    finite, the first step's mask is the host matrix of its (row, column) pairs within the bound, and its SupCon term
    is the oracle's value on that batch's features and that mask"""
    tree, kept = make_supcon_tree(str(tmp_path / "tree"))
    names = [k[0] for k in kept] + ["PMC_extra_one.jpg", "PMC_extra_two.jpg"]
    emb = positive_table(len(names), 32, seed=9)
    order = np.random.default_rng(9).permutation(len(names))
    path = str(tmp_path / "emb.npz")
    np.savez(path, names=np.array(names)[order], emb=emb[order].astype(np.float16))
    calls = []
    real_loss, real_mask = train.supcon_loss, train.embedding_mask

    def spy_mask(words, rows_a, cols_a, rows_b, cols_b):
        m = real_mask(words, rows_a, cols_a, rows_b, cols_b)
        if not calls:
            calls.append(dict(rows=rows_a.tolist(), cols_a=cols_a.tolist(), cols=cols_b.tolist(), mask=m.clone(),
                              same_rows=rows_a is rows_b, kind=type(words).__name__))
        return m

    def spy_loss(feat, **kw):
        l = real_loss(feat, **kw)
        if len(calls) == 1 and "feat" not in calls[0]:
            calls[0].update(feat=feat.detach().clone(), loss=l.detach().clone(), kw=sorted(kw))
        return l

    def no_jaccard(*_a, **_k):
        raise AssertionError("--supcon_mask embeddings must not build the Jaccard mask")

    monkeypatch.setattr(train, "embedding_mask", spy_mask)
    monkeypatch.setattr(train, "jaccard_mask", no_jaccard)
    monkeypatch.setattr(train, "supcon_loss", spy_loss)
    best = train.main(["supcon", "--data_dir", tree, "--supcon_mask", "embeddings", "--caption_embeddings", path, "--lr",
                       "1e-3", "--save_dir", str(tmp_path / "sc")] + MINI + DATA + ["--num_workers", "0"])
    out = capsys.readouterr().out
    lines = [x for x in out.splitlines() if x.startswith("Epoch ")]
    assert len(lines) == 2 and math.isfinite(best), out
    assert all(math.isfinite(float(x.split("Train loss: ")[1].split(",")[0])) for x in lines)
    c = calls[0]
    assert c["kind"] == "CaptionEmbeddings" and c["kw"] == ["mask"] and c["same_rows"]
    assert c["cols_a"] == [0] * len(c["rows"]) and set(c["cols"]) <= {1, 2, 3}
    host = D.CaptionEmbeddings.from_file(path, D.roco_supcon_table(tree))
    assert host.rows == len(kept) and np.array_equal(host.table.numpy(), emb[:len(kept)].astype(np.float16).astype(np.float32))
    ref_mask = host.cosine_host(c["rows"], c["cols_a"], c["rows"], c["cols"])
    got = c["mask"].cpu().numpy()
    err = float(np.abs(got - ref_mask).max())
    print(f"first step: mask vs fp64 host {err:.2e} (bound {bound(32):.2e})")
    assert err <= bound(32)
    assert ((ref_mask > 0) & (ref_mask < 1)).any()                              # a real soft mask
    ref = float(supcon_masked(c["feat"].cpu().double(), c["mask"].cpu()))
    print(f"first step SupCon term {float(c['loss']):.6f} oracle {ref:.6f}")
    assert abs(float(c["loss"]) - ref) <= 1e-4 * abs(ref)
