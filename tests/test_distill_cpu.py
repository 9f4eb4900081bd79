"""CPU side of the distillation task: data.TeacherStates against the reference's own encode_text (fixtures of
tests/golden/make_golden_distill.py), the file format and its refusals, the host refusals of mmvqa_distill_mse, the
option rules of `train distill`, and the headless Model on the CPU."""
import numpy as np
import pytest
import torch

import mmvqa_amd
from mmvqa_amd import data as D
from mmvqa_amd import synth, train
from oracle import mmbert_oracle as O
from distill_helpers import dense_target, load, write_teacher_file

N_CAP = 6


def fixture_teacher(g):
    ids = [g[f"ids{c}"] for c in range(N_CAP)]
    states = [g[f"states{c}"] for c in range(N_CAP)]
    offs = np.concatenate([[0], np.cumsum([len(i) for i in ids])])
    return D.TeacherStates.from_arrays(offs, np.concatenate(ids), np.concatenate(states), int(g["cls_id"]), int(g["sep_id"]))


def test_batch_and_target_equal_the_reference_encode_text(golden_dir):
    """tokens, segment ids, mask (integers equal) and the dense target (bit-equal) of the reference's
    encode_text(..., task='distillation') for captions of 0, 1, exactly T - 8 and more pieces, T in {12, 32}"""
    g = load(golden_dir, "distill_text")
    ts = fixture_teacher(g)
    assert [len(g[f"ids{c}"]) for c in range(N_CAP)] == [0, 1, 4, 5, 24, 26]
    rows = list(range(N_CAP))
    for T in (int(t) for t in g["Ts"]):
        ids, seg, mask, start, count = ts.batch(rows, T, 5)
        assert ids.dtype == seg.dtype == mask.dtype == start.dtype == torch.int64 and count.dtype == torch.int32
        tgt = ts.target_host(rows, T, 5)
        assert tgt.dtype == torch.float64 and tuple(tgt.shape) == (N_CAP, T, 768)
        for c in rows:
            assert torch.equal(ids[c], torch.from_numpy(g[f"tokens{c}_{T}"])), (c, T)
            assert torch.equal(seg[c], torch.from_numpy(g[f"seg{c}_{T}"])), (c, T)
            assert torch.equal(mask[c], torch.from_numpy(g[f"mask{c}_{T}"])), (c, T)
            assert torch.equal(tgt[c].float(), torch.from_numpy(g[f"labels{c}_{T}"])), (c, T)
            assert int(count[c]) == len(g[f"ids{c}"]) and int(start[c]) == int(ts.offsets[c])
        # (start, count) name the same target through the independent gather the GPU tests compare the kernel with
        assert torch.equal(dense_target(ts.states, start, count, T, 7).double(), tgt)


def table_rows(names):
    return [("/somewhere/images/" + n, "caption") for n in names]


def parts(seed=3, n=5, Dm=8, dtype=np.float32):
    rng = np.random.default_rng(seed)
    lens = [0, 1, 3, 7, 2][:n]
    names = [f"img{k}.jpg" for k in range(n)]
    ids = [rng.integers(5, 90, size=m) for m in lens]
    states = [rng.standard_normal((m, Dm)).astype(dtype) for m in lens]
    return names, ids, states


@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64])
def test_file_round_trip_shuffled_superset(tmp_path, dtype):
    names, ids, states = parts(dtype=dtype)
    extra = [("other.jpg", np.array([7, 8], dtype=np.int64), np.ones((2, 8), dtype=dtype)),
             ("bad.jpg", np.array([9], dtype=np.int64), np.full((1, 8), np.nan, dtype=dtype))]   # not kept: may be non-finite
    path = write_teacher_file(str(tmp_path / "t.npz"), names, ids, states, order=[6, 3, 0, 5, 4, 1, 2], extra=extra,
                              dtype=dtype, cls_id=2, sep_id=3)
    keep = [4, 0, 3, 1]                                             # the table's own order, a subset
    ts = D.TeacherStates.from_file(path, table_rows([names[k] for k in keep]))
    assert ts.rows == 4 and ts.dim == 8 and (ts.cls_id, ts.sep_id) == (2, 3)
    assert ts.states.dtype == (torch.float16 if dtype == np.float16 else torch.float32)
    for r, k in enumerate(keep):
        lo, hi = int(ts.offsets[r]), int(ts.offsets[r + 1])
        assert np.array_equal(ts.ids[lo:hi], ids[k])
        want = torch.from_numpy(states[k]).to(ts.states.dtype)
        assert torch.equal(ts.states[lo:hi], want)
    i, s, m, start, count = ts.batch([0, 2], 12, 5)
    assert i[1].tolist() == [2, 0, 0, 0, 0, 0, 3] + ids[3][:4].tolist() + [3]      # 7 pieces cut to T - 8 = 4
    assert count.tolist() == [2, 7] and s[1].tolist() == [0] * 7 + [1] * 5 and m[0].tolist() == [1] * 10 + [0, 0]
    # defaults of the optional scalars
    p2 = write_teacher_file(str(tmp_path / "d.npz"), names, ids, states, dtype=dtype)
    d = D.TeacherStates.from_file(p2, table_rows(names))
    assert (d.cls_id, d.sep_id) == (101, 102)
    with pytest.raises(ValueError, match="outside the embedding table"):
        d.check_vocab(50)
    d.check_vocab(103)


def test_file_refusals(tmp_path):
    names, ids, states = parts()
    rows = table_rows(names)
    good = dict(np.load(write_teacher_file(str(tmp_path / "g.npz"), names, ids, states)))

    def refused(match, table=rows, **change):
        z = {**good, **change}
        z = {k: v for k, v in z.items() if v is not None}
        p = str(tmp_path / "bad.npz")
        np.savez(p, **z)
        with pytest.raises(ValueError, match=match):
            D.TeacherStates.from_file(p, table)

    D.TeacherStates.from_file(str(tmp_path / "g.npz"), rows)
    refused("no teacher states for 1 of the table's 6 rows: missing.jpg", table=rows + table_rows(["missing.jpg"]))
    refused("appears more than once", names=np.array(["img0.jpg"] * 5))
    off = good["offsets"].copy(); off[3] = 0                       # noqa: E702  (decreases)
    refused("never decrease", offsets=off)
    off = good["offsets"].copy(); off[0] = 1                       # noqa: E702
    refused("start at 0", offsets=off)
    refused("all three must agree", ids=good["ids"][:-1])
    refused("all three must agree", states=good["states"][:-1])
    refused("one-dimensional", ids=good["ids"].reshape(1, -1))
    refused("states \\[total, D\\]", states=good["states"].reshape(-1))
    refused("one-dimensional unicode", names=good["names"].reshape(1, -1))
    refused("float16, float32 or float64", states=good["states"].astype(np.int32))
    refused("integer arrays", ids=good["ids"].astype(np.float32))
    refused("offsets for 5 names", offsets=good["offsets"][:-1])
    refused("no array 'ids'", ids=None)
    st = good["states"].copy(); st[-1, 0] = np.inf                 # noqa: E702  (a kept caption)
    refused("non-finite", states=st)
    with pytest.raises(ValueError):                                 # pickled objects are not read
        p = str(tmp_path / "obj.npz")
        np.savez(p, **{**good, "names": np.array(names, dtype=object)})
        D.TeacherStates.from_file(p, rows)
    with pytest.raises(ValueError, match="non-finite"):
        D.TeacherStates.from_arrays([0, 1], [5], np.array([[np.nan]], dtype=np.float32))
    with pytest.raises(ValueError, match="no room"):
        D.TeacherStates.from_arrays([0, 1], [5], np.ones((1, 4), dtype=np.float32)).batch([0], 7, 5)
    with pytest.raises(ValueError, match="3 table rows"):
        D.DistillDataset(rows[:3], D.TeacherStates.from_file(str(tmp_path / "g.npz"), rows))


def test_synthetic_batch_layout():
    (img, ids, seg, mask, start, count), table = synth.distill_batch(4, 12, 16, vocab=64, D=8, seed=5)
    assert tuple(img.shape) == (4, 3, 16, 16) and table.dtype == torch.float32 and table.shape[1] == 8
    assert start.dtype == torch.int64 and count.dtype == torch.int32
    lens = count.tolist()
    assert lens[0] == 0 and lens[1] == 12 - 8 + 1                   # an empty caption and one that is cut
    assert start.tolist() == [sum(lens[:b]) for b in range(4)] and table.shape[0] == sum(lens)
    ts = D.TeacherStates.from_arrays(np.concatenate([[0], np.cumsum(lens)]), np.ones(sum(lens), dtype=np.int64), table.numpy())
    _i, s2, m2, st2, ct2 = ts.batch(range(4), 12, 5)
    assert torch.equal(seg, s2) and torch.equal(mask, m2) and torch.equal(start, st2) and torch.equal(count, ct2)
    for b, n in enumerate(min(v, 4) for v in lens):
        assert ids[b, 0] == 101 % 64 and ids[b, 6] == 102 % 64 and ids[b, 7 + n] == 102 % 64 and (ids[b, 8 + n:] == 0).all()


def test_distill_mse_refuses_bad_arguments_on_the_host():
    """every case returns MMVQA_ERR_ARG and names the function before any HIP call"""
    from mmvqa_amd import _lib as L
    lib = L.lib()
    p = 0x1000                                                     # never dereferenced: every case below is refused first
    good = dict(h=p, ld=8, table=p, f16=0, table_rows=4, start=p, count=p, first=2, B=1, T=4, H=8, row_sq=p, loss=p, dh=p,
                dld=8)
    cases = [({k: None}, b"null operand") for k in ("h", "table", "start", "count", "row_sq", "loss")]
    cases += [({k: 0}, b">= 1") for k in ("B", "T", "H", "table_rows")]
    cases += [({"first": -1}, b"first=-1"), ({"first": 4}, b"first=4"), ({"ld": 7}, b"ld=7 < H=8"), ({"dld": 7}, b"dld=7 < H=8")]
    for change, what in cases:
        a = {**good, **change}
        rc = lib.mmvqa_distill_mse(None, a["h"], a["ld"], a["table"], a["f16"], a["table_rows"], a["start"], a["count"],
                                   a["first"], a["B"], a["T"], a["H"], a["row_sq"], a["loss"], a["dh"], a["dld"], 1.0)
        err = lib.mmvqa_last_error()
        assert rc == -1 and err.startswith(b"mmvqa_distill_mse: ") and what in err, (change, rc, err)


def test_distill_loss_checks_its_arguments():
    h = torch.zeros(2, 12, 8)
    with pytest.raises(mmvqa_amd.MMVQAError, match="GPU tensors only"):
        mmvqa_amd.distill_loss(h, torch.zeros(4, 8), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32))


def test_train_distill_option_rules(capsys):
    mode, a = train.parse_args(["distill", "--run_name", "r"])
    assert mode == "distill" and a.lr == 2e-5 and a.max_position_embeddings == 75 and not hasattr(a, "mlm_prob")
    mode, a = train.parse_args(["distill", "--data_dir", "d", "--teacher_states", "a.npz", "--val_teacher_states", "b.npz"])
    assert (a.teacher_states, a.val_teacher_states) == ("a.npz", "b.npz")
    for argv, what in ((["distill", "--data_dir", "d"], "needs --teacher_states"),
                       (["distill", "--data_dir", "d", "--teacher_states", "a.npz"], "needs --teacher_states"),
                       (["distill", "--teacher_states", "a.npz"], "with --data_dir only"),
                       (["distill", "--val_teacher_states", "a.npz"], "with --data_dir only"),
                       (["distill", "--mixed_precision", "--overlap_adam"], "--overlap_adam cannot be combined"),
                       (["mlm", "--teacher_states", "a.npz"], "unrecognized arguments")):
        with pytest.raises(SystemExit):
            train.parse_args(argv)
        assert what in capsys.readouterr().err, argv


def test_headless_model_on_cpu(tmp_path):
    kw = dict(resnet_layers=(1, 1, 1, 1), resnet_width=8, hidden_size=96, n_layers=2, heads=12, vocab_size=50, emb_vocab=50,
              bert_max_pos=32)
    for tm in ("transformer", "realformer"):
        torch.manual_seed(0)
        m = mmvqa_amd.Model(O.make_args(task="distillation", transformer_model=tm, supcon=True, **kw))
        assert m._desc.head_kind == 2 and m._desc.supcon == 0       # models/mmbert.py:159-161 returns h alone
        mlm = mmvqa_amd.Model(O.make_args(transformer_model=tm, **kw))
        sd, msd = m.state_dict(), mlm.state_dict()
        assert list(sd) == list(msd) and all(sd[k].shape == msd[k].shape for k in sd)
        assert "fc1.weight" in sd and "classifier.2.weight" in sd
    # a distilled checkpoint starts a VQA model (vqamed2019/train.py:125-135)
    path = str(tmp_path / "distilled.pt")
    torch.save(m.state_dict(), path)
    vqa = mmvqa_amd.Model(O.make_args(dataset="VQA-Med", transformer_model="realformer", **kw))
    loaded, _skipped, untouched = mmvqa_amd.checkpoint.load_roco_pretrained(vqa, path)
    assert not untouched and "transformer.mains.0.kqv.weight" in loaded
    assert all(torch.equal(vqa.state_dict()[k], v) for k, v in m.state_dict().items())
    with pytest.raises(NotImplementedError, match="task='pretext'"):
        mmvqa_amd.Model(O.make_args(task="pretext", **kw))
    with pytest.raises(mmvqa_amd.MMVQAError):                        # no CPU fallback for the headless model either
        m(torch.zeros(1, 3, 32, 32), torch.zeros(1, 12, dtype=torch.long), torch.zeros(1, 12, dtype=torch.long),
          torch.ones(1, 12, dtype=torch.long))
