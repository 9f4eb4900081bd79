"""teacher.BertTeacher on the GPU against HF's BertModel (fixture tests/golden/teacher.npz, made by
make_golden_teacher.py) and against the float64 plain-torch restatement of tests/teacher_helpers.py.

Bound: 4 x the distance between the fp32 CPU result and the float64 one (e0 of the fixture; measured here for the
full-width model), over ALL rows, padded ones included."""
import pytest
import torch

import teacher_helpers as TH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden_dir):
    return TH.load(golden_dir)


@pytest.fixture(scope="module")
def small(fx):
    from mmvqa_amd.teacher import BertTeacher
    return BertTeacher.from_state_dict(TH.fixture_state_dict(fx), eps=float(fx["eps"])).to("cuda:0")


def test_fixture_hidden_states(fx, small):
    dev = torch.device("cuda:0")
    ids, lens = torch.from_numpy(fx["a_ids"]).to(dev), torch.from_numpy(fx["a_lens"]).to(dev)
    out = small(ids, lens)
    assert out.shape == (3, 37, 128) and out.dtype == torch.float32
    e0 = float(fx["e0"])
    err = float((out.cpu().double() - torch.from_numpy(fx["a_f64"])).abs().max())
    print(f"fixture (a): |err| {err:.3e}, e0 {e0:.3e}, ratio {err / e0:.2f}")
    assert err <= 4.0 * e0
    assert torch.equal(small(ids, lens), out)                       # bit-equal from call to call


def test_valid_rows_do_not_depend_on_the_padding(fx, small):
    """T grows from max(len) to max(len) + 5: the valid rows stay within the same bound of the same float64 values"""
    dev = torch.device("cuda:0")
    ids = torch.from_numpy(fx["a_ids"])
    lens = torch.from_numpy(fx["a_lens"])
    wide = torch.zeros(3, 42, dtype=torch.int64)
    wide[:, :37] = ids
    out = small(wide.to(dev), lens.to(dev)).cpu().double()
    ref = torch.from_numpy(fx["a_f64"])
    e0 = float(fx["e0"])
    for b, n in enumerate(lens.tolist()):
        err = float((out[b, :n] - ref[b, :n]).abs().max())
        print(f"sample {b} (len {n}) at T = 42: |err| {err:.3e}, ratio {err / e0:.2f}")
        assert err <= 4.0 * e0


def test_full_width_against_float64():
    """12 layers x 768 x 12 heads, B = 2, T = 140 (five key tiles, the last one partial), lens (140, 70)"""
    from mmvqa_amd.teacher import BertTeacher
    dev = torch.device("cuda:0")
    sd = TH.random_state_dict(12, 768, 3072, 300, 160, seed=5)
    g = torch.Generator().manual_seed(6)
    lens = torch.tensor([140, 70], dtype=torch.int32)
    ids = torch.randint(1, 300, (2, 140), generator=g)
    ids[1, 70:] = 0
    with torch.no_grad():
        r64 = TH.bert_forward(sd, ids, lens, dtype=torch.float64)
        r32 = TH.bert_forward(sd, ids, lens, dtype=torch.float32)
    e = float((r32.double() - r64).abs().max())
    teacher = BertTeacher.from_state_dict(sd).to(dev)
    assert (teacher.layers, teacher.hidden, teacher.heads, teacher.inter) == (12, 768, 12, 3072)
    out = teacher(ids.to(dev), lens.to(dev))
    err = float((out.cpu().double() - r64).abs().max())
    print(f"full width: |out| max {float(r64.abs().max()):.2f}, |err| {err:.3e}, torch fp32 on the CPU {e:.3e}, ratio {err / e:.2f}")
    assert err <= 4.0 * e


def test_sentence_means_and_argument_checks(fx, small):
    dev = torch.device("cuda:0")
    ids, lens = torch.from_numpy(fx["a_ids"]).to(dev), torch.from_numpy(fx["a_lens"]).to(dev)
    m = small.sentence_means(ids, lens)
    ref = torch.from_numpy(fx["a_f64"]).mean(1)
    assert m.shape == (3, 128) and float((m.cpu().double() - ref).abs().max()) <= 4.0 * float(fx["e0"])
    assert list(small.parameters()) == [] and small.state_dict() == {}          # frozen: nothing to optimise or save
    for bad_ids, bad_lens in ((ids.int(), lens), (ids, lens.long()), (ids[0], lens), (ids, lens[:2]), (ids.cpu(), lens),
                              (torch.zeros(1, 65, dtype=torch.int64, device=dev), lens[:1])):      # T > max_pos = 64
        with pytest.raises(ValueError):
            small(bad_ids, bad_lens)
