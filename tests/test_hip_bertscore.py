"""mmvqa_bertscore_mask and the teacher at an inner layer on the GPU, against the float64 restatement of
tests/bertscore_helpers.py.

Bound of every comparison: max(4 e_cpu, 2^-22), e_cpu = |fp32 CPU restatement - float64| on the same inputs; it never
comes from the kernel's output.  F is ill-conditioned where P + R is near 0, so F is compared on `common direction +
noise` inputs (P + R >= 0.5 in float64, asserted on the CPU first) and zero-mean inputs are compared on P and R only.

Measured on an MI355X (error / e_cpu, worst of P, R, F over the four shapes): see DESIGN.md section 18."""
import functools

import pytest
import torch

import bertscore_helpers as BH
import teacher_helpers as TH

pytestmark = pytest.mark.gpu

# (n, T, D), the lengths in use: one tile; the tile edges 31 / 32 / 33; two tiles and a row into the third at the
# teacher's full width; sixteen tiles (four per wave) against four
CASES = (((3, 5, 64), (2, 3, 5)), ((4, 33, 128), (2, 31, 32, 33)), ((2, 65, 768), (64, 65)), ((2, 512, 64), (512, 100)))
IDS = ["n3_T5_D64", "n4_T33_D128", "n2_T65_D768", "n2_T512_D64"]


@functools.lru_cache(maxsize=None)
def case(k, kind):
    """inputs, lengths and the float64 reference of case k, computed once and shared"""
    (n, T, D), choices = CASES[k]
    xa, xb = (BH.positive_states if kind == "positive" else BH.zero_mean_states)(n, T, D, seed=10 + k)
    la, lb = BH.lens_cycle(n, choices), BH.lens_cycle(n, choices, shift=0 if n == 2 else 1)
    ref, e_cpu = BH.cpu_error(xa, la, xb, lb)
    if kind == "positive":
        BH.assert_conditioned(ref, la, lb)
    return xa, la, xb, lb, ref, e_cpu


def gpu_scores(xa, la, xb, lb, baseline=0.0):
    import mmvqa_amd
    dev = torch.device("cuda:0")
    out = mmvqa_amd.bertscore_mask(xa.to(dev), la.to(dev), xb.to(dev), lb.to(dev), baseline=baseline, return_pr=True)
    return tuple(t.cpu() for t in out)         # (F, P, R)


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_scores_against_float64(k):
    n = CASES[k][0][0]
    for kind, names in (("positive", "PRF"), ("zero_mean", "PR")):
        xa, la, xb, lb, ref, e_cpu = case(k, kind)
        F, P, R = gpu_scores(xa, la, xb, lb)
        lim = BH.bound(e_cpu)
        for name, got, want in (("P", P, ref[0]), ("R", R, ref[1]), ("F", F, ref[2])):
            assert torch.equal(torch.diagonal(got), torch.ones(n)), f"{name}: the diagonal is not exactly 1"
            if name not in names:
                continue
            err = float((got.double() - want).abs().max())
            print(f"{IDS[k]} {kind} {name}: |err| {err:.3e}, e_cpu {e_cpu:.3e}, bound {lim:.3e}, err / e_cpu "
                  f"{err / max(e_cpu, 1e-30):.2f}, err / bound {err / lim:.2f}")
            assert err <= lim, (IDS[k], kind, name, err, lim)
        assert not torch.isnan(F).any()


def test_baseline_rescaling_on_gpu():
    xa, la, xb, lb, _, _ = case(1, "positive")
    ref, e_cpu = BH.cpu_error(xa, la, xb, lb, baseline=0.3)
    F, P, R = gpu_scores(xa, la, xb, lb, baseline=0.3)
    # F' = (F - b) / (1 - b) stretches F's error by 1 / (1 - b); the CPU's own fp32 error of F' carries that factor too
    assert float((F.double() - ref[2]).abs().max()) <= BH.bound(e_cpu)
    assert float((P.double() - ref[0]).abs().max()) <= BH.bound(e_cpu)          # P and R are not rescaled
    assert torch.equal(torch.diagonal(F), torch.ones(4))
    off = BH.offdiag(4) & ((la[:, None] == 2) | (lb[None, :] == 2))
    empty = (torch.tensor(0.0) - torch.tensor(0.3)) / (torch.tensor(1.0) - torch.tensor(0.3))      # fp32, as the kernel
    assert off.any() and bool((F[off] == empty).all())         # an empty text scores 0 and is rescaled like any score


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_padding_is_never_read_and_launches_repeat(k):
    xa, la, xb, lb, _, _ = case(k, "positive")
    clean = gpu_scores(xa, la, xb, lb)
    again = gpu_scores(xa, la, xb, lb)
    assert all(torch.equal(a, b) for a, b in zip(clean, again)), "two launches differ"
    for value in (1e30, float("nan"), float("inf")):
        got = gpu_scores(BH.poison(xa, la, value), la, BH.poison(xb, lb, value), lb)
        assert all(torch.equal(a, b) for a, b in zip(clean, got)), f"padding filled with {value} changed the output"


def test_a_bad_length_gives_nan_in_its_row_or_column_only():
    xa, _, xb, _, _, _ = case(1, "positive")                 # n 4, T 33
    la = torch.tensor([33, 1, 20, 32], dtype=torch.int32)    # row 1: below 2
    lb = torch.tensor([5, 33, 34, 31], dtype=torch.int32)    # column 2: above T
    # poison beyond the lengths as well: nothing is read for a text with a bad length
    F, P, R = gpu_scores(BH.poison(xa, la, float("nan")), la, BH.poison(xb, lb, float("nan")), lb)
    want = torch.zeros(4, 4, dtype=torch.bool)
    want[1, :] = True
    want[:, 2] = True
    want.fill_diagonal_(False)
    for got in (F, P, R):
        assert torch.equal(torch.isnan(got), want)
        assert torch.isfinite(got[~want]).all() and torch.equal(torch.diagonal(got), torch.ones(4))
    ref = BH.bertscore(xa, la, xb, lb)
    ok = ~want
    _, e_cpu = BH.cpu_error(xa, la, xb, lb)
    assert float((F.double() - ref[2])[ok].abs().max()) <= BH.bound(e_cpu)


def test_host_refusals_launch_nothing():
    from mmvqa_amd import _lib as L
    lib = L.lib()
    dev = torch.device("cuda:0")
    n, T, D = 2, 8, 64
    xa = torch.zeros(n * T * D + 4, dtype=torch.float32, device=dev)
    xb = torch.zeros(n * T * D + 4, dtype=torch.float32, device=dev)
    ln = torch.full((n,), 4, dtype=torch.int32, device=dev)
    out = torch.full((3, n, n), -7.0, dtype=torch.float32, device=dev)
    p = lambda t, off=0: None if t is None else t.data_ptr() + off   # noqa: E731
    good = dict(xa=p(xa), lenA=p(ln), xb=p(xb), lenB=p(ln), mask=p(out[0]), prec=p(out[1]), rec=p(out[2]), n=n, T=T, D=D)
    bad = [dict(xa=None), dict(xb=None), dict(lenA=None), dict(lenB=None), dict(mask=None), dict(prec=None), dict(rec=None),
           dict(n=0), dict(n=65536), dict(T=1), dict(T=513), dict(D=32), dict(D=96), dict(D=1088), dict(xa=p(xa, 4)),
           dict(xb=p(xb, 8))]
    for change in bad:
        a = {**good, **change}
        rc = lib.mmvqa_bertscore_mask(L.stream_ptr(), a["xa"], a["lenA"], a["xb"], a["lenB"], a["mask"], a["prec"], a["rec"],
                                      a["n"], a["T"], a["D"], 0.0)
        assert rc == -1 and lib.mmvqa_last_error().startswith(b"bertscore_mask: "), (change, rc)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a refused call wrote to its outputs"
    a = good
    assert lib.mmvqa_bertscore_mask(L.stream_ptr(), a["xa"], a["lenA"], a["xb"], a["lenB"], a["mask"], a["prec"], a["rec"], n, T,
                                    D, 0.0) == 0
    torch.cuda.synchronize()
    assert bool((torch.diagonal(out, dim1=1, dim2=2) == 1.0).all())
    import mmvqa_amd
    with pytest.raises(mmvqa_amd.MMVQAError):
        mmvqa_amd.bertscore_mask(torch.zeros(2, 8, 64), ln.cpu(), torch.zeros(2, 8, 64), ln.cpu())      # no CPU fallback
    with pytest.raises(ValueError):
        mmvqa_amd.bertscore_mask(xa[:1024].view(2, 8, 64), ln.long(), xb[:1024].view(2, 8, 64), ln)


# ------------------------------------------------------------------------------------------ the teacher at a layer
@pytest.fixture(scope="module")
def fx(golden_dir):
    return TH.load(golden_dir)


@pytest.fixture(scope="module")
def small(fx):
    from mmvqa_amd.teacher import BertTeacher
    return BertTeacher.from_state_dict(TH.fixture_state_dict(fx), eps=float(fx["eps"])).to("cuda:0")


def one_layer(sd):
    return {k: v for k, v in sd.items() if not k.startswith("encoder.layer.1.")}


def test_teacher_hidden_state_of_layer_one(fx, small):
    dev = torch.device("cuda:0")
    ids, lens = torch.from_numpy(fx["a_ids"]), torch.from_numpy(fx["a_lens"])
    e0, eps = float(fx["e0"]), float(fx["eps"])
    out = small(ids.to(dev), lens.to(dev), layer=1).cpu()
    sd = TH.fixture_state_dict(fx)
    with torch.no_grad():
        ref = TH.bert_forward(one_layer(sd), ids, lens, eps=eps, dtype=torch.float64)
    err = float((out.double() - ref).abs().max())
    print(f"layer 1 vs the float64 one-layer cut: {err:.3e}, e0 {e0:.3e}, ratio {err / e0:.2f}")
    assert err <= 4.0 * e0
    assert float((out.double() - torch.from_numpy(fx["a_f64"])).abs().max()) > 100 * e0       # and it is not the last layer
    # HF itself, on the CPU: hidden_states[1] of the two-layer model
    import transformers
    cfg = transformers.BertConfig(vocab_size=sd["embeddings.word_embeddings.weight"].shape[0], hidden_size=128,
                                  num_hidden_layers=2, num_attention_heads=2,
                                  intermediate_size=sd["encoder.layer.0.intermediate.dense.weight"].shape[0],
                                  max_position_embeddings=int(fx["max_pos"]), type_vocab_size=2, layer_norm_eps=eps,
                                  hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    hf = transformers.BertModel(cfg, add_pooling_layer=False).eval()
    missing = hf.load_state_dict(sd, strict=False)
    assert not [k for k in missing.missing_keys if "position_ids" not in k] and not missing.unexpected_keys
    keep = (torch.arange(ids.shape[1])[None, :] < lens[:, None].long()).long()
    with torch.no_grad():
        hs = hf(input_ids=ids, attention_mask=keep, output_hidden_states=True).hidden_states
    assert len(hs) == 3
    errs = []
    for b, n in enumerate(lens.tolist()):           # HF's padded query rows depend on its additive mask; valid rows do not
        errs.append(float((out[b, :n] - hs[1][b, :n]).abs().max()))
    print(f"layer 1 vs transformers' hidden_states[1] (valid rows): {max(errs):.3e}, ratio to e0 {max(errs) / e0:.2f}")
    assert max(errs) <= 4.0 * e0


def test_teacher_layer_none_and_last_are_forward_itself(fx, small):
    dev = torch.device("cuda:0")
    ids, lens = torch.from_numpy(fx["a_ids"]).to(dev), torch.from_numpy(fx["a_lens"]).to(dev)
    today = small(ids, lens)
    assert torch.equal(small(ids, lens, layer=None), today) and torch.equal(small(ids, lens, layer=2), today)
    assert float((today.cpu().double() - torch.from_numpy(fx["a_f64"])).abs().max()) <= 4.0 * float(fx["e0"])
    for bad in (0, 3):
        with pytest.raises(ValueError, match="outside 1..2"):
            small(ids, lens, layer=bad)
    # the C entry point refuses on its own, before any launch
    from mmvqa_amd import _lib as L
    out = torch.full((3, 37, 128), -7.0, device=dev)
    for bad in (0, 3):
        rc = L.lib().mmvqa_bert_forward_layers(small._handle, L.stream_ptr(), L.ptr(ids), L.ptr(lens), 3, 37, bad, L.ptr(out))
        assert rc == -1 and b"n_layers" in L.lib().mmvqa_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def test_teacher_bertscore_mask_end_to_end(fx, small):
    """the fixture's 8 caption / translation pairs through train.teacher_bertscore_mask at layer 1; the oracle is the
    float64 restatement applied to float64 teacher states, the bound comes from the fp32 CPU pipeline's own error"""
    from mmvqa_amd import train
    dev = torch.device("cuda:0")
    cids, clens = torch.from_numpy(fx["c_ids"]), torch.from_numpy(fx["c_lens"])
    n, Tp, Lmax = cids.shape[0] // 2, cids.shape[1], int(fx["max_pos"])
    rows = torch.zeros(2 * n, 1 + Lmax, dtype=torch.int64)
    rows[:, 0] = clens
    rows[:, 1:1 + Tp] = cids
    sd, eps = one_layer(TH.fixture_state_dict(fx)), float(fx["eps"])
    with torch.no_grad():
        h64 = TH.bert_forward(sd, cids, clens, eps=eps, dtype=torch.float64)
        h32 = TH.bert_forward(sd, cids, clens, eps=eps, dtype=torch.float32)
    la, lb = clens[:n], clens[n:]
    for baseline in (0.0, 0.2):
        ref = BH.bertscore(h64[:n], la, h64[n:], lb, baseline, torch.float64)[2]
        cpu = BH.bertscore(h32[:n], la, h32[n:], lb, baseline, torch.float32)[2]
        e = float((cpu.double() - ref).abs().max())
        mask = train.teacher_bertscore_mask(small, rows.to(dev), 1, baseline, Tp).cpu()
        assert tuple(mask.shape) == (n, n) and torch.equal(torch.diagonal(mask), torch.ones(n))
        err = float((mask.double() - ref).abs().max())
        print(f"end to end, baseline {baseline}: |err| {err:.3e}, fp32 CPU pipeline {e:.3e}, bound {BH.bound(e):.3e}, "
              f"ratio {err / max(e, 1e-30):.2f}; F in [{float(ref.min()):.3f}, {float(ref[BH.offdiag(n)].max()):.3f}]")
        assert err <= BH.bound(e)
    # the batch's padding does not enter: a wider cut gives the same mask within the same bound
    wider = train.teacher_bertscore_mask(small, rows.to(dev), 1, 0.2, Tp + 7).cpu()
    assert float((wider.double() - ref).abs().max()) <= BH.bound(e)
