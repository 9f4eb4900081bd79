"""Op tests of csrc/attention.hip: every kernel instance (head dimension D in {8, 12, 64, 96} x key tiles NJ =
ceil(T / 32) in {1, 2, 3, 4} x forward / backward) against the float64 restatements of tests/attention_helpers.py.

NJ = 1 is the HOIST form of both kernels (every load issued up front), NJ >= 2 loads at the point of use, and the
backward's delta exchange across tiles exists only there: the instances are not interchangeable, so each is launched.

(D, NJ, direction) -> test.  Every case runs the forward and then the backward on one descriptor, so both directions
of an instance are covered by the same test id; T in TS = 1 9 31 32 | 33 64 | 65 75 96 | 97 127 128 gives NJ = 1 | 2 | 3
| 4 at its first and last T.
    <8, 1..4>   test_grid[bert-8-T]     BERT form (key mask, no score chain), engine pairing
    <64, 1..4>  test_grid[bert-64-T]    BERT form, engine pairing;  test_grid[rf-64-T] at T = 31 33 75 128 (cross)
    <12, 1..4>  test_grid[rf-12-T]      RealFormer form (query mask, prev_in / prev_out, dprev_in / dprev_out)
    <96, 1..4>  test_grid[rf-96-T]      RealFormer form;  test_grid[bert-96-T] at T = 31 33 75 128 (cross)
    test_grid[rf-D-T-noprev] (D = 12, 96; T = 31 33 75 128): prev_in = NULL (layer 0) and dprev_in = NULL (last layer)
    test_padded_strides: the NJ = 1 and NJ = 3 cases again with row stride + 4, out row stride + 4
    test_dropout: <96, 3> and <12, 2> in the RealFormer form, <8, 2> in the BERT form, p = 0.3
    test_all_masked_sample: <8, 2> BERT form, <12, 2> RealFormer form, one sample with an all-zero mask
    test_exact_zeros: BERT form, D = 8 and 64 at one T per NJ
    test_backward_end_to_end: the grid's backward outputs against float64 from the inputs alone

What every launch is held to (`run`): all outputs are prefilled with NaN and every allocation carries 32 sentinel rows,
NaN in the inputs' gaps and tails; afterwards every element of the operation is finite and within its bound, every
other bit of the output allocations is unchanged, the inputs are unchanged, and a second launch of the same
descriptor gives bit-equal results.  Tolerances: attention_helpers.py (policy 3 of chain_helpers.py per segment =
(sample, head, masked / unmasked rows) for dV, dprev_out and the masked rows of prev_out; analytic per-element bounds,
derived there, for the probabilities, out, dQ, dK and the unmasked rows of prev_out, where an honest kernel does not
stay inside the segment bound or only just).  The backward is checked as a
function of the probabilities the forward kernel saved (isolated), so that the forward's error stays out of its bound.

Worst error / bound per (form, D, NJ, output), measured on an MI355X:
(every case of the file: grid, padded strides, dropout, all-masked sample; probs / out / dq / dk against their analytic
bounds, which are worst-case and therefore far from 1; prev_out, dv, dprev_out against the segment bound)
    form  D  NJ      probs       out  prev_out        dq        dk        dv dprev_out
    bert   8   1       0.09      0.04         -      0.05      0.03      0.35         -
    bert   8   2       0.54      0.26         -      0.03      0.04      0.49         -
    bert   8   3       0.08      0.03         -      0.03      0.03      0.45         -
    bert   8   4       0.07      0.02         -      0.03      0.02      0.40         -
    bert  64   1       0.02      0.01         -      0.01      0.01      0.34         -
    bert  64   2       0.03      0.01         -      0.01      0.01      0.31         -
    bert  64   3       0.03      0.01         -      0.01      0.01      0.34         -
    bert  64   4       0.03      0.01         -      0.01      0.01      0.34         -
    bert  96   1       0.02      0.01         -      0.01      0.00      0.28         -
    bert  96   2       0.02      0.01         -      0.01      0.00      0.25         -
    bert  96   3       0.02      0.01         -      0.01      0.01      0.25         -
    bert  96   4       0.02      0.01         -      0.01      0.01      0.25         -
    rf    12   1       0.09      0.03      0.21      0.04      0.03      0.43      0.59
    rf    12   2       0.08      0.03      0.22      0.03      0.04      0.48      0.60
    rf    12   3       0.08      0.03      0.21      0.03      0.03      0.49      0.45
    rf    12   4       0.08      0.03      0.24      0.02      0.02      0.41      0.53
    rf    64   1       0.03      0.01      0.20      0.01      0.01      0.32      0.45
    rf    64   2       0.02      0.01      0.20      0.01      0.01      0.37      0.60
    rf    64   3       0.03      0.01      0.20      0.01      0.01      0.32      0.51
    rf    64   4       0.03      0.01      0.20      0.01      0.01      0.26      0.36
    rf    96   1       0.02      0.01      0.20      0.01      0.01      0.41      0.72
    rf    96   2       0.02      0.01      0.20      0.01      0.01      0.31      0.51
    rf    96   3       0.02      0.01      0.20      0.01      0.01      0.36      0.78
    rf    96   4       0.02      0.01      0.20      0.01      0.01      0.31      0.60
"""
import ctypes as C
import functools
from types import SimpleNamespace

import pytest
import torch

import attention_helpers as AH
from attention_helpers import F32, F64, NAN, TAIL
from chain_helpers import check, same_bits
from hip_helpers import dev, relerr
from mmvqa_amd import _lib as L

pytestmark = pytest.mark.gpu
SEED = 4321
HEADS = 2


def _nan_like(x):
    return torch.full_like(x, NAN)


def _untouched(buf, owned, what):
    """every element of an output allocation outside the operation still holds the NaN it was prefilled with"""
    b = buf.cpu()
    assert same_bits(b[~owned], _nan_like(b)[~owned]), f"{what}: a store outside the operation's elements"


@functools.lru_cache(maxsize=None)
def run(form, D, T, lens, prev=True, dprev=True, drop_p=0.0, pad=0):
    """forward, forward again, backward, backward again on one descriptor; the structural assertions of the file header;
    returns the case, the kernel's outputs (CPU, fp32, probabilities query-major) and the float64 / fp32 references"""
    c = AH.make_case(form, D, T, lens, prev, dprev, heads=HEADS)
    B, rf = len(lens), form == "rf"
    lay = AH.Layout(form, HEADS, D, pad)
    qkv = lay.pack(B, T, q=c["q"], k=c["k"], v=c["v"]).to(dev())
    dout = lay.pack(B, T, out=c["dout"]).to(dev())
    mask = AH.tail_rows(c["mask"].reshape(B * T), AH.MASK_POISON).to(dev())
    score = torch.full((B * T + TAIL, T, HEADS), NAN)                       # [B, query, key, heads] + tail
    prev_in = None if c["prev_in"] is None else AH.tail_rows(c["prev_in"].reshape(B * T, T, HEADS)).to(dev())
    dprev_in = None if c["dprev_in"] is None else AH.tail_rows(c["dprev_in"].reshape(B * T, T, HEADS)).to(dev())
    out, dqkv = lay.blank("out", B, T).to(dev()), lay.blank("q", B, T).to(dev())
    probs = torch.full((B * HEADS * T + TAIL, T), NAN, device=dev())
    prev_out = score.to(dev()) if rf else None
    dprev_out = score.to(dev()) if rf else None
    inputs = [x for x in (qkv, dout, mask, prev_in, dprev_in) if x is not None]
    before = [x.clone() for x in inputs]
    if rf:
        a = AH.rf_attn_desc(lay, qkv, out, mask, probs, B, T, c["sqrt_d"], prev_in, prev_out, AH.f32(drop_p), SEED)
    else:
        a = AH.bert_attn_desc(lay, qkv, out, mask, probs, B, T, c["sqrt_d"], AH.f32(drop_p), SEED)
    AH.set_bwd(a, lay, dout, dqkv, dprev_in, dprev_out)
    what = f"{form} D={D} T={T} lens={lens} p={drop_p} pad={pad}"

    fwd_out = [x for x in (out, probs, prev_out) if x is not None]
    AH.launch(a, D, 0)
    saved = [x.clone() for x in fwd_out]
    AH.launch(a, D, 0)
    assert all(same_bits(x, y) for x, y in zip(fwd_out, saved)), f"{what}: two forward launches differ"
    bwd_out = [x for x in (dqkv, dprev_out) if x is not None]
    AH.launch(a, D, 1)
    first = [x.clone() for x in bwd_out]
    AH.launch(a, D, 1)
    assert all(same_bits(x, y) for x, y in zip(bwd_out, first)), f"{what}: two backward launches differ"
    assert all(same_bits(x, y) for x, y in zip(fwd_out, saved)), f"{what}: the backward changed a forward output"
    assert all(same_bits(x, y) for x, y in zip(inputs, before)), f"{what}: an input changed"

    _untouched(out, lay.owned(B, T, "out"), what + " out")
    _untouched(dqkv, lay.owned(B, T, "q", "k", "v"), what + " dq|dk|dv")
    tail = torch.zeros(B * HEADS * T + TAIL, T, dtype=torch.bool)
    tail[:B * HEADS * T] = True
    _untouched(probs, tail, what + " probs")
    stail = torch.zeros(B * T + TAIL, T, HEADS, dtype=torch.bool)
    stail[:B * T] = True
    for x, n in ((prev_out, " prev_out"), (dprev_out, " dprev_out")):
        if x is not None:
            _untouched(x, stail, what + n)

    r = SimpleNamespace(c=c, what=what, drop_p=drop_p, form=form, D=D, T=T)
    r.out = lay.unpack(out, "out", B, T)
    r.probs = probs.cpu()[:B * HEADS * T].view(B, HEADS, T, T).transpose(-1, -2).contiguous()   # saved key-major
    r.prev_out = prev_out.cpu()[:B * T].view(B, T, T, HEADS) if rf else None
    r.dq, r.dk, r.dv = (lay.unpack(dqkv, w, B, T) for w in "qkv")
    r.dprev_out = dprev_out.cpu()[:B * T].view(B, T, T, HEADS) if rf else None
    fa = AH.fwd_args(c, drop_p, SEED)
    r.ref, r.cpu = AH.attn_fwd(*fa, F64), AH.attn_fwd(*fa, F32)
    return r


def check_case(r):
    """forward and isolated backward within their bounds; returns {output: worst error / bound}"""
    c, w = r.c, r.what
    fb = AH.fwd_bounds(c, r.ref, r.cpu, r.drop_p, SEED)
    ratios = {"probs": check(r.probs, r.ref[1], fb[1], w + " probs"), "out": check(r.out, r.ref[2], fb[2], w + " out")}
    if r.prev_out is not None:
        ratios["prev_out"] = check(r.prev_out, r.ref[0], fb[0], w + " prev_out")
    ba = AH.bwd_args(c, r.probs, r.drop_p, SEED)       # the kernel's own saved probabilities
    bref = AH.attn_bwd(*ba, F64)
    bb = AH.bwd_bounds(c, r.probs, bref, AH.attn_bwd(*ba, F32), r.drop_p, SEED)
    got = (r.dq, r.dk, r.dv) + ((r.dprev_out,) if r.dprev_out is not None else ())
    for i, (n, x) in enumerate(zip(("dq", "dk", "dv", "dprev_out"), got)):
        ratios[n] = check(x, bref[i], bb[i], f"{w} {n} (isolated)")
    print(f"err/bound {r.form} D={r.D} NJ={AH.nj_of(r.T)} T={r.T} p={r.drop_p}: " + " ".join(f"{n} {x:.2f}" for n, x in ratios.items()))
    return ratios


def _id(case):
    form, D, T, prev, dprev = case
    return f"{form}-{D}-{T}" + ("" if prev else "-noprev")


GRID = AH.grid_cases()


# ----------------------------------------------------------------------------- a. the instance grid
@pytest.mark.parametrize("case", GRID, ids=_id)
def test_grid(case):
    form, D, T, prev, dprev = case
    check_case(run(form, D, T, AH.ragged_lens(T), prev, dprev))


# ----------------------------------------------------------------------------- c. padded strides
@pytest.mark.parametrize("case", [g for g in GRID if AH.nj_of(g[2]) in (1, 3)], ids=_id)
def test_padded_strides(case):
    """row stride + 4 and out row stride + 4: NaN in the inputs' gap columns, the outputs' gap columns bit-identical
    afterwards (`run`), and the values those of the compact run, bit for bit"""
    form, D, T, prev, dprev = case
    r = run(form, D, T, AH.ragged_lens(T), prev, dprev, pad=4)
    check_case(r)
    r0 = run(form, D, T, AH.ragged_lens(T), prev, dprev)
    for n in ("out", "probs", "prev_out", "dq", "dk", "dv", "dprev_out"):
        x, y = getattr(r, n), getattr(r0, n)
        assert x is None or same_bits(x, y), f"{r.what}: {n} differs from the compact layout's"


# ----------------------------------------------------------------------------- b. edge cases
@pytest.mark.parametrize("form,D", [("bert", 8), ("rf", 12)])
def test_all_masked_sample(form, D):
    """a sample whose mask is all zero: every score of it carries the -10000; finite and within the bound"""
    check_case(run(form, D, 40, (40, 0, 17)))


@pytest.mark.parametrize("form,D,T", [("rf", 96, 75), ("rf", 12, 33), ("bert", 8, 33)])
def test_dropout(form, D, T):
    """p = 0.3 on the instances test_hip_dropout.py does not reach: one query-major keep mask in the forward and in
    both passes of the backward; the saved probabilities are those from before dropout"""
    r = run(form, D, T, AH.ragged_lens(T), drop_p=0.3)
    check_case(r)
    assert relerr(r.out, AH.attn_fwd(*AH.fwd_args(r.c), F64)[2]) > 1e-2      # dropout really was applied


# ----------------------------------------------------------------------------- d. exact zeros
@pytest.mark.parametrize("D", [8, 64])
@pytest.mark.parametrize("T", list(AH.NJ_T.values()))
def test_exact_zeros(D, T):
    """BERT form, samples with a valid key: exp(-10000 + ..) underflows to 0 in fp32 and in the float64 reference alike,
    so probs at masked keys and the dk / dv rows of masked keys are exactly 0"""
    r = run("bert", D, T, AH.ragged_lens(T))
    dead = ~r.c["mask"].bool()                                    # [B, key]
    assert bool(dead.any())
    bref = AH.attn_bwd(*AH.bwd_args(r.c, r.ref[1]), F64)
    pk = dead[:, None, None, :].expand_as(r.probs)
    rk = dead[:, None, :, None].expand_as(r.dk)
    assert float(r.ref[1][pk].abs().max()) == 0.0 and float(bref[1][rk].abs().max()) == 0.0 and float(bref[2][rk].abs().max()) == 0.0
    assert float(r.probs[pk].abs().max()) == 0.0, "probs at masked keys"
    assert float(r.dk[rk].abs().max()) == 0.0 and float(r.dv[rk].abs().max()) == 0.0, "dk / dv rows of masked keys"


# ----------------------------------------------------------------------------- e. backward, end to end
@pytest.mark.parametrize("form,D", [("bert", 8), ("bert", 64), ("bert", 96), ("rf", 12), ("rf", 96), ("rf", 64)])
def test_backward_end_to_end(form, D):
    """The kernel's dq / dk / dv / dprev_out of every grid case of one (form, D) against the float64 forward + backward
    from the inputs alone, assert_close at the 1e-4 of the existing attention tests.  Measured on an MI355X, worst
    rel-to-max error over the cases: BERT form 3.8e-7 .. 1.2e-6, RealFormer form 3.2e-7 .. 1.1e-6.

    This test is why the forward kernel takes the softmax of a query-masked row from the unshifted scores (header of
    attention.hip): with the -10000 subtracted first, as the kernel did before, the RealFormer form missed the 1e-4
    with 2.0e-4 .. 3.2e-4 in every output.  fp32 rounds the shifted scores of a masked query row to a grid of 2^-10, its
    probabilities come out ~1.5e-4 off, and dK / dV sum over all query rows; with all-valid masks the same cases gave
    3e-7.  That is also where the 3e-4 / 5e-4 of test_hip_ops.py::test_attention_realformer against an fp32 reference
    came from."""
    worst, bad = {}, []
    for f, d, T, prev, dprev in GRID:
        if (f, d) != (form, D):
            continue
        r = run(f, d, T, AH.ragged_lens(T), prev, dprev)
        bref = AH.attn_bwd(*AH.bwd_args(r.c, r.ref[1]), F64)
        got = (r.dq, r.dk, r.dv) + ((r.dprev_out,) if r.dprev_out is not None else ())
        for n, x, y in zip(("dq", "dk", "dv", "dprev_out"), got, bref):
            e = relerr(x, y)
            worst[n] = max(worst.get(n, 0.0), e)
            if not e <= 1e-4:
                bad.append(f"T={T}{'' if prev else ' noprev'} {n} {e:.1e}")
    print(f"end to end {form} D={D}, worst rel-to-max error: " + " ".join(f"{n} {e:.1e}" for n, e in worst.items()))
    assert not bad, f"{form} D={D}: rel-to-max error > 1e-4 against float64: " + ", ".join(bad)


# ----------------------------------------------------------------------------- f. host refusals
def test_host_refusals():
    """nothing is launched: every pointer is a number that is never dereferenced"""
    lib, p = L.lib(), 0x1000

    def call(head_dim=64, bwd=0, **kw):
        d = L.AttnDesc()
        d.q = d.k = d.v = d.out = d.mask = d.probs = d.dout = d.dq = d.dk = d.dv = p
        d.row_stride, d.head_stride, d.out_row_stride, d.out_head_stride = 3 * 128, 64, 128, 64
        d.B, d.T, d.heads, d.sqrt_d = 2, 16, 2, 8.0
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.mmvqa_attention(C.byref(d), head_dim, bwd, None), lib.mmvqa_last_error()

    for kw, text in ((dict(T=129), b"attention: T=129 > 128 unsupported"),
                     (dict(head_dim=16), b"attention: head_dim=16 unsupported (8,12,64,96)"),
                     (dict(T=0), b"attention: B=2 T=0 heads=2 drop_p=0"),
                     (dict(B=0), b"attention: B=0 T=16 heads=2 drop_p=0"),
                     (dict(heads=0), b"attention: B=2 T=16 heads=0 drop_p=0"),
                     (dict(B=-1), b"attention: B=-1 T=16 heads=2 drop_p=0"),
                     (dict(drop_p=1.0), b"attention: B=2 T=16 heads=2 drop_p=1"),
                     (dict(drop_p=-0.5), b"attention: B=2 T=16 heads=2 drop_p=-0.5"),
                     (dict(drop_p=NAN), b"attention: B=2 T=16 heads=2 drop_p=nan")):
        for bwd in (0, 1):
            rc, err = call(bwd=bwd, **kw)
            assert rc == -1 and err == text, (kw, bwd, rc, err)
