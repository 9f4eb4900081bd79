"""GPU op tests of the non-GEMM chain kernels of csrc/elementwise.hip, called through the C ABI, each against a float64
restatement of the same operation at the shapes where its launch geometry changes, with per-element bounds.  The
references, the bounds and the one tolerance policy are in tests/chain_helpers.py (checked on the CPU by
tests/test_chain_refs_cpu.py).  Every test prints its worst err / bound ratio ("chain ... ratio")."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import chain_helpers as CH  # noqa: E402
from chain_helpers import F32, F64, U23, U24  # noqa: E402
from hip_helpers import L, P, dev, dot_ulps  # noqa: E402

ERR_ARG = -1
NAN = float("nan")


def gpu(t):
    return None if t is None else t.to(dev())


def nanbuf(*shape):
    return torch.full(shape, NAN, device=dev())


def say(what, **ratios):
    print(f"chain {what} ratio: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def refused(rc, tag):
    assert rc == ERR_ARG, f"{tag}: rc {rc}"
    assert tag.encode() in L.lib().mmvqa_last_error(), L.lib().mmvqa_last_error()


# ----------------------------------------------------------------------------- LayerNorm
# H: one float4 per row (4), the j boundaries of the 64-lane float4 loop (256 / 260), LN_MAXV's limit (1024);
# rows: ragged last workgroup (1, 3, 5), rows_per_wave 2 (515) and 4 (2051), neither a multiple of 4 * rpw
LN_CASES = [(1, 4, 0), (3, 96, 0), (5, 256, 0), (5, 260, 0), (3, 768, 0), (5, 1024, 0), (1, 1024, 0), (515, 8, 0), (515, 96, 0),
            (2051, 8, 0), (2051, 96, 0), (5, 260, 100), (3, 768, 100)]


def _ln_inputs(rows, H, off):
    torch.manual_seed(1000 * rows + H + off)
    x = torch.randn(rows, H) + off
    g, b = torch.rand(H) + 0.5, torch.randn(H)
    return x, g, b


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("rows,H,off", LN_CASES)
def test_layernorm_fwd(rows, H, off, with_res):
    """y per row under the 4x rule; rstd under it as one segment; sum_out is ONE fp32 add (exact) and stays unwritten
    without a residual.  The floor's scale for y is max(max|y|, max|s| rstd max|gamma|) of the row: with a common offset
    (mean 100, std 1) every rounding of the mean happens at magnitude 100 and reaches y multiplied by rstd * gamma, and a
    row's whole error is that one rounding, of which a single row's e_cpu is a single draw.  Measured on an MI355X at
    rows 5, H 260, offset 100, row 0: kernel 1.277e-5 (1.7 ulp of the row sum 26000, divided by H), 4 e_cpu 2.77e-6
    (the restatement drew 0.1 ulp there and 1.4 ulp, 4 e_cpu 4.2e-5, in the next row); 2^-22 * 100 * rstd * max|gamma|
    = 3.5e-5.  Without an offset max|s| rstd max|gamma| is of the size of max|y| and the floor is what it was.  mean is a sum of H terms and a division, so its bound is analytic -- (dot_ulps(H) + 1) 2^-23
    mean|s| -- because 4x of a restatement that cancels to a small mean can be 0."""
    x, g, b = _ln_inputs(rows, H, off)
    r = torch.randn(rows, H) * 0.5 if with_res else None
    eps = 1e-12 if H != 96 else 1e-5
    y, s, mean, rstd = nanbuf(rows, H), nanbuf(rows, H), nanbuf(rows), nanbuf(rows)
    xd, rd, gd, bd = gpu(x), gpu(r), gpu(g), gpu(b)
    L.check(L.lib().mmvqa_layernorm_fwd(L.stream_ptr(), P(xd), P(rd), P(gd), P(bd), P(y), P(s), P(mean), P(rstd), rows, H, eps))
    torch.cuda.synchronize()
    s64, m64, r64, y64 = CH.ln_fwd(x, r, g, b, eps, F64)
    s32, m32, r32, y32 = CH.ln_fwd(x, r, g, b, eps, F32)
    if with_res:
        assert torch.equal(s.cpu(), x + r), "sum_out is one correctly rounded add"
    else:
        assert CH.same_bits(s, torch.full((rows, H), NAN)), "sum_out written without a residual"
    carried = s64.abs().amax(-1, keepdim=True) * r64[:, None] * float(g.abs().max())
    ry = CH.check(y, y64, CH.bound_4x(y64, y32, seg=-1, scale=carried), "ln y")
    rm = CH.check(mean, m64, (dot_ulps(H) + 1) * U23 * s64.abs().mean(-1) + 1e-30, "ln mean")
    rr = CH.check(rstd, r64, CH.bound_4x(r64, r32), "ln rstd")
    say(f"layernorm_fwd rows={rows} H={H} off={off} res={with_res}", y=ry, mean=rm, rstd=rr)


@pytest.mark.parametrize("with_dgamma", [False, True])
@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("rows,H,off", LN_CASES)
def test_layernorm_bwd(rows, H, off, with_dres, with_dgamma):
    """dx per row under the 4x rule.  dgamma / dbeta accumulate onto pre-filled buffers: a tree over rows + 1 leaves
    (chain_helpers.colacc_bound; the terms dy * xhat of dgamma carry the two roundings of xhat = (x - mean) * rstd).
    Without dgamma (the Grad-CAM path) dbeta is neither read nor written: a NaN buffer comes back bit-identical."""
    x, g, _ = _ln_inputs(rows, H, off)
    dy = torch.randn(rows, H)
    dres = torch.randn(rows, H) if with_dres else None
    _, m64, r64, _ = CH.ln_fwd(x, None, g, g, 1e-12, F64)
    mean, rstd = m64.float(), r64.float()          # the kernel's inputs: the saved statistics, in fp32
    dg0, db0 = torch.randn(H) * 3, torch.randn(H) * 3
    dx = nanbuf(rows, H)
    dgd = gpu(dg0) if with_dgamma else None
    dbd = gpu(db0) if with_dgamma else nanbuf(H)
    dyd, xd, gd, md, rsd, drd = gpu(dy), gpu(x), gpu(g), gpu(mean), gpu(rstd), gpu(dres)
    L.check(L.lib().mmvqa_layernorm_bwd(L.stream_ptr(), P(dyd), P(xd), P(gd), P(md), P(rsd), P(drd), P(dx), P(dgd), P(dbd), rows, H))
    torch.cuda.synchronize()
    dx64, dg64, db64 = CH.ln_bwd(dy, x, g, mean, rstd, dres, F64)
    dx32, _, _ = CH.ln_bwd(dy, x, g, mean, rstd, dres, F32)
    ratios = dict(dx=CH.check(dx, dx64, CH.bound_4x(dx64, dx32, seg=-1), "ln dx"))
    if with_dgamma:
        xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
        ratios["dgamma"] = CH.check(dgd, dg0.double() + dg64, CH.colacc_bound((dy.double() * xh).abs().sum(0), dg0, rows, extra=2), "ln dgamma")
        ratios["dbeta"] = CH.check(dbd, db0.double() + db64, CH.colacc_bound(dy.double().abs().sum(0), db0, rows), "ln dbeta")
    else:
        assert CH.same_bits(dbd, torch.full((H,), NAN)), "dbeta touched although dgamma is NULL"
    say(f"layernorm_bwd rows={rows} H={H} off={off} dres={with_dres} dgamma={with_dgamma}", **ratios)


def test_layernorm_refuses_an_H_it_cannot_address():
    t = nanbuf(2 * 1028)
    for H in (6, 1028):
        refused(L.lib().mmvqa_layernorm_fwd(L.stream_ptr(), P(t), None, P(t), P(t), P(t), P(t), P(t), P(t), 1, H, 1e-5), "layernorm")
        refused(L.lib().mmvqa_layernorm_bwd(L.stream_ptr(), P(t), P(t), P(t), P(t), P(t), None, P(t), P(t), P(t), 1, H), "layernorm")
    torch.cuda.synchronize()
    assert CH.same_bits(t, torch.full((2 * 1028,), NAN)), "a refused call wrote"


# ----------------------------------------------------------------------------- embeddings
EB, ET, EV, EPOS = 3, 7, 11, 16      # B * T = 21: not a multiple of the 4 rows of a workgroup


def _embed_inputs(H, nv):
    torch.manual_seed(77 + H + nv)
    ids = torch.randint(0, EV, (EB, ET))
    ids[0, 5], ids[0, 6] = 0, 0                       # the padding id, twice in one sample
    ids[1, 5], ids[1, 6], ids[2, 5] = 3, 3, 3         # one word row hit within and across samples
    ids[2, 6] = EV - 1                                # the table's last row
    seg = torch.randint(0, 2, (EB, ET))
    word, pos, typ = torch.randn(EV, H), torch.randn(EPOS, H) * 0.5, torch.randn(2, H) * 0.5
    g, b = torch.rand(H) + 0.5, torch.randn(H)
    vis = torch.randn(nv, EB, H) if nv else None
    return ids, seg, word, pos, typ, g, b, vis


@pytest.mark.parametrize("nv", [0, 5, ET])
@pytest.mark.parametrize("H", [4, 96, 1024])
def test_embed_fwd(H, nv):
    """text rows: out, xhat per row and rstd under the 4x rule; visual rows: out is a copy (exact) and xhat / rstd are
    not written"""
    ids, seg, word, pos, typ, g, b, vis = _embed_inputs(H, nv)
    out, xh, rstd = nanbuf(EB * ET, H), nanbuf(EB * ET, H), nanbuf(EB * ET)
    dv = [gpu(t) for t in (ids, seg, word, pos, typ, g, b, vis)]
    L.check(L.lib().mmvqa_embed_fwd(L.stream_ptr(), *[P(t) for t in dv], P(out), P(xh), P(rstd), EB, ET, H, nv, 1e-12, 0.0, 0))
    torch.cuda.synchronize()
    o64, x64, r64 = CH.embed_fwd(ids, seg, word, pos, typ, g, b, vis, nv, 1e-12, F64)
    o32, x32, r32 = CH.embed_fwd(ids, seg, word, pos, typ, g, b, vis, nv, 1e-12, F32)
    text = (torch.arange(EB * ET) % ET) >= nv
    if nv:
        assert torch.equal(out.cpu()[~text], o32[~text]), "visual rows are copies"
        assert CH.same_bits(xh.cpu()[~text], torch.full((int((~text).sum()), H), NAN)) and bool(torch.isnan(rstd.cpu()[~text]).all())
    ratios = {}
    if bool(text.any()):
        ratios["out"] = CH.check(out.cpu()[text], o64[text], CH.bound_4x(o64[text], o32[text], seg=-1), "embed out")
        ratios["xhat"] = CH.check(xh.cpu()[text], x64[text], CH.bound_4x(x64[text], x32[text], seg=-1), "embed xhat")
        ratios["rstd"] = CH.check(rstd.cpu()[text], r64[text], CH.bound_4x(r64[text], r32[text]), "embed rstd")
    say(f"embed_fwd H={H} nv={nv}", **ratios)


@pytest.mark.parametrize("pad_idx", [0, -1])
@pytest.mark.parametrize("nv", [0, 5, ET])
@pytest.mark.parametrize("H", [4, 96, 1024])
def test_embed_bwd(H, nv, pad_idx):
    """all five gradient buffers are pre-filled: the kernel accumulates.  Table rows that received gradient: 4x rule per
    row on prior + increment; rows that received none (the padding row with pad_idx 0, unused ids and positions): bit
    for bit the prior.  dgamma / dbeta: a tree over the text rows + the prior (colacc_bound; xhat is an input here, so
    dy * xhat rounds once).  dvis is a copy."""
    ids, seg, word, pos, typ, g, b, vis = _embed_inputs(H, nv)
    _, x64, r64 = CH.embed_fwd(ids, seg, word, pos, typ, g, b, vis, nv, 1e-12, F64)
    xhat, rstd = x64.float(), r64.float()
    dout = torch.randn(EB * ET, H)
    prior = [torch.randn(EV, H), torch.randn(EPOS, H), torch.randn(2, H), torch.randn(H) * 3, torch.randn(H) * 3]
    bufs = [gpu(t) for t in prior]
    dvis = nanbuf(max(nv, 1), EB, H)
    dv = [gpu(t) for t in (dout, ids, seg, xhat, rstd, g)]
    L.check(L.lib().mmvqa_embed_bwd(L.stream_ptr(), *[P(t) for t in dv], *[P(t) for t in bufs], P(dvis), EB, ET, H, nv, 0.0, 0, pad_idx))
    torch.cuda.synchronize()
    inc64 = CH.embed_bwd(dout, ids, seg, xhat, rstd, g, EV, EPOS, 2, nv, pad_idx, F64)
    inc32 = CH.embed_bwd(dout, ids, seg, xhat, rstd, g, EV, EPOS, 2, nv, pad_idx, F32)
    text = torch.zeros(EB, ET, dtype=torch.bool)
    text[:, nv:] = True
    hit = [torch.zeros(EV, dtype=torch.bool), torch.zeros(EPOS, dtype=torch.bool), torch.zeros(2, dtype=torch.bool)]
    hit[0][ids[text & (ids != pad_idx)]] = True
    hit[1][nv:ET] = True
    hit[2][seg[text]] = True
    if pad_idx == 0:
        assert not bool(hit[0][0])
    elif nv < ET:
        assert bool(hit[0][0]), "without a padding row id 0 receives gradient"
    ratios = {}
    for k, name in enumerate(("dword", "dpos", "dtype")):
        got, h = bufs[k].cpu(), hit[k]
        assert torch.equal(got[~h], prior[k][~h]), f"{name}: a row that received no gradient changed"
        if bool(h.any()):
            ref, cpu = prior[k].double() + inc64[k], prior[k] + inc32[k]
            ratios[name] = CH.check(got[h], ref[h], CH.bound_4x(ref[h], cpu[h], seg=-1), f"embed {name}")
    n_text = int(text.sum())
    d_t = dout.double().view(EB, ET, H)[text]
    xh_t = xhat.double().view(EB, ET, H)[text]
    if n_text:
        ratios["dgamma"] = CH.check(bufs[3], prior[3].double() + inc64[3], CH.colacc_bound((d_t * xh_t).abs().sum(0), prior[3], n_text), "embed dgamma")
        ratios["dbeta"] = CH.check(bufs[4], prior[4].double() + inc64[4], CH.colacc_bound(d_t.abs().sum(0), prior[4], n_text), "embed dbeta")
    else:
        assert torch.equal(bufs[3].cpu(), prior[3]) and torch.equal(bufs[4].cpu(), prior[4])
    if nv:
        assert torch.equal(dvis.cpu(), dout.view(EB, ET, H)[:, :nv].transpose(0, 1)), "dvis is a copy of the visual rows of dout"
    say(f"embed_bwd H={H} nv={nv} pad_idx={pad_idx}", **ratios)


def test_embed_refuses_an_H_it_cannot_address():
    """forward and backward alike: the backward launcher's refusal was missing (it dropped the columns past 1024 and the
    last H % 4 of a row without a word)"""
    t = nanbuf(2 * 1028)
    z = torch.zeros(4, dtype=torch.long, device=dev())
    for H in (6, 1028):
        refused(L.lib().mmvqa_embed_fwd(L.stream_ptr(), P(z), P(z), P(t), P(t), P(t), P(t), P(t), None, P(t), P(t), P(t),
                                        1, 1, H, 0, 1e-12, 0.0, 0), "embed")
        refused(L.lib().mmvqa_embed_bwd(L.stream_ptr(), P(t), P(z), P(z), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), None,
                                        1, 1, H, 0, 0.0, 0, 0), "embed")
    torch.cuda.synchronize()
    assert CH.same_bits(t, torch.full((2 * 1028,), NAN)), "a refused call wrote"


# ----------------------------------------------------------------------------- mean-pool, L2-norm
@pytest.mark.parametrize("H", [1, 96, 257])
def test_meanpool(H):
    """masks with a hole, an all-zero sample (the 1e-9 clamp: exactly 0), an all-ones sample and a ragged tail;
    forward: T terms + one division; backward: one division, and one add when it accumulates (analytic bounds)"""
    torch.manual_seed(13 + H)
    B, T = 4, 7
    h, dp = torch.randn(B, T, H), torch.randn(B, H)
    mask = torch.ones(B, T, dtype=torch.long)
    mask[0, 2:4] = 0
    mask[1] = 0
    mask[3, 5:] = 0
    hd, md, dpd = gpu(h), gpu(mask), gpu(dp)
    out = nanbuf(B, H)
    L.check(L.lib().mmvqa_meanpool_fwd(L.stream_ptr(), P(hd), P(md), P(out), B, T, H))
    torch.cuda.synchronize()
    rf = CH.check(out, CH.meanpool_fwd(h, mask, F64), CH.meanpool_fwd_bound(h, mask), "meanpool fwd")
    assert float(out[1].abs().max()) == 0.0
    inc = CH.meanpool_bwd(dp, mask, F64)
    dh = nanbuf(B, T, H)                                   # accumulate = 0 overwrites whatever was there
    L.check(L.lib().mmvqa_meanpool_bwd(L.stream_ptr(), P(dpd), P(md), P(dh), B, T, H, 0))
    torch.cuda.synchronize()
    r0 = CH.check(dh, inc, CH.meanpool_bwd_bound(inc, None), "meanpool bwd")
    prior = torch.randn(B, T, H)
    dh = gpu(prior)
    L.check(L.lib().mmvqa_meanpool_bwd(L.stream_ptr(), P(dpd), P(md), P(dh), B, T, H, 1))
    torch.cuda.synchronize()
    r1 = CH.check(dh, prior.double() + inc, CH.meanpool_bwd_bound(inc, prior), "meanpool bwd accumulate")
    assert torch.equal(dh.cpu()[1], prior[1]), "a masked-out sample adds exactly 0"
    say(f"meanpool H={H}", fwd=rf, bwd=r0, bwd_acc=r1)


@pytest.mark.parametrize("D", [1, 96, 128, 130])
@pytest.mark.parametrize("rows", [1, 5, 9])
def test_l2norm(rows, D):
    """y and dx per row under the 4x rule; a zero row gives y = 0, nrm = 1e-12f and a finite dx; a row of magnitude 1e-20
    sits under the clamp too (nrm exactly 1e-12f, y = x / 1e-12f)"""
    torch.manual_seed(5 * rows + D)
    x, dy = torch.randn(rows, D), torch.randn(rows, D)
    clamped = torch.zeros(rows, dtype=torch.bool)
    if rows >= 5:
        x[1] = 0
        x[2] *= 1e-20
        clamped[1:3] = True
    xd, dyd = gpu(x), gpu(dy)
    y, nrm = nanbuf(rows, D), nanbuf(rows)
    L.check(L.lib().mmvqa_l2norm_fwd(L.stream_ptr(), P(xd), P(y), P(nrm), rows, D))
    torch.cuda.synchronize()
    y64, n64 = CH.l2norm_fwd(x, F64)
    y32, n32 = CH.l2norm_fwd(x, F32)
    ry = CH.check(y, y64, CH.bound_4x(y64, y32, seg=-1), "l2norm y")
    assert torch.equal(nrm.cpu()[clamped], torch.full((int(clamped.sum()),), 1e-12)), "the clamp is 1e-12f exactly"
    rn = CH.check(nrm.cpu()[~clamped], n64[~clamped], CH.bound_4x(n64[~clamped], n32[~clamped]), "l2norm nrm")
    if rows >= 5:
        assert float(y[1].abs().max()) == 0.0
    yin, nin = y64.float(), n64.float()                    # the backward kernel's inputs
    dx = nanbuf(rows, D)
    yd, nd = gpu(yin), gpu(nin)
    L.check(L.lib().mmvqa_l2norm_bwd(L.stream_ptr(), P(dyd), P(yd), P(nd), P(dx), rows, D))
    torch.cuda.synchronize()
    d64, d32 = CH.l2norm_bwd(dy, yin, nin, F64), CH.l2norm_bwd(dy, yin, nin, F32)
    assert bool(torch.isfinite(dx).all())
    rd = CH.check(dx, d64, CH.bound_4x(d64, d32, seg=-1), "l2norm dx")
    say(f"l2norm rows={rows} D={D}", y=ry, nrm=rn, dx=rd)


# ----------------------------------------------------------------------------- vocabulary log-softmax
def _rup(V):
    return (V + 3) & ~3


def run_mlm(x, tgt, kernel, ld, dld, pad=1e30, how="aligned", gs_dev=None, mul=1.0, grad=True, out3=False):
    """mmvqa_mlm_loss on x [rows, V] laid out with leading dimension ld, every column past V holding `pad`; dlogits is
    NaN-filled.  `how` selects the kernel by construction and the choice is asserted against the launcher's own
    condition: "aligned" (float4 kernels), "null_lse" (scalar form through row_lse == NULL), "unaligned" (scalar form
    through a base address or a leading dimension that is not 16-byte aligned)."""
    rows, V = x.shape
    off = 1 if how == "unaligned" and ld % 4 == 0 else 0
    lflat = torch.full((rows * ld + 4,), pad, device=dev())
    logits = lflat[off:off + rows * ld].view(rows, ld)
    logits[:, :V] = gpu(x)
    dflat = nanbuf(rows * dld + 4)
    dl = dflat[off:off + rows * dld].view(rows, dld)
    row_loss, pred = nanbuf(rows), torch.full((rows,), -7, dtype=torch.long, device=dev())
    row_lse = None if how == "null_lse" else nanbuf(rows)
    o3 = nanbuf(3) if out3 else None
    td = gpu(tgt)
    fast = row_lse is not None and CH.lsm_fast_ok(logits.data_ptr(), ld, V) and (not grad or CH.lsm_fast_ok(dl.data_ptr(), dld, V))
    assert fast == (kernel == "float4"), "the case does not reach the kernel it is meant for"
    L.check(L.lib().mmvqa_mlm_loss(L.stream_ptr(), P(logits), ld, P(td), P(row_loss), P(row_lse), P(pred), P(dl) if grad else None, dld,
                                   P(gs_dev), mul, rows, V, P(o3)))
    torch.cuda.synchronize()
    return dict(loss=row_loss.cpu(), lse=None if row_lse is None else row_lse.cpu(), pred=pred.cpu(), dl=dl.cpu(),
                out3=None if o3 is None else o3.cpu())


def check_mlm(res, x, tgt, kernel, gs=1.0, grad=True):
    """pred exact (first index); row_lse under the 4x rule; row_loss = lse - x[target] adds one rounding to the bound of
    lse; the gradient per element relative to the probability (chain_helpers.grad_bound, r = max(4 x the fp32 restatement's
    worst relative error, 2^-22), the relative form of max(4 e_cpu, 2^-22); a column of probability 0 must be exactly 0).  The pad columns of dlogits: exactly 0 up to
    round_up(V, 4) and untouched beyond after the float4 kernel (whose __expf term was NOT needed: see the printed
    ratios), all untouched after the scalar kernel."""
    rows, V = x.shape
    lse64, loss64, p64, pred64 = CH.lsm_ref(x, tgt, F64)
    lse32, loss32, p32, _ = CH.lsm_ref(x, tgt, F32)
    assert torch.equal(res["pred"], pred64), f"pred {res['pred'].tolist()} != first index of the maximum {pred64.tolist()}"
    b_lse = CH.bound_4x(lse64, lse32)
    ratios = {}
    if res["lse"] is not None:
        ratios["lse"] = CH.check(res["lse"], lse64, b_lse, "row_lse")
    ratios["loss"] = CH.check(res["loss"], loss64, b_lse + U24 * loss64.abs() * CH.SLACK, "row_loss")
    if grad:
        dl = res["dl"]
        ref = CH.lsm_grad(p64, tgt, gs)
        d32 = CH.lsm_grad(p32, tgt, torch.tensor(gs, dtype=F32))
        r = max(4.0 * CH.grad_rel(d32, ref, p64, tgt, gs), 2.0 ** -22)
        ratios["grad"] = CH.check(dl[:, :V], ref, CH.grad_bound(p64, tgt, gs, r), "dlogits")
        ratios["r"] = r / U24
        up = _rup(V) if kernel == "float4" else V
        assert float(dl[:, V:up].abs().max() if up > V else 0.0) == 0.0, "pad columns of dlogits up to round_up(V, 4) must be 0"
        assert bool(torch.isnan(dl[:, up:]).all()), "dlogits written beyond round_up(V, 4)" if kernel == "float4" else "scalar kernel wrote pad columns"
    return ratios


def _mlm_inputs(rows, V, seed):
    torch.manual_seed(seed)
    x = torch.randn(rows, V) * 2
    tgt = torch.randint(0, V, (rows,))
    tgt[0] = 0                       # targets at column 0 and at column V - 1
    if rows > 1:
        tgt[1] = V - 1
    return x, tgt


VOCABS = [1, 3, 4, 5, 4095, 4096, 4097, 16383, 16384, 16385, 30522, 32769]


@pytest.mark.parametrize("pad", [1e30, NAN])
@pytest.mark.parametrize("extra", [0, 8])
@pytest.mark.parametrize("V", VOCABS)
def test_mlm_float4_kernels(V, extra, pad):
    """lsm_stats_kernel + lsm_grad_kernel: ld = round_up(V, 4) (+ 8), pad columns of the logits holding +1e30 or NaN
    (masked to -inf on read), V around one blockIdx.y piece of the gradient kernel (4096) and one sweep of the
    statistics kernel (16384); extra = 8 also takes the device scalar times gscale_mul (0.37 * 0.5: an exact product)"""
    x, tgt = _mlm_inputs(3, V, V + extra)
    gs_dev = torch.tensor([0.37], device=dev()) if extra else None
    mul = 0.5 if extra else 1.0
    gs = float(torch.tensor(0.37, dtype=F32)) * 0.5 if extra else 1.0
    res = run_mlm(x, tgt, "float4", _rup(V) + extra, _rup(V) + extra, pad=pad, gs_dev=gs_dev, mul=mul)
    say(f"mlm float4 V={V} ld=+{extra} pad={pad}", **check_mlm(res, x, tgt, "float4", gs))


@pytest.mark.parametrize("how", ["null_lse", "unaligned"])
@pytest.mark.parametrize("V", VOCABS)
def test_mlm_scalar_kernel(V, how):
    """lsm_nll_kernel, which the Python path never takes (functional._padded always aligns): through row_lse == NULL
    on aligned rows, and through ld = V (odd V, or V % 4 == 2) or a base address 4 bytes past alignment"""
    x, tgt = _mlm_inputs(3, V, 2 * V + 1)
    gs_dev = torch.tensor([0.37], device=dev())
    ld = _rup(V) if how == "null_lse" else V
    res = run_mlm(x, tgt, "scalar", ld, ld, how=how, gs_dev=gs_dev, mul=2.0)
    assert (res["lse"] is None) == (how == "null_lse")
    say(f"mlm scalar V={V} {how}", **check_mlm(res, x, tgt, "scalar", float(torch.tensor(0.37, dtype=F32)) * 2.0))


@pytest.mark.parametrize("V", [5, 4097, 16385, 30522])
def test_mlm_grad_with_a_supplied_lse(V):
    """lsm_grad_kernel on its own: row_lse is the float64 log-sum-exp rounded to fp32, so the reference is exp(x - that
    value) and no error of the statistics kernel takes part; an unaligned dld is refused and writes nothing"""
    x, tgt = _mlm_inputs(3, V, 3 * V)
    lse = CH.lsm_ref(x, tgt, F64)[0].float()
    ld = _rup(V)
    logits = torch.full((3, ld), NAN, device=dev())
    logits[:, :V] = gpu(x)
    dl = nanbuf(3, ld + 4)
    td, ld_ = gpu(tgt), gpu(lse)
    refused(L.lib().mmvqa_mlm_grad(L.stream_ptr(), P(logits), ld, P(td), P(ld_), P(dl), ld + 1, None, 1.0, 3, V), "mlm_grad")
    torch.cuda.synchronize()
    assert bool(torch.isnan(dl).all()), "a refused call wrote"
    L.check(L.lib().mmvqa_mlm_grad(L.stream_ptr(), P(logits), ld, P(td), P(ld_), P(dl), ld + 4, None, 0.25, 3, V))
    torch.cuda.synchronize()
    p64 = CH.lsm_ref(x, tgt, F64, lse=lse)[2]
    p32 = CH.lsm_ref(x, tgt, F32, lse=lse)[2]
    ref, d32 = CH.lsm_grad(p64, tgt, 0.25), CH.lsm_grad(p32, tgt, 0.25)
    r = max(4.0 * CH.grad_rel(d32, ref, p64, tgt, 0.25), 2.0 ** -22)
    got = dl.cpu()
    ratio = CH.check(got[:, :V], ref, CH.grad_bound(p64, tgt, 0.25, r), "dlogits from a supplied lse")
    assert float(got[:, V:ld].abs().max() if ld > V else 0.0) == 0.0 and bool(torch.isnan(got[:, ld:]).all())
    say(f"mlm_grad supplied lse V={V}", grad=ratio, r=r / U24)


TIE_V = 20000


def _tie_rows():
    """the row maximum duplicated: within one float4; in two lanes of one wave; in two waves -- (13, 113, 281): 113 is
    wave 1 of the 256-thread scalar kernel, 281 (float4 70) wave 1 of the statistics kernel; (300, 4100): the LOWER
    index sits in the HIGHER wave of the statistics kernel (float4 75 -> thread 75, float4 1025 -> thread 1); in one
    thread one sweep apart (i, i + 16384: both kernels); at index 0 and V - 1; across a whole row of equal values"""
    ties = [(9, 10), (9, 22), (13, 113, 281), (300, 4100), (77, 77 + 16384), (0, TIE_V - 1), None]
    torch.manual_seed(41)
    x = (torch.randn(len(ties), TIE_V) * 2).clamp(max=4.0)
    for k, t in enumerate(ties):
        if t is None:
            x[k] = 1.25
        else:
            x[k, list(t)] = 6.5
    first = torch.tensor([0 if t is None else min(t) for t in ties])
    return x, first


@pytest.mark.parametrize("kernel,how", [("float4", "aligned"), ("scalar", "null_lse")])
def test_mlm_ties_give_the_first_index(kernel, how):
    x, first = _tie_rows()
    tgt = torch.full((x.shape[0],), 5000)
    res = run_mlm(x, tgt, kernel, TIE_V, TIE_V, how=how)
    assert torch.equal(res["pred"], first), f"{kernel}: pred {res['pred'].tolist()}, lowest indices {first.tolist()}"
    say(f"mlm ties {kernel}", **check_mlm(res, x, tgt, kernel))


@pytest.mark.parametrize("kernel,how", [("float4", "aligned"), ("scalar", "unaligned")])
def test_mlm_rows_with_blocks_of_minus_infinity(kernel, how):
    """columns [1000, 18000) at -inf: thread 300 of the statistics kernel (float4 300, 1324, 2348, 3372, 4396) sees only
    -inf, thread 950 likewise with no second sweep, thread 500 sees -inf in its first sweep and finite values in its
    second (float4 4596).  Row 1 puts the block at the start, so every thread of either kernel starts its running
    maximum from -inf and most threads of the statistics kernel never leave it.  Targets sit on finite columns;
    the gradient of a -inf column is exactly 0."""
    torch.manual_seed(43)
    x = torch.randn(2, TIE_V) * 2
    x[0, 1000:18000] = -math.inf
    x[1, :16500] = -math.inf
    tgt = torch.tensor([0, TIE_V - 1])
    res = run_mlm(x, tgt, kernel, TIE_V, TIE_V, how=how)
    assert float(res["dl"][0, 1000:18000].abs().max()) == 0.0
    say(f"mlm -inf {kernel}", **check_mlm(res, x, tgt, kernel))


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 700])
def test_mlm_out3(rows):
    """mlm_reduce_kernel (one 256-thread workgroup): the two counts exact, the mean a tree over `rows` row losses and a
    division -- (dot_ulps(rows) + 1) 2^-23 mean|row_loss| -- against the float64 mean of the row losses it was given, and,
    with the mean of the rows' own bounds added, against the mean of the float64 row losses"""
    torch.manual_seed(rows)
    V = 5
    x = torch.randn(rows, V) * 2
    tgt = torch.randint(0, V, (rows,))
    tgt[::3] = x[::3].argmax(-1)          # a third of the rows predicted right, some of them with target 0 (not counted)
    res = run_mlm(x, tgt, "float4", 8, 8, out3=True)
    pred = CH.lsm_ref(x, tgt, F64)[3]
    assert torch.equal(res["pred"], pred)
    nm, nc = int((tgt > 0).sum()), int(((tgt > 0) & (pred == tgt)).sum())
    assert res["out3"][1:].tolist() == [float(nm), float(nc)]
    rl = res["loss"].double()
    b_red = (dot_ulps(rows) + 1) * U23 * rl.abs().mean()
    ratio = CH.check(res["out3"][0], rl.mean(), b_red, "out3 mean of the row losses it was given")
    lse64, loss64 = CH.lsm_ref(x, tgt, F64)[:2]
    b_rows = CH.bound_4x(lse64, CH.lsm_ref(x, tgt, F32)[0]) + U24 * loss64.abs() * CH.SLACK     # as check_mlm bounds a row loss
    ratio64 = CH.check(res["out3"][0], loss64.mean(), b_rows.mean() + b_red, "out3 mean against the float64 mean")
    say(f"mlm out3 rows={rows}", mean=ratio, mean64=ratio64)


# ----------------------------------------------------------------------------- ASL
@pytest.mark.parametrize("gp,gn,eps", [(0, 4, 0.1), (1, 4, 0.1), (0, 0, 0), (2, 1, 0.05)])
@pytest.mark.parametrize("Cc", [2, 5, 255, 256, 257, 1000])
def test_asl(Cc, gp, gn, eps):
    """row loss under the 4x rule (one segment: the rows are of one magnitude); every gradient element relative to its
    probability as for the log-softmax, the target's relative to max(p_t, |ref_t| / gs) (chain_helpers.grad_bound);
    logits of std 1.5 keep every probability away from 0 and 1; ld > C, gscale = 0.3"""
    torch.manual_seed(100 * Cc + gp)
    rows, ld, dld = 5, Cc + 3, Cc + 1
    x = torch.randn(rows, Cc) * 1.5
    tgt = torch.randint(0, Cc, (rows,))
    tgt[0], tgt[1] = 0, Cc - 1
    gs = float(torch.tensor(0.3, dtype=F32))
    logits = torch.full((rows, ld), 1e30, device=dev())
    logits[:, :Cc] = gpu(x)
    dl, row_loss, td = nanbuf(rows, dld), nanbuf(rows), gpu(tgt)
    L.check(L.lib().mmvqa_asl_loss(L.stream_ptr(), P(logits), ld, P(td), P(row_loss), P(dl), dld, rows, Cc, float(gp), float(gn), eps, gs))
    torch.cuda.synchronize()
    l64, d64, p64 = CH.asl_rows(x, tgt, gp, gn, eps, F64)
    l32, d32, _ = CH.asl_rows(x, tgt, gp, gn, eps, F32)
    assert float(p64.min()) > 1e-30 and float(p64.max()) < 1 - 1e-6
    rl = CH.check(row_loss, l64, CH.bound_4x(l64, l32), "asl row loss")
    ref = d64 * gs
    ar = torch.arange(rows)
    tscale = torch.maximum(p64[ar, tgt], ref[ar, tgt].abs() / gs)
    r = max(4.0 * CH.grad_rel(d32 * torch.tensor(gs, dtype=F32), ref, p64, tgt, gs, tscale), 2.0 ** -22)
    got = dl.cpu()
    rg = CH.check(got[:, :Cc], ref, CH.grad_bound(p64, tgt, gs, r, tscale), "asl dlogits")
    assert bool(torch.isnan(got[:, Cc:]).all()), "asl wrote a pad column"
    say(f"asl C={Cc} gamma=({gp},{gn}) eps={eps}", loss=rl, grad=rg, r=r / U24)


# ----------------------------------------------------------------------------- Adam
LR, B1, B2, AEPS = 1e-3, 0.9, 0.999, 1e-8


def _adam_n(cap):
    """float4 count 2 * stride * 3 + stride + 77 for a grid of `cap` workgroups: three unrolled iterations for every
    thread, one full sweep of the tail loop and a ragged one"""
    stride = 256 * cap
    return 4 * (2 * stride * 3 + stride + 77)


def _adam_run(n, gscale, zero_grad, splits=None, verify=False):
    """three steps from one seeded state; with `verify` every step is compared with one float64 step from the fp32
    state the kernel started it from.  Returns final (p, m, v) on the CPU and the worst ratios."""
    gen = torch.Generator().manual_seed(1234)
    p = gpu(torch.randn(n, generator=gen))
    m, v = torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    worst = dict(p=0.0, m=0.0, v=0.0)
    cuts = [0, n] if splits is None else splits
    for step in (1, 2, 3):
        g0 = torch.randn(n, generator=gen) * 3 / gscale * (0.01 if step == 3 else 1.0)
        g = gpu(g0)
        p0, m0, v0 = p.cpu(), m.cpu(), v.cpu()
        for a, b in zip(cuts[:-1], cuts[1:]):
            L.check(L.lib().mmvqa_adam(L.stream_ptr(), P(p) + 4 * a, P(g) + 4 * a, P(m) + 4 * a, P(v) + 4 * a, b - a, LR, B1, B2, AEPS,
                                       step, gscale, zero_grad))
        torch.cuda.synchronize()
        if zero_grad:
            assert torch.equal(g.cpu(), torch.zeros(n)), "zero_grad = 1 must leave g exactly zero"
        else:
            assert CH.same_bits(g, g0), "zero_grad = 0 must leave g untouched"
        if verify:
            p1, m1, v1 = CH.adam_ref(p0, g0, m0, v0, step, LR, B1, B2, AEPS, gscale, F64)
            bp, bm, bv = CH.adam_bounds(p0, g0, m0, v0, step, LR, B1, B2, AEPS, gscale)
            worst["m"] = max(worst["m"], CH.check(m, m1, bm, f"adam m step {step}"))
            worst["v"] = max(worst["v"], CH.check(v, v1, bv, f"adam v step {step}"))
            worst["p"] = max(worst["p"], CH.check(p, p1, bp, f"adam p step {step}"))
    return (p.cpu(), m.cpu(), v.cpu()), worst


@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("gscale", [1.0, 1.0 / 1024])
@pytest.mark.parametrize("cap,n", [("1", _adam_n(1)), ("2", _adam_n(2)), (None, 4), (None, 4104)])
def test_adam(monkeypatch, cap, n, gscale, zero_grad):
    """p, m, v of each of three steps against one float64 torch.optim.Adam step (chain_helpers.adam_ref, checked against
    the optimizer on the CPU) from the state the step started from.  Roundings of `upd`, u = 2^-24 (adam_bounds):
    m: 4 -> u (|m'| + omb1 (|g'| + 2 |g' - m|));  v: 7 -> u (4 g'^2 omb2 + 2 v b2 + v') <= 5 u v';
    p: u |p'| + step_size (dm / denom + |m' / denom| (dv / (2 v') + 7 u)) <= u |p'| + step_size (dm / denom + 9.5 u |q|).
    MMVQA_ADAM_WGS = 1 / 2 makes the grid smaller than the float4 count, so the unrolled non-temporal loop runs (with the
    default cap and n = 4 or 4104 only the tail loop does)."""
    if cap is None:
        monkeypatch.delenv("MMVQA_ADAM_WGS", raising=False)
    else:
        monkeypatch.setenv("MMVQA_ADAM_WGS", cap)
    _, worst = _adam_run(n, gscale, zero_grad, verify=True)
    say(f"adam cap={cap} n={n} gscale={gscale} zero_grad={zero_grad}", **worst)


def test_adam_launch_shapes_are_bit_identical(monkeypatch):
    """one launch, the same range split at 4-aligned offsets into three launches, and workgroup caps 1, 2 and the
    default reach an element through different loops of different launches: p, m, v must agree bit for bit"""
    n = _adam_n(2)
    runs = {}
    for name, cap, splits in (("default", None, None), ("cap 1", "1", None), ("cap 2", "2", None), ("cap 2, three launches", "2", [0, 1000, 5004, n]),
                              ("default, three launches", None, [0, 4, 9000, n])):
        if cap is None:
            monkeypatch.delenv("MMVQA_ADAM_WGS", raising=False)
        else:
            monkeypatch.setenv("MMVQA_ADAM_WGS", cap)
        runs[name] = _adam_run(n, 1.0 / 1024, 0, splits=splits)[0]
    for name, got in runs.items():
        for k, what in enumerate("pmv"):
            assert CH.same_bits(got[k], runs["default"][k]), f"{what} of '{name}' differs from the single default launch"


def test_adam_refuses_a_length_that_is_no_multiple_of_4():
    t = nanbuf(8)
    refused(L.lib().mmvqa_adam(L.stream_ptr(), P(t), P(t), P(t), P(t), 6, LR, B1, B2, AEPS, 1, 1.0, 0), "adam")
    torch.cuda.synchronize()
    assert bool(torch.isnan(t).all())


# ----------------------------------------------------------------------------- colsum, axpy
@pytest.mark.parametrize("wide", [0, 3])
@pytest.mark.parametrize("cols", [1, 255, 256, 257, 600])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 130])
def test_colsum(rows, cols, wide):
    """out[c] += sum_r x[r][c] onto a pre-filled out (chain_helpers.colsum_bound); one magnitude per 64-row block (4, 1,
    0.25), so that a dropped block or a dropped row is far outside the bound; the columns
    of x beyond `cols` (ld = cols + 3) hold NaN and the entries of out beyond `cols` stay untouched"""
    torch.manual_seed(rows * 1000 + cols)
    ld = cols + wide
    x = torch.randn(rows, cols) * torch.tensor([4.0, 1.0, 0.25])[(torch.arange(rows) // 64) % 3][:, None]
    xb = torch.full((rows, ld), NAN)
    xb[:, :cols] = x
    prior = torch.randn(cols + 5)
    xd, out = gpu(xb), gpu(prior)
    L.check(L.lib().mmvqa_colsum(L.stream_ptr(), P(xd), ld, rows, cols, P(out)))
    torch.cuda.synchronize()
    got = out.cpu()
    ratio = CH.check(got[:cols], prior[:cols].double() + x.double().sum(0), CH.colsum_bound(x, prior[:cols], rows), "colsum")
    assert torch.equal(got[cols:], prior[cols:]), "colsum wrote beyond cols"
    say(f"colsum rows={rows} cols={cols} ld=+{wide}", out=ratio)


@pytest.mark.parametrize("a", [1.0, -0.37])
@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 256 + 37])
def test_axpy(n, a):
    """y += a * x: at most two roundings per element (chain_helpers.axpy_bound); n past the 2048-workgroup cap of the
    grid takes the grid-stride loop; the element after the last stays untouched"""
    torch.manual_seed(n)
    x, y0 = torch.randn(n), torch.randn(n + 1)
    a32 = float(torch.tensor(a, dtype=F32))
    xd, y = gpu(x), gpu(y0)
    L.check(L.lib().mmvqa_axpy(L.stream_ptr(), P(y), P(xd), a, n))
    torch.cuda.synchronize()
    got = y.cpu()
    ratio = CH.check(got[:n], y0[:n].double() + a32 * x.double(), CH.axpy_bound(y0[:n], x, a32), "axpy")
    assert float(got[n]) == float(y0[n])
    say(f"axpy n={n} a={a}", y=ratio)


# ----------------------------------------------------------------------------- BatchNorm backward coefficients
@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("slots", [1, 4, 16])
@pytest.mark.parametrize("Cc", [1, 15, 16, 17, 72])
def test_bn_coef_bwd(Cc, slots, training):
    """P, Q, R of dz = P g + Q z + R one by one (chain_helpers.bn_pqr_bounds: double arithmetic, one rounding to float,
    a floor for R's cancellation), dgamma / dbeta accumulated onto pre-filled buffers, and -- in training mode -- the
    kernel's P, Q, R applied on the host in float64 to (g, z) against nn.BatchNorm2d's autograd input gradient in
    float64.  z is mean_c +- a_c with a_c a power of two, balanced signs and an eps that vanishes in float64, so that the mean and invstd the
    kernel is given in fp32 are the exact batch statistics and xhat = +-1: no input rounding enters the comparison.
    C around the 16 channels of a workgroup; the sums scattered over 1, 4 and 16 statistic replicas."""
    torch.manual_seed(17 * Cc + slots)
    N, Hh, Ww = 4, 2, 2
    count = N * Hh * Ww
    mean = torch.randint(-16, 17, (Cc,)).double() / 8
    a = 2.0 ** torch.randint(-1, 2, (Cc,)).double()
    sign = torch.stack([torch.cat([torch.ones(count // 2), -torch.ones(count // 2)])[torch.randperm(count)] for _ in range(Cc)], 1).double()
    z = (mean[None] + a[None] * sign).view(N, Hh, Ww, Cc).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    gamma = (torch.rand(Cc) + 0.5).double()
    G = torch.randn(N, Cc, Hh, Ww, dtype=F64)
    invstd = 1.0 / a
    xhat = (z.detach() - mean[None, :, None, None]) * invstd[None, :, None, None]
    assert bool((xhat.abs() == 1).all())
    st = CH.spread(torch.stack([G.sum((0, 2, 3)), (G * xhat).sum((0, 2, 3))], 1), slots, L.STAT_SLOTS)
    sg, sgx = st.sum(0)[:, 0], st.sum(0)[:, 1]                      # what the replicas really add up to
    std, gd, md, isd = gpu(st), gpu(gamma.float()), gpu(mean.float()), gpu(invstd.float())
    pqr = [nanbuf(Cc) for _ in range(3)]
    dg0, db0 = torch.randn(Cc) * 2, torch.randn(Cc) * 2
    dg, db = gpu(dg0), gpu(db0)
    L.check(L.lib().mmvqa_bn_coef_bwd(L.stream_ptr(), P(std), Cc, float(count), P(gd), P(md), P(isd), training,
                                      P(pqr[0]), P(pqr[1]), P(pqr[2]), P(dg), P(db)))
    torch.cuda.synchronize()
    ref = CH.bn_pqr(sg, sgx, count, gamma, mean, invstd, training)
    bnd = CH.bn_pqr_bounds(sg, sgx, count, gamma, mean, invstd, training)
    ratios = {}
    for k, name in enumerate("PQR"):
        if training or k == 0:
            ratios[name] = CH.check(pqr[k], ref[k], bnd[k] + 1e-300, name)
        else:
            assert float(pqr[k].abs().max()) == 0.0, f"eval mode: {name} must be 0"
    ratios["dgamma"] = CH.check(dg, dg0.double() + sgx, CH.bn_acc_bound(sgx, dg0), "bn dgamma")
    ratios["dbeta"] = CH.check(db, db0.double() + sg, CH.bn_acc_bound(sg, db0), "bn dbeta")
    if training:
        bn = torch.nn.BatchNorm2d(Cc, eps=1e-300).double().train()    # var + 1e-300 == var in float64
        with torch.no_grad():
            bn.weight.copy_(gamma)
        bn(z).backward(G)
        e = lambda t: t.double().cpu()[None, :, None, None]
        zz = z.detach()
        dz = e(pqr[0]) * G + e(pqr[1]) * zz + e(pqr[2])
        mag = e(ref[0]).abs() * G.abs() + e(ref[1]).abs() * zz.abs() + e(ref[2]).abs()
        bound = e(bnd[0]) * G.abs() + e(bnd[1]) * zz.abs() + e(bnd[2]) + 1e-12 * mag + 1e-300
        ratios["dz"] = CH.check(dz, z.grad, bound, "dz = P g + Q z + R against BatchNorm2d's autograd")
    say(f"bn_coef_bwd C={Cc} slots={slots} training={training}", **ratios)
