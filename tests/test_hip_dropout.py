"""Training-mode dropout of every kernel that draws from the dropout stream, through the C ABI, against references that
apply the SAME masks (dropout_helpers restates common.h's hash on the host; DESIGN.md, "Dropout stream").  With the mask
known each op is deterministic: a dropped element must be exactly 0 (exactly R where a residual follows), a kept one is
held to the bound of the dropout-free test of the op."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hip_helpers import *  # noqa: E402,F401,F403
from oracle import mmbert_oracle as O  # noqa: E402
from dropout_helpers import SiteDropout, engine_seed, inject_dropout, keep_tensor, site_seed  # noqa: E402

TOL = 1e-4
SEED = site_seed(engine_seed(11), 1, 2)   # what the engine hands a kernel: some site of some step


def exactly(a, b):
    """same bits (distinguishes -0.0 from 0.0, equates NaN with itself)"""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ----------------------------------------------------------------------------- elementwise kernels
@pytest.mark.parametrize("p", [0.1, 0.3])
@pytest.mark.parametrize("n", [1, 255, 1027, 2 * 524288 + 37])   # the last: more than grid_for's 2048 x 256 threads
def test_dropout_elementwise(n, p):
    """mmvqa_dropout (in place) and mmvqa_dropout_copy (what the engine's backward runs at four sites)"""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    x = torch.where(x.abs() < 1e-3, torch.ones_like(x), x)   # no zeros: the kept set can be read off the output
    keep = keep_tensor(SEED, (n,), p)
    ks = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    want = torch.where(keep, x * torch.tensor(ks), torch.zeros_like(x))   # fp32 product, as the kernels form it
    xd = x.to(dev())
    y = xd.clone()
    L.check(L.lib().mmvqa_dropout(L.stream_ptr(), P(y), n, p, SEED))
    out = torch.full((n,), float("nan"), device=dev())
    L.check(L.lib().mmvqa_dropout_copy(L.stream_ptr(), P(xd), P(out), n, p, SEED))
    torch.cuda.synchronize()
    assert exactly(xd.cpu(), x), "dropout_copy changed its input"
    for what, got in (("dropout", y.cpu()), ("dropout_copy", out.cpu())):
        assert torch.equal(got != 0, keep), f"{what}: kept set differs from keep_mask"
        assert exactly(got[~keep], torch.zeros(int((~keep).sum()))), f"{what}: a dropped element is not 0.0"
        ulps = (got[keep].view(torch.int32).long() - want[keep].view(torch.int32).long()).abs()
        assert int(ulps.max()) <= 1 if ulps.numel() else True, f"{what}: kept value {int(ulps.max())} ulps off"


# ----------------------------------------------------------------------------- igemm forward epilogue
# y = dropout(act(x W^T + b)) + R, Cpre = x W^T + b.  Bound of a kept element, in units of 2^-23:
#   u = x W^T + b: dot_ulps(K) of |x| |W|^T for the product, one rounding for the bias;
#   act: |act'| <= LIP, plus the kernel's own approximation error.  SERF: 2e-6 (1 + |u|), as in test_hip_igemm_fused.py.
#     GELU = u/2 (1 + erff(u / sqrt 2)): argument rounding, erff (<= 2 ulp of 1) and the sum cost < 5e-7 absolute on
#     1 + erf, two products 2^-23 relative: inside the same 2e-6 (1 + |u|).  Measured on an MI355X, the epilogue's
#     activation of its own fp32 Cpre against fp64 of that value, |u| up to 16: GELU 4.5e-7 absolute, 8.1e-8 (1 + |u|);
#     SERF 8.7e-7 absolute, 3.0e-7 (1 + |u|);
#   keep scale 1/(1-p) in fp32 and its product: 2 roundings of |act(u)| / (1-p) <= |u| / (1-p); + R: 1 rounding of the sum.
# As one magnitude for assert_gemm_close: c = dot_ulps(K) + 4 on (LIP (|x| |W|^T + |b|) + act_err / (c 2^-23)) / (1-p) + |R|.
LIP = {"none": 1.0, "gelu": 1.13, "serf": 1.1}
ACTS = {"none": L.ACT_NONE, "gelu": L.ACT_GELU, "serf": L.ACT_SERF}
DROP_P = 0.3


def act64(act, u):
    return {"none": lambda t: t, "gelu": O.gelu, "serf": O.serf}[act](u)


def act_err(act, u):
    return torch.zeros_like(u) if act == "none" else 2e-6 * (1.0 + u.abs())


@functools.lru_cache(maxsize=None)
def linear_case(M, K, N, f16=False):
    """inputs of one shape and the fp64 pre-activation, computed once and shared by its tile / act / split-K cases"""
    g = torch.Generator().manual_seed(M * 7 + K * 3 + N)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
    b, r = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    x64, w64 = (x.half().double(), w.half().double()) if f16 else (x.double(), w.double())
    u = x64 @ w64.T + b.double()
    umag = x64.abs() @ w64.abs().T + b.double().abs()
    keep = keep_tensor(SEED, (M, N), DROP_P)      # index row * N + col: N, not the leading dimension of C
    return (x, w, b, r), u, umag, keep


def run_linear(case, act, tile, prec=L.PREC_F32, splitk=0, ws=None, cnt=None):
    (x, w, b, r), _, _, _ = case
    M, K, N = x.shape[0], x.shape[1], w.shape[0]
    xd, wd, bd, rd = (t.to(dev()) for t in (x, w, b, r))
    ldy = (N + 3) & ~3
    y = torch.full((M, ldy), float("nan"), device=dev())
    pre = torch.full((M, ldy), float("nan"), device=dev())
    d = L.GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.A, d.a_ld, d.g_Cs = P(xd), K, K
    d.B, d.b_ld = P(wd), K
    linear_geom(d)
    d.C, d.c_ld, d.Cpre, d.bias, d.act = P(y), ldy, P(pre), P(bd), ACTS[act]
    d.drop_p, d.drop_seed = DROP_P, SEED
    d.R, d.r_ld = P(rd), N
    d.reserved0 = prec
    if splitk:
        d.splitk, d.sk_ws, d.sk_ws_floats = splitk, P(ws), ws.numel() - 16
        if cnt is not None:
            d.sk_cnt, d.sk_cnt_n = P(cnt), cnt.numel()
    run_igemm(d, L.KIND_FWD, 0, tile)
    return y[:, :N].cpu(), pre[:, :N].cpu()


def check_linear(case, act, y, pre, what):
    (x, w, b, r), u, umag, keep = case
    K = x.shape[1]
    scale = 1.0 / (1.0 - DROP_P)
    c = dot_ulps(K) + 4
    assert_gemm_close(pre, u, umag, dot_ulps(K) + 1, what + " Cpre (no dropout)", TOL)
    assert exactly(y[~keep], r[~keep]), f"{what}: a dropped element is not exactly R"
    ref = act64(act, u) * keep.double() * scale + r.double()
    mag = (LIP[act] * umag + act_err(act, u) / (c * U23)) * scale + r.double().abs()
    mag = torch.where(keep, mag, r.double().abs())
    assert_gemm_close(y, ref, mag, c, what, TOL)


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("M,K,N", [(70, 96, 50), (130, 64, 130), (33, 100, 257)])
def test_igemm_dropout_epilogue(M, K, N, tile):
    """+bias -> Cpre -> act -> dropout -> +R in every tile variant: ragged rows, N % 4 != 0, c_ld != N"""
    case = linear_case(M, K, N)
    for act in ("none", "gelu", "serf"):
        y, pre = run_linear(case, act, tile)
        check_linear(case, act, y, pre, f"M={M} K={K} N={N} {act} tile {tile}")


@pytest.mark.parametrize("ticket", [False, True])
@pytest.mark.parametrize("splitk", [2, 3])
@pytest.mark.parametrize("tile", [3, 5, 6])
def test_igemm_dropout_epilogue_split_k(tile, splitk, ticket):
    """few tiles and a long contraction: the epilogue runs in the finishing launch, or (with tickets) in the last
    workgroup of a tile to arrive -- on the summed partial tiles, with the same mask as the single launch"""
    M, K, N = 98, 768, 72
    case = linear_case(M, K, N)
    pad = ((M + 63) // 64) * ((N + 63) // 64) * 4096   # the ticketed form keeps whole tiles
    part = splitk * (pad if ticket else M * N)    # what `splitk` partial results occupy in the form the case names
    ws = torch.empty(part + 16, device=dev())
    cnt = torch.zeros(256, dtype=torch.int32, device=dev()) if ticket else None
    for act in ("none", "gelu"):
        what = f"{act} tile {tile} splitk {splitk} ticket {ticket}"
        y1, pre1 = run_linear(case, act, tile)
        ws.fill_(float("nan"))
        y, pre = run_linear(case, act, tile, splitk=splitk, ws=ws, cnt=cnt)
        # the launcher may lower the split or fall back to the finishing launch without saying so: either leaves a part
        # of the scratch unwritten (the finishing form keeps M * N floats per split, the ticketed one whole tiles)
        written = ~torch.isnan(ws.cpu())
        assert bool(written[:part].all()), what + f": {int((~written[:part]).sum())} of {part} partial floats unwritten"
        assert not bool(written[part:].any()), what + ": wrote past the partial results"
        if ticket:
            assert int(cnt.abs().sum()) == 0, "tickets not back at zero"
        assert_close(y, y1, 1e-5, what + ": split vs single launch")
        assert_close(pre, pre1, 1e-5, what + ": Cpre split vs single launch")
        assert torch.equal(y == case[0][3], y1 == case[0][3]), what + ": another mask than the single launch"
        check_linear(case, act, y, pre, what)


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 6])
def test_igemm_dropout_epilogue_f16(tile):
    """the f16-operand family shares the fp32 epilogue: reference from the .half()-rounded operands"""
    M, K, N = 130, 64, 130
    case = linear_case(M, K, N, f16=True)
    for act in ("none", "gelu", "serf"):
        y, pre = run_linear(case, act, tile, prec=L.PREC_F16)
        check_linear(case, act, y, pre, f"f16 {act} tile {tile}")


# ----------------------------------------------------------------------------- attention
def attention_reference(qkv, mask, B, T, heads, D, p, seed, dtype):
    """models/transformer.py:19-30 with the kernel's mask on the softmax output; returns (probs before dropout, ctx)"""
    H = heads * D
    q, k, v = (qkv[:, i * H:(i + 1) * H].to(dtype).view(B, T, heads, D).transpose(1, 2) for i in range(3))
    sc = q @ k.transpose(-2, -1) / float(math.sqrt(D))
    sc = sc - 10000.0 * (1.0 - mask[:, None, None, :].to(dtype))
    pr = F.softmax(sc, dim=-1)
    keep = keep_tensor(seed, (B, heads, T, T), p).to(dtype)   # index ((b*heads + head)*T + query)*T + key
    ctx = ((pr * keep / (1.0 - p)) @ v).transpose(1, 2).contiguous().view(B * T, H)
    return pr, ctx


# (T <= 32: single-tile kernels with the hoisted mask; 40, 75, 128: two, three and four key tiles.)  Every case holds the
# 1e-4 of test_attention_bert against the fp64 reference; measured on an MI355X over the six cases, as a fraction of the
# tensor's maximum: probs 2.0e-7 .. 5.7e-7, ctx 1.5e-7 .. 5.6e-7, dqkv 1.5e-7 .. 4.8e-7 (the test prints them).
@pytest.mark.parametrize("B,T,heads,D", [(3, 10, 12, 8), (2, 28, 12, 64), (2, 32, 12, 64), (2, 40, 4, 64),
                                         (1, 75, 2, 64), (1, 128, 2, 64)])
def test_attention_bert_dropout(B, T, heads, D):
    """forward and both passes of the backward kernel regenerate one query-major mask; the saved probabilities are
    key-major and hold the values from before dropout.  Reference: torch autograd in fp64 under the same mask"""
    torch.manual_seed(9)
    p, H = 0.3, heads * D
    qkv = torch.randn(B * T, 3 * H)
    q64 = qkv.double().requires_grad_(True)
    mask = torch.ones(B, T, dtype=torch.long)
    for b in range(B):
        mask[b, T - 2 * b - 1:] = 0
    dctx = torch.randn(B * T, H)
    pr64, ctx64 = attention_reference(q64, mask, B, T, heads, D, p, SEED, torch.float64)
    ctx64.backward(dctx.double())
    qd, md = qkv.to(dev()), mask.to(dev())
    ctx = torch.full((B * T, H), float("nan"), device=dev())
    probs = torch.full((B, heads, T, T), float("nan"), device=dev())
    a = L.AttnDesc()
    a.q, a.k, a.v = P(qd), P(qd) + 4 * H, P(qd) + 8 * H
    a.row_stride, a.head_stride = 3 * H, D
    a.out, a.out_row_stride, a.out_head_stride = P(ctx), H, D
    a.mask, a.mask_on_query, a.probs = P(md), 0, P(probs)
    a.B, a.T, a.heads, a.sqrt_d, a.drop_p, a.seed = B, T, heads, math.sqrt(D), p, SEED
    L.check(L.lib().mmvqa_attention(C.byref(a), D, 0, L.stream_ptr()))
    torch.cuda.synchronize()
    dqkv = torch.full((B * T, 3 * H), float("nan"), device=dev())
    dctxd = dctx.to(dev())
    a.dout, a.dq, a.dk, a.dv = P(dctxd), P(dqkv), P(dqkv) + 4 * H, P(dqkv) + 8 * H
    L.check(L.lib().mmvqa_attention(C.byref(a), D, 1, L.stream_ptr()))
    torch.cuda.synchronize()
    print(f"kernel vs fp64: probs {relerr(probs.transpose(-1, -2), pr64):.2e} ctx {relerr(ctx, ctx64):.2e} "
          f"dqkv {relerr(dqkv, q64.grad):.2e}")
    assert_close(probs.transpose(-1, -2), pr64, TOL, "probs (before dropout, key-major)")
    assert_close(ctx, ctx64, TOL, "ctx")
    assert_close(dqkv, q64.grad, TOL, "dqkv")


@pytest.mark.parametrize("B,T,heads", [(3, 28, 12), (2, 10, 2)])
def test_fused_qkv_attention_dropout(B, T, heads):
    """mmvqa_qkv_attention_fwd under dropout against the masked torch reference itself"""
    torch.manual_seed(31)
    p, D = 0.3, 64
    H = heads * D
    xn = torch.randn(B * T, H)
    W = torch.randn(3 * H, H) / math.sqrt(H)
    bias = torch.randn(3 * H) * 0.1
    mask = torch.ones(B, T, dtype=torch.long)
    for b in range(B):
        mask[b, max(1, T - 2 * (b % 5) - 1):] = 0
    qkv_ref = xn.double() @ W.double().t() + bias.double()
    pr, ctx_ref = attention_reference(qkv_ref, mask, B, T, heads, D, p, SEED, torch.float64)
    xd, Wd, bd, md = xn.to(dev()), W.to(dev()), bias.to(dev()), mask.to(dev())
    qkv = torch.full((B * T, 3 * H), float("nan"), device=dev())
    probs = torch.full((B, heads, T, T), float("nan"), device=dev())
    ctx = torch.full((B * T, H), float("nan"), device=dev())
    L.check(L.lib().mmvqa_qkv_attention_fwd(L.stream_ptr(), P(xd), P(Wd), P(bd), P(md), P(qkv), P(probs), P(ctx), B, T, H,
                                            heads, p, SEED))
    torch.cuda.synchronize()
    assert_close(qkv, qkv_ref, TOL, "q|k|v")
    assert_close(probs.transpose(-1, -2), pr, TOL, "probs (before dropout)")
    assert_close(ctx, ctx_ref, TOL, "ctx")


# ----------------------------------------------------------------------------- embeddings
def test_embed_dropout():
    """text rows are dropped with site (100, 0)'s mask over [B, T, H]; visual-token rows are not, in either direction"""
    torch.manual_seed(8)
    B, T, H, V, nv = 3, 12, 96, 40, 5
    p, base = 0.1, engine_seed(11)
    seed = site_seed(base, 100, 0)
    emb = inject_dropout(O.OracleBertEmbeddings(V, H, 32, hidden_dropout_prob=p), base).train()
    assert isinstance(emb.dropout, SiteDropout)
    ids = torch.randint(0, V, (B, T))
    ids[:, 1:6] = 0
    seg = torch.randint(0, 2, (B, T))
    vis = torch.randn(nv, B, H, requires_grad=True)
    h = emb(ids, seg).clone()
    for n in range(nv):
        h[:, n, :] = vis[n]
    dh = torch.randn(B, T, H)
    h.backward(dh)
    keep = keep_tensor(seed, (B, T, H), p)
    sd = {k: v.detach().to(dev()) for k, v in emb.state_dict().items()}
    out, xh = torch.full((B * T, H), float("nan"), device=dev()), torch.full((B * T, H), float("nan"), device=dev())
    rstd = torch.zeros(B * T, device=dev())
    idsd, segd, visd = ids.to(dev()), seg.to(dev()), vis.detach().to(dev())
    L.check(L.lib().mmvqa_embed_fwd(L.stream_ptr(), P(idsd), P(segd), P(sd["word_embeddings.weight"]),
                                    P(sd["position_embeddings.weight"]), P(sd["token_type_embeddings.weight"]),
                                    P(sd["LayerNorm.weight"]), P(sd["LayerNorm.bias"]), P(visd), P(out), P(xh), P(rstd),
                                    B, T, H, nv, 1e-12, p, seed))
    torch.cuda.synchronize()
    o = out.view(B, T, H).cpu()
    assert exactly(o[:, :nv], vis.detach().transpose(0, 1)), "visual rows are not the visual tokens"
    text, kt = o[:, nv:], keep[:, nv:]
    assert exactly(text[~kt], torch.zeros(int((~kt).sum()))), "a dropped text element is not 0.0"
    assert int((text == 0).sum()) == int((~kt).sum()), "kept set of the text rows differs from keep_mask"
    assert_close(text, h.detach()[:, nv:], TOL, "embed fwd, text rows")
    dw, dp, dt = (torch.zeros_like(sd[k]) for k in ("word_embeddings.weight", "position_embeddings.weight",
                                                     "token_type_embeddings.weight"))
    dg, db = torch.zeros(H, device=dev()), torch.zeros(H, device=dev())
    dvis = torch.full((nv, B, H), float("nan"), device=dev())
    dhd = dh.to(dev())
    L.check(L.lib().mmvqa_embed_bwd(L.stream_ptr(), P(dhd), P(idsd), P(segd), P(xh), P(rstd),
                                    P(sd["LayerNorm.weight"]), P(dw), P(dp), P(dt), P(dg), P(db), P(dvis), B, T, H, nv,
                                    p, seed, 0))
    torch.cuda.synchronize()
    assert exactly(dvis.cpu(), dh[:, :nv].transpose(0, 1)), "dvis is not the incoming gradient (dropout applied?)"
    assert_close(dvis, vis.grad, 1e-6, "dvis")
    assert_close(dw, emb.word_embeddings.weight.grad, TOL, "dword")
    assert torch.all(dw[0] == 0)  # padding_idx row
    assert_close(dp, emb.position_embeddings.weight.grad, TOL, "dpos")
    assert_close(dt, emb.token_type_embeddings.weight.grad, TOL, "dtype")
    assert_close(dg, emb.LayerNorm.weight.grad, TOL, "dgamma")
    assert_close(db, emb.LayerNorm.bias.grad, TOL, "dbeta")
