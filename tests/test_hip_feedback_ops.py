"""Op-level GPU tests of csrc/fbattn.hip through the C ABI: window attention against the growing memory, the layer-weighted
aggregation of a window's hiddens, GEGLU -- forward and backward, each against torch in fp64 on the same inputs.

Bounds.  The probabilities, and everything formed from them, are held to assert_close at 1e-5 (relative to the tensor's
maximum).  On top of that every element is held to its own bound, built from hip_helpers.dot_ulps for the dot products and
propagated through the softmax as written at `attn_bounds` (a first-order forward error analysis: no measured number
enters it)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmvqa_amd import _lib as L  # noqa: E402
from hip_helpers import P, U23, assert_close, assert_within, dev, dot_ulps, relerr  # noqa: E402
from dropout_helpers import rng_uniform  # noqa: E402

HEADS, DH, SEED = 8, 64, 0x1234567
TOL = 1e-5


# ----------------------------------------------------------------------------- window attention
def attn_inputs(B, n_mem, n, T, seed=3):
    g = torch.Generator().manual_seed(seed + n_mem * 7 + n)
    nw = n_mem // 2
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    return dict(q=r(B * n, 512), mem=r(max(nw, 1), 2 * B, 1024), selfkv=r(2 * B, 1024), bias=r(32, HEADS),
                dout=r(B * n, 512), dmem0=r(max(nw, 1) + 1, 2 * B, 1024), dbias0=r(32, HEADS), B=B, n=n, n_mem=n_mem, T=T)


def gather_kv(t, B, n_mem, n, selfkv):
    """[B, heads, keys, 64] keys and values in the order the reference concatenates them: memory (oldest first), then self"""
    mem = t[:n_mem // 2] if n_mem else t[:0]
    rows = mem.reshape(-1, B, 2, 1024).permute(1, 0, 2, 3).reshape(B, n_mem, 1024)       # [b][j = 2w + i]
    if n == 2:
        rows = torch.cat((rows, selfkv.view(B, 2, 1024)), 1)
    k, v = rows[..., :512], rows[..., 512:]
    return tuple(x.reshape(B, -1, HEADS, DH).transpose(1, 2) for x in (k, v))


def keep_scaled(B, n_mem, n, J, T, p):
    if p == 0.0:
        return torch.ones(B, HEADS, n, J, dtype=torch.float64)
    b, h, i, j = np.meshgrid(np.arange(B), np.arange(HEADS), np.arange(n), np.arange(J), indexing="ij")
    idx = ((b * HEADS + h) * T + n_mem + i) * T + j
    return torch.from_numpy((rng_uniform(SEED, idx.astype(np.uint32)) >= np.float32(p)).astype(np.float64) / (1.0 - p))


def attn_reference(x, p):
    """fp64 autograd restatement on leaves q, mem, selfkv, bias"""
    B, n, n_mem, T = x["B"], x["n"], x["n_mem"], x["T"]
    lv = {k: x[k].double().requires_grad_(True) for k in ("q", "mem", "selfkv", "bias")}
    k, v = gather_kv(lv["mem"], B, n_mem, n, lv["selfkv"])
    q = lv["q"].view(B, n, HEADS, DH).transpose(1, 2)
    J = k.shape[2]
    sim = (q @ k.transpose(-1, -2)) * DH ** -0.5
    bucket = (torch.arange(n)[:, None] - torch.arange(J)[None, :]).clamp_min(0)
    sim = sim + lv["bias"][bucket].permute(2, 0, 1)[None]
    if n == 2:
        sim = sim.masked_fill(torch.ones(n, J).triu_(J - n + 1).bool(), -torch.finfo(torch.float64).max)
    pr = sim.softmax(-1)
    keep = keep_scaled(B, n_mem, n, J, T, p)
    out = ((pr * keep) @ v).transpose(1, 2).reshape(B * n, 512)
    out.backward(x["dout"].double())
    return lv, pr.detach(), out.detach(), keep, (q.detach(), k.detach(), v.detach())


def attn_bounds(x, pr, keep, qkv):
    """per-element bounds, in the order of the kernel's arithmetic (u = 2^-23, g(K) = dot_ulps(K) u):
      score   |ds| <= (g(64) + 2u) (sum|q k| scale + |bias|)
      prob    relative <= 2 max|ds| + (J/2 + 8) u =: cp          (exp of s - max, sum of J terms, division; masked: exact 0)
      out     <= (g(J) + cp + 2u) sum_j pd |v|
      dp_j    <= g(64) sum|dout v| keep =: e_dp ; c = sum_j p dp: <= sum p e_dp + (g(J) + cp + u) sum p|dp| =: e_c
      ds_j    <= p (e_dp + e_c) + (cp + 3u) p (|dp| + |c|) =: e_ds
      dq      <= scale (sum_j e_ds |k| + (g(J) + 2u) sum_j |ds||k|)
      dk_j    <= scale (sum_i e_ds |q_i| + 4u sum_i |ds||q_i|) ; dv_j <= (cp + 4u) sum_i pd |dout_i|
    (rows that are added onto earlier contents carry one more rounding of the sum: added by the caller)"""
    q, k, v = qkv
    B, n = x["B"], x["n"]
    J = k.shape[2]
    sc = DH ** -0.5
    g = lambda K: dot_ulps(K) * U23   # noqa: E731
    bias = x["bias"].double().abs().max()
    smag = (q.abs() @ k.abs().transpose(-1, -2)) * sc + bias
    cp = 2 * float(((g(64) + 2 * U23) * smag).max()) + (J / 2 + 8) * U23
    dout = x["dout"].double().view(B, n, HEADS, DH).transpose(1, 2)
    pd = pr * keep
    b = {"cp": cp, "probs": cp * pr + 1e-30}
    b["out"] = (g(J) + cp + 2 * U23) * (pd @ v.abs())
    dp = (dout @ v.transpose(-1, -2)) * keep
    e_dp = g(64) * (dout.abs() @ v.abs().transpose(-1, -2)) * keep
    c = (pr * dp).sum(-1, keepdim=True)
    e_c = (pr * e_dp).sum(-1, keepdim=True) + (g(J) + cp + U23) * (pr * dp.abs()).sum(-1, keepdim=True)
    ds = pr * (dp - c)
    e_ds = pr * (e_dp + e_c) + (cp + 3 * U23) * pr * (dp.abs() + c.abs())
    b["ds"], b["e_ds"] = ds, e_ds
    b["dq"] = sc * (e_ds @ k.abs() + (g(J) + 2 * U23) * (ds.abs() @ k.abs()))
    b["dk"] = sc * (e_ds.transpose(-1, -2) @ q.abs() + 4 * U23 * (ds.abs().transpose(-1, -2) @ q.abs()))
    b["dv"] = (cp + 4 * U23) * (pd.transpose(-1, -2) @ dout.abs())
    return b


def rows_to_layout(t, B, n_mem):
    """[B, heads, keys, 64] (memory keys only) -> [windows, 2B, 512] in the kernel's layout"""
    return t[:, :, :n_mem].transpose(1, 2).reshape(B, n_mem // 2, 2, 512).permute(1, 0, 2, 3).reshape(n_mem // 2, 2 * B, 512)


@pytest.mark.parametrize("n_mem,n,p", [(0, 2, 0.0), (2, 2, 0.0), (10, 2, 0.0), (10, 1, 0.0), (254, 2, 0.0), (10, 2, 0.3)])
def test_window_attention(n_mem, n, p):
    B, T = 3, max(n_mem + n, 12)
    x = attn_inputs(B, n_mem, n, T)
    lv, pr, out_ref, keep, qkv = attn_reference(x, p)
    bnd = attn_bounds(x, pr, keep, qkv)
    J = n_mem + (2 if n == 2 else 0)
    nw = n_mem // 2
    d = {k: x[k].to(dev()) for k in ("q", "mem", "selfkv", "bias", "dout")}
    probs = torch.full((B * HEADS * n, T), float("nan"), device=dev())
    out = torch.full((B * n, 512), float("nan"), device=dev())
    a = L.FbAttnDesc()
    a.q, a.q_ld = P(d["q"]), 512
    if n_mem:
        a.mem_k, a.mem_v, a.mem_win, a.mem_ld = P(d["mem"]), P(d["mem"]) + 4 * 512, 2 * B * 1024, 1024
    if n == 2:
        a.self_k, a.self_v, a.self_ld = P(d["selfkv"]), P(d["selfkv"]) + 4 * 512, 1024
    a.bias, a.probs, a.p_ld, a.out, a.out_ld = P(d["bias"]), P(probs), T, P(out), 512
    a.B, a.n, a.n_mem, a.T, a.scale, a.drop_p, a.seed = B, n, n_mem, T, DH ** -0.5, p, SEED
    L.check(L.lib().mmvqa_fb_attention(C.byref(a), 0, L.stream_ptr()))
    torch.cuda.synchronize()
    pg = probs.view(B, HEADS, n, T)[..., :J]
    print(f"n_mem {n_mem} n {n} p {p}: cp {bnd['cp']:.2e} probs {relerr(pg, pr):.2e} out {relerr(out, out_ref):.2e}")
    assert torch.isnan(probs.view(B, HEADS, n, T)[..., J:]).all()          # nothing written past the keys
    if n == 2:
        assert bool((pg[:, :, 0, J - 1] == 0).all())                       # query 0 does not see self key 1: exactly 0
    assert_within(pg, pr, bnd["probs"], "probs")
    assert_close(pg, pr, TOL, "probs")
    assert_within(out.view(B, n, HEADS, DH).transpose(1, 2), out_ref.view(B, n, HEADS, DH).transpose(1, 2), bnd["out"] + 1e-30, "out")
    assert_close(out, out_ref, TOL, "out")

    # ---- backward: dq and the self dk / dv written, memory rows and the bias table added onto non-zero contents
    dq = torch.full((B * n, 512), float("nan"), device=dev())
    dself = torch.full((2 * B, 1024), float("nan"), device=dev())
    dmem0 = x["dmem0"][:nw + 1].clone()
    dmem, dbias = dmem0.to(dev()), x["dbias0"].to(dev())
    a.dout, a.dout_ld, a.dq, a.dq_ld = P(d["dout"]), 512, P(dq), 512
    if n == 2:
        a.dself_k, a.dself_v, a.dself_ld = P(dself), P(dself) + 4 * 512, 1024
    a.dmem_k, a.dmem_v, a.dbias = P(dmem), P(dmem) + 4 * 512, P(dbias)
    L.check(L.lib().mmvqa_fb_attention(C.byref(a), 1, L.stream_ptr()))
    torch.cuda.synchronize()
    heads = lambda t, r: t.reshape(B, r, HEADS, DH).transpose(1, 2)   # noqa: E731
    assert_within(heads(dq, n), heads(lv["q"].grad, n), bnd["dq"] + 1e-30, "dq")
    assert_close(dq, lv["q"].grad, TOL, "dq")
    if n == 2:
        gs = lv["selfkv"].grad
        assert_within(heads(dself[:, :512], 2), heads(gs[:, :512], 2), bnd["dk"][:, :, n_mem:] + 1e-30, "self dk")
        assert_within(heads(dself[:, 512:], 2), heads(gs[:, 512:], 2), bnd["dv"][:, :, n_mem:] + 1e-30, "self dv")
        assert_close(dself, gs, TOL, "self dk | dv")
    else:
        assert torch.isnan(dself).all()
    dm = dmem.cpu()
    assert torch.equal(dm[nw:], dmem0[nw:])                                # rows >= 2w untouched
    if n_mem:
        want = dmem0[:nw].double() + lv["mem"].grad[:nw]
        add = U23 * want.abs()                                             # the rounding of the sum itself
        assert_within(dm[:nw, :, :512], want[..., :512], rows_to_layout(bnd["dk"], B, n_mem) + add[..., :512], "dmem k")
        assert_within(dm[:nw, :, 512:], want[..., 512:], rows_to_layout(bnd["dv"], B, n_mem) + add[..., 512:], "dmem v")
        assert_close(dm[:nw], want, TOL, "dmem")
    db = dbias.cpu()
    assert torch.equal(db[2:], x["dbias0"][2:])                            # only rows 0 and 1 change
    want = x["dbias0"].double() + lv["bias"].grad
    ds, e_ds = bnd["ds"], bnd["e_ds"]
    terms = B * n * J
    e = torch.zeros(32, HEADS, dtype=torch.float64)
    tot = e_ds.sum((0, 2, 3)) + terms * U23 * ds.abs().sum((0, 2, 3))      # every pair of a head lands in row 0 or row 1
    e[0], e[1] = tot, tot
    assert_within(db[:2], want[:2], e[:2] + 2 * U23 * want[:2].abs() + 1e-30, "dbias")
    if n == 1:
        assert torch.equal(db[1], x["dbias0"][1])                          # a one-token window uses row 0 throughout


def test_window_attention_refuses_what_it_cannot_address():
    lib = L.lib()
    a = L.FbAttnDesc()
    a.q = a.bias = a.probs = a.out = a.mem_k = a.mem_v = a.self_k = a.self_v = 0x1000   # never dereferenced
    a.q_ld = a.out_ld = 512
    a.mem_ld = a.self_ld = 1024
    a.mem_win = 6 * 1024
    a.B, a.n, a.n_mem, a.T, a.p_ld, a.scale = 3, 2, 256, 258, 258, 0.125
    assert lib.mmvqa_fb_attention(C.byref(a), 0, None) == -1 and b"keys <= 256" in lib.mmvqa_last_error()
    a.n_mem, a.n = 0, 1
    assert lib.mmvqa_fb_attention(C.byref(a), 0, None) == -1                # one token and no memory: no keys
    a.n_mem, a.n, a.p_ld = 10, 2, 8
    assert lib.mmvqa_fb_attention(C.byref(a), 0, None) == -1 and b"p_ld" in lib.mmvqa_last_error()


# ----------------------------------------------------------------------------- aggregate
@pytest.mark.parametrize("nh,rows,H", [(3, 6, 96), (5, 32, 768), (3, 32, 96), (5, 6, 768)])
def test_aggregate(nh, rows, H):
    g = torch.Generator().manual_seed(nh * 100 + rows)
    stride = (rows + 5) * H                                                # the hiddens are slices of longer buffers
    hid = torch.randn(nh, stride // H, H, generator=g)
    lw = torch.randn(nh, generator=g)
    dagg = torch.randn(rows, H, generator=g)
    h64, lw64 = hid.double().requires_grad_(True), lw.double().requires_grad_(True)
    sw = lw64.softmax(-1)
    agg_ref = (h64[:, :rows] * sw[:, None, None]).sum(0)
    agg_ref.backward(dagg.double())
    hd, lwd, dd = hid.to(dev()), lw.to(dev()), dagg.to(dev())
    agg = torch.full((rows, H), float("nan"), device=dev())
    L.check(L.lib().mmvqa_fb_aggregate_fwd(L.stream_ptr(), P(hd), stride, nh, P(lwd), P(agg), rows, H))
    torch.cuda.synchronize()
    mag = (hid[:, :rows].double().abs() * sw.detach()[:, None, None]).sum(0)
    assert_within(agg, agg_ref.detach(), (dot_ulps(nh) + 8) * U23 * mag + 1e-30, "agg")   # 8: the softmax weights' own rounding
    assert_close(agg, agg_ref.detach(), TOL, "agg")
    # backward, twice: the scaled gradients are rewritten, d layer_weight accumulates; the top share is added to dtop
    dh = torch.full((nh, rows, H), float("nan"), device=dev())
    dtop0 = torch.randn(rows, H, generator=g)
    dtop = dtop0.to(dev())
    dlw0 = torch.randn(nh, generator=g)
    dlw = dlw0.to(dev())
    for _ in range(2):
        L.check(L.lib().mmvqa_fb_aggregate_bwd(L.stream_ptr(), P(dd), P(hd), stride, nh, P(lwd), P(dh), rows * H, P(dtop),
                                               P(dlw), rows, H))
    torch.cuda.synchronize()
    want = h64.grad[:, :rows]
    assert_close(dh[:nh - 1], want[:nh - 1], TOL, "scaled gradients")
    assert torch.isnan(dh[nh - 1]).all()                                   # the top share went to dtop
    assert_close(dtop, dtop0.double() + 2 * want[nh - 1], TOL, "dtop (added twice)")
    assert_close(dlw, dlw0.double() + 2 * lw64.grad, TOL, "d layer_weight over two calls")
    # without dtop every share is written; without d_layer_weight nothing is accumulated
    dh2 = torch.full((nh, rows, H), float("nan"), device=dev())
    L.check(L.lib().mmvqa_fb_aggregate_bwd(L.stream_ptr(), P(dd), P(hd), stride, nh, P(lwd), P(dh2), rows * H, None, None, rows, H))
    torch.cuda.synchronize()
    assert_close(dh2, want, TOL, "all shares")
    bnd = 8 * U23 * (dagg.double().abs() * sw.detach()[:, None, None])
    assert_within(dh2, want, bnd + 1e-30, "all shares, per element")


# ----------------------------------------------------------------------------- GEGLU
@pytest.mark.parametrize("M,H", [(6, 96), (32, 768), (32, 96), (6, 768)])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_geglu(M, H, p):
    F = 4 * H
    g = torch.Generator().manual_seed(M + H)
    pre = torch.randn(M, 2 * F, generator=g) * 1.5
    dy = torch.randn(M, F, generator=g)
    idx0 = 5 * F                                                           # the window's rows start at row 5 of the sequence
    keep = torch.ones(M, F, dtype=torch.float64)
    if p > 0:
        idx = idx0 + np.arange(M * F, dtype=np.uint32)
        keep = torch.from_numpy((rng_uniform(SEED, idx) >= np.float32(p)).astype(np.float64).reshape(M, F) / (1.0 - p))
    p64 = pre.double().requires_grad_(True)
    u, gate = p64.chunk(2, dim=-1)
    y_ref = torch.nn.functional.gelu(gate) * u * keep
    y_ref.backward(dy.double())
    pd, dyd = pre.to(dev()), dy.to(dev())
    y = torch.full((M, F), float("nan"), device=dev())
    dpre = torch.full((M, 2 * F), float("nan"), device=dev())
    L.check(L.lib().mmvqa_geglu_fwd(L.stream_ptr(), P(pd), P(y), M, F, p, SEED, idx0))
    L.check(L.lib().mmvqa_geglu_bwd(L.stream_ptr(), P(dyd), P(pd), P(dpre), M, F, p, SEED, idx0))
    torch.cuda.synchronize()
    dropped = (keep == 0)
    live = ~dropped & (gate.detach().abs() < 3) & (gate.detach().abs() > 1e-3) & (u.detach().abs() > 1e-3)   # (gelu underflows in fp32 far below)
    assert bool((y.cpu()[dropped] == 0).all()) and bool((y.cpu()[live] != 0).all())       # the forward's mask ...
    assert bool((dpre.cpu()[:, :F][dropped] == 0).all()) and bool((dpre.cpu()[:, F:][dropped] == 0).all())   # ... is the backward's
    if p > 0:
        assert 0.2 < float(dropped.double().mean()) < 0.4
    # erff and expf: a few ulps each, relative to |gate|-sized intermediates (x * 0.5 * (1 + erf)); 16 ulps of the largest
    # factor product bounds both passes
    ymag = (gate.detach().abs() * u.detach().abs() * keep).clamp_min(1e-30)
    assert_within(y, y_ref.detach(), 16 * U23 * ymag, "geglu")
    assert_close(y, y_ref.detach(), TOL, "geglu")
    assert_close(dpre, p64.grad, TOL, "d(u | gate)")


def test_geglu_refuses_an_index_past_32_bits():
    lib = L.lib()
    assert lib.mmvqa_geglu_fwd(None, 0x1000, 0x2000, 1 << 20, 4096, 0.1, 1, 1 << 31) == -1
    assert b"32 bits" in lib.mmvqa_last_error()
