"""The float64 references of tests/attention_helpers.py against torch.autograd in float64, and the tolerance of
tests/test_hip_attention.py against an honest fp32 kernel, both without a GPU.

1. attn_fwd / attn_bwd in float64 against torch.autograd of an independent restatement (F.softmax, einsum): a few
   float64 roundings, 1e-11 of the largest value, as in test_chain_refs_cpu.py.
2. An fp32 emulation of the kernel's association order on the CPU -- strictly sequential accumulation over D for the
   scores and for dP, over the keys for P . V and dQ, over the queries for dK and dV, and the softmax sum and delta as a lane
   accumulates them (each lane half its own keys in order, then one exchange) -- has to stay inside the
   bound the GPU tests use (seg_bound / prev_bound) at every case of their grid: the bound is not tighter than an honest
   fp32 kernel.  The worst error / bound ratios are printed."""
import pytest
import torch
import torch.nn.functional as F

import attention_helpers as AH
from attention_helpers import F32, F64
from dropout_helpers import keep_tensor


def close(a, b, what, tol=1e-11):
    a, b = a.detach().double(), b.detach().double()
    e = float((a - b).abs().max())
    s = max(float(b.abs().max()), 1e-300)
    assert e <= tol * s, f"{what}: {e:.3e} against a largest value of {s:.3e}"


# ----------------------------------------------------------------------------- float64 against autograd
@pytest.mark.parametrize("drop_p", [0.0, 0.3])
@pytest.mark.parametrize("form,prev,dprev", [("bert", False, False), ("rf", True, True), ("rf", False, True),
                                             ("rf", True, False), ("rf", False, False)])
def test_float64_reference_against_autograd(form, drop_p, prev, dprev):
    """both encoder forms, with and without dropout / prev_in / dprev_in, ragged mask (one sample cut to 2 of 11)"""
    T, D, seed = 11, 12, 77
    c = AH.make_case(form, D, T, (T, 7, 2), prev, dprev)
    B, heads = c["q"].shape[:2]
    q, k, v = (c[n].double().requires_grad_(True) for n in "qkv")
    # the zero stands in for an absent prev_in, so that autograd yields dprev_out there too
    pin = (torch.zeros(B, T, T, heads, dtype=F64) if c["prev_in"] is None else c["prev_in"].double()).requires_grad_(True)
    m = c["mask"].double()
    att = torch.einsum("bhid,bhjd->bijh", q, k) / c["sqrt_d"] + pin
    att = att - 10000.0 * (1.0 - (m[:, :, None, None] if form == "rf" else m[:, None, :, None]))
    pr = F.softmax(att, dim=2)
    pd = pr
    if drop_p > 0:
        keep = keep_tensor(seed, (B, heads, T, T), drop_p).double().permute(0, 2, 3, 1)
        pd = pr * keep / (1.0 - AH.f32(drop_p))
    out = torch.einsum("bijh,bhjd->bhid", pd, v)
    loss = (out * c["dout"].double()).sum()
    if c["dprev_in"] is not None:
        loss = loss + (att * c["dprev_in"].double()).sum()
    loss.backward()

    args = (c["mask"], c["mask_on_query"])
    prev_out, probs, o = AH.attn_fwd(c["q"], c["k"], c["v"], *args, c["prev_in"], c["sqrt_d"], drop_p, seed, F64)
    close(prev_out, att, "prev_out")
    close(probs, pr.permute(0, 3, 1, 2), "probs")
    close(o, out, "out")
    dq, dk, dv, dpo = AH.attn_bwd(c["q"], c["k"], c["v"], c["dout"], probs, c["dprev_in"], *args, c["sqrt_d"], drop_p, seed, F64)
    close(dq, q.grad, "dq")
    close(dk, k.grad, "dk")
    close(dv, v.grad, "dv")
    close(dpo, pin.grad, "dprev_out")
    if drop_p > 0:
        assert float((o - AH.attn_fwd(c["q"], c["k"], c["v"], *args, c["prev_in"], c["sqrt_d"], 0.0, 0, F64)[2]).abs().max()) > 1e-2


# ----------------------------------------------------------------------------- the fp32 emulation against the bound
def _seq(n, term, idx=None):
    """sum of term(i) in fp32, strictly in order, over i < n (or over the list idx)"""
    idx = list(range(n)) if idx is None else idx
    acc = term(idx[0])
    for i in idx[1:]:
        acc = acc + term(i)
    return acc


def _tile_row(e, lh):
    return (e & 3) + 8 * (e >> 2) + 4 * lh


def _mfma_rows(n):
    """the row pairs one v_mfma_f32_32x32x2_f32 after the other contracts over n rows held as accumulator tiles:
    register e of tile t carries row 32 t + tile_row(e, 0) in lane half 0 and 32 t + tile_row(e, 1) in half 1"""
    pairs = [(32 * t + _tile_row(e, 0), 32 * t + _tile_row(e, 1)) for t in range((n + 31) // 32) for e in range(16)]
    return [tuple(r for r in pr if r < n) for pr in pairs if pr[0] < n]


def _mfma_sum(pairs, term):
    """acc <- acc + (term(r0) + term(r1)) per instruction, in fp32 and in order"""
    acc = None
    for pr in pairs:
        step = term(pr[0]) if len(pr) == 1 else term(pr[0]) + term(pr[1])
        acc = step if acc is None else acc + step
    return acc


def _mfma_dot(D):
    """tile_product over the two half rows: instruction s contracts elements s and D / 2 + s"""
    return [(s, D // 2 + s) for s in range(D // 2)]


def _lane_sum(T, term):
    """a sum over the keys that a lane keeps in registers: each lane half adds its own keys of every tile in order (rows
    0-3, 8-11, .. of a tile in half 0, rows 4-7, 12-15, .. in half 1: wave_tile.h tile_row), then one exchange adds the
    two halves"""
    half = [[j for j in range(T) if ((j & 31) >> 2) & 1 == h] for h in (0, 1)]
    a = _seq(T, term, half[0])
    return a + _seq(T, term, half[1]) if half[1] else a


def emul_fwd(c, drop_p, seed):
    q, k, v = c["q"], c["k"], c["v"]
    B, heads, T, D = q.shape
    s = _mfma_sum(_mfma_dot(D), lambda d: q[..., :, None, d] * k[..., None, :, d]) / c["sqrt_d"]
    if c["prev_in"] is not None:
        s = s + c["prev_in"].permute(0, 3, 1, 2)
    m = c["mask"].float()
    sm = s - 10000.0 * (1.0 - (m[:, None, :, None] if c["mask_on_query"] else m[:, None, None, :]))
    if not c["mask_on_query"]:      # a query mask shifts the whole row: the kernel's softmax takes the unshifted scores
        s = sm
    ex = torch.exp(s - s.amax(-1, keepdim=True))
    probs = ex * (1.0 / _lane_sum(T, lambda j: ex[..., j:j + 1]))
    pd = probs * AH._keep_scale(B, heads, T, drop_p, seed, F32) if drop_p > 0 else probs
    out = _mfma_sum(_mfma_rows(T), lambda j: pd[..., :, j, None] * v[..., None, j, :])
    return sm.permute(0, 2, 3, 1).contiguous(), probs, out


def emul_bwd(c, probs, drop_p, seed):
    q, k, v, do = c["q"], c["k"], c["v"], c["dout"]
    B, heads, T, D = q.shape
    dp = _mfma_sum(_mfma_dot(D), lambda d: do[..., :, None, d] * v[..., None, :, d])
    pd = probs
    if drop_p > 0:
        ks = AH._keep_scale(B, heads, T, drop_p, seed, F32)
        dp, pd = dp * ks, probs * ks
    delta = _lane_sum(T, lambda j: dp[..., j:j + 1] * probs[..., j:j + 1])
    ds = probs * dp - probs * delta
    if c["dprev_in"] is not None:
        ds = ds + c["dprev_in"].permute(0, 3, 1, 2)
    g = ds / c["sqrt_d"]
    dq = _mfma_sum(_mfma_rows(T), lambda j: g[..., :, j, None] * k[..., None, j, :])
    dk = _mfma_sum(_mfma_rows(T), lambda i: g[..., i, :, None] * q[..., None, i, :])
    dv = _mfma_sum(_mfma_rows(T), lambda i: pd[..., i, :, None] * do[..., None, i, :])
    return dq, dk, dv, ds.permute(0, 2, 3, 1).contiguous()


def ratio(x, ref, bound):
    err = (x.double() - ref.double()).abs()
    r = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    return float(r.max())


def emulation_ratios(c, drop_p=0.0, seed=0):
    """worst error / bound of the emulation per output, with the bounds exactly as test_hip_attention.py builds them"""
    fa = AH.fwd_args(c, drop_p, seed)
    ref, emu = AH.attn_fwd(*fa, F64), emul_fwd(c, drop_p, seed)
    fb = AH.fwd_bounds(c, ref, AH.attn_fwd(*fa, F32), drop_p, seed)
    r = {"probs": ratio(emu[1], ref[1], fb[1]), "out": ratio(emu[2], ref[2], fb[2])}
    if c["mask_on_query"]:
        r["prev_out"] = ratio(emu[0], ref[0], fb[0])
    ba = AH.bwd_args(c, emu[1], drop_p, seed)
    bref, bemu = AH.attn_bwd(*ba, F64), emul_bwd(c, emu[1], drop_p, seed)
    bb = AH.bwd_bounds(c, emu[1], bref, AH.attn_bwd(*ba, F32), drop_p, seed)
    for i, n in enumerate(("dq", "dk", "dv") + (("dprev_out",) if c["mask_on_query"] else ())):
        r[n] = ratio(bemu[i], bref[i], bb[i])
    return r


def test_fp32_emulation_stays_inside_the_bound():
    worst = {}
    cases = [(f, D, T, AH.ragged_lens(T), p, dp, 0.0) for f, D, T, p, dp in AH.grid_cases()]
    cases += [("bert", 8, 40, (40, 0, 17), True, True, 0.0), ("rf", 12, 40, (40, 0, 17), True, True, 0.0)]
    cases += [("rf", 96, 75, AH.ragged_lens(75), True, True, 0.3), ("rf", 12, 33, AH.ragged_lens(33), True, True, 0.3),
              ("bert", 8, 33, AH.ragged_lens(33), True, True, 0.3)]
    for form, D, T, lens, prev, dprev, drop_p in cases:
        r = emulation_ratios(AH.make_case(form, D, T, lens, prev, dprev), drop_p, 4321)
        for n, x in r.items():
            assert x <= 1.0, f"{form} D={D} T={T} p={drop_p}: the fp32 emulation's {n} is {x:.2f} of the bound"
            key = (form, n)
            if x > worst.get(key, (0.0,))[0]:
                worst[key] = (x, D, T)
    for (form, n), (x, D, T) in sorted(worst.items()):
        print(f"emulation / bound, worst over the grid: {form:4s} {n:9s} {x:.2f} at D={D} T={T}")
