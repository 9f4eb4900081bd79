"""The float64 references of tests/chain_helpers.py against torch.autograd in float64, without a GPU: what the GPU op
tests of tests/test_hip_chain_ops.py compare the kernels with is itself checked here against torch's own modules.
Everything runs in float64, so the tolerance is a few float64 roundings: 1e-11 relative to the largest value."""
import math

import torch
import torch.nn.functional as F

import chain_helpers as CH
from oracle import mmbert_oracle as O

F64 = torch.float64


def close(a, b, what, tol=1e-11):
    a, b = a.detach().double(), b.detach().double()
    e = float((a - b).abs().max()) if a.numel() else 0.0
    s = max(float(b.abs().max()), 1e-300) if b.numel() else 1.0
    assert e <= tol * s, f"{what}: {e:.3e} against a largest value of {s:.3e}"


def test_layernorm_reference():
    torch.manual_seed(0)
    for rows, H, with_res, with_dres in ((5, 96, True, True), (3, 4, False, False), (7, 260, True, False)):
        x = (torch.randn(rows, H, dtype=F64) + 100).requires_grad_(True)
        r = torch.randn(rows, H, dtype=F64) if with_res else None
        g, b = (torch.rand(H, dtype=F64) + 0.5).requires_grad_(True), torch.randn(H, dtype=F64).requires_grad_(True)
        y_ref = F.layer_norm(x if r is None else x + r, (H,), g, b, 1e-5)
        dy = torch.randn(rows, H, dtype=F64)
        y_ref.backward(dy)
        s, mean, rstd, y = CH.ln_fwd(x.detach(), r, g.detach(), b.detach(), 1e-5, F64)
        close(y, y_ref, "y")
        close(mean, s.mean(-1), "mean")
        close(rstd, 1 / torch.sqrt(s.var(-1, unbiased=False) + 1e-5), "rstd")
        dres = torch.randn(rows, H, dtype=F64) if with_dres else None
        dx, dg, db = CH.ln_bwd(dy, s, g.detach(), mean, rstd, dres, F64)
        close(dx, x.grad if dres is None else x.grad + dres, "dx")
        close(dg, g.grad, "dgamma")
        close(db, b.grad, "dbeta")


def test_embedding_reference():
    torch.manual_seed(1)
    B, T, H, V = 3, 7, 96, 11
    for nv, pad_idx in ((0, 0), (5, 0), (5, -1), (T, 0)):
        emb = O.OracleBertEmbeddings(V, H, 16, pad_token_id=0 if pad_idx == 0 else None).double().eval()
        ids = torch.randint(0, V, (B, T))
        ids[0, 5], ids[1, 5], ids[1, 6], ids[2, 6] = 0, 3, 3, V - 1
        seg = torch.randint(0, 2, (B, T))
        vis = torch.randn(nv, B, H, dtype=F64, requires_grad=True)
        h = emb(ids, seg).clone()
        for n in range(nv):
            h[:, n, :] = vis[n]
        dh = torch.randn(B, T, H, dtype=F64)
        h.backward(dh)
        sd = {k: v.detach() for k, v in emb.state_dict().items()}
        w, p, t = sd["word_embeddings.weight"], sd["position_embeddings.weight"], sd["token_type_embeddings.weight"]
        g, b = sd["LayerNorm.weight"], sd["LayerNorm.bias"]
        out, xh, rstd = CH.embed_fwd(ids, seg, w, p, t, g, b, vis.detach(), nv, 1e-12, F64)
        close(out.view(B, T, H), h, f"embed fwd nv={nv}")
        dw, dp, dty, dg, db, dvis = CH.embed_bwd(dh.view(B * T, H), ids, seg, xh, rstd, g, V, 16, 2, nv, pad_idx, F64)
        z = lambda prm: torch.zeros_like(prm) if prm.grad is None else prm.grad
        close(dw, z(emb.word_embeddings.weight), f"dword nv={nv} pad={pad_idx}")
        if pad_idx == 0:
            assert float(dw[0].abs().max()) == 0.0
        elif nv < T:
            assert float(dw[0].abs().max()) > 0.0     # id 0 does receive gradient without a padding row
        close(dp, z(emb.position_embeddings.weight), "dpos")
        close(dty, z(emb.token_type_embeddings.weight), "dtype")
        close(dg, z(emb.LayerNorm.weight), "dgamma")
        close(db, z(emb.LayerNorm.bias), "dbeta")
        if nv:
            close(dvis, vis.grad, "dvis")


def test_meanpool_and_l2norm_reference():
    torch.manual_seed(2)
    B, T, H = 4, 7, 5
    h = torch.randn(B, T, H, dtype=F64, requires_grad=True)
    mask = torch.ones(B, T, dtype=torch.long)
    mask[0, 2:4] = 0
    mask[1] = 0
    ref = O.mean_pooling(h, mask).double()
    dp = torch.randn(B, H, dtype=F64)
    ref.backward(dp)
    # the oracle's mask is .float(): with 0 / 1 entries and float64 h the product and the count are the same numbers
    close(CH.meanpool_fwd(h.detach(), mask, F64), ref, "meanpool", 1e-7)
    close(CH.meanpool_bwd(dp, mask, F64), h.grad, "meanpool bwd", 1e-7)
    assert float(CH.meanpool_fwd(h.detach(), mask, F64)[1].abs().max()) == 0.0
    x = torch.randn(5, 9, dtype=F64)
    x[2] = 0
    x[3] *= 1e-20
    x.requires_grad_(True)
    y_ref = F.normalize(x, dim=1)
    dy = torch.randn(5, 9, dtype=F64)
    y_ref.backward(dy)
    y, nrm = CH.l2norm_fwd(x.detach(), F64)
    close(y, y_ref, "l2norm")
    assert float(nrm[2]) == 1e-12 and float(nrm[3]) == 1e-12 and float(y[2].abs().max()) == 0.0
    ok = torch.tensor([0, 1, 4])      # away from the clamp, where F.normalize's gradient is the projection formula
    close(CH.l2norm_bwd(dy, y, nrm, F64)[ok], x.grad[ok], "l2norm bwd")
    close(CH.l2norm_bwd(dy, y, nrm, F64)[2:4], dy[2:4] / 1e-12, "l2norm bwd under the clamp: dy / eps", 1e-7)


def test_log_softmax_reference():
    torch.manual_seed(3)
    rows, V = 4, 37
    x = (torch.randn(rows, V, dtype=F64) * 2).requires_grad_(True)
    with torch.no_grad():
        x[1, 5:20] = -math.inf
        x[2, 3] = x[2, 30] = 9.0      # a tie: first index
        x[3] = 1.5                    # a whole row of equal values
    tgt = torch.tensor([0, V - 1, 4, 7])
    lp = x.log_softmax(-1)
    rl = F.nll_loss(lp, tgt, reduction="none")
    (rl.sum() * 0.37).backward()
    lse, loss, p, pred = CH.lsm_ref(x.detach(), tgt, F64)
    close(loss, rl, "row loss")
    close(CH.lsm_grad(p, tgt, 0.37), x.grad, "dlogits")
    assert pred.tolist() == [int(x[0].argmax()), int(x[1].argmax()), 3, 0]
    assert torch.equal(pred, lp.argmax(-1))
    close(F.nll_loss(lp, tgt), O.mlm_loss(x.detach()[None], tgt[None])[0], "mean")
    # with a supplied lse the probabilities are exp(x - that lse)
    close(CH.lsm_ref(x.detach(), tgt, F64, lse=lse + 0.25)[2], p * math.exp(-0.25), "supplied lse")


def test_asl_reference():
    torch.manual_seed(4)
    for Cc in (2, 5, 257):
        for gp, gn, eps in ((0, 4, 0.1), (1, 4, 0.1), (0, 0, 0), (2, 1, 0.05)):
            x = (torch.randn(6, Cc, dtype=F64) * 1.5).requires_grad_(True)
            tgt = torch.randint(0, Cc, (6,))
            ref = O.asl_single_label(x, tgt, gp, gn, eps)
            ref.backward()
            loss, d, p = CH.asl_rows(x.detach(), tgt, gp, gn, eps, F64)
            close(loss.mean(), ref, f"asl loss C={Cc} {gp, gn, eps}")
            close(d / 6, x.grad, f"asl grad C={Cc} {gp, gn, eps}")
            close(p, x.detach().softmax(-1), "p")


def test_adam_reference():
    torch.manual_seed(5)
    n = 64
    for gscale in (1.0, 1.0 / 1024):
        prm = torch.nn.Parameter(torch.randn(n, dtype=F64))
        opt = torch.optim.Adam([prm], lr=1e-3)
        p, m, v = prm.detach().clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
        for step in (1, 2, 3):
            g = torch.randn(n, dtype=F64) * 3
            prm.grad = g * gscale
            opt.step()
            p, m, v = CH.adam_ref(p, g, m, v, step, 1e-3, 0.9, 0.999, 1e-8, gscale, F64)
            close(p, prm.detach(), f"p step {step}")
            st = opt.state[prm]
            close(m, st["exp_avg"], "m")
            close(v, st["exp_avg_sq"], "v")
        # the bound functions give positive finite numbers and order of magnitude 2^-24 of the values
        bp, bm, bv = CH.adam_bounds(p.float(), g.float(), m.float(), v.float(), 3, 1e-3, 0.9, 0.999, 1e-8, gscale)
        assert bool((bv <= 5.01 * CH.U24 * CH.adam_ref(p.float(), g.float(), m.float(), v.float(), 3, 1e-3, 0.9, 0.999, 1e-8,
                                                       gscale, F64)[2] + 1e-29).all())
        assert bool(torch.isfinite(bp).all() and (bp > 0).all() and torch.isfinite(bm).all())


def test_batchnorm_backward_coefficients_reference():
    torch.manual_seed(6)
    N, Cc, Hh, Ww = 3, 5, 4, 4
    z = (torch.randn(N, Cc, Hh, Ww, dtype=F64) * 1.5 + 0.3).requires_grad_(True)
    bn = torch.nn.BatchNorm2d(Cc).double().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
    G = torch.randn(N, Cc, Hh, Ww, dtype=F64)
    bn(z).backward(G)
    count = N * Hh * Ww
    mean = z.detach().mean((0, 2, 3))
    invstd = 1 / torch.sqrt(z.detach().var((0, 2, 3), unbiased=False) + bn.eps)
    xh = (z.detach() - mean[None, :, None, None]) * invstd[None, :, None, None]
    sg, sgx = G.sum((0, 2, 3)), (G * xh).sum((0, 2, 3))
    P, Q, R = CH.bn_pqr(sg, sgx, count, bn.weight.detach(), mean, invstd, True)
    e = lambda t: t[None, :, None, None]
    close(e(P) * G + e(Q) * z.detach() + e(R), z.grad, "dz = P g + Q z + R")
    close(sgx, bn.weight.grad, "dgamma")
    close(sg, bn.bias.grad, "dbeta")
    # eval mode: a fixed affine map of the running statistics
    bn.eval()
    z2 = z.detach().clone().requires_grad_(True)
    bn(z2).backward(G)
    inv_run = 1 / torch.sqrt(bn.running_var + bn.eps)
    P, Q, R = CH.bn_pqr(sg, sgx, count, bn.weight.detach(), bn.running_mean, inv_run, False)
    close(e(P) * G, z2.grad, "eval dz")
    assert float(Q.abs().max()) == 0.0 and float(R.abs().max()) == 0.0
    # the replicas of `spread` add up to the sums they were made from
    st = CH.spread(torch.stack([sg, sgx], 1), 4)
    close(st.sum(0), torch.stack([sg, sgx], 1), "spread")
    assert float(st[4:].abs().max()) == 0.0


def test_policy_helpers():
    ref = torch.tensor([[1.0, 2.0], [1e-6, -3e-6]], dtype=F64)
    cpu = ref + torch.tensor([[1e-6, 0.0], [0.0, 0.0]], dtype=F64)
    b = CH.bound_4x(ref, cpu, seg=-1)
    assert torch.allclose(b[0], torch.full((2,), 4e-6, dtype=F64)) and torch.allclose(b[1], torch.full((2,), 3e-6 * 2.0 ** -22, dtype=F64))
    assert abs(CH.check(ref + 0.5 * b, ref, b, "half") - 0.5) < 1e-6
    try:
        CH.check(ref + 2 * b, ref, b, "outside")
    except AssertionError:
        pass
    else:
        raise AssertionError("a value outside the bound passed")
    nan = torch.full((3,), float("nan"))
    assert CH.same_bits(nan, nan.clone()) and not CH.same_bits(nan, torch.zeros(3))
    assert CH.lsm_fast_ok(64, 8, 5) and not CH.lsm_fast_ok(68, 8, 5) and not CH.lsm_fast_ok(64, 5, 5) and not CH.lsm_fast_ok(64, 4, 5)
    p = torch.tensor([[0.25, 0.75]], dtype=F64)
    gb = CH.grad_bound(p, torch.tensor([1]), 2.0, 1e-6)
    assert torch.allclose(gb, torch.tensor([[2 * 0.25e-6, 2 * (0.75e-6 + 2.0 ** -23)]], dtype=F64))
