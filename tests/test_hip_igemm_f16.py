"""f16-operand family of the implicit GEMM (mmvqa_gemm_desc.reserved0 = PREC_F16): both operands rounded to fp16
(nearest-even) where they enter LDS, 32x32x16 MFMA, fp32 accumulation and the shared fp32 epilogues.  References are
torch fp64 products of the .half()-rounded operands (after the prologue), at 1e-4 of the tensor max."""
import math

import pytest
import torch
import torch.nn.functional as F

from mmvqa_amd import _lib as L
from hip_helpers import (P, assert_close, conv_desc_dgrad, conv_desc_fwd, conv_desc_wgrad, dev, from_nhwc, linear_geom,
                         nhwc, run_igemm, w_ohwi)

pytestmark = pytest.mark.gpu
TOL = 1e-4


def h(t):
    """the operand as the f16 family sees it: fp16 nearest-even, then exact in fp64"""
    return t.float().half().double()


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 6])
@pytest.mark.parametrize("cfg", [(2, 14, 14, 128, 192, 3, 1, 1), (3, 9, 9, 64, 80, 1, 1, 0), (2, 12, 12, 40, 72, 3, 2, 1),
                                 (2, 10, 10, 64, 96, 1, 2, 0)])
def test_f16_conv_every_tile_variant(cfg, tile):
    """forward with BN+ReLU prologue and statistics, data gradient with ReLU mask and backward statistics, weight gradient
    with BN+ReLU B prologue: uniform-tap loaders (3x3 with halo, 1x1) and general ones (3x3 s2 with 40 channels, 1x1 s2)"""
    N, H, W, Cin, Cout, K, s, p = cfg
    torch.manual_seed(11)
    x_raw = torch.randn(N, Cin, H, W)
    sc, sh = torch.rand(Cin) + 0.5, torch.randn(Cin) * 0.3
    w = torch.randn(Cout, Cin, K, K) / math.sqrt(Cin * K * K)
    a = torch.relu(x_raw * sc[None, :, None, None] + sh[None, :, None, None])
    z_ref = F.conv2d(h(a), h(w), stride=s, padding=p)
    OH, OW = z_ref.shape[2:]
    xd, wd = nhwc(x_raw), w_ohwi(w)
    scd, shd = sc.to(dev()), sh.to(dev())
    z = torch.zeros(N * OH * OW, Cout, device=dev())
    stat = torch.zeros(L.STAT_SLOTS, Cout, 2, dtype=torch.float64, device=dev())
    d, _, _ = conv_desc_fwd(xd, wd, N, H, W, Cin, Cout, K, s, p, z)
    d.a_pro, d.a_c0, d.a_c1 = L.PRO_AFFINE_RELU, P(scd), P(shd)
    d.stat1, d.stat_bwd = P(stat), 0
    d.reserved0 = L.PREC_F16
    run_igemm(d, L.KIND_FWD, tile=tile)
    assert_close(from_nhwc(z, N, OH, OW, Cout), z_ref, TOL, "z")
    zo = from_nhwc(z, N, OH, OW, Cout).double()
    st = stat.sum(0).cpu()
    assert_close(st[:, 0], zo.sum(dim=(0, 2, 3)), 1e-5, "sum")
    assert_close(st[:, 1], (zo ** 2).sum(dim=(0, 2, 3)), 1e-5, "sumsq")
    G = torch.randn(N, Cout, OH, OW)
    Gd = nhwc(G)
    g_in = torch.nn.grad.conv2d_input(a.shape, h(w), h(G), stride=s, padding=p)
    mu, istd = torch.randn(Cin) * 0.1, torch.rand(Cin) + 0.5
    mud, isd = mu.to(dev()), istd.to(dev())
    dx = torch.zeros(N * H * W, Cin, device=dev())
    bst = torch.zeros(L.STAT_SLOTS, Cin, 2, dtype=torch.float64, device=dev())
    d = conv_desc_dgrad(Gd, wd, N, H, W, Cin, Cout, K, s, p, dx)
    d.Mk, d.mk_ld, d.mk_s, d.mk_b = P(xd), Cin, P(scd), P(shd)
    d.stat1, d.stat_bwd, d.Z1, d.z1_ld, d.mean1, d.invstd1 = P(bst), 1, P(xd), Cin, P(mud), P(isd)
    d.reserved0 = L.PREC_F16
    run_igemm(d, L.KIND_DGRAD, tile=tile)
    mask = (x_raw * sc[None, :, None, None] + sh[None, :, None, None] > 0).double()
    g_ref = g_in * mask
    assert_close(from_nhwc(dx, N, H, W, Cin), g_ref, TOL, "dgrad")
    xhat = ((x_raw - mu[None, :, None, None]) * istd[None, :, None, None]).double()
    dxo = from_nhwc(dx, N, H, W, Cin).double()
    bs = bst.sum(0).cpu()
    assert_close(bs[:, 0], dxo.sum(dim=(0, 2, 3)), 1e-4, "sum g")
    assert_close(bs[:, 1], (dxo * xhat).sum(dim=(0, 2, 3)), 1e-4, "sum g xhat")
    dw = torch.zeros(Cout, K * K * Cin, device=dev())
    d = conv_desc_wgrad(Gd, xd, N, H, W, Cin, Cout, K, s, p, dw)
    d.b_pro, d.b_c0, d.b_c1 = L.PRO_AFFINE_RELU, P(scd), P(shd)
    d.reserved0 = L.PREC_F16
    run_igemm(d, L.KIND_WGRAD, tile=tile)
    w_ref = torch.nn.grad.conv2d_weight(h(a), w.shape, h(G), stride=s, padding=p)
    assert_close(dw.view(Cout, K, K, Cin).permute(0, 3, 1, 2), w_ref, TOL, "wgrad")


def test_f16_stem_conv():
    """7x7 s2 stem on the NCHW image (3 channels, general loaders): forward and weight gradient"""
    torch.manual_seed(3)
    N, H, W, Cout = 2, 20, 22, 16
    img = torch.randn(N, 3, H, W)
    w = torch.randn(Cout, 3, 7, 7) / 12
    z_ref = F.conv2d(h(img), h(w), stride=2, padding=3)
    OH, OW = z_ref.shape[2:]
    imgd, wd = img.to(dev()), w_ohwi(w)
    z = torch.zeros(N * OH * OW, Cout, device=dev())
    d = L.GemmDesc()
    d.M, d.N, d.K = N * OH * OW, Cout, 147
    d.A, d.g_nchw = P(imgd), 1
    d.g_SH, d.g_SW, d.g_Cs, d.g_OH, d.g_OW = H, W, 3, OH, OW
    d.g_KH = d.g_KW = 7
    d.g_stride, d.g_pad = 2, 3
    d.B, d.b_ld, d.C, d.c_ld = P(wd), 147, P(z), Cout
    d.reserved0 = L.PREC_F16
    run_igemm(d, L.KIND_FWD, 1)
    assert_close(from_nhwc(z, N, OH, OW, Cout), z_ref, TOL, "stem z")
    G = torch.randn(N, Cout, OH, OW)
    Gd = nhwc(G)
    one, zero = torch.ones(Cout, device=dev()), torch.zeros(Cout, device=dev())
    dw = torch.zeros(Cout, 147, device=dev())
    d = L.GemmDesc()
    d.M, d.N, d.K = Cout, 147, N * OH * OW
    d.A, d.A2, d.a_ld, d.a_pro, d.a_c0, d.a_c1, d.a_c2 = P(Gd), P(z), Cout, L.PRO_DZ, P(one), P(zero), P(zero)
    d.B, d.g_nchw = P(imgd), 1
    d.g_SH, d.g_SW, d.g_Cs, d.g_OH, d.g_OW = H, W, 3, OH, OW
    d.g_KH = d.g_KW = 7
    d.g_stride, d.g_pad = 2, 3
    d.C, d.c_ld, d.c_atomic = P(dw), 147, 1
    d.reserved0 = L.PREC_F16
    run_igemm(d, L.KIND_WGRAD, 1)
    w_ref = torch.nn.grad.conv2d_weight(h(img), w.shape, h(G), stride=2, padding=3)
    assert_close(dw.view(Cout, 7, 7, 3).permute(0, 3, 1, 2), w_ref, TOL, "stem dw")


def _linear(x, w, out, bias=None, act=L.ACT_NONE, tile=0, residual=None):
    M, K = x.shape
    N = w.shape[0]
    d = L.GemmDesc()
    d.M, d.N, d.K = M, N, K
    linear_geom(d)
    d.g_Cs = K
    d.A, d.a_ld, d.B, d.b_ld, d.C, d.c_ld = P(x), K, P(w), K, P(out), N
    if bias is not None:
        d.bias = P(bias)
    if residual is not None:
        d.R, d.r_ld = P(residual), N
    d.act = act
    d.reserved0 = L.PREC_F16
    run_igemm(d, L.KIND_FWD, tile=tile)


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 6])
@pytest.mark.parametrize("M,K,N,act", [(70, 96, 50, "gelu"), (130, 200, 90, "serf"), (256, 768, 2304, "gelu")])
def test_f16_linear_ragged_bias_act_residual(M, K, N, act, tile):
    """linear shapes whose M / N / K are not multiples of the tile, with bias + GELU / SERF + residual epilogue"""
    from oracle import mmbert_oracle as O
    torch.manual_seed(5)
    x, w, b, r = torch.randn(M, K), torch.randn(N, K) / math.sqrt(K), torch.randn(N), torch.randn(M, N)
    out = torch.zeros(M, N, device=dev())
    _linear(x.to(dev()), w.to(dev()), out, b.to(dev()), L.ACT_GELU if act == "gelu" else L.ACT_SERF, tile, r.to(dev()))
    pre = h(x) @ h(w).t() + b.double()
    ref = (F.gelu(pre) if act == "gelu" else O.serf(pre)) + r.double()
    assert_close(out, ref, TOL, "linear")


def test_f16_rounding_is_nearest_even():
    """operands on an fp16 rounding tie (1 + 3*2^-11: nearest-even goes UP to 1 + 2^-9) and just past one: the result is
    the nearest-even product, not the round-toward-zero one (1 + 2^-10)"""
    M, K, N = 64, 64, 64
    for v in (1.0 + 3 * 2.0 ** -11, 1.0 + 3 * 2.0 ** -11 + 2.0 ** -20):
        x = torch.full((M, K), v, device=dev())
        w = torch.full((N, K), 1.0, device=dev())
        out = torch.zeros(M, N, device=dev())
        _linear(x, w, out)
        rne = K * (1.0 + 2.0 ** -9)
        assert float(torch.tensor(v).half()) == 1.0 + 2.0 ** -9
        assert bool((out == rne).all()), f"{v}: {out.unique().tolist()} != {rne}"


def test_f16_bit_is_honoured():
    """operands whose fp16 rounding error is large: the result equals the rounded product and is far from the fp32 one"""
    torch.manual_seed(9)
    M, K, N = 96, 128, 80
    x = (torch.randint(0, 2, (M, K)).float() * 2 - 1) * (1.0 + 2.0 ** -12)   # +-(1 + 2^-12) -> +-1 in fp16
    w = torch.randn(N, K)
    out = torch.zeros(M, N, device=dev())
    _linear(x.to(dev()), w.to(dev()), out)
    ref16 = h(x) @ h(w).t()
    ref32 = x.double() @ w.double().t()
    assert_close(out, ref16, TOL, "rounded")
    assert (out.cpu().double() - ref32).abs().max().item() > 20 * (out.cpu().double() - ref16).abs().max().item()


def test_f16_split_k_with_scratch():
    """split-K over workgroups of a data-gradient-like linear product (partial tiles in the caller's scratch)"""
    torch.manual_seed(2)
    M, K, N = 64, 4096, 64
    x, w = torch.randn(M, K), torch.randn(N, K) / 64
    xd, wd = x.to(dev()), w.to(dev())
    out = torch.zeros(M, N, device=dev())
    ws = torch.zeros(8 * M * N, device=dev())
    d = L.GemmDesc()
    d.M, d.N, d.K = M, N, K
    linear_geom(d)
    d.g_Cs = K
    d.A, d.a_ld, d.B, d.b_ld, d.C, d.c_ld = P(xd), K, P(wd), K, P(out), N
    d.sk_ws, d.sk_ws_floats, d.splitk = P(ws), ws.numel(), 4
    d.reserved0 = L.PREC_F16
    run_igemm(d, L.KIND_FWD, tile=3)
    assert_close(out, h(x) @ h(w).t(), TOL, "split-K")


@pytest.mark.parametrize("cfg", [(2, 14, 14, 128, 192, 3, 1, 1), (3, 9, 9, 64, 80, 1, 1, 0), (2, 12, 12, 40, 72, 3, 2, 1)])
def test_f16_batchnorm_backward_prologue_and_pixel_table(cfg):
    """data and weight gradient through the BatchNorm-backward A prologue dz = P*G + Q*z + R (uniform-tap loaders with
    halo, 1x1, general); the 3x3 stride-1 weight gradient again through the per-pixel tap table (uniform-tap weight
    gradient with halo mask) on both 64x64 tiles"""
    N, H, W, Cin, Cout, K, s, p = cfg
    torch.manual_seed(2)
    x_raw = torch.randn(N, Cin, H, W)
    sc, sh = torch.rand(Cin) + 0.5, torch.randn(Cin) * 0.3
    w = torch.randn(Cout, Cin, K, K) / math.sqrt(Cin * K * K)
    a = torch.relu(x_raw * sc[None, :, None, None] + sh[None, :, None, None])
    xd, wd = nhwc(x_raw), w_ohwi(w)
    scd, shd = sc.to(dev()), sh.to(dev())
    OH, OW = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
    z = torch.zeros(N * OH * OW, Cout, device=dev())
    d, _, _ = conv_desc_fwd(xd, wd, N, H, W, Cin, Cout, K, s, p, z)
    d.a_pro, d.a_c0, d.a_c1 = L.PRO_AFFINE_RELU, P(scd), P(shd)
    d.reserved0 = L.PREC_F16
    run_igemm(d, L.KIND_FWD)
    G = torch.randn(N * OH * OW, Cout)
    Pc, Qc, Rc = torch.rand(Cout) + 0.5, torch.randn(Cout) * 0.1, torch.randn(Cout) * 0.1
    dz = G * Pc + z.cpu() * Qc + Rc                                     # the operand the prologue forms, [pixel][channel]
    dz4 = dz.view(N, OH, OW, Cout).permute(0, 3, 1, 2)
    Gd = G.to(dev())
    coef = [t.to(dev()) for t in (Pc, Qc, Rc)]
    mu, istd = torch.randn(Cin) * 0.1, torch.rand(Cin) + 0.5
    dx = torch.zeros(N * H * W, Cin, device=dev())
    bst = torch.zeros(L.STAT_SLOTS, Cin, 2, dtype=torch.float64, device=dev())
    d = conv_desc_dgrad(Gd, wd, N, H, W, Cin, Cout, K, s, p, dx)
    d.A2, d.a_pro, d.a_c0, d.a_c1, d.a_c2 = P(z), L.PRO_DZ, P(coef[0]), P(coef[1]), P(coef[2])
    d.Mk, d.mk_ld, d.mk_s, d.mk_b = P(xd), Cin, P(scd), P(shd)
    mud, isd = mu.to(dev()), istd.to(dev())
    d.stat1, d.stat_bwd, d.Z1, d.z1_ld, d.mean1, d.invstd1 = P(bst), 1, P(xd), Cin, P(mud), P(isd)
    d.reserved0 = L.PREC_F16
    run_igemm(d, L.KIND_DGRAD)
    mask = (x_raw * sc[None, :, None, None] + sh[None, :, None, None] > 0).double()
    g_ref = torch.nn.grad.conv2d_input(a.shape, h(w), h(dz4), stride=s, padding=p) * mask
    assert_close(from_nhwc(dx, N, H, W, Cin), g_ref, TOL, "dgrad")
    dw = torch.zeros(Cout, K * K * Cin, device=dev())
    d = conv_desc_wgrad(Gd, xd, N, H, W, Cin, Cout, K, s, p, dw)
    d.A2, d.a_pro, d.a_c0, d.a_c1, d.a_c2 = P(z), L.PRO_DZ, P(coef[0]), P(coef[1]), P(coef[2])
    d.b_pro, d.b_c0, d.b_c1 = L.PRO_AFFINE_RELU, P(scd), P(shd)
    d.reserved0 = L.PREC_F16
    run_igemm(d, L.KIND_WGRAD)
    w_ref = torch.nn.grad.conv2d_weight(h(a), w.shape, h(dz4), stride=s, padding=p)
    assert_close(dw.view(Cout, K, K, Cin).permute(0, 3, 1, 2), w_ref, TOL, "wgrad")
    if K > 1 and s == 1 and OH == H and Cin % 64 == 0:
        tab = torch.zeros(N * OH * OW, dtype=torch.int32, device=dev())
        L.check(L.lib().mmvqa_pixmask(L.stream_ptr(), P(tab), N, OH, OW, H, W, K, K, s, p))
        d.pixmask = P(tab)
        for tile in (3, 6):
            dw.zero_()
            run_igemm(d, L.KIND_WGRAD, tile=tile)
            assert_close(dw.view(Cout, K, K, Cin).permute(0, 3, 1, 2), w_ref, TOL, f"wgrad (pixel table, tile {tile})")


def _spread(sums, slots):
    Cc = sums.shape[0]
    stat = torch.zeros(L.STAT_SLOTS, Cc, 2, dtype=torch.float64)
    w = torch.rand(slots, Cc, 2, dtype=torch.float64)
    stat[:slots] = w / w.sum(0, keepdim=True) * sums[None]
    return stat.to(dev())


def _fold(stat, slots, bwd, publish, count, gamma, **kw):
    f = L.BnFold()
    f.stat, f.slots, f.bwd, f.publish, f.count, f.gamma = P(stat), slots, bwd, publish, float(count), P(gamma)
    f.eps, f.reps, f.keep = 1e-5, 1, 0.9
    for k in ("beta", "mean", "invstd", "out0", "out1", "out2", "out3", "run_mean", "run_var", "nbt", "dgamma", "dbeta"):
        if k in kw:
            setattr(f, k, P(kw[k]))
    return f


@pytest.mark.parametrize("cfg", [(2, 10, 10, 128, 64, 1, 1, 0, 4, 0), (3, 8, 8, 128, 128, 3, 1, 1, 2, 3),
                                 (2, 12, 12, 64, 128, 3, 2, 1, 1, 6), (2, 9, 9, 8, 16, 3, 1, 1, 4, 0)])
def test_f16_batchnorm_folded_in_the_consumer(cfg):
    """A prologues folded from raw BatchNorm sums in the kernel's setup (LDS coefficient table; Cin = 8: the launcher's
    coefficient launch in front): forward conv(relu(bn(z1))), data and weight gradient through the folded backward"""
    N, H, W, Cin, Cout, K, s, p, slots, tile = cfg
    torch.manual_seed(11)
    z1 = torch.randn(N, Cin, H, W) * 1.5 + 0.3
    bn = torch.nn.BatchNorm2d(Cin).train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.3)
    w = torch.randn(Cout, Cin, K, K) / math.sqrt(Cin * K * K)
    a1 = torch.relu(bn(z1)).detach()
    z2 = F.conv2d(h(a1), h(w), stride=s, padding=p)
    OH, OW = z2.shape[2:]
    sums = torch.stack([z1.double().sum(dim=(0, 2, 3)), (z1.double() ** 2).sum(dim=(0, 2, 3))], 1)
    stat = _spread(sums, slots)
    g, b = bn.weight.detach().to(dev()), bn.bias.detach().to(dev())
    outs = [torch.zeros(Cin, device=dev()) for _ in range(4)]
    rm, rv = torch.zeros(Cin, device=dev()), torch.ones(Cin, device=dev())
    nbt = torch.zeros(1, dtype=torch.int64, device=dev())
    xd, wd = nhwc(z1), w_ohwi(w)
    zo = torch.zeros(N * OH * OW, Cout, device=dev())
    d, _, _ = conv_desc_fwd(xd, wd, N, H, W, Cin, Cout, K, s, p, zo)
    d.a_pro = L.PRO_AFFINE_RELU
    d.a_fold = _fold(stat, slots, 0, 1, N * H * W, g, beta=b, out0=outs[0], out1=outs[1], out2=outs[2], out3=outs[3],
                     run_mean=rm, run_var=rv, nbt=nbt)
    d.reserved0 = L.PREC_F16
    run_igemm(d, L.KIND_FWD, tile=tile)
    assert_close(from_nhwc(zo, N, OH, OW, Cout), z2, TOL, "conv(relu(bn(z1))) with the fold")
    bn2 = torch.nn.BatchNorm2d(Cout).train()
    with torch.no_grad():
        bn2.weight.uniform_(0.5, 1.5)
    z2f = z2.float()
    z2d = z2f.clone().requires_grad_(True)
    G = torch.randn(N, Cout, OH, OW)
    bn2(z2d).backward(G)
    dz2 = z2d.grad
    mean2 = z2f.mean(dim=(0, 2, 3))
    invstd2 = 1.0 / torch.sqrt(z2f.var(dim=(0, 2, 3), unbiased=False) + 1e-5)
    xhat2 = (z2f - mean2[None, :, None, None]) * invstd2[None, :, None, None]
    bs = torch.stack([G.double().sum(dim=(0, 2, 3)), (G * xhat2).double().sum(dim=(0, 2, 3))], 1)
    bstat = _spread(bs, slots)
    g2, m2d, i2d = bn2.weight.detach().to(dev()), mean2.to(dev()), invstd2.to(dev())
    pqr = [torch.zeros(Cout, device=dev()) for _ in range(3)]
    dg, db = torch.zeros(Cout, device=dev()), torch.zeros(Cout, device=dev())
    Gd, z2n = nhwc(G), nhwc(z2f)
    dx = torch.zeros(N * H * W, Cin, device=dev())
    d = conv_desc_dgrad(Gd, wd, N, H, W, Cin, Cout, K, s, p, dx)
    d.A2, d.a_pro = P(z2n), L.PRO_DZ
    d.a_fold = _fold(bstat, slots, 1, 1, N * OH * OW, g2, mean=m2d, invstd=i2d, out0=pqr[0], out1=pqr[1], out2=pqr[2],
                     dgamma=dg, dbeta=db)
    d.reserved0 = L.PREC_F16
    run_igemm(d, L.KIND_DGRAD, tile=tile)
    # the operand the prologue forms from the published coefficients, dz2 = fma(G, P, fma(z2, Q, R)) in fp32 (torch's own
    # BatchNorm backward differs from it in the last bits, which moves single fp16 roundings): checked against torch's
    # dz2 in fp32, then rounded as the kernel rounds it
    Pq, Qq, Rq = (t.cpu().double()[None, :, None, None] for t in pqr)
    dz2k = (G.double() * Pq + (z2f.double() * Qq + Rq).float().double()).float()
    assert_close(dz2k, dz2, 1e-5, "published P, Q, R")
    dz2 = dz2k
    g_ref = torch.nn.grad.conv2d_input(a1.shape, h(w), h(dz2), stride=s, padding=p)
    assert_close(from_nhwc(dx, N, H, W, Cin), g_ref, TOL, "dgrad through the folded BatchNorm backward")
    assert_close(dg, bn2.weight.grad, 1e-5, "dgamma")
    dw = torch.zeros(Cout, K * K * Cin, device=dev())
    d = conv_desc_wgrad(Gd, xd, N, H, W, Cin, Cout, K, s, p, dw)
    d.A2, d.a_pro = P(z2n), L.PRO_DZ
    d.a_fold = _fold(bstat, slots, 1, 0, N * OH * OW, g2, mean=m2d, invstd=i2d)
    d.b_pro, d.b_c0, d.b_c1 = L.PRO_AFFINE_RELU, P(outs[0]), P(outs[1])
    d.reserved0 = L.PREC_F16
    run_igemm(d, L.KIND_WGRAD, tile=tile)
    w_ref = torch.nn.grad.conv2d_weight(h(a1), w.shape, h(dz2), stride=s, padding=p)
    assert_close(dw.view(Cout, K, K, Cin).permute(0, 3, 1, 2), w_ref, TOL, "wgrad through the folded BatchNorm backward")


def test_f16_tap_epilogues_serf():
    """tap 1x1 convolution v = mean_hw(serf(f W^T)) (EPI_TAP_FWD) and its backward du (EPI_TAP_BWD)"""
    from oracle import mmbert_oracle as O
    torch.manual_seed(4)
    N, HW, Cc, Hd = 3, 49, 64, 96
    f = torch.randn(N, HW, Cc)
    w = torch.randn(Hd, Cc) / math.sqrt(Cc)
    pre = (h(f) @ h(w).t()).requires_grad_(True)
    v_ref = O.serf(pre).mean(1)
    dv = torch.randn(N, Hd)
    v_ref.backward(dv.double())
    fd, wd, dvd = f.reshape(N * HW, Cc).to(dev()), w.to(dev()), dv.to(dev())
    v = torch.zeros(N, Hd, device=dev())
    d = L.GemmDesc()
    d.M, d.N, d.K = N * HW, Hd, Cc
    d.A, d.a_ld, d.g_Cs, d.B, d.b_ld = P(fd), Cc, Cc, P(wd), Cc
    linear_geom(d)
    d.epi_mode, d.act, d.tap_HW, d.tap_out, d.C, d.c_ld = L.EPI_TAP_FWD, L.ACT_SERF, HW, P(v), P(v), Hd
    d.reserved0 = L.PREC_F16
    run_igemm(d, L.KIND_FWD)
    assert_close(v, v_ref, TOL, "tap v")
    du = torch.zeros(N * HW, Hd, device=dev())
    d.epi_mode, d.tap_out, d.tap_dv, d.C = L.EPI_TAP_BWD, None, P(dvd), P(du)
    run_igemm(d, L.KIND_FWD)
    assert_close(du.view(N, HW, Hd), pre.grad, TOL, "tap du")


@pytest.mark.parametrize("cfg,tile,splitk", [((2, 7, 7, 256, 72, 1, 1, 0), 3, 3), ((1, 7, 7, 128, 40, 3, 1, 1), 6, 2)])
def test_f16_ticketed_split_k(cfg, tile, splitk):
    """K split over workgroups with the caller's tickets: the last workgroup of a tile sums the partial tiles and runs the
    epilogue (BN statistics); the tickets are zero again afterwards"""
    N, H, W, Cin, Cout, K, s, p = cfg
    torch.manual_seed(5)
    x_raw = torch.randn(N, Cin, H, W)
    sc, sh = torch.rand(Cin) + 0.5, torch.randn(Cin) * 0.3
    w = torch.randn(Cout, Cin, K, K) / math.sqrt(Cin * K * K)
    a = torch.relu(x_raw * sc[None, :, None, None] + sh[None, :, None, None])
    z_ref = F.conv2d(h(a), h(w), stride=s, padding=p)
    OH, OW = z_ref.shape[2:]
    M = N * OH * OW
    xd, wd = nhwc(x_raw), w_ohwi(w)
    scd, shd = sc.to(dev()), sh.to(dev())
    ws = torch.full((splitk * ((M + 63) // 64) * ((Cout + 63) // 64) * 4096,), float("nan"), device=dev())
    cnt = torch.zeros(256, dtype=torch.int32, device=dev())
    z = torch.zeros(M, Cout, device=dev())
    stat = torch.zeros(L.STAT_SLOTS, Cout, 2, dtype=torch.float64, device=dev())
    d, _, _ = conv_desc_fwd(xd, wd, N, H, W, Cin, Cout, K, s, p, z)
    d.a_pro, d.a_c0, d.a_c1 = L.PRO_AFFINE_RELU, P(scd), P(shd)
    d.stat1, d.stat_bwd = P(stat), 0
    d.splitk, d.sk_ws, d.sk_ws_floats = splitk, P(ws), ws.numel()
    d.sk_cnt, d.sk_cnt_n = P(cnt), cnt.numel()
    d.reserved0 = L.PREC_F16
    run_igemm(d, L.KIND_FWD, tile=tile)
    assert_close(from_nhwc(z, N, OH, OW, Cout), z_ref, TOL, "z (ticketed split-K)")
    zo = from_nhwc(z, N, OH, OW, Cout).double()
    st = stat.sum(0).cpu()
    assert_close(st[:, 0], zo.sum(dim=(0, 2, 3)), 1e-5, "sum")
    assert int(cnt.abs().sum()) == 0
