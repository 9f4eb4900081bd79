"""Stride-2 data gradients in the compact form (csrc/igemm.hip, S2C): the output pixels are split by parity into four
classes and each class contracts only the taps that reach it.  A row of a class is not a pixel index any more, so every
case checks EVERY element on its own (hip_helpers.assert_gemm_close / assert_within): one wrong parity class, a swapped
H / W or a wrong epilogue address cannot hide under the tensor's maximum.  The reference is float64 autograd of
F.conv2d on the CPU, computed once per shape.

Per-element bound of a plain data gradient: dot_ulps(K) * 2^-23 * (|dz| (*) |w|), K = KH*KW*Cout terms as launched (the
taps that do not reach a pixel contribute exact zeros, a shorter chain only lowers the error).  With the BatchNorm
backward prologue (dz = P G + Q z + R, coefficients folded in the kernel from the raw sums) the operand itself carries
rounding: invstd / mean arrive rounded to fp32 (1/2 ulp each), P = gamma invstd, Q (invstd twice, a sum, a quotient) and
R = -(P mean(G) - Q mean(z)-like terms) take at most 5 roundings each, the two fmas of the prologue 2 more: under 16 ulps
of |P||G| + |Q||z| + |P||mean G| + |Q||mean z| (the constituents of R, not |R|: R may cancel), hence
(dot_ulps(K) + 16) on that magnitude."""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hip_helpers import *  # noqa: E402,F401,F403
from test_hip_ops import _fold, _spread  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "dgrad_s2_child.py")

# N, H, W, Cin, Cout, K, stride, pad
S3 = [(2, 8, 8, 64, 64, 3, 2, 1),     # a class has 32 rows: less than one row tile
      (2, 12, 8, 64, 64, 3, 2, 1),    # H != W
      (3, 16, 16, 64, 64, 3, 2, 1),   # 192 rows per class: several row tiles, images straddle tiles
      (2, 8, 8, 48, 128, 3, 2, 1)]    # ragged columns
S1 = [(n, h, w, ci, co, 1, 2, 0) for (n, h, w, ci, co, _, _, _) in S3]


def dgrad_ref(G, w, shape, s, p):
    """float64 gradient of conv2d with respect to its input, for the output gradient G"""
    x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.double(), stride=s, padding=p).backward(G.double())
    return x.grad


@functools.lru_cache(maxsize=None)
def case(cfg, seed=21):
    """seeded operands of one shape, the float64 reference and the per-element magnitude |dz| (*) |w| (never modified)"""
    N, H, W, Cin, Cout, K, s, p = cfg
    g = torch.Generator().manual_seed(seed)
    OH, OW = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
    G = torch.randn(N, Cout, OH, OW, generator=g)
    w = torch.randn(Cout, Cin, K, K, generator=g) / math.sqrt(Cout * K * K)
    ref = dgrad_ref(G, w, (N, Cin, H, W), s, p)
    mag = dgrad_ref(G.abs(), w.abs(), (N, Cin, H, W), s, p)
    return G, w, ref, mag, OH, OW


def rows(t):
    """NCHW reference -> [pixel][channel] as the kernels store it"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def tapless(cfg):
    """[pixel] mask of the output pixels no tap of the kernel reaches"""
    N, H, W, Cin, Cout, K, s, p = cfg
    ys, xs = torch.arange(H), torch.arange(W)
    hit_y = torch.zeros(H, dtype=torch.bool)
    hit_x = torch.zeros(W, dtype=torch.bool)
    for k in range(K):
        hit_y |= (ys + p - k) % s == 0
        hit_x |= (xs + p - k) % s == 0
    return ~(hit_y[:, None] & hit_x[None, :]).expand(N, H, W).reshape(-1)


def nan_out(cfg):
    N, H, W, Cin = cfg[:4]
    return torch.full((N * H * W, Cin), float("nan"), device=dev())   # an unwritten pixel shows


@pytest.mark.parametrize("cfg", S3 + S1)
def test_plain_data_gradient(cfg):
    N, H, W, Cin, Cout, K, s, p = cfg
    G, w, ref, mag, OH, OW = case(cfg)
    Gd, wd = nhwc(G), w_ohwi(w)
    dx = nan_out(cfg)
    d = conv_desc_dgrad(Gd, wd, N, H, W, Cin, Cout, K, s, p, dx)
    run_igemm(d, L.KIND_DGRAD)
    assert_gemm_close(dx, rows(ref), rows(mag), dot_ulps(K * K * Cout), f"dgrad {cfg}")
    if K == 1:
        t = tapless(cfg)
        assert int(t.sum()) == 3 * N * H * W // 4
        assert bool((dx.cpu()[t] == 0).all()), "a pixel without a tap must be exactly 0"


@pytest.mark.parametrize("cfg", S1 + S3[:1])
def test_residual_is_added_per_pixel(cfg):
    """the tap gradient R rides on the epilogue: pixels without a tap equal R exactly"""
    N, H, W, Cin, Cout, K, s, p = cfg
    G, w, ref, mag, OH, OW = case(cfg)
    Gd, wd = nhwc(G), w_ohwi(w)
    R = torch.randn(N * H * W, Cin, generator=torch.Generator().manual_seed(5))
    Rd = R.to(dev())
    dx = nan_out(cfg)
    d = conv_desc_dgrad(Gd, wd, N, H, W, Cin, Cout, K, s, p, dx)
    d.R, d.r_ld = P(Rd), Cin
    run_igemm(d, L.KIND_DGRAD)
    # one more addition of an fp32 value: + 1 ulp of (mag + |R|)
    assert_gemm_close(dx, rows(ref) + R.double(), rows(mag) + R.abs().double(), dot_ulps(K * K * Cout) + 1, f"dgrad + R {cfg}")
    if K == 1:
        t = tapless(cfg)
        assert torch.equal(dx.cpu()[t], R[t]), "a pixel without a tap must equal R exactly"


def mask_operands(cfg, seed=7):
    """pre-activation of the producer with |x * sc + sh| >= 0.05: the ReLU decision does not hang on a rounding"""
    N, H, W, Cin = cfg[:4]
    g = torch.Generator().manual_seed(seed)
    sc, sh = torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g) * 0.3
    t = (torch.rand(N, Cin, H, W, generator=g) + 0.05) * torch.where(torch.rand(N, Cin, H, W, generator=g) < 0.5, -1.0, 1.0)
    x_raw = (t - sh[None, :, None, None]) / sc[None, :, None, None]
    mu, istd = torch.randn(Cin, generator=g) * 0.1, torch.rand(Cin, generator=g) + 0.5
    return x_raw, sc, sh, t > 0, mu, istd


@pytest.mark.parametrize("cfg", [S3[1], S3[2], S3[3], S1[1], S1[2]])
def test_relu_mask_and_backward_statistics(cfg):
    """the epilogue the engine attaches to layerN.0.conv2 / downsample: ReLU mask of the producer (Mk, mk_s, mk_b), the
    tap gradient R and the BatchNorm-backward sums (stat1 over Z1, mean1, invstd1), all read at the PIXEL row"""
    N, H, W, Cin, Cout, K, s, p = cfg
    G, w, ref, mag, OH, OW = case(cfg)
    x_raw, sc, sh, keep, mu, istd = mask_operands(cfg)
    Gd, wd, xd = nhwc(G), w_ohwi(w), nhwc(x_raw)
    scd, shd, mud, isd = sc.to(dev()), sh.to(dev()), mu.to(dev()), istd.to(dev())
    R = torch.randn(N * H * W, Cin, generator=torch.Generator().manual_seed(6))
    Rd = R.to(dev())
    dx = nan_out(cfg)
    bst = torch.zeros(L.STAT_SLOTS, Cin, 2, dtype=torch.float64, device=dev())
    d = conv_desc_dgrad(Gd, wd, N, H, W, Cin, Cout, K, s, p, dx)
    d.Mk, d.mk_ld, d.mk_s, d.mk_b = P(xd), Cin, P(scd), P(shd)
    d.R, d.r_ld = P(Rd), Cin
    d.stat1, d.stat_bwd, d.Z1, d.z1_ld, d.mean1, d.invstd1 = P(bst), 1, P(xd), Cin, P(mud), P(isd)
    run_igemm(d, L.KIND_DGRAD)
    k = rows(keep.double())
    g_ref = (rows(ref) + R.double()) * k
    assert_gemm_close(dx, g_ref, (rows(mag) + R.abs().double()) * k, dot_ulps(K * K * Cout) + 1, f"masked dgrad {cfg}")
    xhat = rows((x_raw.double() - mu.double()[None, :, None, None]) * istd.double()[None, :, None, None])
    bs = bst.sum(0).cpu()
    assert_close(bs[:, 0], g_ref.sum(0), 1e-5, "sum g")
    assert_close(bs[:, 1], (g_ref * xhat).sum(0), 1e-5, "sum g xhat")


@pytest.mark.parametrize("cfg,tile", [(S3[1], 0), (S3[2], 5), (S1[2], 3)])
def test_folded_batchnorm_backward_publishes_once(cfg, tile):
    """PRO_DZ with a_fold: workgroup (0,0,0) of the ONE launch publishes P / Q / R and adds to dgamma / dbeta -- once, not
    once per parity class -- and every class contracts dz = P G + Q z + R"""
    N, H, W, Cin, Cout, K, s, p = cfg
    G, w, _, _, OH, OW = case(cfg)
    g = torch.Generator().manual_seed(9)
    z2 = torch.randn(N, Cout, OH, OW, generator=g) * 1.5 + 0.3
    gamma = torch.rand(Cout, generator=g) + 0.5
    M2 = N * OH * OW
    zz, GG = z2.double(), G.double()
    mean = zz.mean(dim=(0, 2, 3))
    invstd = 1.0 / torch.sqrt(zz.var(dim=(0, 2, 3), unbiased=False) + 1e-5)
    bc = lambda v: v[None, :, None, None]
    xhat = (zz - bc(mean)) * bc(invstd)
    sG, sGx = GG.sum(dim=(0, 2, 3)), (GG * xhat).sum(dim=(0, 2, 3))
    Pc = gamma.double() * invstd
    dz = bc(Pc) * (GG - bc(sG / M2) - xhat * bc(sGx / M2))          # BatchNorm backward through the batch statistics
    Qc = -Pc * invstd * sGx / M2
    dz_mag = bc(Pc.abs()) * (GG.abs() + bc(sG.abs() / M2)) + bc(Qc.abs()) * (zz.abs() + bc(mean.abs()))
    ref = dgrad_ref(dz, w, (N, Cin, H, W), s, p)
    mag = dgrad_ref(dz_mag, w.abs(), (N, Cin, H, W), s, p)
    slots = 4
    bstat = _spread(torch.stack([sG, sGx], 1), slots)
    g2, m2d, i2d = gamma.to(dev()), mean.float().to(dev()), invstd.float().to(dev())
    pqr = [torch.full((Cout,), float("nan"), device=dev()) for _ in range(3)]
    dg, db = torch.zeros(Cout, device=dev()), torch.zeros(Cout, device=dev())
    Gd, z2n, wd = nhwc(G), nhwc(z2), w_ohwi(w)
    dx = nan_out(cfg)
    d = conv_desc_dgrad(Gd, wd, N, H, W, Cin, Cout, K, s, p, dx)
    d.A2, d.a_pro = P(z2n), L.PRO_DZ
    d.a_fold = _fold(bstat, slots, 1, 1, M2, g2, mean=m2d, invstd=i2d, out0=pqr[0], out1=pqr[1], out2=pqr[2], dgamma=dg, dbeta=db)
    run_igemm(d, L.KIND_DGRAD, tile=tile)
    assert_gemm_close(dx, rows(ref), rows(mag), dot_ulps(K * K * Cout) + 16, f"dgrad through the folded BatchNorm backward {cfg}")
    assert_close(dg, sGx, 1e-5, "dgamma (once)")
    assert_close(db, sG, 1e-5, "dbeta (once)")
    assert_close(pqr[0], Pc, 1e-5, "published P")
    assert_close(pqr[1], Qc, 1e-5, "published Q")
    # the same launch on the published coefficients
    dx2 = nan_out(cfg)
    d = conv_desc_dgrad(Gd, wd, N, H, W, Cin, Cout, K, s, p, dx2)
    d.A2, d.a_pro, d.a_c0, d.a_c1, d.a_c2 = P(z2n), L.PRO_DZ, P(pqr[0]), P(pqr[1]), P(pqr[2])
    run_igemm(d, L.KIND_DGRAD, tile=tile)
    assert_gemm_close(dx2, rows(ref), rows(mag), dot_ulps(K * K * Cout) + 16, f"dgrad on the published coefficients {cfg}")


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("cfg", [S3[2], S1[2]])
def test_every_tile(cfg, tile):
    N, H, W, Cin, Cout, K, s, p = cfg
    G, w, ref, mag, OH, OW = case(cfg)
    x_raw, sc, sh, keep, mu, istd = mask_operands(cfg)
    Gd, wd, xd = nhwc(G), w_ohwi(w), nhwc(x_raw)
    scd, shd, mud, isd = sc.to(dev()), sh.to(dev()), mu.to(dev()), istd.to(dev())
    dx = nan_out(cfg)
    bst = torch.zeros(L.STAT_SLOTS, Cin, 2, dtype=torch.float64, device=dev())
    d = conv_desc_dgrad(Gd, wd, N, H, W, Cin, Cout, K, s, p, dx)
    d.Mk, d.mk_ld, d.mk_s, d.mk_b = P(xd), Cin, P(scd), P(shd)
    d.stat1, d.stat_bwd, d.Z1, d.z1_ld, d.mean1, d.invstd1 = P(bst), 1, P(xd), Cin, P(mud), P(isd)
    run_igemm(d, L.KIND_DGRAD, tile=tile)
    k = rows(keep.double())
    assert_gemm_close(dx, rows(ref) * k, rows(mag) * k, dot_ulps(K * K * Cout), f"tile {tile} {cfg}")
    xhat = rows((x_raw.double() - mu.double()[None, :, None, None]) * istd.double()[None, :, None, None])
    bs = bst.sum(0).cpu()
    assert_close(bs[:, 0], (rows(ref) * k).sum(0), 1e-5, "sum g")
    assert_close(bs[:, 1], (rows(ref) * k * xhat).sum(0), 1e-5, "sum g xhat")


@pytest.mark.parametrize("ticket", [True, False])
@pytest.mark.parametrize("cfg,tile,splitk", [(S3[2], 3, 3), (S3[2], 6, 8), (S1[2], 6, 2)])
def test_split_k(cfg, tile, splitk, ticket):
    """K split over workgroups: the classes have 4 / 2 / 2 / 1 (or 1 / 0 / 0 / 0) taps, so the splits of a short class run
    without K-tiles and still publish a partial tile / draw their ticket.  Tickets back at zero, nothing written behind
    the announced end of the scratch."""
    N, H, W, Cin, Cout, K, s, p = cfg
    G, w, ref, mag, OH, OW = case(cfg)
    x_raw, sc, sh, keep, mu, istd = mask_operands(cfg)
    Gd, wd, xd = nhwc(G), w_ohwi(w), nhwc(x_raw)
    scd, shd, mud, isd = sc.to(dev()), sh.to(dev()), mu.to(dev()), istd.to(dev())
    M = N * H * W
    tiles = 4 * ((M // 4 + 63) // 64) * ((Cin + 63) // 64)        # the ticketed form keeps whole 64x64 tiles per class
    floats = splitk * (tiles * 4096 if ticket else M * Cin)
    ws = torch.full((floats + 16,), float("nan"), device=dev())
    cnt = torch.zeros(256, dtype=torch.int32, device=dev())
    dx = nan_out(cfg)
    bst = torch.zeros(L.STAT_SLOTS, Cin, 2, dtype=torch.float64, device=dev())
    d = conv_desc_dgrad(Gd, wd, N, H, W, Cin, Cout, K, s, p, dx)
    d.Mk, d.mk_ld, d.mk_s, d.mk_b = P(xd), Cin, P(scd), P(shd)
    d.stat1, d.stat_bwd, d.Z1, d.z1_ld, d.mean1, d.invstd1 = P(bst), 1, P(xd), Cin, P(mud), P(isd)
    d.splitk, d.sk_ws, d.sk_ws_floats = splitk, P(ws), floats
    if ticket:
        d.sk_cnt, d.sk_cnt_n = P(cnt), cnt.numel()
    run_igemm(d, L.KIND_DGRAD, tile=tile)
    k = rows(keep.double())
    assert_gemm_close(dx, rows(ref) * k, rows(mag) * k, dot_ulps(K * K * Cout), f"split-K {cfg}")
    bs = bst.sum(0).cpu()
    assert_close(bs[:, 0], (rows(ref) * k).sum(0), 1e-5, "sum g")
    assert int(cnt.abs().sum()) == 0, "tickets not back at zero"
    assert bool(torch.isnan(ws[floats:]).all()), "written behind the end of the scratch"
    assert not bool(torch.isnan(ws[:M * Cin]).any()), "the K split did not run"


@pytest.mark.parametrize("cfg", [(2, 7, 7, 64, 64, 3, 2, 1),     # odd sides: the dense walk
                                 (2, 7, 9, 64, 64, 1, 2, 0),
                                 (2, 8, 8, 40, 72, 3, 2, 1),     # general loaders
                                 (2, 8, 8, 64, 64, 7, 2, 3)])    # 7x7 / s2 / p3: classes of 16 / 12 / 12 / 9 taps
def test_other_stride2_data_gradients(cfg):
    N, H, W, Cin, Cout, K, s, p = cfg
    G, w, ref, mag, OH, OW = case(cfg)
    Gd, wd = nhwc(G), w_ohwi(w)
    dx = nan_out(cfg)
    d = conv_desc_dgrad(Gd, wd, N, H, W, Cin, Cout, K, s, p, dx)
    run_igemm(d, L.KIND_DGRAD)
    assert_gemm_close(dx, rows(ref), rows(mag), dot_ulps(K * K * Cout), f"dgrad {cfg}")


@pytest.mark.parametrize("tile", [0, 3, 5])
def test_bit_identical_to_the_dense_walk(tile, tmp_path):
    """the taps of a class are walked in ascending (kh, kw) like the dense walk, and the products the dense walk adds
    for the other taps are exact zeros: without a K split every element is bit-identical.  The dense walk is a
    per-process switch (MMVQA_DGRAD_S2_DENSE), so it runs in a child process."""
    cfg = S3[2]
    N, H, W, Cin, Cout, K, s, p = cfg
    G, w, ref, mag, OH, OW = case(cfg)
    Gd, wd = nhwc(G), w_ohwi(w)
    dx = nan_out(cfg)
    d = conv_desc_dgrad(Gd, wd, N, H, W, Cin, Cout, K, s, p, dx)
    run_igemm(d, L.KIND_DGRAD, tile=tile)
    torch.save({"cfg": cfg, "G": G, "w": w, "tile": tile}, tmp_path / "case.pt")
    env = dict(os.environ, MMVQA_DGRAD_S2_DENSE="1", MMVQA_IGEMM_LOG="1")
    r = subprocess.run([sys.executable, CHILD, str(tmp_path / "case.pt"), str(tmp_path / "out.pt")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    dense = torch.load(tmp_path / "out.pt")
    assert "igemm kind" in r.stderr and "compact" not in r.stderr, r.stderr[-2000:]   # the child really took the dense walk
    assert torch.equal(dx.cpu(), dense["dx"]), f"{int((dx.cpu() != dense['dx']).sum())} elements differ from the dense walk"
