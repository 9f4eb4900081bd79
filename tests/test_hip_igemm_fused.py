"""Op tests of the implicit-GEMM prologues and epilogues that only the end-to-end tests checked before:

- PRO_AFFINE_SILU / PRO_SILU_GATE on the A side of a forward product (EfficientNetV2 MBConv projections, engine.cpp
  eff_conv_fwd) with the fp64 BatchNorm statistics, every tile and the split-K forms;
- the same prologues on the B side of a weight gradient with the BatchNorm-backward prologue on A (eff_conv_wgrad);
- the tap epilogues EPI_TAP_FWD (v = mean_hw act(A' W^T)) and EPI_TAP_BWD (du = dv / HW * act'(A' W^T)) over every
  tile, both loader families, ReLU and SERF, with and without the BatchNorm-ReLU prologue (engine.cpp tap_fwd / tap_bwd).

The references are fp64 on the CPU from the same fp32 inputs.  Every output element is held to its own error bound
(hip_helpers.dot_ulps: the fp32 rounding of a K-term dot product, plus the prologue's own rounding), so a dropped K
term or a gate read from another image fails in any row, whatever that row's magnitude; assert_close at 1e-4 of the
tensor's maximum stays as the second check."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hip_helpers import *  # noqa: E402,F401,F403
from oracle import mmbert_oracle as O  # noqa: E402

TOL = 1e-4
TILES = [1, 2, 3, 4, 5, 6]

# Rounding of the prologues, in units of 2^-23 of the magnitude their error is measured against:
# SiLU (+ gate): t = x*sc + sh costs <= 2^-23 (|x sc| + |sh|), silu is 1.1-Lipschitz; silu_f = t / (1 + exp(-t)) with the
# hardware exp: its argument rounding adds <= 2^-24 t^2 s(1-s) <= 0.44 * 2^-24 absolute, the exp, add, reciprocal and
# product <= 5 * 2^-24 relative; the gate product one more 2^-24.  Measured against (|x sc| + |sh| + 1) * gate that is
# < 4 * 2^-23; 8 leaves room for a two-ulp reciprocal.
SILU_ULPS = 8
# BatchNorm backward dz = G*P + z*Q + R: two products and two adds, <= 2^-23 (|G P| + |z Q| + |R|).
DZ_ULPS = 2
# BatchNorm + ReLU: t = x*sc + sh, <= 2^-23 (|x sc| + |sh|); ReLU is exact.
RELU_ULPS = 1
# Statistics: each thread sums at most 16 of its rows in fp32 (general_epilogue, 128x128 tile) before fp64 takes over:
# <= 8 * 2^-23 of sum |z|; the square adds one rounding.
STAT_ULPS = 9


def silu_inputs(N, H, W, Cin, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    sc = torch.rand(Cin, generator=g) + 0.5
    sh = torch.randn(Cin, generator=g) * 0.5          # nonzero: a padded tap must give 0, not silu(sh)
    gate = torch.rand(N, Cin, generator=g) * 0.9 + 0.1   # drawn independently per image
    return x, sc, sh, gate


def silu_operand64(x, sc, sh, gate):
    """A' = silu(x*sc + sh) [* gate[img, c]] in fp64 (NCHW) and the magnitude its fp32 rounding is bounded by"""
    t = x.double() * sc.double()[None, :, None, None]
    a = F.silu(t + sh.double()[None, :, None, None])
    mag = t.abs() + sh.double().abs()[None, :, None, None] + 1.0
    if gate is not None:
        a = a * gate.double()[:, :, None, None]
        mag = mag * gate.double()[:, :, None, None]
    return a, mag


def stat_bounds(ref, e):
    """per-channel bounds of the fp64 (sum, sum of squares) of z given the per-element bound e of z (NCHW)"""
    b_sum = e.sum(dim=(0, 2, 3)) + STAT_ULPS * U23 * ref.abs().sum(dim=(0, 2, 3))
    b_sq = (2 * ref.abs() * e + e * e).sum(dim=(0, 2, 3)) + STAT_ULPS * U23 * (ref * ref).sum(dim=(0, 2, 3))
    return b_sum, b_sq


# ----------------------------------------------------------------------------- forward: SiLU (+ gate) on A
# (N, H, W, Cin, Cout, K, stride, pad).  1x1: HW = 49 / 196 / 225 puts image boundaries inside 64- and 128-row tiles;
# Cin multiples of 4, not all of the K-tile; Cout ragged against 64 and 128.  3x3 SAME stride 1 and stride 2: the
# kernel accepts them, and a padded tap must contribute 0.
FWD_SHAPES = [(2, 7, 7, 64, 72, 1, 1, 0), (3, 14, 14, 176, 136, 1, 1, 0), (5, 15, 15, 304, 200, 1, 1, 0),
              (4, 7, 7, 640, 100, 1, 1, 0), (2, 9, 9, 40, 48, 3, 1, 1), (2, 10, 10, 64, 72, 3, 2, 1)]


@functools.lru_cache(maxsize=None)
def fwd_case(shape, gated):
    N, H, W, Cin, Cout, K, s, p = shape
    x, sc, sh, gate = silu_inputs(N, H, W, Cin, seed=sum(shape))
    if not gated:
        gate = None
    g = torch.Generator().manual_seed(7 + Cin)
    w = torch.randn(Cout, Cin, K, K, generator=g) / math.sqrt(Cin * K * K)
    a, amag = silu_operand64(x, sc, sh, gate)
    ref = F.conv2d(a, w.double(), stride=s, padding=p)
    mag = F.conv2d(amag, w.double().abs(), stride=s, padding=p)
    c = dot_ulps(K * K * Cin) + SILU_ULPS
    return (x, sc, sh, gate, w), ref, mag, c


def run_fwd(shape, inputs, tile, splitk=0, ws=None, cnt=None):
    N, H, W, Cin, Cout, K, s, p = shape
    x, sc, sh, gate, w = inputs
    xd, wd, scd, shd = nhwc(x), w_ohwi(w), sc.to(dev()), sh.to(dev())
    OH, OW = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
    z = torch.full((N * OH * OW, Cout), float("nan"), device=dev())   # every element must be written
    stat = torch.zeros(L.STAT_SLOTS, Cout, 2, dtype=torch.float64, device=dev())
    d, _, _ = conv_desc_fwd(xd, wd, N, H, W, Cin, Cout, K, s, p, z)
    d.a_c0, d.a_c1 = P(scd), P(shd)
    if gate is None:
        d.a_pro = L.PRO_AFFINE_SILU
    else:
        gd = gate.to(dev())
        d.a_pro, d.gate, d.gate_hw = L.PRO_SILU_GATE, P(gd), OH * OW
    d.stat1, d.stat_bwd = P(stat), 0
    if splitk:
        d.splitk, d.sk_ws, d.sk_ws_floats = splitk, P(ws), ws.numel()
        if cnt is not None:
            d.sk_cnt, d.sk_cnt_n = P(cnt), cnt.numel()
    run_igemm(d, L.KIND_FWD, tile=tile)
    return from_nhwc(z, N, OH, OW, Cout), stat.sum(0).cpu()


def check_fwd(z, st, ref, mag, c, what):
    assert_gemm_close(z, ref, mag, c, what, TOL)
    b_sum, b_sq = stat_bounds(ref, c * U23 * mag)
    assert_within(st[:, 0], ref.sum(dim=(0, 2, 3)), b_sum, what + " sum")
    assert_within(st[:, 1], (ref * ref).sum(dim=(0, 2, 3)), b_sq, what + " sumsq")
    assert_close(st[:, 0], ref.sum(dim=(0, 2, 3)), 1e-5, what + " sum")
    assert_close(st[:, 1], (ref * ref).sum(dim=(0, 2, 3)), 1e-5, what + " sumsq")


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("gated", [False, True], ids=["silu", "silu_gate"])
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fwd_silu_prologue(shape, gated, tile):
    """z = conv(silu(x*sc + sh) [* gate[img, c]]) and its fp64 statistics, general loaders, every tile"""
    inputs, ref, mag, c = fwd_case(shape, gated)
    z, st = run_fwd(shape, inputs, tile)
    check_fwd(z, st, ref, mag, c, f"z tile {tile}")


@pytest.mark.parametrize("ticket", [False, True], ids=["finish", "ticket"])
@pytest.mark.parametrize("splitk", [2, 3, 8])
@pytest.mark.parametrize("shape,tile", [((4, 7, 7, 640, 100, 1, 1, 0), 5), ((5, 15, 15, 304, 200, 1, 1, 0), 6),
                                        ((3, 14, 14, 176, 136, 1, 1, 0), 3)], ids=["640-t5", "304-t6", "176-t3"])
def test_fwd_silu_gate_split_k(shape, tile, splitk, ticket):
    """the gated forward with K split over workgroups into the caller's scratch (sk_ws, as set_sk gives the engine's
    launches): with the finishing launch, or with tickets (sk_cnt) and the last workgroup of a tile running the epilogue"""
    inputs, ref, mag, c = fwd_case(shape, True)
    N, H, W, Cin, Cout = shape[:5]
    M = N * H * W
    tiles = ((M + 63) // 64) * ((Cout + 63) // 64)
    ws = torch.full((splitk * (tiles * 4096 if ticket else M * Cout),), float("nan"), device=dev())
    cnt = torch.zeros(tiles + 8, dtype=torch.int32, device=dev()) if ticket else None
    z, st = run_fwd(shape, inputs, tile, splitk, ws, cnt)
    check_fwd(z, st, ref, mag, c, f"z split {splitk} tile {tile}")
    if ticket:
        assert int(cnt.abs().sum()) == 0, "tickets not back at zero"


# ----------------------------------------------------------------------------- weight gradient: dz on A, SiLU (+ gate) on B
# K = N*OH*OW ragged against every K-tile; Cout multiples of 4 (the [k][row] A loader reads float4 of channels)
WGRAD_SHAPES = [(3, 7, 7, 176, 72, 1, 1, 0), (5, 15, 15, 64, 136, 1, 1, 0), (2, 14, 14, 304, 40, 1, 1, 0),
                (2, 9, 9, 40, 48, 3, 1, 1), (2, 10, 10, 64, 72, 3, 2, 1)]


@functools.lru_cache(maxsize=None)
def wgrad_case(shape, gated):
    N, H, W, Cin, Cout, K, s, p = shape
    x, sc, sh, gate = silu_inputs(N, H, W, Cin, seed=sum(shape) + 1)
    if not gated:
        gate = None
    OH, OW = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
    g = torch.Generator().manual_seed(11 + Cout)
    G, z = torch.randn(N, Cout, OH, OW, generator=g), torch.randn(N, Cout, OH, OW, generator=g)
    Pc, Qc, Rc = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.3, torch.randn(Cout, generator=g) * 0.1
    bc = lambda t: t.double()[None, :, None, None]
    dz = G.double() * bc(Pc) + z.double() * bc(Qc) + bc(Rc)
    dzmag = (G.double() * bc(Pc)).abs() + (z.double() * bc(Qc)).abs() + bc(Rc).abs()
    a, amag = silu_operand64(x, sc, sh, gate)
    w64 = torch.zeros(Cout, Cin, K, K, dtype=torch.float64, requires_grad=True)
    F.conv2d(a, w64, stride=s, padding=p).backward(dz)
    mag = torch.nn.grad.conv2d_weight(amag, (Cout, Cin, K, K), dzmag, stride=s, padding=p)
    c = dot_ulps(N * OH * OW) + SILU_ULPS + DZ_ULPS
    return (x, sc, sh, gate, G, z, Pc, Qc, Rc), w64.grad, mag, c


@pytest.mark.parametrize("tile", [0] + TILES)
@pytest.mark.parametrize("gated", [False, True], ids=["silu", "silu_gate"])
@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wgrad_silu_prologue(shape, gated, tile):
    """dW = sum_pix dz[pix, co] * silu(x*sc + sh)[pix@tap, ci] [* gate[n, ci]] with dz = G*P + z*Q + R folded on load:
    eff_conv_wgrad's descriptor (c_atomic, the launcher's default split), every tile"""
    N, H, W, Cin, Cout, K, s, p = shape
    (x, sc, sh, gate, G, z, Pc, Qc, Rc), ref, mag, c = wgrad_case(shape, gated)
    OH, OW = G.shape[2:]
    xd, Gd, zd = nhwc(x), nhwc(G), nhwc(z)
    scd, shd, Pd, Qd, Rd = (t.to(dev()) for t in (sc, sh, Pc, Qc, Rc))
    dw = torch.zeros(Cout, K * K * Cin, device=dev())
    d = conv_desc_wgrad(Gd, xd, N, H, W, Cin, Cout, K, s, p, dw)
    d.A2, d.a_pro, d.a_c0, d.a_c1, d.a_c2 = P(zd), L.PRO_DZ, P(Pd), P(Qd), P(Rd)
    d.b_c0, d.b_c1 = P(scd), P(shd)
    if gate is None:
        d.b_pro = L.PRO_AFFINE_SILU
    else:
        gd = gate.to(dev())
        d.b_pro, d.gate, d.gate_hw = L.PRO_SILU_GATE, P(gd), OH * OW
    run_igemm(d, L.KIND_WGRAD, tile=tile)
    out = dw.view(Cout, K, K, Cin).permute(0, 3, 1, 2)
    assert_gemm_close(out, ref, mag, c, f"dW tile {tile}", TOL)


# ----------------------------------------------------------------------------- tap epilogues
def act64(act, u):
    return torch.relu(u) if act == "relu" else O.serf(u)


def dact64(act, u):
    if act == "relu":
        return (u > 0).double()
    sp = F.softplus(u)   # (no clamp needed: |u| stays far below the 50 of the reference's min(x, 50))
    return torch.erf(sp) + u * (2.0 / math.sqrt(math.pi)) * torch.exp(-sp * sp) * torch.sigmoid(u)


# Activations in fp32: ReLU is exact; the kernel's SERF / SERF' carry their own approximation error (common.h: measured
# 9e-7 / 1e-6 absolute against fp64), bounded here by 2e-6 (1 + |u|).  |SERF'| <= 1.09, |ReLU'| <= 1.
def act_err(act, u):
    return torch.zeros_like(u) if act == "relu" else 2e-6 * (1.0 + u.abs())


LIP = {"relu": 1.0, "serf": 1.1}


def run_tap(N, HW, Cc, Hd, act, pro, tile, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(N * HW, Cc, generator=g)
    sc, sh = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
    w = torch.randn(Hd, Cc, generator=g) / math.sqrt(Cc)
    dv = torch.randn(N, Hd, generator=g)
    fd, wd, dvd, scd, shd = (t.to(dev()) for t in (f, w, dv, sc, sh))
    v = torch.zeros(N, Hd, device=dev())
    d = L.GemmDesc()
    d.M, d.N, d.K = N * HW, Hd, Cc
    d.A, d.a_ld, d.g_Cs, d.B, d.b_ld = P(fd), Cc, Cc, P(wd), Cc
    linear_geom(d)
    if pro:
        d.a_pro, d.a_c0, d.a_c1 = L.PRO_AFFINE_RELU, P(scd), P(shd)
    d.epi_mode, d.act, d.tap_HW, d.tap_out, d.C, d.c_ld = L.EPI_TAP_FWD, L.ACT_RELU if act == "relu" else L.ACT_SERF, HW, P(v), P(v), Hd
    run_igemm(d, L.KIND_FWD, tile=tile)
    du = torch.full((N * HW, Hd), float("nan"), device=dev())
    d.epi_mode, d.tap_out, d.tap_dv, d.C = L.EPI_TAP_BWD, None, P(dvd), P(du)
    run_igemm(d, L.KIND_FWD, tile=tile)
    return (f, sc, sh, w, dv), v.cpu(), du.cpu()


def check_tap(N, HW, Cc, Hd, act, pro, tile, seed=0):
    (f, sc, sh, w, dv), v, du = run_tap(N, HW, Cc, Hd, act, pro, tile, seed)
    c = dot_ulps(Cc) + (RELU_ULPS if pro else 0)
    w64, wabs = w.double().T, w.double().abs().T
    v_ref, v_bnd = torch.zeros(N, Hd, dtype=torch.float64), torch.zeros(N, Hd, dtype=torch.float64)
    what = f"tap N={N} HW={HW} C={Cc} Hd={Hd} {act} pro={pro} tile {tile}"
    mid_all = []
    for n in range(N):   # one image at a time: the product shape's fp64 temporaries stay small
        x = f[n * HW:(n + 1) * HW].double()
        if pro:
            t = x * sc.double()
            a, amag = torch.relu(t + sh.double()), t.abs() + sh.double().abs()
        else:
            a, amag = x, x.abs()
        u = a @ w64
        e_u = c * U23 * (amag @ wabs)
        y = act64(act, u)
        # v = sum_r act(u_r) * (1/HW) in fp32: inv_hw and the product 2 roundings, the sum over HW rows (per-thread
        # runs, LDS and global atomics: one tree) at most HW - 1 more
        v_ref[n] = y.mean(0)
        v_bnd[n] = (LIP[act] * e_u + act_err(act, u)).mean(0) + (HW / 2 + 1) * U23 * y.abs().mean(0)
        # du = dv * (1/HW) * act'(u): act' over the interval u +- e_u (ReLU' may flip where |u| <= e_u), then the
        # kernel's act' error and 3 roundings
        s = dv[n].double() / HW
        lo_d, hi_d = dact64(act, u - e_u), dact64(act, u + e_u)
        md = dact64(act, u)
        lo = torch.minimum(torch.minimum(lo_d, hi_d), md) * s
        hi = torch.maximum(torch.maximum(lo_d, hi_d), md) * s
        lo, hi = torch.minimum(lo, hi), torch.maximum(lo, hi)
        slack = s.abs() * act_err(act, u) + 2 * U23 * torch.maximum(lo.abs(), hi.abs())
        du_n = du[n * HW:(n + 1) * HW]
        assert_within(du_n, (lo + hi) / 2, (hi - lo) / 2 + slack, f"{what}: du image {n}")
        mid_all.append(torch.where(lo_d == hi_d, md * s, du_n.double()))   # (ReLU' ambiguous at |u| <= e_u)
    assert_within(v, v_ref, v_bnd, what + ": v")
    assert_close(v, v_ref, TOL, what + ": v")
    assert_close(du, torch.cat(mid_all), TOL, what + ": du")


# every tile x loader family (C = 40: general loaders, C = 256 / 512: uniform-tap loaders) x act; the prologue, HW and Hd
# rotate through the cases so that each family / act pair meets both prologues, every HW and both widths
def tap_cases():
    cases = []
    for tile in TILES:
        for fam in range(2):
            for ai, act in enumerate(("relu", "serf")):
                Cc = 40 if fam == 0 else (256, 512)[(tile + ai) % 2]
                HW = (49, 196, 784)[(tile + fam + ai) % 3]
                Hd = (96, 768)[(tile // 2 + ai + fam) % 2]
                N = {49: 5, 196: 3, 784: 2}[HW]
                cases.append((N, HW, Cc, Hd, act, bool((tile + fam) % 2), tile))
    return cases


@pytest.mark.parametrize("N,HW,Cc,Hd,act,pro,tile", tap_cases())
def test_tap_epilogues(N, HW, Cc, Hd, act, pro, tile):
    check_tap(N, HW, Cc, Hd, act, pro, tile, seed=tile * 7 + Cc)


@pytest.mark.parametrize("act", ["relu", "serf"])
def test_tap_epilogues_product_shape(act):
    """ResNet config 2's first tap: 16 images of 56x56, 256 channels with BatchNorm-ReLU on load, 768 wide, at the
    launcher's default tile (128x128 here)"""
    check_tap(16, 3136, 256, 768, act, True, 0, seed=3)
