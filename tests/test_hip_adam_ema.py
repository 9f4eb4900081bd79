"""mmvqa_adam_ema / mmvqa_adam_groups_ema / mmvqa_swap through the C ABI (csrc/elementwise.hip: adam_kernel<U, true>,
adam_groups_kernel<true>, swap_kernel).  Adam itself must not move by a bit; the average is held to the float64
recurrence of tests/ema_helpers.py.

Shapes, the smallest at which each path can go wrong: n = 4 is one float4; n = 2052 with MMVQA_ADAM_WGS=1 is one
workgroup of 256 threads over 513 float4, so thread 0 runs the unrolled loop (float4 0 and 256) and the tail loop
(float4 512); the table [0, 8) decoupled with weight decay, [8, 1032) frozen, [1032, 2052) L2 has both boundaries inside
a wave's 256 floats."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from mmvqa_amd import _lib as L  # noqa: E402
from hip_helpers import dev, P  # noqa: E402
from ema_helpers import ema_bound, ema_f64_step, magnitude, same_bits  # noqa: E402

LR, B1, B2, EPS, GSCALE, K = 1e-2, 0.9, 0.999, 1e-8, 0.5, 8
ROWS = [(8, LR, 0.01, L.ADAM_DECOUPLED), (1024, 0.0, 0.0, L.ADAM_FROZEN), (1020, 3e-3, 0.1, L.ADAM_L2)]
FROZEN_LO, FROZEN_HI, N_TABLE = 8, 1032, 2052
SHAPES = [(4, None), (2052, "1")]


def table(rows):
    host = (L.AdamSeg * len(rows))()
    pos = 0
    for h, (n, lr, wd, mode) in zip(host, rows):
        h.begin, h.end, h.lr, h.weight_decay, h.mode = pos, pos + n, lr, wd, mode
        pos += n
    return host, torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev()), len(rows)


def set_cap(monkeypatch, cap):
    if cap is None:
        monkeypatch.delenv("MMVQA_ADAM_WGS", raising=False)
    else:
        monkeypatch.setenv("MMVQA_ADAM_WGS", cap)


def adam(buf, n, step, ema=None, decay=None, tab=None, lo=0, cnt=None):
    """one launch of the plain or (ema given) averaging entry point, flat or (tab given) over the segment table"""
    p, g, m, v = (P(t) for t in buf[:4])
    cnt = n if cnt is None else cnt
    lib, s = L.lib(), L.stream_ptr()
    if tab is None:
        if ema is None:
            return L.check(lib.mmvqa_adam(s, p, g, m, v, n, LR, B1, B2, EPS, step, GSCALE, 1))
        return L.check(lib.mmvqa_adam_ema(s, p, g, m, v, P(ema), n, LR, B1, B2, EPS, step, GSCALE, 1, decay))
    host, devt, nseg = tab
    if ema is None:
        return L.check(lib.mmvqa_adam_groups(s, p, g, m, v, lo, cnt, C.cast(host, C.c_void_p), P(devt), nseg, B1, B2, EPS,
                                             step, GSCALE, 1))
    return L.check(lib.mmvqa_adam_groups_ema(s, p, g, m, v, P(ema), lo, cnt, C.cast(host, C.c_void_p), P(devt), nseg, B1,
                                             B2, EPS, step, GSCALE, 1, decay))


def start(n, seed):
    """(p, m, v, ema) on the host: a few steps into a run, the average away from the parameters"""
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=gen)
    return gen, p0, torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 0.01, torch.randn(n, generator=gen)


def run_against_plain(n, decay, tab, frozen=None):
    """K steps of the averaging form beside the plain form on equal inputs: p, g, m, v bit-equal after every step, the
    average within ema_bound of the float64 recurrence fed with the kernel's own p_new.  -> (ema, p) at the end"""
    gen, p0, m0, v0, e0 = start(n, 5)
    a = [p0.to(dev()), None, m0.to(dev()), v0.to(dev())]
    b = [p0.to(dev()), None, m0.to(dev()), v0.to(dev())]
    ema = e0.to(dev())
    E = e0.double()
    M = magnitude(p0, e0)
    for step in range(1, K + 1):
        g0 = torch.randn(n, generator=gen)
        a[1], b[1] = g0.to(dev()), g0.to(dev())
        adam(a, n, step, tab=tab)
        adam(b, n, step, ema=ema, decay=decay, tab=tab)
        torch.cuda.synchronize()
        for x, y, what in zip(a, b, "pgmv"):
            assert same_bits(x, y), f"{what} differs from the plain form at step {step}"
        assert same_bits(b[1], torch.zeros(n))
        E_next = ema_f64_step(E, b[0], decay)
        if frozen is not None:
            E_next[frozen[0]:frozen[1]] = E[frozen[0]:frozen[1]]
        E = E_next
        M = max(M, magnitude(b[0], ema))
        dist = (ema.double().cpu() - E).abs().max().item()
        bound = ema_bound(step, M)
        print(f"n={n} decay={decay} step {step}: |ema - f64| {dist:.3e}, bound {bound:.3e}")
        assert dist <= bound, f"step {step}: |ema - f64| {dist:.3e} > {bound:.3e}"
    return ema, b[0], ema_bound(K, M)


@pytest.mark.parametrize("decay", [0.5, 0.999, 0.0])
@pytest.mark.parametrize("n, cap", SHAPES)
def test_adam_ema_leaves_adam_alone_and_averages(monkeypatch, n, cap, decay):
    set_cap(monkeypatch, cap)
    ema, p, bound = run_against_plain(n, decay, None)
    if decay == 0.5:     # control: a kernel that merely copied p into ema would be far outside the bound
        assert (ema - p).abs().max().item() > 100 * bound
    if decay == 0.0:     # omd = 1: fmaf(p - e, 1, e); the float64 recurrence gives p itself
        assert (ema.double() - p.double()).abs().max().item() <= bound


@pytest.mark.parametrize("decay", [0.5, 0.999])
@pytest.mark.parametrize("cap", [None, "1"])
def test_adam_groups_ema_leaves_adam_alone_and_averages(monkeypatch, cap, decay):
    set_cap(monkeypatch, cap)
    ema, p, bound = run_against_plain(N_TABLE, decay, table(ROWS), frozen=(FROZEN_LO, FROZEN_HI))
    if decay == 0.5:
        live = torch.ones(N_TABLE, dtype=torch.bool)
        live[FROZEN_LO:FROZEN_HI] = False
        assert (ema - p).abs().cpu()[live].max().item() > 100 * bound


@pytest.mark.parametrize("cap", [None, "1"])
def test_frozen_segment_is_neither_read_nor_written(monkeypatch, cap):
    """ema, p, m, v of the frozen segment hold NaNs with a payload each before and the same bits after, and the
    neighbours stay finite (a read would have spread them); its g is zeroed"""
    set_cap(monkeypatch, cap)
    n, lo, hi = N_TABLE, FROZEN_LO, FROZEN_HI
    gen, p0, m0, v0, e0 = start(n, 9)
    g0 = torch.randn(n, generator=gen)
    nan = torch.tensor(float("nan")).view(torch.int32).item()
    for i, t in enumerate((p0, m0, v0, e0)):
        t[lo:hi] = torch.full((hi - lo,), nan + 1 + i, dtype=torch.int32).view(torch.float32)
    buf = [t.to(dev()) for t in (p0, g0, m0, v0)]
    ema = e0.to(dev())
    adam(buf, n, 1, ema=ema, decay=0.9, tab=table(ROWS))
    torch.cuda.synchronize()
    for x, x0, what in ((buf[0], p0, "p"), (buf[2], m0, "m"), (buf[3], v0, "v"), (ema, e0, "ema")):
        assert same_bits(x[lo:hi], x0[lo:hi]), f"{what} of the frozen segment changed"
        assert bool(torch.isfinite(x[:lo]).all()) and bool(torch.isfinite(x[hi:]).all()), what
        assert not same_bits(x[:lo], x0[:lo]) and not same_bits(x[hi:], x0[hi:]), f"{what} outside the frozen segment did not move"
    assert same_bits(buf[1], torch.zeros(n))


@pytest.mark.parametrize("cap", [None, "1"])
def test_ranged_launches_equal_one_launch(monkeypatch, cap):
    """[0, 1028) then [1028, 2052) with the global table give the bits of the one launch on all five buffers (1028 lies
    inside the frozen segment, one float4 before its end: each piece crosses a boundary of the table)"""
    set_cap(monkeypatch, cap)
    n, tab = N_TABLE, table(ROWS)
    out = []
    for pieces in ([(0, n)], [(0, 1028), (1028, n)]):
        gen, p0, m0, v0, e0 = start(n, 13)
        buf = [p0.to(dev()), None, m0.to(dev()), v0.to(dev())]
        ema = e0.to(dev())
        for step in (1, 2, 3):
            buf[1] = torch.randn(n, generator=gen).to(dev())
            for lo, hi in pieces:
                adam(buf, n, step, ema=ema, decay=0.9, tab=tab, lo=lo, cnt=hi - lo)
        torch.cuda.synchronize()
        out.append(buf + [ema])
    for x, y, what in zip(out[0], out[1], ("p", "g", "m", "v", "ema")):
        assert same_bits(x, y), f"{what}: ranged launches differ from the one launch"
    assert not same_bits(out[0][4][:8], start(n, 13)[4][:8])      # ... and the average did move


@pytest.mark.parametrize("n", [4, 2052])
def test_swap(n):
    gen = torch.Generator().manual_seed(17)
    a0, b0 = torch.randn(n + 4, generator=gen), torch.randn(n + 4, generator=gen)   # 4 floats beyond n: not touched
    a, b = a0.to(dev()), b0.to(dev())
    L.check(L.lib().mmvqa_swap(L.stream_ptr(), P(a), P(b), n))
    torch.cuda.synchronize()
    assert same_bits(a[:n], b0[:n]) and same_bits(b[:n], a0[:n])
    assert same_bits(a[n:], a0[n:]) and same_bits(b[n:], b0[n:])
    L.check(L.lib().mmvqa_swap(L.stream_ptr(), P(a), P(b), n))
    torch.cuda.synchronize()
    assert same_bits(a, a0) and same_bits(b, b0)
