"""mmvqa_adam_groups through the C ABI: Adam over a device-resident segment table {begin, end, lr, weight_decay, mode}
in one launch (csrc/elementwise.hip, adam_groups_kernel)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from mmvqa_amd import _lib as L  # noqa: E402
from hip_helpers import dev, P  # noqa: E402

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
L2, DEC, FROZEN = L.ADAM_L2, L.ADAM_DECOUPLED, L.ADAM_FROZEN


def table(rows):
    """[(n_floats, lr, wd, mode)] -> (host ctypes array, the same bytes on the device, nseg, [(lo, hi)])"""
    host = (L.AdamSeg * len(rows))()
    pos, spans = 0, []
    for h, (n, lr, wd, mode) in zip(host, rows):
        h.begin, h.end, h.lr, h.weight_decay, h.mode = pos, pos + n, lr, wd, mode
        spans.append((pos, pos + n))
        pos += n
    devt = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev())
    return host, devt, len(rows), spans


def launch(p, g, m, v, lo, n, tab, step, gscale, zero_grad):
    host, devt, nseg, _ = tab
    return L.lib().mmvqa_adam_groups(L.stream_ptr(), P(p), P(g), P(m), P(v), lo, n, C.cast(host, C.c_void_p), P(devt), nseg,
                                     B1, B2, EPS, step, gscale, zero_grad)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def set_cap(monkeypatch, cap):
    if cap is None:
        monkeypatch.delenv("MMVQA_ADAM_WGS", raising=False)
    else:
        monkeypatch.setenv("MMVQA_ADAM_WGS", cap)


# ----------------------------------------------------------------------------- 1. one segment = mmvqa_adam
@pytest.mark.parametrize("cap", [None, "2"])
@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("n", [4, 1028, 2 ** 20 + 12])
def test_one_segment_is_bit_equal_to_mmvqa_adam(monkeypatch, n, zero_grad, cap):
    """one segment, mode 0, weight decay 0: p, m, v and g of three steps equal mmvqa_adam's bit for bit (a condition).
    With the default workgroup cap the grid covers n = 2^20 + 12 and only the tail loop runs; MMVQA_ADAM_WGS=2 (read
    by both launchers) makes the grid smaller than the array, so that the unrolled loop and the tail both run."""
    set_cap(monkeypatch, cap)
    gen = torch.Generator().manual_seed(7)
    p0 = torch.randn(n, generator=gen)
    tab = table([(n, LR, 0.0, L2)])
    a = [p0.to(dev()), None, torch.zeros(n, device=dev()), torch.zeros(n, device=dev())]
    b = [p0.to(dev()), None, torch.zeros(n, device=dev()), torch.zeros(n, device=dev())]
    for step in (1, 2, 3):
        g0 = torch.randn(n, generator=gen) * (0.01 if step == 3 else 1.0)
        a[1], b[1] = g0.to(dev()), g0.to(dev())
        L.check(L.lib().mmvqa_adam(L.stream_ptr(), P(a[0]), P(a[1]), P(a[2]), P(a[3]), n, LR, B1, B2, EPS, step, 0.25, zero_grad))
        L.check(launch(*b, 0, n, tab, step, 0.25, zero_grad))
        torch.cuda.synchronize()
        for x, y, what in zip(a, b, "pgmv"):
            assert same_bits(x, y), f"{what} differs from mmvqa_adam at step {step}"
        assert same_bits(b[1], torch.zeros(n) if zero_grad else g0)


# ----------------------------------------------------------------------------- 2. mixed table against torch
SIZES = (4, 8, 1020, 65536, 4)
MODES = (DEC, L2, FROZEN, DEC, L2)
LRS = (1e-3, 3e-3, 7e-4, 2e-4, 5e-3)
WDS = (0.01, 0.1, 0.3, 0.05, 0.02)
MIXED = [(n, lr, wd, mode) for n, lr, wd, mode in zip(SIZES, LRS, WDS, MODES)]


def adam_f64(p, g, m, v, step, lr, wd, mode):
    """float64 restatement of one torch.optim.Adam(weight_decay=) (mode 0) / torch.optim.AdamW (mode 1) step"""
    if mode == L2:
        g = g + wd * p
    else:
        p = p * (1.0 - lr * wd)
    m = m + (g - m) * (1.0 - B1)
    v = v * B2 + g * g * (1.0 - B2)
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + EPS)
    return p, m, v


@pytest.fixture(scope="module")
def mixed_reference():
    """five steps of the mixed table on the CPU: torch's fp32 optimizers (foreach=False, one param group per segment)
    and the float64 restatement from the same start and the same gradients.  Computed once, never modified."""
    gen = torch.Generator().manual_seed(11)
    n = sum(SIZES)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * (0.05 if s == 4 else 1.0) for s in range(5)]
    gscale = 0.5
    spans = table(MIXED)[3]
    prm = [torch.nn.Parameter(p0[lo:hi].clone()) for lo, hi in spans]
    opts = []
    for mode, cls in ((DEC, torch.optim.AdamW), (L2, torch.optim.Adam)):
        gs = [dict(params=[prm[i]], lr=LRS[i], weight_decay=WDS[i]) for i in range(5) if MODES[i] == mode]
        opts.append(cls(gs, lr=1.0, betas=(B1, B2), eps=EPS, foreach=False))
    p64 = [p0[lo:hi].double() for lo, hi in spans]
    m64 = [torch.zeros_like(t) for t in p64]
    v64 = [torch.zeros_like(t) for t in p64]
    for s, g in enumerate(grads, start=1):
        for i, (lo, hi) in enumerate(spans):
            gi = g[lo:hi] * gscale            # exact in fp32: the kernel's g * grad_scale
            if MODES[i] == FROZEN:
                continue
            prm[i].grad = gi.clone()
            p64[i], m64[i], v64[i] = adam_f64(p64[i], gi.double(), m64[i], v64[i], s, LRS[i], WDS[i], MODES[i])
        for o in opts:
            o.step()
    state = {}
    for o in opts:
        state.update(o.state)
    t32 = [(prm[i].detach(), state[prm[i]]["exp_avg"] if MODES[i] != FROZEN else torch.zeros(SIZES[i]),
            state[prm[i]]["exp_avg_sq"] if MODES[i] != FROZEN else torch.zeros(SIZES[i])) for i in range(5)]
    return dict(p0=p0, grads=grads, gscale=gscale, spans=spans, t32=t32, t64=list(zip(p64, m64, v64)))


def run_mixed(ref, pieces=None, zero_grad=1):
    n = sum(SIZES)
    tab = table(MIXED)
    p, m, v = ref["p0"].to(dev()), torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    for s, g0 in enumerate(ref["grads"], start=1):
        g = g0.to(dev())
        for lo, hi in (pieces or [(0, n)]):
            L.check(launch(p, g, m, v, lo, hi - lo, tab, s, ref["gscale"], zero_grad))
        torch.cuda.synchronize()
        assert same_bits(g, torch.zeros(n) if zero_grad else g0)
    return p.cpu(), m.cpu(), v.cpu()


def test_mixed_table_against_torch(mixed_reference):
    """segments of 4, 8, 1020, 65536 and 4 floats with modes (AdamW, Adam+L2, frozen, AdamW, Adam+L2), distinct lr and
    weight decay, five steps with grad_scale 0.5.  Per tensor, |kernel - torch fp32| <= 4 x |torch fp32 - float64
    restatement| (max over the tensor; p, m and v each).  The frozen segment keeps its start value and zero moments."""
    ref = mixed_reference
    got = run_mixed(ref)
    for i, (lo, hi) in enumerate(ref["spans"]):
        for k, what in enumerate("pmv"):
            x = got[k][lo:hi]
            if MODES[i] == FROZEN:
                assert same_bits(x, ref["p0"][lo:hi] if k == 0 else torch.zeros(hi - lo)), f"frozen segment {i}: {what} moved"
                continue
            t32, t64 = ref["t32"][i][k], ref["t64"][i][k]
            dist = (t32.double() - t64).abs().max().item()
            err = (x.double() - t32.double()).abs().max().item()
            print(f"segment {i} (n={hi - lo}, mode {MODES[i]}) {what}: |kernel - torch| {err:.3e}, |torch - f64| {dist:.3e}, "
                  f"bit-equal {same_bits(x, t32)}")
            assert err <= 4 * dist, f"segment {i} {what}: {err:.3e} > 4 x {dist:.3e}"


# ----------------------------------------------------------------------------- 3. a frozen segment is not touched
@pytest.mark.parametrize("zero_grad", [0, 1])
def test_frozen_segment_is_neither_read_nor_written(zero_grad):
    """p, m, v of the frozen segment hold NaN before and the same bits after (a read would have spread them: the
    neighbours stay finite); its g is zero with zero_grad and untouched without.  The boundaries (260 and 780 floats)
    fall inside a wave's 256 floats, so the lane-by-lane lookup runs too."""
    rows = [(260, LR, 0.01, DEC), (520, 0.0, 0.0, FROZEN), (1024, LR, 0.1, L2)]
    tab = table(rows)
    (_, _), (lo, hi), (_, n) = tab[3]
    gen = torch.Generator().manual_seed(3)
    p0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    m0, v0 = torch.zeros(n), torch.zeros(n)
    nan = torch.tensor(float("nan")).view(torch.int32).item()
    for i, t in enumerate((p0, m0, v0)):
        t[lo:hi] = torch.full((hi - lo,), nan + 1 + i, dtype=torch.int32).view(torch.float32)   # NaNs with a payload each
    p, g, m, v = (t.to(dev()) for t in (p0, g0, m0, v0))
    L.check(launch(p, g, m, v, 0, n, tab, 1, 1.0, zero_grad))
    torch.cuda.synchronize()
    for x, x0, what in ((p, p0, "p"), (m, m0, "m"), (v, v0, "v")):
        assert same_bits(x[lo:hi], x0[lo:hi]), f"{what} of the frozen segment changed"
        assert bool(torch.isfinite(x[:lo]).all()) and bool(torch.isfinite(x[hi:]).all())
        assert not same_bits(x[:lo], x0[:lo]) and not same_bits(x[hi:], x0[hi:]), f"{what} outside the frozen segment did not move"
    if zero_grad:
        assert same_bits(g, torch.zeros(n))
    else:
        assert same_bits(g, g0)


# ----------------------------------------------------------------------------- 4. ranged launches = one launch
@pytest.mark.parametrize("cap", [None, "1"])
def test_ranged_launches_equal_one_launch(monkeypatch, mixed_reference, cap):
    """launches over pieces [lo, hi) of the buffer, each with the global table, give the bits of the one launch; pieces
    begin at a segment start, in the middle of a segment (20 000 and 40 004 lie inside the 65 536-float one, 500 inside
    the frozen one) and inside one wave of a boundary (1028 + 4)."""
    set_cap(monkeypatch, cap)
    n = sum(SIZES)
    one = run_mixed(mixed_reference)
    pieces = [(40004, n - 4), (0, 12), (12, 500), (500, 1036), (1036, 20000), (n - 4, n), (20000, 40004)]
    assert sorted(pieces)[0][0] == 0 and all(a[1] == b[0] for a, b in zip(sorted(pieces), sorted(pieces)[1:]))
    ranged = run_mixed(mixed_reference, pieces)
    for x, y, what in zip(one, ranged, "pmv"):
        assert same_bits(x, y), f"{what}: ranged launches differ from the one launch"


# ----------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_buffers_untouched():
    """every misuse named in include/mmvqa.h returns MMVQA_ERR_ARG (-1) on the host, before any HIP call: the poisoned
    buffers still hold their NaNs afterwards"""
    n = 64
    bufs = [torch.full((n,), float("nan"), device=dev()) for _ in range(4)]
    good = table([(32, LR, 0.0, L2), (32, LR, 0.0, DEC)])
    lib = L.lib()

    def call(tab=good, lo=0, cnt=n, ptrs=None, nseg=None, host=True, devp=True):
        h, d, ns, _ = tab
        a = [P(t) for t in bufs] if ptrs is None else ptrs
        return lib.mmvqa_adam_groups(L.stream_ptr(), a[0], a[1], a[2], a[3], lo, cnt, C.cast(h, C.c_void_p) if host else None,
                                     P(d) if devp else None, ns if nseg is None else nseg, B1, B2, EPS, 1, 1.0, 1)

    def edited(**kw):
        t = table([(32, LR, 0.0, L2), (32, LR, 0.0, DEC)])
        for k, val in kw.items():
            i, field = int(k[-1]), k[:-1]
            setattr(t[0][i], field, val)
        return t

    ptrs = [P(t) for t in bufs]
    cases = {
        "null p": dict(ptrs=[None] + ptrs[1:]), "null g": dict(ptrs=[ptrs[0], None] + ptrs[2:]),
        "null m": dict(ptrs=ptrs[:2] + [None, ptrs[3]]), "null v": dict(ptrs=ptrs[:3] + [None]),
        "null host table": dict(host=False), "null device table": dict(devp=False),
        "lo % 4": dict(lo=2, cnt=4), "n % 4": dict(cnt=6), "negative lo": dict(lo=-4),
        "nseg 0": dict(nseg=0), "nseg 4097": dict(nseg=4097),
        "beyond the table": dict(cnt=n + 4),
        "unsorted": dict(tab=edited(begin0=32, end0=64, begin1=0, end1=32)),
        "overlapping": dict(tab=edited(begin1=28)), "gapped": dict(tab=edited(begin1=36)),
        "not from 0": dict(tab=edited(begin0=4)), "empty segment": dict(tab=edited(end0=0, begin1=0)),
        "misaligned": dict(tab=edited(end0=30, begin1=30)),
        "unknown mode": dict(tab=edited(mode1=3)), "negative mode": dict(tab=edited(mode0=-1)),
    }
    for what, kw in cases.items():
        rc = call(**kw)
        assert rc == -1 and lib.mmvqa_last_error().startswith(b"adam_groups:"), (what, rc, lib.mmvqa_last_error())
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in bufs)
    assert call() == 0          # the same buffers with the good table: accepted
