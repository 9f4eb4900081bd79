"""mmvqa_distill_mse through the C ABI: the target gathered on the fly from the resident teacher table against a dense
target built with torch on the device (distill_helpers.dense_target, roco_utils.py:196-197).

dh is two IEEE operations per element ((h - target) * gscale), so it must be BIT-equal to torch's.  The loss is a sum of
non-negative terms added in a fixed order: against float64 on the same fp32 inputs its relative error is at most
(L + 4) 2^-24, L = the longest chain of additions a summand passes through (csrc/distill.hip's header: lane chain + 6
butterfly levels + the finishing launch's thread chain, butterfly and the four waves); the 4 covers the rounding of
h - target (twice in its square), the quotient and the rounding of the float64 reference to compare."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from mmvqa_amd import _lib as L  # noqa: E402
from hip_helpers import P, dev  # noqa: E402
from distill_helpers import dense_target  # noqa: E402

SHAPES = [(1, 4, 5, 2), (2, 9, 64, 7), (3, 12, 96, 7), (2, 11, 1000, 3), (2, 75, 768, 7)]   # (B, T, H, first)
SENTINEL = 777.0


def chain_length(B, T, H):
    return 4 * math.ceil(H / 256) + 6 + math.ceil(B * T / 256) + 6 + 2


def round4(n):
    return (n + 3) & ~3


def carve(n_floats, unaligned, fill=None, seed=0):
    """a float view of n_floats whose base is 16-byte aligned, or 4 bytes past such an address"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    buf = torch.empty(n_floats + 8, dtype=torch.float32, device=dev())
    off = (-(buf.data_ptr() // 4) % 4) + (1 if unaligned else 0)
    v = buf[off:off + n_floats]
    assert (v.data_ptr() % 16 == 0) != unaligned
    if fill is None:
        v.copy_(torch.randn(n_floats, generator=g))
    else:
        v.fill_(fill)
    return v


class Case:
    def __init__(self, B, T, H, first, counts, starts=None, ld=None, unaligned=False, f16=False, seed=0, table_rows=None):
        self.B, self.T, self.H, self.first, self.f16 = B, T, H, first, f16
        self.M, self.ld = B * T, ld or H
        M, ld = self.M, self.ld
        self.h = carve(M * ld, unaligned, seed=seed).view(M, ld)
        self.dh = carve(M * ld, unaligned, fill=SENTINEL).view(M, ld)
        g = torch.Generator().manual_seed(seed + 1)
        if starts is None:                        # captions back to back, with rows of data the batch does not own in between
            starts, o = [], 3
            for c in counts:
                starts.append(o)
                o += max(c, 0) + 2
        rows = table_rows if table_rows is not None else max(max(s + max(c, 0) for s, c in zip(starts, counts)) + 2, 1)
        t32 = torch.randn(rows, H, generator=g).to(dev())
        self.table = t32.half() if f16 else t32
        self.rows = rows
        self.start = torch.tensor(starts, dtype=torch.int64, device=dev())
        self.count = torch.tensor(counts, dtype=torch.int32, device=dev())
        self.row_sq = torch.full((M,), SENTINEL, dtype=torch.float32, device=dev())
        self.loss = torch.full((), SENTINEL, dtype=torch.float32, device=dev())
        self.gscale = torch.tensor(2.0 / (M * H), dtype=torch.float32)          # float32(2 gloss / (B T H)), gloss = 1

    def launch(self, table=None, f16=None, dh=True):
        table = self.table if table is None else table
        f16 = self.f16 if f16 is None else f16
        L.check(L.lib().mmvqa_distill_mse(L.stream_ptr(), P(self.h), self.ld, P(table), int(f16), self.rows, P(self.start),
                                          P(self.count), self.first, self.B, self.T, self.H, P(self.row_sq), P(self.loss),
                                          P(self.dh) if dh else None, self.ld if dh else 0, float(self.gscale)))
        return self.row_sq.clone(), self.loss.clone(), self.dh.clone()

    def target(self):
        return dense_target(self.table.float(), self.start.tolist(), self.count.tolist(), self.T, self.first).view(self.M, self.H)

    def check(self, what):
        B, T, H, M = self.B, self.T, self.H, self.M
        row_sq, loss, dh = self.launch()
        x, tgt = self.h[:, :H], self.target()
        want = (x - tgt) * self.gscale.to(dev())
        assert torch.equal(dh[:, :H], want), f"{what}: dh differs from (h - target) * gscale in {(dh[:, :H] != want).sum().item()} elements"
        assert (dh[:, H:] == SENTINEL).all(), f"{what}: columns from H on were written"     # H % 4 == 0 on the vector path:
        #                                                                    no column between H and round_up(H, 4) to zero
        d64 = x.double() - tgt.double()
        bound = (chain_length(B, T, H) + 4) * 2.0 ** -24
        r64 = (d64 * d64).sum(1)
        assert ((row_sq.double() - r64).abs() <= bound * r64).all(), f"{what}: row_sq"
        l64 = float(r64.sum() / (M * H))
        err = abs(float(loss) - l64) / l64
        print(f"{what}: loss rel err {err:.2e} (bound {bound:.2e})")
        assert err <= bound, f"{what}: loss {float(loss)!r} vs {l64!r}: {err:.3e} > {bound:.3e}"
        # the same bits on a second launch, and the same loss without dh
        r2, l2, d2 = self.launch()
        assert torch.equal(r2, row_sq) and torch.equal(l2, loss) and torch.equal(d2, dh), f"{what}: two launches differ"
        self.loss.fill_(SENTINEL)
        _, l3, d3 = self.launch(dh=False)
        assert torch.equal(l3, loss) and torch.equal(d3, dh), f"{what}: dh = NULL changes the loss (or dh was written)"
        return row_sq, loss, dh


@pytest.mark.parametrize("B,T,H,first", SHAPES)
def test_distill_mse_against_dense_target(B, T, H, first):
    """every count of {0, 1, T - first - 1, T (clamped)} at every shape; leading dimension H and round_up(H, 4) + 4;
    aligned bases (vector path where H % 4 == 0) and a base 4 bytes off (scalar path); fp32 and fp16 tables.  The table
    holds data around every caption, so a row outside the caption that read the table would not see a zero target."""
    choices = [0, 1, T - first - 1, T]
    for rot in range(0, 4, B):
        counts = [choices[(rot + b) % 4] for b in range(B)]
        for ld in (H, round4(H) + 4):
            for unaligned in (False, True):
                for f16 in (False, True):
                    c = Case(B, T, H, first, counts, ld=ld, unaligned=unaligned, f16=f16, seed=rot)
                    row_sq, loss, dh = c.check(f"counts {counts} ld {ld} unaligned {unaligned} f16 {f16}")
                    if f16:      # an fp16-sourced table gives the bits of the fp32 table of its cast
                        r32, l32, d32 = c.launch(table=c.table.float(), f16=False)
                        assert torch.equal(r32, row_sq) and torch.equal(l32, loss) and torch.equal(d32, dh)


def test_rows_outside_the_caption_have_a_zero_target():
    """one caption in the middle of a table full of data: only rows first .. first + n - 1 see it"""
    B, T, H, first = 2, 12, 96, 7
    c = Case(B, T, H, first, counts=[2, 9], starts=[5, 20], table_rows=40)
    row_sq, _, dh = c.launch()
    g = float(c.gscale)
    x = c.h[:, :H]
    plain = x * c.gscale.to(dev())                       # (h - 0) * gscale
    own = torch.zeros(B * T, dtype=torch.bool)
    own[first:first + 2] = True                          # sample 0: 2 tokens
    own[T + first:T + first + 4] = True                  # sample 1: 9 clamped to T - first - 1 = 4
    assert torch.equal(dh[~own.to(dev())][:, :H], plain[~own.to(dev())]) and g > 0
    assert not torch.isclose(dh[own.to(dev())][:, :H], plain[own.to(dev())]).all(1).any()
    t = c.table.float()
    assert torch.equal(dh[first, :H], (x[first] - t[5]) * c.gscale.to(dev()))
    assert torch.equal(dh[T + first + 3, :H], (x[T + first + 3] - t[23]) * c.gscale.to(dev()))


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("unaligned", [False, True])
def test_bad_samples_give_nan_in_their_rows_only(unaligned, f16):
    """start < 0, count < 0 and start + n > table_rows: NaN in exactly that sample's row_sq and dh rows, finite (and
    right) elsewhere; the loss is NaN"""
    B, T, H, first = 4, 12, 96, 7
    rows = 30
    bad_cases = {"start < 0": (-1, 3), "count < 0": (2, -1), "start + n > table_rows": (rows - 2, 3)}
    for what, (s_bad, c_bad) in bad_cases.items():
        for victim in (0, 2):
            starts, counts = [1, 6, 11, 16], [3, 0, 4, 9]
            starts[victim], counts[victim] = s_bad, c_bad
            c = Case(B, T, H, first, counts, starts=starts, unaligned=unaligned, f16=f16, table_rows=rows)
            row_sq, loss, dh = c.launch()
            vr = torch.zeros(B * T, dtype=torch.bool, device=dev())
            vr[victim * T:(victim + 1) * T] = True
            assert torch.isnan(row_sq[vr]).all() and torch.isnan(dh[vr][:, :H]).all(), what
            assert torch.isfinite(row_sq[~vr]).all() and torch.isfinite(dh[~vr][:, :H]).all(), what
            assert torch.isnan(loss), what
            ok_s, ok_c = list(starts), list(counts)
            ok_s[victim], ok_c[victim] = 0, 0
            tgt = dense_target(c.table.float(), ok_s, ok_c, T, first).view(B * T, H)
            want = (c.h[:, :H] - tgt) * c.gscale.to(dev())
            assert torch.equal(dh[~vr][:, :H], want[~vr]), what
    # the last rows of the table are still reachable: start + n == table_rows is in range
    c = Case(B, T, H, first, [3, 0, 4, 9], starts=[1, 6, 11, rows - 4], unaligned=unaligned, f16=f16, table_rows=rows)
    c.check("caption at the end of the table")


def test_distill_loss_function_and_no_grad():
    """mmvqa_amd.distill_loss: loss and gradient against torch's mse_loss with autograd; no gradient is computed under
    no_grad; argument checks"""
    import mmvqa_amd
    import torch.nn.functional as F
    B, T, H = 3, 12, 96
    g = torch.Generator().manual_seed(4)
    h = torch.randn(B, T, H, generator=g).to(dev()).requires_grad_(True)
    table = torch.randn(20, H, generator=g).to(dev())
    start = torch.tensor([0, 4, 9], dtype=torch.int64, device=dev())
    count = torch.tensor([4, 0, 7], dtype=torch.int32, device=dev())
    tgt = dense_target(table, start.tolist(), count.tolist(), T, 7)
    for tab in (table, table.half()):
        h.grad = None
        loss = mmvqa_amd.distill_loss(h, tab, start, count, 5)
        (loss * 3.0).backward()
        h2 = h.detach().clone().requires_grad_(True)
        ref = F.mse_loss(h2.double(), dense_target(tab.float(), start.tolist(), count.tolist(), T, 7).double())
        (ref * 3.0).backward()
        assert abs(float(loss.detach()) - float(ref.detach())) <= (chain_length(B, T, H) + 4) * 2.0 ** -24 * float(ref.detach())
        assert (h.grad.double() - h2.grad).abs().max() <= 4 * 2.0 ** -24 * h2.grad.abs().max()
    with torch.no_grad():
        l2 = mmvqa_amd.distill_loss(h, table, start, count, 5)
    assert not l2.requires_grad and abs(float(l2) - float(F.mse_loss(h.detach(), tgt))) <= 1e-6 * float(l2)
    assert not mmvqa_amd.distill_loss(h.detach(), table, start, count).requires_grad
    for bad in (dict(teacher=table[:, :95].contiguous()), dict(teacher=table.double()), dict(teacher=table.cpu()),
                dict(start=start.int()), dict(count=count.long()), dict(start=start[:2]), dict(count=count.cpu()),
                dict(h=h.detach()[0])):
        kw = dict(h=h, teacher=table, start=start, count=count)
        kw.update(bad)
        with pytest.raises(ValueError):
            mmvqa_amd.distill_loss(kw["h"], kw["teacher"], kw["start"], kw["count"], 5)
