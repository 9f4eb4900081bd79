"""mmvqa_soft_ce_loss on the GPU: the three modes against the fp64 restatement (tests/label_smoothing_helpers.py), the
reference's own numbers (tests/golden/label_smoothing.npz), and the identities the kernel must keep."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import mmvqa_amd  # noqa: E402
from mmvqa_amd import _lib as L  # noqa: E402
from mmvqa_amd import functional as F  # noqa: E402
from hip_helpers import dev  # noqa: E402
import label_smoothing_helpers as H  # noqa: E402

TOL = 1e-4          # loss: relative; gradient: of its maximum (the project's kernel rule)
SM = 0.1
# (rows, C, |x| scale): single row and tiny C; scalar tail + a copy through _padded; config 5's own shape; a tail on the
# register path with large logits; the streaming form just past its threshold (2048) and at three pieces
SHAPES = [(1, 3, 1.0), (5, 23, 3.0), (64, 1552, 4.0), (7, 1553, 80.0), (3, 2049, 30.0), (3, 4100, 30.0)]
_CASES = {}


def truth(rows, C, scale):
    """the seeded case and its fp64 losses / gradients per mode, computed once and shared"""
    key = (rows, C, scale)
    if key not in _CASES:
        x, tgt, cat, table = H.case(rows, C, scale, seed=1000 + C + rows)
        ref = {}
        for mode in (H.HARD, H.UNIFORM, H.CATEGORY):
            ref[mode] = H.loss_and_grad(x.double(), H.soft_targets(mode, tgt, C, SM, table, cat))
        _CASES[key] = (x, tgt, cat, table, ref)
    return _CASES[key]


def run(x, tgt, mode, table=None, cat=None, smoothing=SM):
    xg = x.to(dev()).requires_grad_(True)
    loss = mmvqa_amd.soft_ce_loss(xg, tgt.to(dev()), mode, smoothing, None if table is None else table.to(dev()),
                                  None if cat is None else cat.to(dev()))
    loss.backward()
    return loss.detach().cpu(), xg.grad.cpu()


def check(loss, grad, ref, what):
    rl, rg = ref
    print(f"{what}: loss {float(loss):.7f} ref {float(rl):.7f} rel {abs(float(loss) - float(rl)) / abs(float(rl)):.2e}; "
          f"grad err/max {float((grad.double() - rg).abs().max() / rg.abs().max()):.2e}")
    assert abs(float(loss) - float(rl)) <= TOL * abs(float(rl)), what
    assert float((grad.double() - rg).abs().max()) <= TOL * float(rg.abs().max()), what


@pytest.mark.parametrize("rows,C,scale", SHAPES)
@pytest.mark.parametrize("mode", [H.HARD, H.UNIFORM, H.CATEGORY])
def test_kernel_matches_fp64_restatement(rows, C, scale, mode):
    x, tgt, cat, table, ref = truth(rows, C, scale)
    loss, grad = run(x, tgt, mode, table, cat)
    check(loss, grad, ref[mode], f"mode {mode} [{rows}, {C}]")


@pytest.mark.parametrize("rows,C,scale", [(5, 23, 3.0), (3, 2049, 30.0)])
def test_unaligned_rows_take_the_scalar_path(rows, C, scale):
    """the ABI with ld = dld = table_ld = C (odd) and bases off 16 bytes: no vector access is possible"""
    x, tgt, cat, table, ref = truth(rows, C, scale)
    off = lambda t: torch.cat([torch.zeros(1), t.reshape(-1)]).to(dev())[1:].view(t.shape)   # noqa: E731  (base + 4 bytes)
    xg, tb = off(x), off(table)
    assert xg.data_ptr() % 16 and tb.data_ptr() % 16
    out = torch.full((rows * C + 1,), 7.0, device=dev())
    dl = out[1:].view(rows, C)
    row_loss, loss = torch.empty(rows, device=dev()), torch.empty((), device=dev())
    tg, cg = tgt.to(dev()), cat.to(dev())            # held: a temporary's memory is reused by the next allocation
    L.check(L.lib().mmvqa_soft_ce_loss(L.stream_ptr(), L.ptr(xg), C, L.ptr(tg), L.ptr(cg), L.ptr(tb), C,
                                       table.shape[0], H.CATEGORY, SM, L.ptr(row_loss), L.ptr(loss), L.ptr(dl), C, rows, C,
                                       1.0 / rows))
    check(loss.cpu(), dl.cpu(), ref[H.CATEGORY], f"scalar path [{rows}, {C}]")
    assert float(out[0]) == 7.0                                          # nothing written in front of the first row


@pytest.mark.parametrize("Cn", [23, 1552])
def test_reference_fixture_replays(Cn):
    g, t = H.fixture(), f"c{Cn}_"
    sm = float(g["smoothing"])
    x, tgt, cat = (torch.from_numpy(g[t + k]) for k in ("logits", "target", "category"))
    crit = mmvqa_amd.CategorySmoothing(H.fixture_rows(g, Cn), Cn, sm).to(dev())
    xg = x.to(dev()).requires_grad_(True)
    loss = crit(xg, tgt.to(dev()), cat.to(dev()))
    loss.backward()
    check(loss.detach().cpu(), xg.grad.cpu(), (torch.tensor(float(g[t + "loss"])), torch.from_numpy(g[t + "dlogits"]).double()),
          f"fixture category C={Cn}")
    uni = mmvqa_amd.LabelSmoothing(sm)
    xg = x.to(dev()).requires_grad_(True)
    loss = uni(xg, tgt.to(dev()))
    loss.backward()
    check(loss.detach().cpu(), xg.grad.cpu(),
          (torch.tensor(float(g[t + "uniform_loss"])), torch.from_numpy(g[t + "uniform_dlogits"]).double()), f"fixture uniform C={Cn}")
    for c, k in ((crit, "eval_loss"), (uni, "uniform_eval_loss")):       # eval branch: cross entropy, category ignored
        ev = float(c.eval()(x.to(dev()), tgt.to(dev()), torch.zeros_like(cat).to(dev())))
        assert abs(ev - float(g[t + k])) <= TOL * abs(float(g[t + k]))
        c.train()


@pytest.mark.parametrize("rows,C", [(64, 1552), (3, 4100)])
def test_hard_mode_is_the_ce_path(rows, C):
    """loss within 1e-6 relative, gradient within 1e-6 of its maximum, on unit-variance logits (an untrained head), where
    an fp32 ulp of lse = ln C + 1/2 moves the gradient by less than 1e-7 of its maximum (lse_ulp_share): there the
    bound measures the kernels and not the rounding of lse.  The shapes of the kernel test follow below."""
    x, tgt, _cat, _table = H.case(rows, C, 1.0, seed=500 + C)
    assert lse_ulp_share(x, tgt) < 1e-7
    hard_against_mlm(x, tgt, 1e-6, 1e-6, f"unit variance [{rows}, {C}]")


def lse_ulp_share(x, tgt):
    """what ONE fp32 ulp of a row's log-sum-exp does to the gradient, as a share of the gradient's largest entry, from
    fp64: every p_j = exp(x_j - lse) moves by the relative amount ulp(lse), so the share is max_rows(p_max ulp(lse)) / rows
    over max |p - onehot| / rows"""
    xd = x.double()
    lse, p = torch.logsumexp(xd, 1), torch.softmax(xd, 1)
    ulp = 2.0 ** (torch.floor(torch.log2(lse.abs())) - 23)
    g = p - torch.nn.functional.one_hot(tgt, x.shape[1])
    return float((p.max(1).values * ulp).max() / g.abs().max())


@pytest.mark.parametrize("rows,C,scale", SHAPES)
def test_hard_mode_against_the_ce_path_at_the_kernel_shapes(rows, C, scale):
    """The same identity at the shapes of the kernel test.  Both paths evaluate lse in fp32 with different summation
    orders (mlm_loss: 1024 threads, hardware exp), so the two values may be neighbouring floats on either side of the
    true one: two ulps apart.  The gradient bound is therefore 1e-6 plus twice lse_ulp_share, which is computed from
    the fp64 softmax alone: 3.7e-7 at (5, 23), 1.8e-6 at (64, 1552, |x| ~ 4), 3.1e-5 at (7, 1553, |x| ~ 80).  The loss
    bound stays 1e-6: an ulp of lse is at most 1.3e-7 of these losses."""
    x, tgt, _cat, _table, _ref = truth(rows, C, scale)
    hard_against_mlm(x, tgt, 1e-6, 1e-6 + 2.0 * lse_ulp_share(x, tgt), f"[{rows}, {C}] |x| ~ {scale}")


def hard_against_mlm(x, tgt, tol_loss, tol_grad, what):
    loss, grad = run(x, tgt, H.HARD)
    xg = x.to(dev()).requires_grad_(True)
    ce = mmvqa_amd.mlm_loss(xg, tgt.to(dev()))[0]
    ce.backward()
    print(f"hard vs mlm_loss {what}: loss rel {abs(float(loss) - float(ce)) / abs(float(ce)):.2e}, "
          f"grad err/max {float((grad - xg.grad.cpu()).abs().max() / xg.grad.abs().max()):.2e} (bound {tol_grad:.2e})")
    assert abs(float(loss) - float(ce)) <= tol_loss * abs(float(ce)), what
    assert float((grad - xg.grad.cpu()).abs().max()) <= tol_grad * float(xg.grad.abs().max()), what


@pytest.mark.parametrize("rows,C,scale", [(5, 23, 3.0), (64, 1552, 4.0), (3, 2049, 30.0)])
def test_category_mode_without_smoothing_is_the_hard_mode(rows, C, scale):
    x, tgt, cat, table, _ref = truth(rows, C, scale)
    l0, g0 = run(x, tgt, H.HARD)
    l2, g2 = run(x, tgt, H.CATEGORY, torch.zeros_like(table), cat, smoothing=0.0)
    assert torch.equal(l0, l2) and torch.equal(g0, g2)                   # bit-equal


def test_upstream_gradient_and_determinism():
    x, tgt, cat, table, _ref = truth(64, 1552, 4.0)
    l1, g1 = run(x, tgt, H.CATEGORY, table, cat)
    l2, g2 = run(x, tgt, H.CATEGORY, table, cat)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)                   # two runs are bit-equal
    xg = x.to(dev()).requires_grad_(True)
    (3.0 * mmvqa_amd.soft_ce_loss(xg, tgt.to(dev()), H.CATEGORY, SM, table.to(dev()), cat.to(dev()))).backward()
    assert torch.equal(xg.grad.cpu(), 3.0 * g1)                          # one fp32 multiply by 3 either way


def test_no_gradient_wanted_writes_no_dlogits(monkeypatch):
    """the public path under torch.no_grad() with logits that DO require grad, and with grad mode on for logits that
    do not: the launch gets a null dlogits, nothing of the gradient's size is allocated, nothing is saved"""
    x, tgt, cat, table, _ref = truth(64, 1552, 4.0)
    tg, cg, tb = tgt.to(dev()), cat.to(dev()), table.to(dev())
    l1, _g = run(x, tgt, H.CATEGORY, table, cat)
    calls, inner = [], F._soft_ce

    def spy(*a):
        out = inner(*a)
        calls.append((a[-1], out[2]))
        return out

    monkeypatch.setattr(F, "_soft_ce", spy)
    grad_bytes = 64 * 1552 * 4
    for xg, ctx in ((x.to(dev()).requires_grad_(True), torch.no_grad()), (x.to(dev()), torch.enable_grad())):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with ctx:
            ln = mmvqa_amd.soft_ce_loss(xg, tg, H.CATEGORY, SM, tb, cg)
        torch.cuda.synchronize()
        assert torch.cuda.max_memory_allocated() - before < grad_bytes    # no [rows, ld] buffer ever existed
        assert not ln.requires_grad and ln.grad_fn is None and torch.equal(ln.cpu(), l1)
        want, dl = calls.pop()
        assert want is False and dl is None and not calls
    xg = x.to(dev()).requires_grad_(True)                                 # and with a gradient wanted it is there
    ln = mmvqa_amd.soft_ce_loss(xg, tg, H.CATEGORY, SM, tb, cg)
    want, dl = calls.pop()
    assert want is True and dl.shape == (64, 1552) and ln.requires_grad
    with pytest.raises(mmvqa_amd.MMVQAError, match="nothing is moved"):
        mmvqa_amd.soft_ce_loss(xg, tgt, H.CATEGORY, SM, tb, cg)            # a host target is refused, not copied
    with pytest.raises(mmvqa_amd.MMVQAError, match="nothing is moved"):
        mmvqa_amd.soft_ce_loss(xg, tg, H.CATEGORY, SM, tb, cat)


@pytest.mark.parametrize("C", [23, 2049])
def test_bad_target_or_category_poisons_its_row_only(C):
    rows = 6
    x, tgt, cat, table = H.case(rows, C, 3.0, seed=77)
    xp, ld = F._padded(x.to(dev()))
    tdev = F._padded(table.to(dev()))[0]
    _l, good_rows, good_dl = F._soft_ce(xp, ld, tgt.to(dev()), H.CATEGORY, SM, tdev, cat.to(dev()), True)
    bt, bc = tgt.clone(), cat.clone()
    bt[1], bt[2] = -1, C                        # target outside [0, C)
    bc[4], bc[5] = -1, table.shape[0]           # category outside [0, n_cat)
    loss, row_loss, dl = F._soft_ce(xp, ld, bt.to(dev()), H.CATEGORY, SM, tdev, bc.to(dev()), True)
    torch.cuda.synchronize()
    bad = torch.tensor([False, True, True, False, True, True])
    assert bool(torch.isnan(row_loss.cpu()[bad]).all()) and bool(torch.isnan(dl.cpu()[bad][:, :C]).all())
    assert torch.equal(row_loss.cpu()[~bad], good_rows.cpu()[~bad])      # the neighbours are untouched, bit for bit
    assert torch.equal(dl.cpu()[~bad], good_dl.cpu()[~bad])
    assert bool(torch.isnan(loss.cpu()))
    _l, rl0, _d = F._soft_ce(xp, ld, bt.to(dev()), H.HARD, 0.0, None, None, True)     # hard mode: the target check alone
    assert torch.isnan(rl0.cpu()).tolist() == [False, True, True, False, False, False]
