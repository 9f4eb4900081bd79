"""mmvqa_amd.amp.GradScaler + FusedAdam against torch.amp.GradScaler("cuda") + torch.optim.Adam on one flat parameter,
driven by the same gradient sequence (finite steps, inf / -inf / nan in the first element, the last element and a
ragged tail, growth_interval 3): scale, growth tracker and skip decisions bit-equal at every step; parameters and
Adam moments bit-unchanged over skipped steps and bit-equal to FusedAdam.step(grad_scale=inv_scale) on the others."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import mmvqa_amd  # noqa: E402
from mmvqa_amd.amp import GradScaler  # noqa: E402


class Flat:
    """what FusedAdam needs of a model: the flat parameter and gradient buffers"""

    def __init__(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        self.flat_params = torch.randn(n, generator=g).cuda()
        self.flat_grads = torch.zeros(n, device="cuda")


def bad(n, where, val):
    idx = {"first": [0], "last": [n - 1], "tail": list(range(n - 3, n))}[where]
    return idx, val


def sequence(n):
    inf, nan = float("inf"), float("nan")
    seq = [None, None, ("first", inf), None, None, None, ("last", -inf), None, ("tail", nan), None, None, None, None,
           ("first", nan), None, None, None]
    g = torch.Generator().manual_seed(3)
    for s in seq:
        grad = torch.randn(n, generator=g) * 1e3
        if s is not None:
            idx, v = bad(n, *s)
            grad[idx] = v
        yield grad


def test_scaler_matches_torch_grad_scaler():
    n = 4100   # not a multiple of the 1024 floats a workgroup of the check covers per pass
    ours = Flat(n, 0)
    opt = mmvqa_amd.FusedAdam(ours, lr=1e-3)
    ctl = Flat(n, 0)   # control: the same FusedAdam driven by hand with inv_scale
    opt_ctl = mmvqa_amd.FusedAdam(ctl, lr=1e-3)
    sc = GradScaler(init_scale=2.0 ** 10, growth_interval=3)
    p_t = torch.nn.Parameter(ours.flat_params.clone())
    adam_t = torch.optim.Adam([p_t], lr=1e-3)
    sc_t = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10, growth_interval=3)
    for step, grad in enumerate(sequence(n)):
        g = grad.cuda()
        one = torch.ones(1, device="cuda")
        assert sc.scale(one).item() == sc_t.scale(one).item(), step   # (the gradients below stand for scaled ones)
        scale_before = sc.get_scale()
        assert scale_before == sc_t.get_scale(), step
        ours.flat_grads.copy_(g)
        p_t.grad = g.clone()
        p0, m0, v0, c0 = ours.flat_params.clone(), opt.m.clone(), opt.v.clone(), opt.step_count
        sc.step(opt)
        sc_t.step(adam_t)
        skipped = sc.found_inf()
        assert skipped == (not torch.isfinite(g).all().item()), step
        # torch's decision: its per-device found_inf of this step
        t_found = sum(v.item() for v in sc_t._per_optimizer_states[id(adam_t)]["found_inf_per_device"].values())
        assert skipped == bool(t_found), step
        if skipped:
            assert torch.equal(ours.flat_params, p0) and torch.equal(opt.m, m0) and torch.equal(opt.v, v0)
            assert opt.step_count == c0
        else:
            inv = torch.tensor([scale_before], dtype=torch.float32).double().reciprocal().float().item()
            ctl.flat_grads.copy_(g)
            opt_ctl.step(grad_scale=inv)
            assert torch.equal(ours.flat_params, ctl.flat_params), step
            assert torch.equal(opt.m, opt_ctl.m) and torch.equal(opt.v, opt_ctl.v), step
        sc.update()
        sc_t.update()
        assert sc.get_scale() == sc_t.get_scale(), (step, sc.get_scale(), sc_t.get_scale())
        assert sc._get_growth_tracker() == sc_t._get_growth_tracker(), step
    assert sc.get_scale() != 2.0 ** 10   # the sequence both grew and backed off the scale


def test_scaler_state_dict_round_trip():
    ours = Flat(100, 1)
    opt = mmvqa_amd.FusedAdam(ours, lr=1e-3)
    sc = GradScaler(init_scale=256.0, growth_interval=2)
    for _ in range(3):
        ours.flat_grads.normal_()
        sc.step(opt)
        sc.update()
    sd = sc.state_dict()
    assert set(sd) == set(torch.amp.GradScaler("cuda").state_dict())
    sc2 = GradScaler()
    sc2.load_state_dict(sd)
    assert sc2.state_dict() == sd
    ours.flat_grads.normal_()
    sc2.scale(torch.ones(1, device="cuda"))
    assert sc2.get_scale() == sd["scale"] and sc2._get_growth_tracker() == sd["_growth_tracker"]


@pytest.mark.parametrize("n,offset", [(4099, 0), (4099, 1), (3, 2), (1 << 20, 3)])
@pytest.mark.parametrize("where", [None, "first", "last", "tail"])
def test_unscale_kernel_ragged_and_misaligned(n, offset, where):
    """mmvqa_amp_unscale against torch._amp_foreach_non_finite_check_and_unscale_ on lengths that are not multiples of 4
    and on buffers that start off the 16-byte boundary (the scalar branch): same flag, bit-equal unscaled values"""
    from mmvqa_amd import _lib as L
    g = torch.Generator().manual_seed(n + offset)
    base = torch.randn(n + offset, generator=g).cuda() * 1e3
    buf = base[offset:]
    pre = base[:offset].clone()
    if where is not None:
        idx, v = bad(n, where, float("nan") if where == "tail" else float("inf"))
        buf[idx] = v
    ref = buf.clone()
    inv = torch.full((1,), 1.0 / 3000.0, device="cuda")
    found_t = torch.zeros(1, device="cuda")
    torch._amp_foreach_non_finite_check_and_unscale_([ref], found_t, inv)
    found = torch.zeros(1, device="cuda")
    L.check(L.lib().mmvqa_amp_unscale(L.stream_ptr(), L.ptr(buf), n, L.ptr(inv), L.ptr(found), 1))
    torch.cuda.synchronize()
    assert float(found) == float(found_t) == (0.0 if where is None else 1.0)
    fin = torch.isfinite(ref)
    assert torch.equal(buf[fin], ref[fin]) and torch.equal(torch.isfinite(buf), fin)
    assert torch.equal(base[:offset], pre)
