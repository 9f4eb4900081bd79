"""Frozen backbone and optimizer groups on the whole model: requires_grad is honoured, the backbone's backward pass is
skipped (mmvqa_engine_set_frozen), FusedAdam takes groups, weight decay and frozen parameters (mmvqa_adam_groups)."""
import copy

import pytest
import torch
from torch.optim import lr_scheduler

pytestmark = pytest.mark.gpu

import mmvqa_amd  # noqa: E402
from mmvqa_amd import synth  # noqa: E402
from mmvqa_amd.optim import no_decay  # noqa: E402
from mmvqa_amd.train import _SchedShim  # noqa: E402
from hip_helpers import dev, relerr  # noqa: E402
from test_hip_model import TOL, build_pair, compare_grads, mini_args, oracle_loss  # noqa: E402

BACKBONE = "transformer.trans.model."
EFF = dict(cnn_encoder="tf_efficientnetv2_m", effnet_depth_div=8)
DROPOUT = dict(hidden_dropout_prob=0.3, emb_dropout_prob=0.1, rf_dropout_prob=0.1)
B, T, HW = 3, 12, 32


def reference_freeze(model):
    """models/image_encoding.py:50-51, where self.parameters() are the backbone's"""
    for p in model.transformer.trans.model.parameters():
        p.requires_grad = False


def backbone_range(hip):
    r = [(lo, hi) for name, _, lo, hi in hip._param_ranges() if name.startswith(BACKBONE)]
    assert all(a[1] == b[0] for a, b in zip(r, r[1:]))      # one contiguous range
    return r[0][0], r[-1][1]


def batch(kind, args, seed=5):
    if kind == "vqa":
        return synth.vqa_batch(B, T, HW, vocab=args.emb_vocab, n_classes=args.vocab_size, seed=seed)
    return synth.roco_batch(B, T, HW, vocab=args.vocab_size, seed=seed, mlm_prob=0.3)


def hip_loss(kind, out, tgt):
    return mmvqa_amd.asl_loss(out[0], tgt) if kind == "vqa" else mmvqa_amd.mlm_loss(out, tgt)[0]


def frozen_case(args, kind, bn_stats, dropout_seed=None, stat_tol=1e-4):
    orc, hip = build_pair(args, seed=0, dropout_seed=dropout_seed)
    img, ids, seg, mask, tgt = batch(kind, args)
    reference_freeze(orc)
    orc.train()
    if bn_stats == "running":                 # backbone.eval() inside model.train()
        for m in orc.transformer.trans.model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.eval()
        hip.freeze_backbone(bn_stats="running")
    else:
        reference_freeze(hip)
    before = {k: v.detach().clone() for k, v in orc.state_dict().items()}
    orc64 = copy.deepcopy(orc).double()       # (keeps requires_grad, the train / eval flags and the injected dropout)
    out_ref = orc(img, ids, seg, mask)
    loss_ref = oracle_loss(kind, out_ref, tgt, B)
    loss_ref.backward()
    oracle_loss(kind, orc64(img.double(), ids, seg, mask), tgt, B).backward()
    hip.train()
    if dropout_seed is not None:
        hip.set_seed(dropout_seed)
    dimg, dids, dseg, dmask, dtgt = (t.to(dev()) for t in (img, ids, seg, mask, tgt))
    out = hip(dimg, dids, dseg, dmask)
    loss = hip_loss(kind, out, dtgt)
    logits, logits_ref = (out[0], out_ref[0]) if kind == "vqa" else (out, out_ref)
    e = relerr(logits, logits_ref)
    assert e <= TOL, f"logits rel err {e:.2e}"
    assert abs(float(loss) - float(loss_ref)) <= TOL * abs(float(loss_ref)), (float(loss), float(loss_ref))
    loss.backward()
    torch.cuda.synchronize()
    compare_grads(orc, hip, orc64)            # every unfrozen gradient; a frozen one must be None or zero there
    frozen = [n for n, p in hip.named_parameters() if n.startswith(BACKBONE)]
    assert len(frozen) > 20
    hp = dict(hip.named_parameters())
    assert all(hp[n].grad is None and not hp[n].requires_grad for n in frozen)
    assert sum(p.grad is not None for n, p in hp.items() if not n.startswith(BACKBONE)) > 20
    lo, hi = backbone_range(hip)
    assert float(hip.flat_grads[lo:hi].abs().max()) == 0.0, "the frozen range of flat_grads is not exactly zero"
    assert float(hip.flat_grads[hi:].abs().max()) > 0.0
    osd, hsd = orc.state_dict(), hip.state_dict()
    moved = 0
    for k, v in osd.items():
        if "running_" in k or k.endswith("num_batches_tracked"):
            if bn_stats == "running":
                assert torch.equal(v, before[k]), f"oracle {k} moved"
                assert torch.equal(hsd[k].cpu(), before[k]), f"{k} is not bit-unchanged"
            elif "running_" in k:
                assert relerr(hsd[k], v) <= stat_tol, f"{k}: {relerr(hsd[k], v):.2e}"
                moved += int(not torch.equal(v, before[k]))
            else:
                assert int(hsd[k]) == int(v) > int(before[k]), k
    assert bn_stats == "running" or moved > 20
    return hip


# ----------------------------------------------------------------------------- 6 / 7: against the oracle
@pytest.mark.parametrize("kind,kw", [("mlm", dict(transformer_model="transformer")),
                                     ("vqa", dict(transformer_model="realformer", dataset="VQA-Med")),
                                     ("mlm", dict(transformer_model="transformer", **EFF))],
                         ids=["mlm-transformer", "vqa-realformer", "effnet"])
def test_frozen_backbone_against_the_oracle(kind, kw):
    """both models frozen with the reference's own (commented-out) lines: logits, loss and every unfrozen gradient within
    run_case's rule (TOL, or 5 x the fp32 oracle's distance from its fp64 run); frozen parameters have no .grad and an
    exactly zero range in flat_grads; the running statistics move as the oracle's do"""
    frozen_case(mini_args(**kw), kind, "batch")


@pytest.mark.parametrize("kw", [dict(), EFF], ids=["resnet", "effnet"])
def test_frozen_backbone_on_running_statistics(kw):
    """freeze_backbone(bn_stats="running") against the oracle with its backbone BatchNorms in .eval() and the rest in
    train mode, dropout on with the engine's masks: the same bounds; running_mean / running_var / num_batches_tracked
    bit-unchanged"""
    frozen_case(mini_args(**DROPOUT, **kw), "mlm", "running", dropout_seed=21)


# ----------------------------------------------------------------------------- 8: the compute is skipped
def region_launches(hip, fn):
    hip.profile(True)
    fn()
    torch.cuda.synchronize()
    r = hip.profile_read_regions()
    hip.profile(False)
    return {reg: sum(c["launches"] for c in cls.values()) for reg, cls in r.items()}


# launches of one unfrozen forward + backward of the mini models at B 3, T 12, 32 x 32, recorded from the parent commit
PARENT_COUNTS = {
    "resnet": {"backbone": 56, "tap": 20, "qkv": 8, "attention": 4, "encoder_rest": 30, "heads": 13, "embed": 2, "bn_coef": 2,
               "qkv_attention_fused": 0},
    "effnet": {"backbone": 135, "tap": 20, "qkv": 8, "attention": 4, "encoder_rest": 30, "heads": 13, "embed": 2, "bn_coef": 22,
               "qkv_attention_fused": 0},
}


@pytest.mark.parametrize("cnn", ["resnet", "effnet"])
def test_frozen_backward_launches_nothing_in_the_backbone(cnn):
    """Model.profile counts per region.  Frozen forward + backward: the backbone and BatchNorm-coefficient regions count
    what a train-mode forward under no_grad counts (the backward adds nothing there), the tap region counts the five
    forward taps plus recompute and weight gradient of each (5 + 2 * 5).  Unfrozen, the counts are the parent commit's
    (PARENT_COUNTS above: one forward + backward of the mini model at B 3, T 12, 32 x 32 on the parent build)."""
    args = mini_args(**(EFF if cnn == "effnet" else {}))
    _, hip = build_pair(args, seed=2)
    hip.train()
    img, ids, seg, mask, tgt = (t.to(dev()) for t in batch("mlm", args))

    def fwd_bwd():
        mmvqa_amd.mlm_loss(hip(img, ids, seg, mask), tgt)[0].backward()

    def fwd_only():
        with torch.no_grad():
            hip(img, ids, seg, mask)

    full = region_launches(hip, fwd_bwd)
    fwd = region_launches(hip, fwd_only)
    hip.freeze_backbone()
    froz = region_launches(hip, fwd_bwd)
    hip.unfreeze_backbone()
    again = region_launches(hip, fwd_bwd)
    print(f"{cnn}: unfrozen {full}\n forward {fwd}\n frozen {froz}")
    assert fwd["tap"] == 5
    assert froz["backbone"] == fwd["backbone"] and froz["bn_coef"] == fwd["bn_coef"]
    assert froz["tap"] == 5 + 2 * 5
    assert full["backbone"] > fwd["backbone"] and full["tap"] == 5 + 3 * 5
    for reg in ("qkv", "attention", "encoder_rest", "heads", "embed", "qkv_attention_fused"):
        assert froz[reg] == full[reg], reg          # everything above the taps runs as always
    assert again == full
    assert full == PARENT_COUNTS[cnn]


# ----------------------------------------------------------------------------- 9 / 10: optimizers and a frozen backbone
def train_batches(n, seed0=20):
    return [tuple(t.to(dev()) for t in synth.roco_batch(B, T, HW, vocab=50, seed=seed0 + i, mlm_prob=0.3)) for i in range(n)]


def step(model, opt, b):
    img, ids, seg, mask, tgt = b
    opt.zero_grad()
    mmvqa_amd.mlm_loss(model(img, ids, seg, mask), tgt)[0].backward()
    opt.step()


def assert_follows(pa, pb, lr, names, what):
    """the rule of test_stock_torch_adam_steps_the_flat_buffer: at most 1 % of a tensor's elements off by more than
    0.05 lr (elements whose gradient is ~0 are decided by the order of the float atomics)"""
    for n in names:
        if n.endswith("proj_k.bias"):     # gradient identically 0 in exact arithmetic: pure noise
            continue
        off = ((pa[n].detach() - pb[n].detach()).abs() > 0.05 * lr).float().mean().item()
        assert off <= 0.01, f"{what}: {n}: {off:.3f} of the elements differ"


def test_freezing_mid_training_keeps_parameters_and_moments():
    """two steps unfrozen (m and v non-zero), then two steps frozen: the backbone's parameters, m and v are bit-equal to
    their values after step two; the rest follows a torch.optim.Adam twin frozen at the same point"""
    args = mini_args()
    _, a = build_pair(args, seed=9)
    _, b = build_pair(args, seed=9)
    a.train(), b.train()
    lr = 1e-3
    opt_a = mmvqa_amd.FusedAdam(a, lr=lr)
    bs = train_batches(4)
    opt_b = None
    for i, bt in enumerate(bs):
        if i == 2:
            lo, hi = backbone_range(a)
            torch.cuda.synchronize()
            kept = [t[lo:hi].clone() for t in (a.flat_params, opt_a.m, opt_a.v)]
            assert all(float(t.abs().max()) > 0 for t in kept)
            a.freeze_backbone()
            reference_freeze(b)
            for p in b.transformer.trans.model.parameters():
                p.grad = None                       # torch.optim.Adam skips a parameter without .grad
        step(a, opt_a, bt)
        if opt_b is None:
            img, ids, seg, mask, tgt = bt
            mmvqa_amd.mlm_loss(b(img, ids, seg, mask), tgt)[0].backward()
            opt_b = torch.optim.Adam(b.parameters(), lr=lr)
            opt_b.step()
        else:
            step(b, opt_b, bt)
    torch.cuda.synchronize()
    for t, k, what in zip((a.flat_params, opt_a.m, opt_a.v), kept, ("parameters", "m", "v")):
        assert torch.equal(t[lo:hi], k), f"backbone {what} changed while frozen"
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert_follows(pa, pb, lr, [n for n in pa if not n.startswith(BACKBONE)], "after freezing")
    assert float((a.flat_params[hi:] - b.flat_params[hi:]).abs().max()) < 10 * lr


def test_stock_torch_adam_leaves_a_frozen_backbone_alone():
    """torch.optim.Adam(model.parameters()) on a model frozen with the reference's lines: the backbone is bit-unchanged
    after two steps, the rest moves"""
    args = mini_args()
    _, m = build_pair(args, seed=9)
    m.train()
    reference_freeze(m)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    lo, hi = backbone_range(m)
    start = m.flat_params.clone()
    for bt in train_batches(2):
        step(m, opt, bt)
    torch.cuda.synchronize()
    assert torch.equal(m.flat_params[lo:hi], start[lo:hi]), "a frozen backbone parameter moved"
    moved = (m.flat_params[hi:] != start[hi:]).float().mean().item()
    assert moved > 0.5, moved


# ----------------------------------------------------------------------------- 11: groups end to end
def test_groups_follow_torch_adamw_and_the_scheduler():
    """FusedAdam(groups=[backbone at lr / 10, no_decay tensors without decay], weight_decay=0.01) against
    torch.optim.AdamW with the same three groups on a twin, two steps; then ReduceLROnPlateau scales every group's lr
    and the third update uses the new values (compared as the step's own displacement, at the new rates)"""
    args = mini_args()
    _, a = build_pair(args, seed=9)
    _, b = build_pair(args, seed=9)
    a.train(), b.train()
    lr, wd = 1e-3, 0.01
    opt_a = mmvqa_amd.FusedAdam(a, lr=lr, weight_decay=wd,
                                groups=[dict(match=BACKBONE, lr=lr / 10), dict(match=no_decay, weight_decay=0.0)])
    assert [g["lr"] for g in opt_a.param_groups] == [lr, lr / 10, lr]
    assert [g["weight_decay"] for g in opt_a.param_groups] == [wd, wd, 0.0]
    pb = dict(b.named_parameters())
    sets = [[], [], []]
    for n, p in pb.items():
        sets[1 if n.startswith(BACKBONE) else 2 if no_decay(n) else 0].append(p)
    rate = {n: (lr / 10 if n.startswith(BACKBONE) else lr) for n in pb}
    bs = train_batches(3)
    img, ids, seg, mask, tgt = bs[0]
    step(a, opt_a, bs[0])
    mmvqa_amd.mlm_loss(b(img, ids, seg, mask), tgt)[0].backward()
    opt_b = torch.optim.AdamW([dict(params=sets[0], lr=lr, weight_decay=wd), dict(params=sets[1], lr=lr / 10, weight_decay=wd),
                               dict(params=sets[2], lr=lr, weight_decay=0.0)], lr=lr)
    opt_b.step()
    step(a, opt_a, bs[1]), step(b, opt_b, bs[1])
    torch.cuda.synchronize()
    pa = dict(a.named_parameters())
    for n in pa:
        assert_follows(pa, pb, rate[n], [n], "two steps with groups")
    scheds = [lr_scheduler.ReduceLROnPlateau(_SchedShim(opt_a), patience=0, factor=0.1),
              lr_scheduler.ReduceLROnPlateau(opt_b, patience=0, factor=0.1)]
    for s in scheds:
        s.step(1.0), s.step(2.0)
    new = [g["lr"] for g in opt_a.param_groups]
    assert all(abs(x - y / 10) <= 1e-12 for x, y in zip(new, (lr, lr / 10, lr))), new
    assert all(abs(ga["lr"] - gb["lr"]) <= 1e-15 for ga, gb in zip(opt_a.param_groups, opt_b.param_groups))
    before_a, before_b = a.flat_params.clone(), b.flat_params.clone()
    key = opt_a._key
    step(a, opt_a, bs[2]), step(b, opt_b, bs[2])
    torch.cuda.synchronize()
    assert opt_a._key != key            # the table was rebuilt for the new rates
    da, db = a.flat_params - before_a, b.flat_params - before_b
    for n, _, lo, hi in a._param_ranges():
        if n.endswith("proj_k.bias"):
            continue
        r = rate[n] / 10
        off = ((da[lo:hi] - db[lo:hi]).abs() > 0.05 * r).float().mean().item()
        assert off <= 0.01, f"third step at the reduced rate: {n}: {off:.3f} of the elements differ"
        assert float(da[lo:hi].abs().max()) <= 3 * r, f"{n} moved further than the reduced rate allows"


# ----------------------------------------------------------------------------- 12: overlap_backward, GradScaler.step
def grouped(model, lr=1e-3):
    return mmvqa_amd.FusedAdam(model, lr=lr, weight_decay=0.01,
                               groups=[dict(match="classifier.", lr=lr / 10), dict(match=no_decay, weight_decay=0.0)])


def test_overlap_and_scaler_with_groups_and_a_frozen_backbone():
    """on FIXED gradients: ranged updates driven as overlap_backward() drives them, and GradScaler.step on gradients
    multiplied by its scale, give the bits of the plain step() of the same configuration (groups, weight decay, frozen
    backbone), step after step; a step skipped for an inf leaves parameters, moments and the step count untouched;
    in a real backward the announcements still partition the buffer and the frozen backbone stays where it is"""
    args = mini_args()
    models = [build_pair(args, seed=11)[1] for _ in range(3)]
    for m in models:
        m.train()
        m.freeze_backbone()
    a, b, c = models
    opt_a, opt_b, opt_c = grouped(a), grouped(b), grouped(c)
    n = a.flat_params.numel()
    lo, hi = backbone_range(a)
    start = a.flat_params.clone()
    opt_b.overlap_backward()
    scaler = mmvqa_amd.amp.GradScaler(init_scale=2.0 ** 10)
    cuts = [0, 4 * (n // 12), 4 * (n // 7), 4 * (n // 5), n - 4 * (n // 9), n]   # [cuts[3], cuts[4]) is never announced
    gen = torch.Generator(device="cuda").manual_seed(5)
    for it in range(2):
        g = torch.randn(n, device=dev(), generator=gen)
        a.flat_grads.copy_(g), b.flat_grads.copy_(g), c.flat_grads.copy_(g * 2.0 ** 10)
        ev = torch.cuda.Event()
        ev.record()
        for l, h in ((cuts[4], cuts[5]), (cuts[0], cuts[1]), (cuts[2], cuts[3]), (cuts[1], cuts[2])):
            opt_b._on_ready(l, h, ev)
        opt_a.step(), opt_b.step()
        scaler.scale(torch.ones(1, device=dev()))
        scaler.step(opt_c)
        scaler.update()
        torch.cuda.synchronize()
        assert opt_a._segs is not None      # the table-driven kernel ran
        for o, m, what in ((opt_b, b, "overlap_backward"), (opt_c, c, "GradScaler.step")):
            assert torch.equal(a.flat_params, m.flat_params) and torch.equal(opt_a.m, o.m) and torch.equal(opt_a.v, o.v), \
                f"{what} differs from the plain step at step {it + 1}"
            assert float(m.flat_grads.abs().max()) == 0.0
        assert opt_b._done == []
    assert torch.equal(a.flat_params[lo:hi], start[lo:hi]) and float(opt_a.m[lo:hi].abs().max()) == 0.0
    assert not torch.equal(a.flat_params[hi:], start[hi:])
    # a skipped step
    keep = [t.clone() for t in (c.flat_params, opt_c.m, opt_c.v)]
    c.flat_grads.copy_(torch.randn(n, device=dev(), generator=gen))
    c.flat_grads[hi + 5] = float("inf")
    scaler.scale(torch.ones(1, device=dev()))
    assert scaler.step(opt_c) is None and scaler.found_inf()
    scaler.update()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip((c.flat_params, opt_c.m, opt_c.v), keep)) and opt_c.step_count == 2
    # a real backward beside the ranged updates
    img, ids, seg, mask, tgt = train_batches(1)[0]
    before = b.flat_params.clone()
    opt_b.zero_grad()
    mmvqa_amd.mlm_loss(b(img, ids, seg, mask), tgt)[0].backward()
    done = sorted(opt_b._done)
    assert done[0][0] == 0 and done[-1][1] == n and all(x[1] == y[0] for x, y in zip(done, done[1:]))
    opt_b.step()
    torch.cuda.synchronize()
    assert torch.equal(b.flat_params[lo:hi], before[lo:hi]) and not torch.equal(b.flat_params[hi:], before[hi:])
    assert float(b.flat_grads.abs().max()) == 0.0
