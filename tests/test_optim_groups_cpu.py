"""Host side of the optimizer groups (no GPU): group matching on the real tensor table of the mini models, segment
merging and its limit, the refusals of FusedAdam and of mmvqa_adam_groups, the state_dict round trip, train.py's options."""
import ctypes as C

import pytest
import torch

import mmvqa_amd
from mmvqa_amd import _lib as L
from mmvqa_amd import train
from mmvqa_amd.optim import FusedAdam, assign_groups, merge_segments, no_decay
from oracle import mmbert_oracle as O

BACKBONE = "transformer.trans.model."


def mini(**kw):
    d = dict(resnet_layers=(1, 1, 1, 1), resnet_width=8, hidden_size=96, n_layers=2, heads=12, vocab_size=50, emb_vocab=50,
             bert_max_pos=32)
    d.update(kw)
    return mmvqa_amd.Model(O.make_args(**d))


MINIS = (dict(), dict(transformer_model="realformer", supcon=True), dict(cnn_encoder="tf_efficientnetv2_m", effnet_depth_div=8),
         dict(transformer_model="feedback-transformer"), dict(dataset="VQA-Med"))


@pytest.mark.parametrize("kw", MINIS, ids=["resnet", "realformer-supcon", "effnet", "feedback", "vqa"])
def test_no_decay_is_every_bias_and_norm_scale(kw):
    """on the real tensor tables: no_decay accepts exactly the one-dimensional tensors -- biases, LayerNorm (the embedding
    LayerNorm included) and BatchNorm scales and shifts -- except the feedback encoder's layer_weight, which is neither"""
    m = mini(**kw)
    got = {n for n, _ in m.named_parameters() if no_decay(n)}
    want = {n for n, p in m.named_parameters() if p.dim() <= 1 and not n.endswith("block.layer_weight")}
    assert got == want, sorted(got ^ want)
    assert {"transformer.bert_embedding.LayerNorm.weight", "transformer.trans.model.bn1.weight", "fc1.bias"} <= got
    assert not any(no_decay(n) for n, p in m.named_parameters() if p.dim() > 1)


def test_group_matching_first_match_wins():
    names = [BACKBONE + "conv1.weight", BACKBONE + "bn1.weight", "fc1.weight", "fc1.bias", "classifier.1.weight"]
    groups = [dict(match=BACKBONE), dict(match=no_decay), dict(match=("fc1.", "classifier."))]
    assert assign_groups(names, groups) == [1, 1, 3, 2, 2]                  # bn1.weight: the backbone group came first
    assert assign_groups(names, groups[1:]) == [0, 1, 2, 1, 1]              # unmatched -> the default group 0
    assert assign_groups(names, [dict(match=lambda n: n.endswith("weight"))]) == [1, 1, 1, 0, 1]


def test_segments_partition_the_buffer_and_merge():
    m = mini()
    lr, wd = 1e-3, 0.01
    opt = FusedAdam(m, lr=lr, weight_decay=wd, groups=[dict(match=BACKBONE, lr=lr / 10), dict(match=no_decay, weight_decay=0.0)])
    assert [g["lr"] for g in opt.param_groups] == [lr, lr / 10, lr] and [g["weight_decay"] for g in opt.param_groups] == [wd, wd, 0.0]
    assert all(g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8 for g in opt.param_groups)
    segs = opt.segments()
    assert segs[0][0] == 0 and segs[-1][1] == m.flat_params.numel()
    assert all(a[1] == b[0] for a, b in zip(segs, segs[1:])) and all(s[0] % 4 == 0 and s[1] % 4 == 0 and s[1] > s[0] for s in segs)
    assert all(a[2:] != b[2:] for a, b in zip(segs, segs[1:])), "adjacent segments with equal settings were not merged"
    assert len(segs) < len(list(m.named_parameters()))
    ranges = {n: (lo, hi) for n, _, lo, hi in m._param_ranges()}
    byname = lambda n: next(s for s in segs if s[0] <= ranges[n][0] < s[1])
    assert byname(BACKBONE + "layer1.0.conv1.weight")[2:] == (lr / 10, wd, L.ADAM_DECOUPLED)
    assert byname(BACKBONE + "layer1.0.bn1.weight")[2:] == (lr / 10, wd, L.ADAM_DECOUPLED)     # first match wins
    assert byname("fc1.bias")[2:] == (lr, 0.0, L.ADAM_DECOUPLED) and byname("fc1.weight")[2:] == (lr, wd, L.ADAM_DECOUPLED)
    # the whole backbone is one segment (one group, contiguous); frozen it is one mode-2 segment without settings
    lo, hi = ranges[BACKBONE + "conv1.weight"][0], ranges[BACKBONE + "fc.bias"][1]
    assert byname(BACKBONE + "conv1.weight")[:2] == (lo, hi)
    m.freeze_backbone()
    assert (lo, hi, 0.0, 0.0, L.ADAM_FROZEN) in opt.segments()
    assert m._frozen_state() == (L.FREEZE_BACKBONE, ((lo, hi),))
    m.freeze_backbone("running")
    assert m._frozen_state()[0] == L.FREEZE_BACKBONE | L.FREEZE_BN_STATS
    m.unfreeze_backbone()
    assert m._frozen_state() == (0, ()) and opt.segments() == segs
    # one tensor frozen elsewhere: no engine flag (its gradient is computed and discarded), a range of its own
    m.fc1.bias.requires_grad_(False)
    assert m._frozen_state() == (0, (ranges["fc1.bias"],))
    assert FusedAdam(m, lr=lr, decoupled=False).segments()[0][4] == L.ADAM_L2


def test_merge_and_the_segment_limit():
    rows = [(0, 4, 1e-3, 0.0, 1), (4, 8, 1e-3, 0.0, 1), (8, 12, 1e-3, 0.1, 1), (12, 16, 5.0, 7.0, 2), (16, 20, 9.0, 1.0, 2)]
    assert merge_segments(rows) == [(0, 8, 1e-3, 0.0, 1), (8, 12, 1e-3, 0.1, 1), (12, 20, 0.0, 0.0, 2)]
    alt = [(4 * i, 4 * i + 4, 1e-3, float(i % 2), 1) for i in range(L.ADAM_MAX_SEGS)]
    assert len(merge_segments(alt)) == L.ADAM_MAX_SEGS
    with pytest.raises(L.MMVQAError, match="4097 segments"):
        merge_segments(alt + [(4 * L.ADAM_MAX_SEGS, 4 * L.ADAM_MAX_SEGS + 4, 1e-3, float(L.ADAM_MAX_SEGS % 2), 1)])


def test_per_group_betas_and_eps_are_refused():
    m = mini()
    for bad in (dict(match="fc1.", betas=(0.8, 0.9)), dict(match="fc1.", eps=1e-6), dict(lr=1e-3)):
        with pytest.raises(ValueError, match="a group is"):
            FusedAdam(m, groups=[bad])
    opt = FusedAdam(m, groups=[dict(match="fc1.", lr=1e-4)])
    opt.param_groups[1]["betas"] = (0.8, 0.9)        # changed behind the constructor's back: refused at the next step
    with pytest.raises(L.MMVQAError, match="shared by all groups"):
        opt._plan(1)


def test_state_dict_round_trip_and_resume_refusal(tmp_path):
    m = mini()
    groups = [dict(match=BACKBONE, lr=1e-4), dict(match=no_decay, weight_decay=0.0)]
    a = FusedAdam(m, lr=1e-3, weight_decay=0.01, groups=groups)
    a.m.normal_(), a.v.uniform_()
    a.step_count = 7
    a.param_groups[1]["lr"] = 1e-5                   # what ReduceLROnPlateau leaves behind
    torch.save(a.state_dict(), tmp_path / "opt.pt")
    sd = torch.load(tmp_path / "opt.pt", weights_only=True)
    b = FusedAdam(m, lr=1e-3, weight_decay=0.01, groups=groups)
    dicts = [id(g) for g in b.param_groups]
    b.load_state_dict(sd)
    assert torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and b.step_count == 7
    assert [g["lr"] for g in b.param_groups] == [1e-3, 1e-5, 1e-3] and [id(g) for g in b.param_groups] == dicts
    assert b.segments() == a.segments()
    for other in (FusedAdam(m, lr=1e-3), FusedAdam(m, lr=1e-3, weight_decay=0.01, groups=groups[:1]),
                  FusedAdam(m, lr=1e-3, weight_decay=0.01, groups=groups, decoupled=False)):
        with pytest.raises(L.MMVQAError, match="optimizer groups .* differ"):
            other.load_state_dict(sd)
    # a state_dict written before there were groups loads into an optimizer without groups
    old = {k: v for k, v in FusedAdam(m, lr=1e-3).state_dict().items() if k != "group_spec"}
    FusedAdam(m, lr=2e-3).load_state_dict(old)
    with pytest.raises(L.MMVQAError, match="optimizer groups .* differ"):
        b.load_state_dict(old)


def test_train_options():
    mode, args = train.parse_args(["mlm"])
    assert (args.weight_decay, args.adam_l2, args.decay_all, args.backbone_lr, args.freeze_backbone, args.freeze_bn_stats) == \
        (0.0, False, False, None, False, False)
    assert train.optimizer_groups(args) == dict(lr=args.lr, weight_decay=0.0, decoupled=True)     # today's optimizer
    for loop in ("mlm", "vqa", "supcon", "distill"):
        _, args = train.parse_args([loop, "--weight_decay", "0.01", "--backbone_lr", "1e-5", "--adam_l2"])
        kw = train.optimizer_groups(args)
        assert kw["weight_decay"] == 0.01 and kw["decoupled"] is False and len(kw["groups"]) == 3
        names = [BACKBONE + "layer1.0.conv1.weight", BACKBONE + "layer1.0.bn1.weight", "fc1.weight", "fc1.bias"]
        g = kw["groups"]
        assert assign_groups(names, g) == [2, 1, 0, 3]
        assert (g[0]["lr"], g[0]["weight_decay"], g[1]["lr"], g[2]["weight_decay"]) == (1e-5, 0.0, 1e-5, 0.0)
    _, args = train.parse_args(["vqa", "--weight_decay", "0.01", "--decay_all", "--clip"])
    assert train.optimizer_groups(args) == dict(lr=args.lr, weight_decay=0.01, decoupled=True) and args.clip is True
    _, args = train.parse_args(["mlm", "--freeze_backbone", "--freeze_bn_stats"])
    assert args.freeze_backbone and args.freeze_bn_stats
    for bad in (["--freeze_bn_stats"], ["--freeze_backbone", "--backbone_lr", "1e-5"], ["--weight_decay", "-1"]):
        with pytest.raises(SystemExit):
            train.parse_args(["mlm"] + bad)


def test_adam_groups_refuses_bad_arguments_on_the_host():
    """as tests/test_abi.py does for the other entry points: MMVQA_ERR_ARG and a message before any HIP call (no GPU here,
    the pointers are never dereferenced)"""
    lib = L.lib()
    assert lib.mmvqa_sizeof_adam_seg() == C.sizeof(L.AdamSeg) == 40

    def tab(*rows):
        t = (L.AdamSeg * len(rows))()
        for h, (b, e, mode) in zip(t, rows):
            h.begin, h.end, h.lr, h.weight_decay, h.mode = b, e, 1e-3, 0.0, mode
        return t

    good = tab((0, 32, 0), (32, 64, 2))
    p = 0x1000

    def call(t=good, lo=0, n=64, ptr=p, dev=p, nseg=None):
        return lib.mmvqa_adam_groups(None, ptr, p, p, p, lo, n, C.cast(t, C.c_void_p) if t is not None else None, dev,
                                     len(t) if nseg is None and t is not None else (nseg or 1), 0.9, 0.999, 1e-8, 1, 1.0, 1)

    cases = (dict(ptr=None), dict(t=None), dict(dev=None), dict(lo=2), dict(n=62), dict(lo=-4), dict(nseg=0), dict(nseg=4097),
             dict(n=68), dict(t=tab((32, 64, 0), (0, 32, 0))), dict(t=tab((0, 32, 0), (28, 64, 0))), dict(t=tab((0, 32, 0), (36, 64, 0))),
             dict(t=tab((0, 30, 0), (30, 64, 0))), dict(t=tab((4, 64, 0))), dict(t=tab((0, 32, 0), (32, 64, 3))),
             dict(t=tab((0, 0, 0), (0, 64, 0))))
    for kw in cases:
        rc = call(**kw)
        assert rc == -1 and lib.mmvqa_last_error().startswith(b"adam_groups:"), (kw, rc, lib.mmvqa_last_error())
    assert call(n=0) == 0          # nothing to do: accepted, nothing launched
    m = mini()
    assert lib.mmvqa_engine_set_frozen(m._handle, 2) == -1 and b"set_frozen:" in lib.mmvqa_last_error()
    assert lib.mmvqa_engine_set_frozen(m._handle, 4) == -1
    assert all(lib.mmvqa_engine_set_frozen(m._handle, f) == 0 for f in (1, 3, 0))
