"""GPU parity of Model.forward_grouped against the CPU oracle in fp32 and fp64.

The oracle's semantics are given here, on the test side: the forward of the oracle's image encoder (transformer.trans) is
replaced by one that returns tuple(v[group] for v in original(img)) -- the backbone and its BatchNorms see the NI images,
prepare_input overwrites the visual rows of sample b with the tokens of image group[b], and autograd supplies the
scatter-add of the token gradients.  Nothing under oracle/ changes: the instance does (the way
test_hip_amp_model.emulate_f16 swaps forwards).

Every tensor has the rule of test_hip_model.py: within max(TOL, 5 x the fp32 oracle's own distance from its fp64 run) of
the fp64 run, with that file's TOL -- logits, loss, every parameter gradient, the BatchNorm running statistics;
num_batches_tracked exactly."""
import copy
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import mmvqa_amd  # noqa: E402
from mmvqa_amd import synth, _lib as L  # noqa: E402
from hip_helpers import dev, relerr  # noqa: E402
from dropout_helpers import engine_seed  # noqa: E402
from test_hip_model import TOL, DROPOUT, build_pair, mini_args, oracle_loss, compare_grads  # noqa: E402
from test_hip_amp_model import emulate_f16  # noqa: E402
from test_hip_feedback_model import build_pair as build_feedback_pair, fb_args  # noqa: E402

BACKBONE = "transformer.trans.model."


def group_oracle(orc, group):
    """the oracle of a grouped batch: see the module docstring"""
    trans = orc.transformer.trans
    original = trans.forward
    trans.forward = lambda img: tuple(v[group] for v in original(img))
    return orc


def grouped_inputs(args, counts, T, hw, kind, seed=5):
    NI, V = len(counts), args.vocab_size
    if kind == "vqa":
        return synth.vqa_grouped_batch(NI, counts, T, hw, vocab=args.emb_vocab, n_classes=V, seed=seed)
    B = sum(counts)
    img, ids, seg, mask, tgt = synth.roco_batch(B, T, hw, vocab=V, seed=seed, mlm_prob=0.3)
    group = torch.repeat_interleave(torch.arange(NI), torch.tensor(counts))
    return img[:NI].contiguous(), group, ids, seg, mask, tgt


def hip_loss(kind, out, tgt):
    return mmvqa_amd.asl_loss(out[0], tgt) if kind == "vqa" else mmvqa_amd.mlm_loss(out, tgt)[0]


def first(out, kind):
    return out[0] if kind == "vqa" else out


class Checker:
    """collects (name, error, tolerance) of every tensor outside its rule"""

    def __init__(self):
        self.bad, self.n = [], 0

    def __call__(self, name, got, r32, r64, tol=TOL):
        t = max(tol, 5 * relerr(r32, r64))
        e = relerr(got, r64)
        self.n += 1
        if not e <= t:
            self.bad.append(f"{name} {e:.2e} (tol {t:.1e})")

    def direct(self, name, x, y, r32, r64, tol=TOL):
        """x against y, two results of the code under test, with the tolerance the oracle pair gives the tensor"""
        t = max(tol, 5 * relerr(r32, r64))
        e = relerr(x, y)
        self.n += 1
        if not e <= t:
            self.bad.append(f"{name} {e:.2e} between the two runs (tol {t:.1e})")

    def done(self):
        assert not self.bad, f"{len(self.bad)} of {self.n} tensors outside their rule: " + ", ".join(self.bad[:12])


def oracle_step(orc, orc64, batch, kind, group=None):
    """one step of the fp32 and the fp64 oracle -> (out32, loss32, out64, loss64); group=None: the plain model"""
    img, ids, seg, mask, tgt = batch
    B = ids.shape[0]
    if group is not None:
        group_oracle(orc, group)
        group_oracle(orc64, group)
    out = orc(img, ids, seg, mask)
    loss = oracle_loss(kind, out, tgt, B)
    loss.backward()
    out64 = orc64(img.double(), ids, seg, mask)
    loss64 = oracle_loss(kind, out64, tgt, B)
    loss64.backward()
    return out, loss, out64, loss64


def same_step(a, b, orc, orc64, kind, ref):
    """Two HIP steps held to EACH OTHER: a and b are (model, logits, loss) of two runs that compute the same thing.
    They run the same launches on the same numbers and differ by what the order of the BatchNorm atomics leaves, which
    the existing tests record as not bit-equal.  The comparison is the two runs'; the tolerance of a tensor is the
    rule's, max(TOL, 5 x the fp32 oracle's distance from its fp64 run) -- the noise fp32 arithmetic leaves in it."""
    out, loss_ref, out64, loss64 = ref
    (ma, la, sa), (mb, lb, sb) = a, b
    chk = Checker()
    chk.direct("logits", la, lb, first(out, kind).detach(), first(out64, kind).detach())
    chk.direct("loss", sa.detach().reshape(1), sb.detach().reshape(1), loss_ref.detach().reshape(1), loss64.detach().reshape(1))
    pa, pb, p64 = dict(ma.named_parameters()), dict(mb.named_parameters()), dict(orc64.named_parameters())
    n = 0
    for name, p in orc.named_parameters():
        if p.grad is None:
            continue
        assert pa[name].grad is not None and pb[name].grad is not None, name
        chk.direct(name, pa[name].grad, pb[name].grad, p.grad, p64[name].grad)
        n += 1
    assert n > 20, n
    ba, bb, b64 = dict(ma.named_buffers()), dict(mb.named_buffers()), dict(orc64.named_buffers())
    for name, buf in orc.named_buffers():
        if name.endswith(("running_mean", "running_var")):
            chk.direct(name, ba[name], bb[name], buf, b64[name])
        elif name.endswith("num_batches_tracked"):
            assert int(ba[name]) == int(bb[name]), name
    chk.done()


def check_step(hip, orc, orc64, kind, logits, loss, ref):
    """logits, loss, gradients and BatchNorm buffers of the HIP model against the oracle pair, each under its rule"""
    out, loss_ref, out64, loss64 = ref
    chk = Checker()
    chk("logits", logits, first(out, kind), first(out64, kind))
    chk("loss", loss.detach().reshape(1), loss_ref.detach().reshape(1), loss64.detach().reshape(1))
    hp, p64 = dict(hip.named_parameters()), dict(orc64.named_parameters())
    n = 0
    for name, p in orc.named_parameters():
        g = hp[name].grad
        if p.grad is None:
            assert g is None or float(g.abs().max()) == 0.0, f"{name}: the oracle has no gradient"
            continue
        assert g is not None, f"{name}: missing gradient"
        chk(name, g, p.grad, p64[name].grad)
        n += 1
    assert n > 20, n
    hb, b64 = dict(hip.named_buffers()), dict(orc64.named_buffers())
    for name, b in orc.named_buffers():
        if name.endswith(("running_mean", "running_var")):
            chk(name, hb[name], b, b64[name])
        elif name.endswith("num_batches_tracked"):
            assert int(hb[name]) == int(b), name
    chk.done()


def run_grouped(args, counts, T, hw, kind, training=True, dropout_seed=None, builder=build_pair, autocast=False,
                freeze=False, seed=0):
    orc, hip = builder(args, seed, dropout_seed)
    img, group, ids, seg, mask, tgt = grouped_inputs(args, counts, T, hw, kind)
    orc64 = copy.deepcopy(orc).double()
    if autocast:
        emulate_f16(orc)
        emulate_f16(orc64)
    for m in (orc, orc64, hip):
        m.train(training)
    if freeze:
        hip.freeze_backbone()
        for o in (orc, orc64):
            for n, p in o.named_parameters():
                if n.startswith(BACKBONE):
                    p.requires_grad_(False)
    ref = oracle_step(orc, orc64, (img, ids, seg, mask, tgt), kind, group)
    dimg, dids, dseg, dmask, dtgt = (t.to(dev()) for t in (img, ids, seg, mask, tgt))
    if dropout_seed is not None:
        hip.set_seed(dropout_seed)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        out = hip.forward_grouped(dimg, group, dids, dseg, dmask)
        if dropout_seed is not None:   # the base seed the oracle's masks were drawn from is the one the engine received
            assert hip._seed_ctr == engine_seed(dropout_seed)
        if kind == "vqa":
            assert out[1] == 0 and out[2] == 0
        logits = first(out, kind)
        loss = hip_loss(kind, out, dtgt)
    assert logits.dtype == torch.float32 and logits.shape[0] == sum(counts)
    loss.backward()
    torch.cuda.synchronize()
    check_step(hip, orc, orc64, kind, logits, loss, ref)
    return SimpleNamespace(orc=orc, orc64=orc64, hip=hip, batch=(img, group, ids, seg, mask, tgt), logits=logits.detach(),
                           loss=loss.detach(), ref=ref)


def vqa_args(**kw):
    return mini_args(dataset="VQA-Med", vocab_size=23, **kw)


# NI >= 2 in train mode: the deepest map of the mini ResNet at 32 x 32 is 1 x 1, and torch refuses train-mode BatchNorm
# over a single value per channel
@pytest.mark.parametrize("tm", ["transformer", "realformer"])
def test_resnet_vqa_uneven_groups(tm):
    run_grouped(vqa_args(transformer_model=tm), [1, 3, 2], T=10, hw=32, kind="vqa")


@pytest.mark.parametrize("tm", ["transformer", "realformer"])
def test_one_question_per_image_is_the_ungrouped_step(tm):
    """counts [1, 1, 1]: the oracle's rule, and the ungrouped forward + backward of a fresh model on the same inputs
    (expand and sum are copies here): logits, loss, every gradient and the BatchNorm buffers of the two HIP steps are
    held to each other (same_step)."""
    args = vqa_args(transformer_model=tm)
    r = run_grouped(args, [1, 1, 1], T=10, hw=32, kind="vqa")
    img, group, ids, seg, mask, tgt = r.batch
    assert group.tolist() == [0, 1, 2]
    _, plain = build_pair(args, 0)
    plain.train()
    dimg, dids, dseg, dmask, dtgt = (t.to(dev()) for t in (img, ids, seg, mask, tgt))
    out = plain(dimg, dids, dseg, dmask)
    loss = mmvqa_amd.asl_loss(out[0], dtgt)
    loss.backward()
    same_step((r.hip, r.logits, r.loss), (plain, out[0].detach(), loss.detach()), r.orc, r.orc64, "vqa", r.ref)


def test_effnet_vqa():
    run_grouped(vqa_args(cnn_encoder="tf_efficientnetv2_m", effnet_depth_div=8), [2, 3], T=10, hw=64, kind="vqa")


# Two images in train mode run at 64 x 64, where the deepest map is 2 x 2.  At 32 x 32 it is 1 x 1 and layer4's BatchNorms
# normalise TWO values per channel: the output is +-gamma + beta whatever the input, the input gradient is the
# cancellation residual g - mean(g) - xhat mean(g xhat) = +-(g1 - g2)/2 * eps / (var + eps), and every gradient below it
# carries that residual's rounding.  The UNGROUPED step of the parent code misses the rule there in the same way (measured:
# feedback-transformer, B = 2, T = 8, 32 x 32, every backbone gradient 4.1e-3 .. 4.8e-3 against 1e-3; B = 3 passes), so
# the shape would test BatchNorm's conditioning, not the grouping.
def test_mlm_head():
    run_grouped(mini_args(), [2, 2], T=12, hw=64, kind="mlm")


def test_feedback_transformer():
    run_grouped(fb_args(dataset="VQA-Med", vocab_size=23), [1, 2], T=8, hw=64, kind="vqa", builder=build_feedback_pair)


def test_eval_mode():
    """running statistics: per-image arithmetic, BatchNorm buffers untouched; the gradient still sums over the questions"""
    run_grouped(vqa_args(), [4, 1], T=10, hw=32, kind="vqa", training=False)


def test_dropout():
    """the dropout sites are those of the B text rows, as in the ungrouped step: the oracle under the engine's own masks"""
    run_grouped(vqa_args(**DROPOUT), [1, 3, 2], T=10, hw=32, kind="vqa", dropout_seed=11)


def test_fp16_autocast():
    """the mixed-precision mode against the operand-rounding oracle of test_hip_amp_model.py; the two new kernels are fp32.
    Four images at 32 x 32: the image count and size of that file's VQA case (test_mixed_step_vqa_head, B = 4), the
    shape at which the mode's parity rule is established.  With three images there the fp32 emulating oracle is itself
    3 % from its fp64 run (tolerances of 6 - 21 %), which checks little."""
    run_grouped(vqa_args(), [1, 3, 2, 1], T=10, hw=32, kind="vqa", autocast=True, seed=31)


def test_frozen_backbone():
    """freeze_backbone(): tap and encoder gradients as the oracle's, no gradient below the taps"""
    hip = run_grouped(vqa_args(), [1, 3, 2], T=10, hw=32, kind="vqa", freeze=True).hip
    n = 0
    for name, p, lo, hi in hip._param_ranges():
        if name.startswith(BACKBONE):
            assert p.grad is None, name
            assert float(hip.flat_grads[lo:hi].abs().max()) == 0.0, name
            n += 1
    assert n > 10
    assert dict(hip.named_parameters())["transformer.trans.conv2.weight"].grad is not None


def test_uniform_multiplicity_equals_the_duplicated_batch():
    """counts [2, 2, 2]: every image counts twice in the duplicated batch img[group], so its BatchNorm means and biased
    variances are the grouped batch's, and so are the parameter gradients: the grouped step's
    gradients also match the PLAIN oracle run on the duplicated batch.  (The running variances differ by the unbiased
    n / (n - 1) factor and are not compared.)"""
    args = vqa_args(transformer_model="realformer")
    r = run_grouped(args, [2, 2, 2], T=10, hw=32, kind="vqa")
    hip, (img, group, ids, seg, mask, tgt) = r.hip, r.batch
    orc, _ = build_pair(args, 0)
    orc64 = copy.deepcopy(orc).double()
    orc.train()
    orc64.train()
    oracle_step(orc, orc64, (img[group], ids, seg, mask, tgt), "vqa")
    compare_grads(orc, hip, orc64)


def test_state_errors_and_no_trace():
    args = vqa_args()
    orc, hip = build_pair(args, 0)
    init_sd = {k: v.detach().clone() for k, v in orc.state_dict().items()}
    img, group, ids, seg, mask, tgt = grouped_inputs(args, [1, 3, 2], 10, 32, "vqa")
    dimg, dids, dseg, dmask, dtgt = (t.to(dev()) for t in (img, ids, seg, mask, tgt))
    hip.train()
    out = hip.forward_grouped(dimg, group, dids, dseg, dmask)
    mmvqa_amd.asl_loss(out[0], dtgt).backward()
    # the engine's own answers on a grouped plan
    lib = L.lib()
    q = torch.zeros(64, device=dev())
    assert lib.mmvqa_engine_forward(hip._handle, L.stream_ptr(), L.ptr(dimg), L.ptr(dids), L.ptr(dseg), L.ptr(dmask),
                                    L.ptr(q), 24, None, 0, 0) == -3
    assert lib.mmvqa_engine_feature_map(hip._handle, None, None, None, None) == -3
    assert lib.mmvqa_engine_backward_feature(hip._handle, L.stream_ptr(), L.ptr(q), 24, L.ptr(q)) == -3
    assert lib.mmvqa_engine_forward_tokens(hip._handle, L.stream_ptr(), L.ptr(q), L.ptr(dids), L.ptr(dseg), L.ptr(dmask),
                                           L.ptr(q), 24, None) == -3
    # visual tokens of the grouped step: one set per IMAGE
    vis = hip._read_visual_tokens(len(img))
    assert vis.shape == (3, 5, args.hidden_size) and bool(torch.isfinite(vis).all())
    # directly after forward_grouped the Model refuses attribution and cached-token forwards
    dup = dimg[group.to(dev())]
    with pytest.raises(L.MMVQAError, match="grouped"):
        hip.feature_gradient(dup, dids, dseg, dmask)
    with pytest.raises(L.MMVQAError, match="grouped"):
        hip.forward_tokens(torch.zeros(6, 5, args.hidden_size, device=dev()), dids, dseg, dmask)
    # a plain forward re-plans transparently, and the step is the one of a model that never saw a grouped batch
    torch.cuda.synchronize()
    hip.load_state_dict(init_sd)
    hip.zero_grad(set_to_none=True)
    fresh = mmvqa_amd.Model(args)
    fresh.load_state_dict(init_sd)
    fresh.to(dev()).train()
    orc64 = copy.deepcopy(orc).double()
    orc.train()
    orc64.train()
    ref = oracle_step(orc, orc64, (img[group], ids, seg, mask, tgt), "vqa")
    steps = []
    for m in (hip, fresh):
        o = m(dup, dids, dseg, dmask)
        loss = mmvqa_amd.asl_loss(o[0], dtgt)
        loss.backward()
        check_step(m, orc, orc64, "vqa", o[0], loss, ref)
        steps.append((m, o[0].detach(), loss.detach()))
    same_step(steps[0], steps[1], orc, orc64, "vqa", ref)      # the reused model's step IS the fresh model's, within noise
    assert not hip._plan_is_grouped()
    hip.feature_gradient(dup, dids, dseg, dmask)   # valid again
