"""Mixed-precision forward / backward of the whole model (Model.forward inside torch.autocast("cuda", float16)) against
an emulating oracle: the CPU oracle with every nn.Conv2d / nn.Linear forward replaced by a test-side autograd.Function
that rounds both operands of each of the three products (forward, data gradient, weight gradient) to fp16 and computes
them in fp64 -- rounding the finished data gradient instead (.half().float() on the output) would not be the contract."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import mmvqa_amd  # noqa: E402
from mmvqa_amd import synth  # noqa: E402
from oracle import mmbert_oracle as O  # noqa: E402
from hip_helpers import dev, relerr  # noqa: E402
from dropout_helpers import engine_seed  # noqa: E402
from test_hip_model import build_pair, mini_args, oracle_loss  # noqa: E402


def r16(t):
    return t.detach().half().double()


class _ConvF16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, padding):
        ctx.save_for_backward(x, w)
        ctx.conf = (stride, padding)
        ctx.has_bias = b is not None
        y = F.conv2d(r16(x), r16(w), None, stride, padding)
        if b is not None:
            y = y + b.double()[None, :, None, None]
        return y.to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        stride, padding = ctx.conf
        gx = torch.nn.grad.conv2d_input(x.shape, r16(w), r16(g), stride, padding).to(x.dtype)
        gw = torch.nn.grad.conv2d_weight(r16(x), w.shape, r16(g), stride, padding).to(w.dtype)
        return gx, gw, g.sum((0, 2, 3)) if ctx.has_bias else None, None, None


class _LinF16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        y = r16(x) @ r16(w).t()
        if b is not None:
            y = y + b.double()
        return y.to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gx = (r16(g) @ r16(w)).to(x.dtype)
        gw = (r16(g).reshape(-1, g.shape[-1]).t() @ r16(x).reshape(-1, x.shape[-1])).to(w.dtype)
        gb = g.reshape(-1, g.shape[-1]).sum(0) if ctx.has_bias else None
        return gx, gw, gb


def emulate_f16(model):
    """swap the forward of every nn.Conv2d / nn.Linear instance of the oracle for the operand-rounding Function"""
    for m in model.modules():
        if isinstance(m, torch.nn.Conv2d):
            assert m.groups == 1 and m.dilation == (1, 1)
            m.forward = (lambda mm: lambda x: _ConvF16.apply(x, mm.weight, mm.bias, mm.stride, mm.padding))(m)
        elif isinstance(m, torch.nn.Linear):
            m.forward = (lambda mm: lambda x: _LinF16.apply(x, mm.weight, mm.bias))(m)
    return model


def run_mixed_case(args, B, T, hw, kind, seed=31, tune=False, dropout_seed=None):
    """HIP mixed step (forward + loss + backward under fp16 autocast) against the emulating oracle in fp64: logits (and
    SupCon features), loss, every parameter gradient and the BatchNorm running statistics, each within
    max(1e-3, 5 x the fp32 emulating oracle's own distance from fp64) -- the rule of the fp32 parity tests.
    tune="both": the default launch choices and the tuned ones (Model.tune under autocast) against one oracle run.
    dropout_seed: training-mode dropout, the oracle under the engine's own masks (test_hip_model.run_case)."""
    import copy
    orc, hip = build_pair(args, seed, dropout_seed)
    init_sd = {k: v.detach().clone() for k, v in orc.state_dict().items()}
    orc.train()
    o64 = emulate_f16(copy.deepcopy(orc).double().train())
    emulate_f16(orc)
    V = args.vocab_size
    if kind == "vqa":
        img, ids, seg, mask, tgt = synth.vqa_batch(B, T, hw, vocab=args.emb_vocab, n_classes=V, seed=8)
    else:
        img, ids, seg, mask, tgt = synth.roco_batch(B, T, hw, vocab=V, seed=8, mlm_prob=0.4)
    ref = orc(img, ids, seg, mask)
    loss_ref = oracle_loss(kind, ref, tgt, B)
    loss_ref.backward()
    ref64 = o64(img.double(), ids, seg, mask)
    loss64 = oracle_loss(kind, ref64, tgt, B)
    loss64.backward()
    dimg, dids, dseg, dmask, dtgt = (t.to(dev()) for t in (img, ids, seg, mask, tgt))

    def check(what, name, got, r32, r64):
        tol = max(1e-3, 5 * relerr(r32, r64))
        e = relerr(got, r64)
        assert e <= tol, f"{what}{name}: {e:.2e} > {tol:.2e}"

    for tuned in {"both": (False, True)}.get(tune, (bool(tune),)):
        if hip is None:
            hip = mmvqa_amd.Model(args)
            hip.load_state_dict(init_sd)
            hip.to(dev())
        hip.train()
        what = "tuned launches: " if tuned else ""
        with torch.autocast("cuda", dtype=torch.float16):
            if tuned:
                assert hip.tune(dimg, dids, dseg, dmask) > 20
            if dropout_seed is not None:
                hip.set_seed(dropout_seed)
            out = hip(dimg, dids, dseg, dmask)
            if dropout_seed is not None:   # the oracle's masks and the engine's come from one base seed
                assert hip._seed_ctr == engine_seed(dropout_seed), (hip._seed_ctr, engine_seed(dropout_seed))
            if kind == "vqa":
                logits, lr32, lr64 = out[0], ref[0], ref64[0]
                loss = mmvqa_amd.asl_loss(logits, dtgt)
            elif kind == "supcon":
                logits, feat = out
                lr32, lr64 = ref[0], ref64[0]
                check(what, "feat", feat, ref[1], ref64[1])
                loss = mmvqa_amd.mlm_loss(logits, dtgt)[0] + mmvqa_amd.supcon_loss(mmvqa_amd.split_feat(feat, B // 2))
            else:
                logits, lr32, lr64 = out, ref, ref64
                loss = mmvqa_amd.mlm_loss(logits, dtgt)[0]
        assert logits.dtype == torch.float32
        check(what, "logits", logits, lr32, lr64)
        check(what, "loss", loss.detach().reshape(1), loss_ref.detach().reshape(1), loss64.detach().reshape(1))
        loss.backward()
        torch.cuda.synchronize()
        hp, p64 = dict(hip.named_parameters()), dict(o64.named_parameters())
        n = 0
        for name, p in orc.named_parameters():
            if p.grad is None:
                continue
            assert hp[name].grad is not None, name
            check(what, name, hp[name].grad, p.grad, p64[name].grad)
            n += 1
        assert n > 30
        hb, b64 = dict(hip.named_buffers()), dict(o64.named_buffers())
        for name, b in orc.named_buffers():
            if name.endswith("running_mean") or name.endswith("running_var"):
                check(what, name, hb[name], b, b64[name])
        hip = None


@pytest.mark.parametrize("tm", ["transformer", "realformer"])
def test_mixed_step_mlm(tm):
    run_mixed_case(mini_args(transformer_model=tm), B=3, T=12, hw=32, kind="mlm", tune="both")


def test_mixed_step_mlm_dropout():
    """the f16 epilogues and the unfused attention route under dropout (hidden 0.3, embeddings 0.1)"""
    run_mixed_case(mini_args(hidden_dropout_prob=0.3, emb_dropout_prob=0.1, rf_dropout_prob=0.1), B=3, T=12, hw=32,
                   kind="mlm", tune="both", dropout_seed=14)


def test_mixed_step_mlm_supcon():
    run_mixed_case(mini_args(transformer_model="realformer", supcon=True), B=4, T=11, hw=32, kind="supcon", tune="both")


def test_mixed_step_vqa_head():
    """fc1 and classifier.* of the VQA head"""
    run_mixed_case(mini_args(dataset="VQA-Med", vocab_size=23), B=4, T=10, hw=32, kind="vqa", tune="both")


def test_mixed_step_full_config2():
    """BASELINE.json configs[1] at full depth and width (resnet152, 224x224, hidden 768, 4 layers, T 32, vocab 30522),
    batch 2: the mixed step's distance from the fp64 emulating oracle at full size"""
    run_mixed_case(O.make_args(hidden_dropout_prob=0.0, emb_dropout_prob=0.0, rf_dropout_prob=0.0), B=2, T=32, hw=224,
                   kind="mlm")


def test_mixed_differs_from_fp32_and_leaves_no_trace():
    """the mode is really on (logits differ from the fp32 forward), and an fp32 forward / backward after a mixed one is
    bit-identical to the same on a fresh model"""
    args = mini_args()
    img, ids, seg, mask, tgt = (t.to(dev()) for t in synth.roco_batch(2, 10, 32, vocab=50, seed=4, mlm_prob=0.4))

    def fp32_step(m):
        out = m(img, ids, seg, mask)
        mmvqa_amd.mlm_loss(out, tgt)[0].backward()
        return out.detach().clone(), m.flat_grads.detach().clone()

    _, a = build_pair(args, seed=5)
    _, b = build_pair(args, seed=5)
    a.train(); b.train()
    with torch.autocast("cuda", dtype=torch.float16):
        mixed = a(img, ids, seg, mask)
        lm = mmvqa_amd.mlm_loss(mixed, tgt)[0]
    a.flat_grads.zero_()
    bufs = b._flat[1].clone()
    a._flat[1].copy_(bufs)
    lm.backward()
    a.flat_grads.zero_()
    a._flat[1].copy_(bufs)
    a._flat[2].copy_(b._flat[2])
    out_a, g_a = fp32_step(a)
    out_b, g_b = fp32_step(b)
    # (not bit-equal run to run in any mode: the BatchNorm statistics are fp64 atomics in arrival order)
    e_fp32, e_mixed = relerr(out_a, out_b), relerr(mixed, out_b)
    assert e_fp32 < 1e-5 and relerr(g_a, g_b) < 1e-4, (e_fp32, relerr(g_a, g_b))
    assert e_mixed > 20 * max(e_fp32, 1e-7), (e_mixed, e_fp32)


def test_unsupported_autocast_refused():
    args = mini_args()
    _, hip = build_pair(args, seed=1)
    img, ids, seg, mask, _ = (t.to(dev()) for t in synth.roco_batch(2, 10, 32, vocab=50, seed=4))
    with pytest.raises(NotImplementedError, match="float16"):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            hip(img, ids, seg, mask)
    eff = mmvqa_amd.Model(mini_args(cnn_encoder="tf_efficientnetv2_m", effnet_depth_div=8)).to(dev())
    with pytest.raises(NotImplementedError, match="ResNet"):
        with torch.autocast("cuda", dtype=torch.float16):
            eff(img, ids, seg, mask)
