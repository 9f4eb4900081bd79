"""Attribution methods beyond Grad-CAM on the GPU: the channel-weight, Eigen-CAM and ablated-token
kernels against the fp64 restatements of cam_methods_helpers, forward_tokens against the full forward and against the
oracle, the promise that nothing else moves, Ablation-CAM end to end against an oracle that zeroes one channel through a
forward hook, every method through attribute(), one full-size pass and the sub-command.

Op level: relerr <= 1e-5 against fp64 (the bound of test_hip_gradcam.test_resize_and_overlay).  Model level: the check()
rule of test_hip_gradcam, max(1e-3, 5 x relerr(fp32 oracle, fp64 oracle)) against the fp64 oracle."""
import csv

import pytest
import torch

pytestmark = pytest.mark.gpu

import mmvqa_amd  # noqa: E402
from mmvqa_amd import _lib as L  # noqa: E402
from mmvqa_amd import gradcam as G  # noqa: E402
from mmvqa_amd import synth  # noqa: E402
from oracle import mmbert_oracle as O  # noqa: E402
from hip_helpers import dev, relerr  # noqa: E402
from test_hip_model import build_oracle, mini_args  # noqa: E402
from test_hip_gradcam import C, DROP, EFF, check, make_case  # noqa: E402

import cam_methods_helpers as CH  # noqa: E402
import gradcam_helpers as GH  # noqa: E402

OP_TOL = 1e-5
# Eigen-CAM's unit-vector bound.  The kernel runs EIG_ITERS = 64 power iterations on G = X X^T.  With the eigenvalue ratio
# lambda2 / lambda1 = sigma2^2 / sigma1^2 <= 0.25 the component outside u1 shrinks by 0.25 per iteration: after 64 it is
# tan(theta0) * 0.25^64 ~ 3e-39 * tan(theta0), nothing in fp32 for any start that is not orthogonal to u1 to 30 digits.
# What remains is rounding: every entry of G is a C-term fp32 dot product summed 4 x (C / 256) terms per lane and 6
# shuffle levels deep, relative error <= ~(C / 64 + 6) * 6e-8 <= 2.3e-6 of |x_p| |x_q| at C = 2048, so
# |dG|_F <= 2.3e-6 * trace(G), and the eigenvector moves by at most |dG| / (lambda1 - lambda2) <= 2.3e-6 * (trace / lambda1) /
# 0.75.  The planted inputs have trace / lambda1 < 3 (asserted): <= 1e-5, plus ~1e-6 per matrix-vector product of the last
# iterations.  1e-4 leaves a factor of ten over that worst case; resid = |G u - lambda u| / lambda is of the same order.
EIG_TOL = 1e-4


# ------------------------------------------------------------------------------------------------ op level
@pytest.mark.parametrize("H,W,Cc", CH.WEIGHT_MAPS)
@pytest.mark.parametrize("kind", CH.WEIGHT_KINDS)
def test_channel_weights(H, W, Cc, kind):
    A, dA = CH.weight_inputs(H, W, Cc, kind)
    m1, m2 = CH.pole_margins(A, dA)                                # on the reference alone: away from the formulas' own poles
    assert m1 >= 1e-3 and m2 >= 1e-3, (m1, m2)
    Ad, dAd = A.to(dev()), dA.to(dev())
    for method, ref in (("gradcam++", CH.weights_gradcampp), ("xgradcam", CH.weights_xgradcam)):
        w = G.cam_weights(Ad, dAd, method)
        w64 = ref(A, dA)
        e = relerr(w, w64)
        print(f"{method} {kind} {H}x{W}x{Cc}: w relerr {e:.2e}")
        assert e <= OP_TOL
        cam, up, overlay, valid = G.cam_from_weights(Ad, (2 * H, 3 * W), w=w)
        cam64, v64 = CH.cam_from_weights(A, w.cpu())              # the kernel's own weights through the fp64 tail
        e = relerr(cam, cam64)
        print(f"{method} {kind} {H}x{W}x{Cc}: cam relerr {e:.2e}")
        assert e <= OP_TOL and valid.cpu().tolist() == [int(v) for v in v64] and overlay is None
        assert relerr(up, GH.bilinear_resize(cam.cpu(), 2 * H, 3 * W)) <= OP_TOL


@pytest.mark.parametrize("H,W,Cc", [(7, 7, 512), (7, 7, 2048), (5, 9, 48), (16, 16, 8), (1, 1, 4)])
def test_gradcam_weights_through_the_new_path_are_bit_equal(H, W, Cc):
    g = torch.Generator().manual_seed(H * W + Cc)
    A = torch.randn(3, H, W, Cc, generator=g).abs().to(dev())
    dA = (torch.randn(3, H, W, Cc, generator=g) + 0.05).to(dev())
    image = torch.randint(0, 256, (3, 40, 36, 3), generator=g, dtype=torch.uint8).to(dev())
    cam0, up0, ov0, v0 = G.cam_from_maps(A, dA, (40, 36), image)
    w = G.cam_weights(A, dA, "gradcam")
    cam1, up1, ov1, v1 = G.cam_from_weights(A, (40, 36), w=w, image_u8=image)
    assert torch.equal(cam0, cam1) and torch.equal(up0, up1) and torch.equal(ov0, ov1) and torch.equal(v0, v1)
    assert relerr(w, dA.double().mean(dim=(1, 2))) <= OP_TOL


@pytest.mark.parametrize("H,W,Cc", CH.EIGEN_MAPS)
def test_eigencam_planted(H, W, Cc):
    A = CH.eigen_inputs(H, W, Cc)
    raw64, gap = CH.eigencam_raw(A)
    import numpy as np
    for b in range(A.shape[0]):                                    # preconditions on the fp64 decomposition alone
        s = np.linalg.svd(CH.centred(A[b]), compute_uv=False)
        assert float(gap[b]) <= 0.25 and CH.sign_margin(raw64[b]) >= 1.25
        assert float((s ** 2).sum() / s[0] ** 2) < 3.0             # trace / lambda1 of the derivation above
    raw, resid = G.eigencam_raw(A.to(dev()))
    for b in range(A.shape[0]):
        got, want = raw[b].double().cpu().flatten(), raw64[b].flatten()
        e = float((got / got.norm() - want / want.norm()).norm())
        print(f"{H}x{W}x{Cc} sample {b}: gap {float(gap[b]):.3f} unit-vector error {e:.2e} resid {float(resid[b]):.2e} "
              f"scale {float(got.norm() / want.norm()):.6f}")
        assert e <= EIG_TOL and float(resid[b]) <= EIG_TOL
        j = int(want.abs().argmax())
        assert float(got[j]) > 0 and int(got.abs().argmax()) == j  # the sign rule
        assert abs(float(got.norm() / want.norm()) - 1) <= EIG_TOL
    cam, _, _, valid = G.cam_from_weights(A.to(dev()), (H, W), raw=raw)
    cam64, _ = CH.cam_from_raw(raw.cpu())
    assert relerr(cam, cam64) <= OP_TOL and valid.cpu().tolist() == [1] * A.shape[0]


def test_eigencam_degenerate_maps():
    for A in (torch.zeros(2, 7, 7, 64), torch.randn(2, 1, 1, 64)):
        Ad = A.to(dev())
        raw, resid = G.eigencam_raw(Ad)
        cam, up, _, valid = G.cam_from_weights(Ad, (8, 8), raw=raw)
        assert float(raw.abs().max()) == 0.0 and float(resid.abs().max()) == 0.0
        assert valid.cpu().tolist() == [0, 0] and float(cam.abs().max()) == 0.0 and float(up.abs().max()) == 0.0


@pytest.mark.parametrize("H,W,Cc,hidden,act,c0,nc", [
    (7, 7, 512, 768, "serf", 0, 512), (7, 7, 512, 768, "relu", 0, 512), (2, 2, 256, 96, "serf", 0, 256),
    (5, 9, 48, 96, "serf", 0, 48), (5, 9, 48, 96, "relu", 40, 8)], ids=["serf768", "relu768", "2x2", "5x9", "ragged"])
def test_ablated_tokens(H, W, Cc, hidden, act, c0, nc):
    g = torch.Generator().manual_seed(H * W + Cc + hidden)
    A = torch.randn(2, H, W, Cc, generator=g).abs()
    Wt = torch.randn(hidden, Cc, generator=g) / Cc ** 0.5
    if nc * hidden <= 256 * 96:                                    # zero the channel, convolve, activate, average: every channel
        want = CH.ablated_tokens(A, Wt, act, c0, nc)
    else:                                                          # at 512 x 768 that form takes the CPU half a minute: it is the
        want = CH.ablated_tokens_rank1(A, Wt, act, c0, nc)         # reference on 32 channels and pins the one-product form on them
        for c in CH.border_channels(nc, 128):
            assert relerr(want[:, c], CH.ablated_tokens(A, Wt, act, c0 + c, 1)[:, 0]) < 1e-12
    code = L.ACT_RELU if act == "relu" else L.ACT_SERF
    got, u = G.ablated_tokens(A.to(dev()), Wt.to(dev()), code, c0, nc)
    assert got.shape == (2, nc, hidden)
    e = relerr(got, want)
    print(f"ablated tokens {H}x{W}x{Cc} hidden {hidden} {act} [{c0}, {c0 + nc}): relerr {e:.2e}")
    assert e <= OP_TOL
    if nc > 4:                                                     # a later chunk reuses u and equals the same channels of the whole
        part, _ = G.ablated_tokens(A.to(dev()), Wt.to(dev()), code, c0 + 3, nc - 4, u)
        assert torch.equal(part, got[:, 3:nc - 1])


def test_ablation_weights_kernel():
    s = torch.tensor([2.0, 0.0, -1.5])
    s_abl = torch.randn(3, 300, generator=torch.Generator().manual_seed(1))
    w = torch.empty(3, 300, device=dev())
    sd, sad = s.to(dev()), s_abl.to(dev())
    L.check(L.lib().mmvqa_ablation_weights(L.stream_ptr(), L.ptr(sd), L.ptr(sad), 3, 300, L.ptr(w)))
    assert relerr(w, CH.ablation_weights(s, s_abl)) <= OP_TOL and float(w[1].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ forward from tokens
FB = dict(transformer_model="feedback-transformer", fb_dropout_prob=0.0)
TOKEN_CASES = [
    ("resnet_transformer_vqa", dict(dataset="VQA-Med", vocab_size=C, transformer_model="transformer", **DROP)),
    ("effnet_realformer_vqa", dict(dataset="VQA-Med", vocab_size=C, transformer_model="realformer", **EFF, **DROP)),
    ("resnet_feedback_vqa", dict(dataset="VQA-Med", vocab_size=C, **FB)),
    ("resnet_realformer_mlm", dict(transformer_model="realformer")),
    ("effnet_transformer_mlm_supcon", dict(transformer_model="transformer", supcon=True, **EFF)),
    ("resnet_feedback_mlm", dict(**FB)),
]


@pytest.mark.parametrize("name,kw", TOKEN_CASES, ids=[c[0] for c in TOKEN_CASES])
def test_forward_tokens_equals_forward(name, kw):
    torch.manual_seed(5)
    hip = mmvqa_amd.Model(mini_args(**kw)).to(dev())
    img, ids, seg, mask, _ = (t.to(dev()) for t in synth.vqa_batch(3, 10, 64, vocab=50, n_classes=C, seed=6))

    def first(out):
        out = out[0] if isinstance(out, tuple) else out
        return out[0] if isinstance(out, tuple) else out           # VQA: (logits, 0, 0); SupCon: (logits, feat)

    hip.eval()
    with torch.no_grad():
        full1 = hip(img, ids, seg, mask)
        full2 = hip(img, ids, seg, mask)
    hip.train()                                                    # the token calls run in eval mode whatever the model's mode
    vis = hip.visual_tokens(img)
    assert hip.training and vis.shape == (3, 5, 96)
    tok = hip.forward_tokens(vis, ids, seg, mask)
    assert hip.training and type(tok) is type(full1)
    floor = max(1e-5, 5 * relerr(first(full1), first(full2)))
    e = relerr(first(tok), first(full1))
    print(f"{name}: forward_tokens vs forward {e:.2e} (floor {floor:.1e})")
    assert first(tok).shape == first(full1).shape and e <= floor
    if kw.get("supcon"):
        assert relerr(tok[1], full1[1]) <= max(1e-5, 5 * relerr(full1[1], full2[1]))
    if kw.get("dataset") == "VQA-Med":
        assert tok[1:] == (0, 0)


def test_one_image_three_questions_against_the_oracle():
    orc, hip, (img, ids, seg, mask, _) = make_case(dict(transformer_model="realformer", **EFF, **DROP), 64, 74, False)
    img1 = img[:1].repeat(3, 1, 1, 1)                              # one image, the three questions of the batch
    orc.eval()
    with torch.no_grad():
        l32 = orc(img1, ids, seg, mask)[0]
        l64 = orc.double()(img1.double(), ids, seg, mask)[0]
    vis = hip.visual_tokens(img[:1].to(dev()))                     # computed at batch size 1 ...
    assert vis.shape == (1, 5, 96)
    logits = hip.forward_tokens(vis.expand(3, -1, -1), ids.to(dev()), seg.to(dev()), mask.to(dev()))[0]   # ... used at 3
    check("logits from repeated tokens", logits, l32, l64)


def test_forward_tokens_moves_nothing_and_bars_the_backward():
    args = mini_args(dataset="VQA-Med", vocab_size=C, transformer_model="transformer")
    a = mmvqa_amd.Model(args)
    b = mmvqa_amd.Model(args)
    b.load_state_dict(a.state_dict())
    a.to(dev()), b.to(dev())
    img, ids, seg, mask, tgt = (t.to(dev()) for t in synth.vqa_batch(4, 10, 64, vocab=50, n_classes=C, seed=32))

    def step(m):
        m.train()
        loss = mmvqa_amd.asl_loss(m(img, ids, seg, mask)[0], tgt)
        loss.backward()
        return loss.detach().clone()

    for m in (a, b):
        m.set_seed(7)
        step(m)
    assert float(a.flat_grads.abs().max()) > 0
    snap = [t.clone() for t in (a.flat_grads, a.flat_params, a._flat[1], a._flat[2])]
    vis = a.visual_tokens(img)
    out = a.forward_tokens(vis, ids, seg, mask)[0]
    torch.cuda.synchronize()
    assert a.training and out.shape == (4, C) and not out.requires_grad
    for before, after in zip(snap, (a.flat_grads, a.flat_params, a._flat[1], a._flat[2])):
        assert torch.equal(before, after)
    # the feature map in the workspace is not these tokens': the attribution backward is refused
    dA = torch.empty(4, 2, 2, 256, device=dev())
    g = torch.zeros(4, 24, device=dev())
    rc = L.lib().mmvqa_engine_backward_feature(a._handle, L.stream_ptr(), L.ptr(g), 24, L.ptr(dA))
    assert rc == -3 and b"visual tokens" in L.lib().mmvqa_last_error()
    rc = L.lib().mmvqa_engine_backward(a._handle, L.stream_ptr(), L.ptr(g), 24, None)
    assert rc == -3
    for dt in (torch.float16, torch.bfloat16):
        with torch.autocast("cuda", dtype=dt):
            with pytest.raises(NotImplementedError, match="autocast"):
                a.forward_tokens(vis, ids, seg, mask)
            with pytest.raises(NotImplementedError, match="autocast"):
                a.visual_tokens(img)
    # a following training step equals the twin's that never ran from tokens (the rule of test_nothing_else_moves)
    b._seed_ctr = a._seed_ctr = 99
    la, lb = step(a), step(b)
    assert relerr(la.reshape(1), lb.reshape(1)) < 1e-5, (float(la), float(lb))
    assert relerr(a.flat_grads, b.flat_grads) < 1e-4


# ------------------------------------------------------------------------------------------------ the methods on mini models
# (name, args, seed): seeds checked on the CPU oracle alone for the preconditions asserted below
ABL_CASES = [
    ("resnet_transformer", dict(transformer_model="transformer"), 51),
    ("effnet_realformer", dict(transformer_model="realformer", **EFF, **DROP), 74),
]


def oracle_case(kw, seed, B=2, T=10, hw=64):
    """the CPU half of test_hip_gradcam.make_case: the oracle and the batch, nothing on the GPU"""
    args = mini_args(dataset="VQA-Med", vocab_size=C, **kw)
    orc = build_oracle(args, seed)
    batch = synth.vqa_batch(B, T, hw, vocab=args.emb_vocab, n_classes=C, seed=seed)
    return args, orc, batch


def hip_twin(args, orc):
    hip = mmvqa_amd.Model(args)
    hip.load_state_dict(orc.state_dict())
    return hip.to(dev())


def ablation_oracle(kw, seed):
    """-> (args, orc, batch, channels, A32, A64, w32, w64, s64) on the oracle alone"""
    args, orc, (img, ids, seg, mask, tgt) = oracle_case(kw, seed)
    _, A32, _, _ = GH.oracle_feature_gradient(orc, img, ids, seg, mask, tgt)
    _, A64, _, _ = GH.oracle_feature_gradient(orc, img, ids, seg, mask, tgt, double=True)
    Cc = A64.shape[3]
    nc = max(1, min(Cc, G.ABLATION_VARIANTS // img.shape[0]))
    channels = CH.border_channels(Cc, nc)
    s32, sa32 = CH.oracle_ablated_scores(orc, img, ids, seg, mask, tgt, channels)
    s64, sa64 = CH.oracle_ablated_scores(orc, img, ids, seg, mask, tgt, channels, double=True)
    return args, orc, (img, ids, seg, mask, tgt), channels, A32, A64, CH.ablation_weights(s32, sa32), CH.ablation_weights(s64, sa64), s64


@pytest.mark.parametrize("name,kw,seed", ABL_CASES, ids=[c[0] for c in ABL_CASES])
def test_ablationcam_end_to_end(name, kw, seed):
    args, orc, (img, ids, seg, mask, tgt), channels, A32, A64, w32, w64, s64 = ablation_oracle(kw, seed)
    assert len(channels) == 32 and channels[0] == 0 and channels[-1] == A64.shape[3] - 1
    # the cap: w = (s - s_c) / s cancels, an oracle that is itself noisy would make the 5 x rule vacuous
    assert bool((s64.abs() > 0).all()) and relerr(w32, w64) <= 2e-2, relerr(w32, w64)
    hip = hip_twin(args, orc)
    hip.train()
    d = [t.to(dev()) for t in (img, ids, seg, mask)]
    res = G.attribute(hip, *d, method="ablationcam", target=tgt.to(dev()))
    assert hip.training and res.method == "ablationcam" and res.resid is None
    assert res.weights.shape == (img.shape[0], A64.shape[3])
    check("ablation weights", res.weights[:, channels], w32, w64)
    w_gpu = res.weights.cpu()
    check("cam", res.cam, CH.cam_from_weights(A32, w_gpu)[0], CH.cam_from_weights(A64, w_gpu)[0])
    assert res.valid.cpu().tolist() == [int(v) for v in CH.cam_from_weights(A64, w_gpu)[1]]


# seeds per (case, method): the ones whose fp64 oracle meets the preconditions asserted in the test (checked on the CPU)
_SEEDS = {("resnet_transformer", "gradcam++"): 51, ("resnet_transformer", "xgradcam"): 51, ("resnet_transformer", "eigencam"): 51,
          ("effnet_realformer", "gradcam++"): 12, ("effnet_realformer", "xgradcam"): 74, ("effnet_realformer", "eigencam"): 12}
METHOD_CASES = [(n, kw, _SEEDS[n, m], m) for (n, kw, _) in ABL_CASES for m in ("gradcam++", "xgradcam", "eigencam")]


def method_oracle(kw, seed, method):
    """-> (args, orc, batch, per precision: (A, raw map before the ReLU)) on the oracle alone"""
    args, orc, (img, ids, seg, mask, tgt) = oracle_case(kw, seed, B=3)
    out = []
    for double in (False, True):
        _, A, dA, _ = GH.oracle_feature_gradient(orc, img, ids, seg, mask, tgt, double=double)
        if method == "eigencam":
            raw = CH.eigencam_raw(A)[0]
        else:
            raw = CH.raw_from_weights(A, CH.weights_gradcampp(A, dA) if method == "gradcam++" else CH.weights_xgradcam(A, dA))
        out.append((A, dA, raw))
    return args, orc, (img, ids, seg, mask, tgt), out


@pytest.mark.parametrize("name,kw,seed,method", METHOD_CASES, ids=[f"{c[0]}-{c[3]}" for c in METHOD_CASES])
def test_methods_through_attribute(name, kw, seed, method):
    args, orc, (img, ids, seg, mask, tgt), ((A32, dA32, raw32), (A64, dA64, raw64)) = method_oracle(kw, seed, method)
    flat = raw64.flatten(1)                                        # the precondition of the Grad-CAM test, on the oracle first
    assert bool((flat.max(1).values > 0).all()), flat.max(1).values
    assert bool((flat.max(1).values >= 1e-2 * flat.abs().max(1).values).all())
    if method == "eigencam":
        gap = CH.eigencam_raw(A64)[1]
        # random mini weights on a 2 x 2 map have no planted gap; 0.7 still lets the 64 iterations converge (0.7^64 ~ 1e-10,
        # far below this test's 1e-3), and a 10 % sign margin is a hundred times the tolerance
        assert bool((gap <= 0.7).all()), gap
        assert all(CH.sign_margin(raw64[b]) >= 1.1 and CH.sign_margin(raw32[b]) >= 1.1 for b in range(3))
    hip = hip_twin(args, orc)
    d = [t.to(dev()) for t in (img, ids, seg, mask)]
    res = G.attribute(hip, *d, method=method, target=tgt.to(dev()), image_u8=G.image_u8_from_normalised(d[0]))
    assert res.method == method and res.overlay.shape == (3, 64, 64, 3) and res.heatmap.shape == (3, 64, 64)
    check("cam", res.cam, CH.cam_from_raw(raw32)[0], CH.cam_from_raw(raw64)[0])
    assert res.valid.cpu().tolist() == [1, 1, 1]
    if method == "eigencam":
        assert res.weights is None and res.resid.shape == (3,) and float(res.resid.max()) <= 1e-3
    else:
        ref = CH.weights_gradcampp if method == "gradcam++" else CH.weights_xgradcam
        check("weights", res.weights, ref(A32, dA32), ref(A64, dA64))
        assert res.resid is None


def test_attribute_gradcam_is_grad_cam():
    _, hip, (img, ids, seg, mask, tgt) = make_case(dict(transformer_model="transformer"), 64, 51, False)
    d = [t.to(dev()) for t in (img, ids, seg, mask)]
    image = G.image_u8_from_normalised(d[0])
    a = G.grad_cam(hip, *d, target=tgt.to(dev()), image_u8=image)
    b = G.attribute(hip, *d, method="gradcam", target=tgt.to(dev()), image_u8=image)
    floor = max(1e-5, 5 * relerr(a.cam, G.grad_cam(hip, *d, target=tgt.to(dev())).cam))
    assert relerr(b.cam, a.cam) <= floor and torch.equal(a.valid, b.valid) and torch.equal(a.target, b.target)
    assert b.method == "gradcam" and b.weights.shape == (3, 256) and b.resid is None


def test_full_size_config5_every_method():
    """tf_efficientnetv2_m at full depth + RealFormer + VQA head, 224 x 224, B = 2: shapes, finiteness, valid"""
    args = O.make_args(cnn_encoder="tf_efficientnetv2_m", transformer_model="realformer", heads=8, dataset="VQA-Med",
                       vocab_size=1552, emb_vocab=30522)
    torch.manual_seed(3)
    hip = mmvqa_amd.Model(args).to(dev()).eval()
    img, ids, seg, mask, _ = (t.to(dev()) for t in synth.vqa_batch(2, 28, 224, vocab=30522, n_classes=1552, seed=9))
    image = G.image_u8_from_normalised(img)
    for method in G.METHODS:
        res = G.attribute(hip, img, ids, seg, mask, method=method, image_u8=image)
        assert res.cam.shape == (2, 7, 7) and res.heatmap.shape == (2, 224, 224) and res.overlay.shape == (2, 224, 224, 3)
        assert torch.equal(res.target, res.logits.argmax(1))
        for x in (res.cam, res.heatmap) + (() if res.weights is None else (res.weights,)):
            assert bool(torch.isfinite(x).all()), method
        valid = res.valid.cpu().tolist()
        top = res.cam.flatten(1).max(1).values.cpu().tolist()
        print(f"{method}: valid {valid}" + ("" if res.resid is None else f" resid {res.resid.cpu().tolist()}"))
        assert all(t == (1.0 if v else 0.0) for t, v in zip(top, valid))
        if method == "gradcam":                                    # the precondition holds: test_hip_gradcam's full-size pass
            assert valid == [1, 1]
        if method == "eigencam":                                   # a non-constant map always has a positive entry after the sign rule
            assert valid == [1, 1] and res.weights is None and bool(torch.isfinite(res.resid).all())
        else:
            assert res.weights.shape == (2, 512)


def test_gradcam_subcommand_methods(tmp_path):
    from PIL import Image
    from mmvqa_amd import train
    mini = ["--resnet_layers", "1", "1", "1", "1", "--resnet_width", "8", "--hidden_size", "96", "--n_layers", "2",
            "--emb_vocab", "64", "--max_position_embeddings", "16", "--num_classes", "11", "--batch_size", "4"]
    out = tmp_path / "pp"
    index = train.main(["gradcam", "--test_samples", "6", "--method", "gradcam++", "--target", "predicted", "--save_dir", str(out)] + mini)
    rows = list(csv.reader(open(out / "gradcam_index.csv")))
    assert rows[0] == ["image", "category", "question_index", "target", "predicted", "valid", "method"]
    assert len(rows) == 7 and len(index) == 6 and all(r[6] == "gradcam++" and r[3] == r[4] for r in rows[1:])
    for r in rows[1:]:
        with Image.open(out / r[0]) as im:
            assert im.size == (224, 224) and im.mode == "RGB"
    assert len(list(out.glob("*.png"))) == 6
    train.main(["gradcam", "--test_samples", "4", "--save_dir", str(tmp_path / "plain")] + mini)
    rows = list(csv.reader(open(tmp_path / "plain" / "gradcam_index.csv")))
    assert rows[0] == ["image", "category", "question_index", "target", "predicted", "valid"] and len(rows[1]) == 6
