"""CPU checks of the attribution methods beyond Grad-CAM: the fp64 restatements agree with their
element-by-element twins and with numpy's SVD, the inputs of the GPU op tests keep away from the formulas' poles, the
sub-command parses --method, scorecam is refused in one sentence, and the new entry points refuse bad arguments on the
host (no GPU here: the pointers are never dereferenced)."""
import numpy as np
import pytest
import torch

import cam_methods_helpers as CH
import gradcam_helpers as GH


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("kind", CH.WEIGHT_KINDS)
def test_weight_formulas_twice(kind):
    g = torch.Generator().manual_seed(3)
    A = torch.randn(2, 2, 3, 8, generator=g)
    A = A.abs() if kind != "signed" else A + 1.0
    dA = torch.randn(2, 2, 3, 8, generator=g)
    if kind == "zeros":
        dA[torch.rand(2, 2, 3, 8, generator=g) < 0.4] = 0.0
        assert int((dA == 0).sum()) > 0
    assert rel(CH.weights_gradcampp(A, dA), CH.weights_loops(A, dA, "gradcam++")) < 1e-12
    assert rel(CH.weights_xgradcam(A, dA), CH.weights_loops(A, dA, "xgradcam")) < 1e-12
    w = CH.weights_xgradcam(A, dA)
    cam, valid = CH.cam_from_weights(A, w)
    assert rel(cam, CH.cam_from_weights_loops(A, w)) < 1e-12
    # with Grad-CAM's own weights the shared tail is Grad-CAM
    cam_gc, _ = GH.reference_cam(A, dA)
    assert rel(CH.cam_from_weights(A, dA.double().mean(dim=(1, 2)))[0], cam_gc) < 1e-12


def test_gradcampp_zero_gradient_contributes_nothing():
    A = torch.ones(1, 1, 2, 4)
    dA = torch.zeros(1, 1, 2, 4)
    assert float(CH.weights_gradcampp(A, dA).abs().max()) == 0.0
    dA[0, 0, 0, 1] = 0.5                           # S = 2: alpha = .25 / (.5 + 2 * .125 + 1e-7), w = .5 * alpha
    w = CH.weights_gradcampp(A, dA)
    assert abs(float(w[0, 1]) - 0.5 * 0.25 / (0.75 + 1e-7)) < 1e-15 and float(w[0, 0]) == 0.0


@pytest.mark.parametrize("H,W,C", CH.EIGEN_MAPS + [(3, 2, 5)])
def test_eigencam_helper_against_svd(H, W, C):
    A = CH.eigen_inputs(H, W, C) if (H, W, C) in CH.EIGEN_MAPS else torch.randn(2, H, W, C)
    raw, gap = CH.eigencam_raw(A)
    for b in range(A.shape[0]):
        want = CH.eigencam_raw_svd(A[b])
        assert rel(raw[b].flatten(), want) < 1e-9
        j = int(np.argmax(np.abs(want)))
        assert want[j] > 0 and float(raw[b].flatten()[j]) > 0
        assert abs(float(raw[b].sum())) < 1e-9 * float(raw[b].abs().sum())     # centred columns: a sum rule cannot fix the sign
        s = np.linalg.svd(CH.centred(A[b]), compute_uv=False)
        assert abs(float(gap[b]) - (s[1] / s[0]) ** 2) < 1e-9


def test_eigencam_helper_degenerate():
    raw, _ = CH.eigencam_raw(torch.zeros(1, 3, 3, 8))
    assert float(raw.abs().max()) == 0.0
    raw, _ = CH.eigencam_raw(torch.randn(2, 1, 1, 8))
    assert float(raw.abs().max()) == 0.0
    assert CH.fix_sign(np.array([1.0, -1.0]))[0] == 1.0 and CH.fix_sign(np.array([-1.0, 1.0]))[0] == 1.0   # ties: lowest index


@pytest.mark.parametrize("act", ["serf", "relu"])
def test_ablated_tokens_twice(act):
    g = torch.Generator().manual_seed(11)
    A = torch.randn(2, 2, 2, 8, generator=g)
    Wt = torch.randn(6, 8, generator=g)
    assert rel(CH.ablated_tokens(A, Wt, act, 3, 4), CH.ablated_tokens_loops(A, Wt, act, 3, 4)) < 1e-12
    # the rank-1 form the kernel uses, and the GPU test at large sizes: u - W[n, c] * A[p, c]
    assert rel(CH.ablated_tokens_rank1(A, Wt, act, 0, 8), CH.ablated_tokens(A, Wt, act, 0, 8)) < 1e-12


def test_ablation_weights_twice():
    s = torch.tensor([2.0, 0.0, -1.5])
    s_abl = torch.randn(3, 5, generator=torch.Generator().manual_seed(1))
    w = CH.ablation_weights(s, s_abl)
    assert torch.equal(w, CH.ablation_weights_loops(s, s_abl))
    assert float(w[1].abs().max()) == 0.0 and abs(float(w[0, 0]) - (2.0 - float(s_abl[0, 0])) / 2.0) < 1e-15


def test_border_channels():
    ch = CH.border_channels(64, 21)
    assert len(ch) == 32 and len(set(ch)) == 32
    assert {0, 63, 20, 21, 41, 42, 43}.issubset(ch)                   # 43 = 64 - 21: where the moved-back last chunk starts


@pytest.mark.parametrize("H,W,C", CH.WEIGHT_MAPS)
@pytest.mark.parametrize("kind", CH.WEIGHT_KINDS)
def test_gpu_weight_inputs_keep_away_from_the_poles(H, W, C, kind):
    """the preconditions the GPU op test asserts, checked here first on the reference alone"""
    A, dA = CH.weight_inputs(H, W, C, kind)
    m1, m2 = CH.pole_margins(A, dA)
    print(f"|S_c| / sum|a| >= {m1:.2e}, |2g^2 + S g^3| / 2g^2 >= {m2:.2e}")
    assert m1 >= 1e-3 and m2 >= 1e-3
    if kind == "zeros":
        assert int((dA == 0).sum()) > 0 or dA.numel() < 16


@pytest.mark.parametrize("H,W,C", CH.EIGEN_MAPS)
def test_gpu_eigen_inputs_have_a_gap_and_a_sign(H, W, C):
    raw, gap = CH.eigencam_raw(CH.eigen_inputs(H, W, C))
    for b in range(raw.shape[0]):
        print(f"gap {float(gap[b]):.3f} sign margin {CH.sign_margin(raw[b]):.2f}")
        assert float(gap[b]) <= 0.25 and CH.sign_margin(raw[b]) >= 1.25


def test_method_parsing():
    from mmvqa_amd import train
    mode, args = train.parse_args(["gradcam"])
    assert mode == "gradcam" and args.method == "gradcam"
    for m in ("gradcam", "gradcam++", "xgradcam", "eigencam", "ablationcam"):
        assert train.parse_args(["gradcam", "--method", m])[1].method == m
    for bad in ("scorecam", "GradCAM"):
        with pytest.raises(SystemExit):
            train.parse_args(["gradcam", "--method", bad])
    with pytest.raises(SystemExit):
        train.parse_args(["eval", "--method", "xgradcam"])             # the flag belongs to the gradcam sub-command


def test_scorecam_and_unknown_methods_are_refused():
    from mmvqa_amd import gradcam as G
    assert "scorecam" not in G.METHODS and G.METHODS[0] == "gradcam"
    with pytest.raises(NotImplementedError, match="scorecam is not built: it needs C whole-model forwards") as ei:
        G.attribute(None, None, None, None, None, method="scorecam")
    assert str(ei.value).count(".") == 0 or str(ei.value).rstrip(".").count(". ") == 0   # one sentence
    with pytest.raises(ValueError, match="layercam"):
        G.attribute(None, None, None, None, None, method="layercam")
    assert G.Attribution._fields == G.GradCam._fields + ("method", "weights", "resid")


def test_new_entry_points_refuse_bad_arguments_on_the_host():
    from mmvqa_amd import _lib as L
    lib = L.lib()
    p, q = 0x1000, 0x2000
    tail = (p, p, None, 0, 0, None, None, 0.4, None)                  # cam, valid, up, IH, IW, image, jet, alpha, overlay
    table = (
        ("cam_weights", (None, 3, p, p, 2, 7, 7, 64, p), b"cam_weights: method=3"),
        ("cam_weights", (None, 1, p, None, 2, 7, 7, 64, p), b"cam_weights: null A / dA / w"),
        ("cam_weights", (None, 1, p, p, 2, 17, 16, 64, p), b"cam_weights: B=2, map 17x16 (at most 256 positions)"),
        ("cam_weights", (None, 2, p, p, 2, 7, 7, 66, p), b"cam_weights: C=66 must be a multiple of 4, at most 4096"),
        ("cam_weights", (None, 2, p, p, 2, 7, 7, 4100, p), b"cam_weights: C=4100"),
        ("cam_weights", (None, 2, p + 4, p, 2, 7, 7, 64, p), b"cam_weights: A / dA must be 16-byte aligned"),
        ("cam_from_weights", (None, p, p, p, 2, 7, 7, 64) + tail, b"cam_from_weights: exactly one of w and raw"),
        ("cam_from_weights", (None, p, None, None, 2, 7, 7, 64) + tail, b"cam_from_weights: exactly one of w and raw"),
        ("cam_from_weights", (None, None, p, None, 2, 7, 7, 64) + tail, b"cam_from_weights: w needs A"),
        ("cam_from_weights", (None, p, p, None, 0, 7, 7, 64) + tail, b"cam_from_weights: B=0"),
        ("cam_from_weights", (None, p, p, None, 2, 7, 7, 64, p, p, p, 0, 8, None, None, 0.4, None), b"cam_from_weights: output size 0x8"),
        ("cam_from_weights", (None, p, p, None, 2, 7, 7, 64, p, p, None, 8, 8, None, None, 0.4, p), b"cam_from_weights: overlay needs image_u8"),
        ("eigencam_raw", (None, p, 2, 7, 7, 64, None, p, p), b"eigencam_raw: null A / gram / raw / resid"),
        ("eigencam_raw", (None, p, 2, 32, 9, 64, p, p, p), b"eigencam_raw: B=2, map 32x9"),
        ("eigencam_raw", (None, p, 2, 7, 7, 6, p, p, p), b"eigencam_raw: C=6"),
        ("ablated_tokens", (None, p, p, None, 2, 49, 64, 96, 3, 0, 8, 1, p), b"ablated_tokens: null A / W / u / tokens"),
        ("ablated_tokens", (None, p, p, p, 2, 257, 64, 96, 3, 0, 8, 1, p), b"ablated_tokens: B=2, map 257x1"),
        ("ablated_tokens", (None, p, p, p, 2, 49, 62, 96, 3, 0, 8, 1, p), b"ablated_tokens: C=62"),
        ("ablated_tokens", (None, p, p, p, 2, 49, 64, 98, 3, 0, 8, 1, p), b"ablated_tokens: hidden=98"),
        ("ablated_tokens", (None, p, p, p, 2, 49, 64, 96, 2, 0, 8, 1, p), b"ablated_tokens: act=2"),
        ("ablated_tokens", (None, p, p, p, 2, 49, 64, 96, 3, 60, 8, 1, p), b"ablated_tokens: channels [60, 60 + 8) outside [0, 64)"),
        ("ablated_tokens", (None, p, p, p, 2, 49, 64, 96, 3, -1, 8, 1, p), b"ablated_tokens: channels [-1"),
        ("ablated_tokens", (None, p, p, p, 2, 49, 64, 96, 3, 0, 0, 1, p), b"ablated_tokens: channels [0, 0 + 0)"),
        ("ablation_weights", (None, p, None, 2, 64, p), b"ablation_weights: null"),
        ("ablation_weights", (None, p, p, 0, 64, p), b"ablation_weights: B=0 C=64"),
        ("engine_visual_tokens", (None, None), b"visual_tokens: null engine"),
        ("engine_forward_tokens", (None, None, p, p, p, p, p, 24, None), b"forward_tokens: null pointer"),
    )
    for name, args, what in table:
        rc = getattr(lib, "mmvqa_" + name)(*args)
        err = lib.mmvqa_last_error()
        assert rc == -1 and what in err, (name, what, rc, err)


def test_engine_token_entry_points_refuse_without_a_plan():
    """an engine that was never planned answers MMVQA_ERR_STATE (-3), a null token pointer MMVQA_ERR_ARG"""
    import ctypes as C
    import mmvqa_amd
    from mmvqa_amd import _lib as L
    from oracle import mmbert_oracle as O
    m = mmvqa_amd.Model(O.make_args(resnet_layers=(1, 1, 1, 1), resnet_width=8, hidden_size=96, n_layers=1, heads=12,
                                    vocab_size=50, emb_vocab=50, bert_max_pos=32))
    lib, p = L.lib(), 0x1000
    vp = C.c_void_p()
    assert lib.mmvqa_engine_visual_tokens(m._handle, C.byref(vp)) == -3 and b"engine_visual_tokens" in lib.mmvqa_last_error()
    assert lib.mmvqa_engine_forward_tokens(m._handle, None, p, p, p, p, p, 52, None) == -3
    assert b"engine_forward_tokens: plan/bind first" in lib.mmvqa_last_error()
    assert lib.mmvqa_engine_forward_tokens(m._handle, None, None, p, p, p, p, 52, None) == -1
    # fp32 operands only: in the f16 operand mode the call is an argument error, whatever the engine's state
    assert lib.mmvqa_engine_set_precision(m._handle, L.PREC_F16) == 0
    assert lib.mmvqa_engine_forward_tokens(m._handle, None, p, p, p, p, p, 52, None) == -1
    assert b"engine_forward_tokens: runs with fp32 operands" in lib.mmvqa_last_error()
    assert lib.mmvqa_engine_set_precision(m._handle, L.PREC_F32) == 0
    assert lib.mmvqa_engine_forward_tokens(m._handle, None, p, p, p, p, p, 52, None) == -3
