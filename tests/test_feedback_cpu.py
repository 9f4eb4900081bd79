"""CPU checks of the Feedback-Transformer encoder: the test oracle (tests/feedback_helpers.FeedbackBlock) is pinned to the
reference's class through golden vectors, and mmvqa_amd.Model keeps the reference's state_dict protocol for it (names,
shapes, the one to_kv weight under all its names, checkpoints)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mmvqa_amd
from mmvqa_amd import _lib as L
from mmvqa_amd import checkpoint as CK
from mmvqa_amd.model import desc_from_args
from oracle import mmbert_oracle as O
import feedback_helpers as FH

GOLDEN = (("d2_t12", "feedback.npz"), ("d1_t2", "feedback.npz"), ("d2_t11", "feedback_odd.npz"))


def relerr(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("tag,fname", GOLDEN)
def test_helper_block_equals_the_reference(golden_dir, tag, fname):
    """fp32 helper against the reference's fp32 results, each tensor within max(1e-5, 5 x the reference's own recorded
    distance from its fp64 run); state_dict key list and the parameters that receive a gradient are the reference's"""
    z = np.load(os.path.join(golden_dir, fname))
    dim, depth, B, T, seed, ntok = (int(v) for v in z[f"{tag}/cfg"])
    blk = FH.seeded_weights(FH.FeedbackBlock(ntok, dim, depth, 0.1), seed).eval()
    assert list(blk.state_dict().keys()) == [str(k) for k in z[f"{tag}/keys"]]
    assert [n for n, _ in blk.named_parameters()] == [str(k) for k in z[f"{tag}/param_names"]]
    x = torch.from_numpy(z[f"{tag}/x"]).requires_grad_(True)
    out = blk(x)
    out.backward(torch.from_numpy(z[f"{tag}/dy"]))
    tol = max(1e-5, 5 * float(z[f"{tag}/fp64_dist"]))
    errs = {"out": relerr(out.detach(), torch.from_numpy(z[f"{tag}/out"])), "dx": relerr(x.grad, torch.from_numpy(z[f"{tag}/dx"]))}
    want = {k[len(tag) + 6:] for k in z.files if k.startswith(f"{tag}/grad/")}
    got = {n for n, p in blk.named_parameters() if p.grad is not None}
    assert got == want, (sorted(got - want), sorted(want - got))
    assert ("layer_weight" in got) == (T > 2)            # the last window's memory is never read
    assert not any(n.startswith(("token_emb", "to_logits")) for n in got)
    for n, p in blk.named_parameters():
        if p.grad is not None:
            errs[n] = relerr(p.grad, torch.from_numpy(z[f"{tag}/grad/{n}"]))
    bad = {k: v for k, v in errs.items() if not v <= tol}
    assert not bad, (tol, bad)


def fb_args(**kw):
    d = dict(resnet_layers=(1, 1, 1, 1), resnet_width=8, hidden_size=96, n_layers=3, heads=12, vocab_size=50, emb_vocab=50,
             bert_max_pos=512, hidden_dropout_prob=0.0, emb_dropout_prob=0.0, transformer_model="feedback-transformer")
    d.update(kw)
    return O.make_args(**d)


def test_state_dict_is_the_references():
    args = fb_args()
    torch.manual_seed(0)
    orc = FH.oracle_model(args)
    hip = mmvqa_amd.Model(args)
    osd, hsd = orc.state_dict(), hip.state_dict()
    assert {k: tuple(v.shape) for k, v in osd.items()} == {k: tuple(v.shape) for k, v in hsd.items()}
    kv = [k for k in hsd if k.endswith("to_kv.weight") or k.endswith("shared_kv_proj.weight")]
    assert len(kv) == args.n_layers + 1
    assert len({hsd[k].data_ptr() for k in kv}) == 1                      # one tensor under all its names
    names = [n for n, _ in hip.named_parameters()]
    assert [n for n in names if "to_kv" in n or "shared_kv" in n] == ["transformer.block.layers.0.0.fn.fn.to_kv.weight"]
    assert sorted(names) == sorted(n for n, _ in orc.named_parameters())
    hip.load_state_dict(osd)                                              # strict
    for k, v in hip.state_dict().items():
        assert torch.equal(v, osd[k]), k
    # a checkpoint whose aliases differ (never written by the reference) resolves to the first name
    odd = dict(osd)
    odd["transformer.block.shared_kv_proj.weight"] = torch.zeros_like(osd["transformer.block.shared_kv_proj.weight"])
    hip.load_state_dict(odd)
    assert torch.equal(hip.state_dict()["transformer.block.shared_kv_proj.weight"],
                       osd["transformer.block.layers.0.0.fn.fn.to_kv.weight"])


def test_the_reference_tests_feedback_first_and_the_dropout_option_is_read():
    d = desc_from_args(fb_args())
    assert d.encoder == L.ENC_FEEDBACK and abs(d.p_fb_drop - 0.1) < 1e-7 and d.fb_tokens == 50
    assert abs(desc_from_args(fb_args(fb_dropout_prob=0.25)).p_fb_drop - 0.25) < 1e-7
    assert desc_from_args(fb_args(transformer_model="realformer")).encoder == L.ENC_REALFORMER
    assert desc_from_args(fb_args(transformer_model="transformer")).encoder == L.ENC_TRANSFORMER


@pytest.mark.parametrize("T", [1, 257])
def test_sequence_lengths_outside_the_memory_are_refused(T):
    hip = mmvqa_amd.Model(fb_args(n_layers=1))
    z = torch.zeros(2, T, dtype=torch.long)
    with pytest.raises(ValueError, match="2 <= T <= 256"):
        hip(torch.zeros(2, 3, 64, 64), z, z, z)
    lib = L.lib()
    assert lib.mmvqa_engine_plan(hip._handle, 2, T, 64, 64) == 0           # the engine's own check: MMVQA_ERR_ARG
    assert b"2 <= T <= 256" in lib.mmvqa_last_error()
    assert lib.mmvqa_engine_plan(hip._handle, 2, 256, 64, 64) > 0


def test_too_many_layers_for_one_aggregation_are_refused():
    with pytest.raises(L.MMVQAError, match="at most 15"):
        mmvqa_amd.Model(fb_args(n_layers=16))


def test_checkpoint_round_trip_and_roco_to_vqa(tmp_path):
    args = fb_args()
    torch.manual_seed(1)
    src = mmvqa_amd.Model(args)
    path = str(tmp_path / "roco.pt")
    torch.save(src.state_dict(), path)
    saved = CK.read_state_dict(path)
    assert len([k for k in saved if "to_kv" in k or "shared_kv" in k]) == args.n_layers + 1
    torch.manual_seed(2)
    dst = mmvqa_amd.Model(args)
    CK.load_model(dst, path)                                              # strict: every alias is expected and present
    for k, v in src.state_dict().items():
        assert torch.equal(dst.state_dict()[k], v), k
    # ROCO -> VQA (vqamed2019/train.py:125-137): key-filtered load, then the classifier is swapped
    torch.manual_seed(3)
    vqa = mmvqa_amd.Model(fb_args(dataset="VQA-Med"))
    loaded, skipped, untouched = CK.load_roco_pretrained(vqa, path)
    assert not skipped and not untouched and "transformer.block.shared_kv_proj.weight" in loaded
    vqa.classifier[2] = torch.nn.Linear(96, 7)
    vsd = vqa.state_dict()
    assert vsd["transformer.block.token_emb.weight"].shape == (50, 96)     # num_tokens does not follow the new head
    for k, v in src.state_dict().items():
        if not k.startswith("classifier.2."):
            assert torch.equal(vsd[k], v), k
    kv = [k for k in vsd if k.endswith("to_kv.weight") or k.endswith("shared_kv_proj.weight")]
    assert len(kv) == args.n_layers + 1 and len({vsd[k].data_ptr() for k in kv}) == 1
