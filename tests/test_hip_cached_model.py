"""Training from cached visual tokens on the whole model: TokenCache.fill + Model.forward_cached +
backward against the oracle with everything under transformer.trans frozen, against the project's own frozen full step,
the launch counts, the engine's state machine and the cache's fingerprint."""
import copy
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import mmvqa_amd  # noqa: E402
from mmvqa_amd import _lib as L  # noqa: E402
from mmvqa_amd.tokens import TokenCache  # noqa: E402
from hip_helpers import dev, relerr  # noqa: E402
from test_hip_model import TOL, build_pair, compare_grads, mini_args, oracle_loss  # noqa: E402
from test_hip_freeze import B, DROPOUT, EFF, HW, T, batch, hip_loss, region_launches  # noqa: E402
import test_hip_feedback_model as TF  # noqa: E402

VISUAL = "transformer.trans."
FB_DROPOUT = dict(fb_dropout_prob=0.3, emb_dropout_prob=0.1)
CASES = {
    "mlm-transformer": ("mlm", dict(transformer_model="transformer"), DROPOUT, build_pair),
    "vqa-realformer": ("vqa", dict(transformer_model="realformer", dataset="VQA-Med"), DROPOUT, build_pair),
    "effnet": ("mlm", dict(transformer_model="transformer", **EFF), DROPOUT, build_pair),
    "feedback": ("mlm", dict(transformer_model=TF.FB, fb_dropout_prob=0.0), FB_DROPOUT, TF.build_pair),
}


def freeze_oracle(orc):
    """every parameter under transformer.trans frozen, the backbone's BatchNorms in .eval(), the rest in train mode"""
    orc.train()
    for p in orc.transformer.trans.parameters():
        p.requires_grad = False
    for m in orc.transformer.trans.model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()


def filled_cache(hip, img, n_images=7, views=2, view=1, rows=(5, 0, 6)):
    """a cache larger than the batch whose rows `rows` of view `view` hold the tokens of img"""
    cache = TokenCache(hip, n_images, views=views)
    cache.fill(list(rows), img, view=view)
    return cache, list(rows), [view] * len(rows)


@pytest.mark.parametrize("dropout", [False, True], ids=["plain", "dropout"])
@pytest.mark.parametrize("case", list(CASES))
def test_cached_step_against_the_oracle(case, dropout):
    """logits, loss and every unfrozen gradient within compare_grads' rule (TOL, or 5 x the fp32 oracle's distance from
    its fp64 run); with dropout the oracle applies the engine's masks of the same seed, as frozen_case does.  Frozen
    parameters have no .grad, their range of flat_grads is exactly zero, every BatchNorm buffer is bit-unchanged."""
    kind, kw, drop_kw, pair = CASES[case]
    args = mini_args(**{**kw, **(drop_kw if dropout else {})})
    seed = 21 if dropout else None
    orc, hip = pair(args, seed=0, dropout_seed=seed)
    img, ids, seg, mask, tgt = batch(kind, args)
    freeze_oracle(orc)
    before = {k: v.detach().clone() for k, v in orc.state_dict().items()}
    orc64 = copy.deepcopy(orc).double()
    out_ref = orc(img, ids, seg, mask)
    loss_ref = oracle_loss(kind, out_ref, tgt, B)
    loss_ref.backward()
    oracle_loss(kind, orc64(img.double(), ids, seg, mask), tgt, B).backward()

    hip.freeze_visual().train()
    dimg, dids, dseg, dmask, dtgt = (t.to(dev()) for t in (img, ids, seg, mask, tgt))
    hip.set_seed(5)
    cache, index, view = filled_cache(hip, dimg)
    assert hip._seed_ctr == 5 and hip.training            # the fill restores the dropout counter and the mode
    if dropout:
        hip.set_seed(seed)
    out = hip.forward_cached(cache, index, view, dids, dseg, dmask)
    assert hip._seed_ctr != (seed if dropout else 5)      # ... and a cached step advances it as forward does
    loss = hip_loss(kind, out, dtgt)
    logits, logits_ref = (out[0], out_ref[0]) if kind == "vqa" else (out, out_ref)
    if kind == "vqa":
        assert out[1] == 0 and out[2] == 0
    e = relerr(logits, logits_ref)
    print(f"{case} dropout={dropout}: logits {e:.2e}, loss {float(loss.detach()):.6f} (oracle {float(loss_ref.detach()):.6f})")
    assert e <= TOL, f"logits rel err {e:.2e}"
    assert abs(float(loss) - float(loss_ref)) <= TOL * abs(float(loss_ref)), (float(loss), float(loss_ref))
    loss.backward()
    torch.cuda.synchronize()
    compare_grads(orc, hip, orc64)
    hp = dict(hip.named_parameters())
    frozen = [n for n in hp if n.startswith(VISUAL)]
    assert len(frozen) > 25 and all(hp[n].grad is None and not hp[n].requires_grad for n in frozen)
    assert sum(p.grad is not None for n, p in hp.items() if not n.startswith(VISUAL)) > 20
    lo, hi = hip.token_range()
    assert float(hip.flat_grads[lo:hi].abs().max()) == 0.0, "the frozen range of flat_grads is not exactly zero"
    assert float(hip.flat_grads[:lo].abs().max()) > 0.0 and float(hip.flat_grads[hi:].abs().max()) > 0.0
    hsd = hip.state_dict()
    n_buf = 0
    for k, v in before.items():
        if "running_" in k or k.endswith("num_batches_tracked"):
            assert torch.equal(hsd[k].cpu(), v), f"{k} is not bit-unchanged"
            n_buf += 1
    assert n_buf > 20


def enc_ranges(hip):
    """[(name, lo, hi)] of the tensors outside transformer.trans: embeddings, encoder, heads"""
    return [(n, lo, hi) for n, _, lo, hi in hip._param_ranges() if not n.startswith(VISUAL)]


def test_cached_step_against_the_full_frozen_step():
    """same weights, same dropout seed: the cached step's encoder, heads and embedding gradients against the full
    freeze_backbone(bn_stats="running") step's.  The yardstick is the full step against itself, eight repeats after the
    first (the weight gradients are summed by float atomics; the tokens are pooled by them): the cached step may differ
    from the first full step by at most 3 x the largest difference among the repeats."""
    args = mini_args(transformer_model="realformer", dataset="VQA-Med", **DROPOUT)
    _, hip = build_pair(args, seed=4)
    hip.freeze_backbone(bn_stats="running").train()
    img, ids, seg, mask, tgt = (t.to(dev()) for t in batch("vqa", args))
    lo, hi = hip.token_range()

    def full():
        hip.set_seed(33)
        hip.flat_grads.zero_()
        out = hip(img, ids, seg, mask)[0]
        mmvqa_amd.asl_loss(out, tgt).backward()
        torch.cuda.synchronize()
        g = hip.flat_grads.detach().clone()
        g[lo:hi] = 0                                           # the taps' gradient is the full step's alone
        return out.detach().clone(), g

    l0, g0 = full()
    scale = float(g0.abs().max())
    control = [full() for _ in range(8)]
    n_logits = max(float((l - l0).abs().max()) for l, _ in control) / float(l0.abs().max())
    n_grads = max(float((g - g0).abs().max()) for _, g in control) / scale
    cache, index, view = filled_cache(hip, img)
    hip.set_seed(33)
    hip.flat_grads.zero_()
    out = hip.forward_cached(cache, index, view, ids, seg, mask)[0]
    mmvqa_amd.asl_loss(out, tgt).backward()
    torch.cuda.synchronize()
    g1 = hip.flat_grads.detach().clone()
    assert float(g1[lo:hi].abs().max()) == 0.0
    e_logits = float((out - l0).abs().max()) / float(l0.abs().max())
    e_grads = float((g1 - g0).abs().max()) / scale
    print(f"cached vs full: logits {e_logits:.3e} (control {n_logits:.3e}), gradients {e_grads:.3e} (control {n_grads:.3e})")
    assert e_logits <= 3 * n_logits, f"logits: cached vs full {e_logits:.3e}, full vs itself {n_logits:.3e}"
    assert e_grads <= 3 * n_grads, f"gradients: cached vs full {e_grads:.3e}, full vs itself {n_grads:.3e}"
    worst = max(((float((g1[a:b] - g0[a:b]).abs().max()) / scale, n) for n, a, b in enc_ranges(hip)))
    print("largest per-tensor difference:", worst)


@pytest.mark.parametrize("cnn", ["resnet", "effnet"])
def test_cached_step_launches_nothing_below_the_tokens(cnn):
    """Model.profile's counts per region: a cached forward + backward shows no launch in backbone, tap and bn_coef, and
    the counts of the full step everywhere above the tokens"""
    args = mini_args(**(EFF if cnn == "effnet" else {}))
    _, hip = build_pair(args, seed=2)
    hip.train()
    img, ids, seg, mask, tgt = (t.to(dev()) for t in batch("mlm", args))
    cache, index, view = filled_cache(hip, img)

    def full():
        mmvqa_amd.mlm_loss(hip(img, ids, seg, mask), tgt)[0].backward()

    def cached():
        mmvqa_amd.mlm_loss(hip.forward_cached(cache, index, view, ids, seg, mask), tgt)[0].backward()

    f, c = region_launches(hip, full), region_launches(hip, cached)
    print(f"{cnn}: full {f}\n cached {c}")
    assert c["backbone"] == 0 and c["tap"] == 0 and c["bn_coef"] == 0
    assert f["backbone"] > 0 and f["tap"] > 0
    for reg in ("qkv", "attention", "encoder_rest", "heads", "embed", "qkv_attention_fused"):
        assert c[reg] == f[reg], reg


def test_engine_state_machine():
    """after forward_cached both backward entry points of the full path answer MMVQA_ERR_STATE; after a plain forward
    the cached backward does; a plain step directly after a cached one gives the gradients it gives without it"""
    args = mini_args(dataset="VQA-Med")
    _, hip = build_pair(args, seed=6)
    hip.train()
    img, ids, seg, mask, tgt = (t.to(dev()) for t in batch("vqa", args))
    lib, h, st = L.lib(), hip._handle, L.stream_ptr

    def plain():
        hip.set_seed(3)
        hip.flat_grads.zero_()
        out = hip(img, ids, seg, mask)[0]
        mmvqa_amd.asl_loss(out, tgt).backward()
        torch.cuda.synchronize()
        return out.detach().clone(), hip.flat_grads.detach().clone()

    l0, g0 = plain()
    ctl = [plain() for _ in range(3)]
    cache, index, view = filled_cache(hip, img)
    out = hip.forward_cached(cache, index, view, ids, seg, mask)[0]
    V = out.shape[1]
    ld = (V + 3) & ~3
    g = torch.zeros(B, ld, device=dev())
    dA = torch.zeros(1 << 16, device=dev())
    assert lib.mmvqa_engine_backward(h, st(), L.ptr(g), ld, None) == -3
    assert b"engine_backward: run forward first" in lib.mmvqa_last_error()
    assert lib.mmvqa_engine_backward_feature(h, st(), L.ptr(g), ld, L.ptr(dA)) == -3
    assert b"the last forward ran from given visual tokens" in lib.mmvqa_last_error()
    mmvqa_amd.asl_loss(out, tgt).backward()               # the cached backward itself is still valid
    # the tokens the cached forward ran from are where mmvqa_engine_visual_tokens says
    assert torch.equal(hip._read_visual_tokens(B), cache.tokens[index, view])
    l1, g1 = plain()
    n0 = max(float((c[1] - g0).abs().max()) for c in ctl)
    assert float((l1 - l0).abs().max()) <= 3 * max(float((c[0] - l0).abs().max()) for c in ctl)
    assert float((g1 - g0).abs().max()) <= 3 * n0, (float((g1 - g0).abs().max()), n0)
    assert lib.mmvqa_engine_backward_cached(h, st(), L.ptr(g), ld, None) == -3
    assert b"engine_backward_cached: run mmvqa_engine_forward_cached first" in lib.mmvqa_last_error()
    # eval-mode tokens (forward_tokens) do not open the cached backward either
    hip.eval()
    hip.forward_tokens(cache.tokens[index, view], ids, seg, mask)
    assert lib.mmvqa_engine_backward_cached(h, st(), L.ptr(g), ld, None) == -3
    # a grouped plan refuses the cached forward
    hip.train()
    hip.forward_grouped(img, [0, 1, 2], ids, seg, mask)
    with pytest.raises(mmvqa_amd.MMVQAError, match="forward_cached: the last step was a grouped one"):
        hip.forward_cached(cache, index, view, ids, seg, mask)
    maps = torch.tensor(index + view, dtype=torch.int32, device=dev())
    buf = torch.empty(B, ld, device=dev())
    assert lib.mmvqa_engine_forward_cached(h, st(), L.ptr(cache.tokens), 7, 2, L.ptr(maps), C.c_void_p(maps.data_ptr() + 4 * B),
                                           L.ptr(ids), L.ptr(seg), L.ptr(mask), L.ptr(buf), ld, None, 1, 9) == -3
    assert b"engine_forward_cached: the plan is grouped" in lib.mmvqa_last_error()
    with torch.autocast("cuda", dtype=torch.float16):
        with pytest.raises(NotImplementedError, match="fp32 in this version"):
            hip.forward_cached(cache, index, view, ids, seg, mask)


def test_unfrozen_taps_get_nothing_from_a_cached_step():
    """without freeze_visual the parameters under transformer.trans. still receive nothing: their .grad stays what it
    was (None), their range of flat_grads keeps its contents, and the announcements partition the buffer"""
    args = mini_args()
    _, hip = build_pair(args, seed=8)
    hip.train()
    img, ids, seg, mask, tgt = (t.to(dev()) for t in batch("mlm", args))
    cache, index, view = filled_cache(hip, img)
    lo, hi = hip.token_range()
    hip.flat_grads[lo:hi] = 1.5
    done = []
    hip.set_grad_ready_hook(lambda a, b: done.append((a, b)))
    mmvqa_amd.mlm_loss(hip.forward_cached(cache, index, view, ids, seg, mask), tgt)[0].backward()
    hip.set_grad_ready_hook(None)
    torch.cuda.synchronize()
    done.sort()
    n = hip.flat_params.numel()
    assert done[0][0] == 0 and done[-1][1] == n and all(x[1] == y[0] for x, y in zip(done, done[1:])), done
    assert (lo, hi) in done
    assert bool((hip.flat_grads[lo:hi] == 1.5).all())
    hp = dict(hip.named_parameters())
    assert all(p.grad is None for nme, p in hp.items() if nme.startswith(VISUAL))
    assert sum(p.grad is not None for nme, p in hp.items() if not nme.startswith(VISUAL)) > 20


def test_fingerprint_save_and_load(tmp_path):
    """check passes on the model that filled the cache and raises once a backbone weight, a tap or a running statistic
    moves; save / load round-trip tokens and fingerprint"""
    args = mini_args(dataset="VQA-Med")
    _, hip = build_pair(args, seed=1)
    img = batch("vqa", args)[0].to(dev())
    cache, index, view = filled_cache(hip, img)
    cache.check(hip)
    path = str(tmp_path / "cache.npz")
    cache.save(path)
    twin = TokenCache(hip, 7, views=2).load(path)
    assert torch.equal(twin.tokens, cache.tokens) and torch.equal(twin.fingerprint, cache.fingerprint)
    twin.check(hip)
    with pytest.raises(ValueError, match="this cache is"):
        TokenCache(hip, 6, views=2).load(path)
    hp = dict(hip.named_parameters())
    # the tokens are visual_tokens' own.  Not bit for bit: a token is a mean over the feature map's positions summed by
    # float atomics, whose order differs from run to run (at most 256 positions here: a few 1e-6).  A wrong row, view or
    # image is an O(1) difference; the bound is a tenth of the parity tolerance.
    e = relerr(cache.tokens[index, view], hip.visual_tokens(img))
    print(f"cache.fill vs visual_tokens: {e:.2e}")
    assert e <= TOL / 10
    assert float(cache.tokens[[1, 2, 3, 4]].abs().max()) == 0.0 and float(cache.tokens[index, 0].abs().max()) == 0.0
    for name in ("transformer.trans.model.layer2.0.conv1.weight", "transformer.trans.conv3.weight"):
        with torch.no_grad():
            keep = hp[name].detach().clone()
            hp[name][(0,) * hp[name].dim()] += 0.25
        with pytest.raises(mmvqa_amd.MMVQAError, match="the token cache is stale"):
            cache.check(hip)
        with pytest.raises(mmvqa_amd.MMVQAError, match="TokenCache.fill: the model has changed since this cache's first fill"):
            cache.fill([1], img[:1], view=0)                # a later fill from other weights would pass check() afterwards
        with torch.no_grad():
            hp[name].copy_(keep)
        cache.check(hip)
    cache.fill([1], img[:1], view=0)
    # freeze_visual and its inverse
    hip.freeze_visual()
    hip.unfreeze_backbone()
    assert not hp["transformer.trans.conv3.weight"].requires_grad and hp["transformer.trans.model.conv1.weight"].requires_grad
    hip.freeze_visual().unfreeze_visual()
    assert all(p.requires_grad for p in hp.values()) and hip._frozen_state()[0] == 0
    rv = dict(hip.named_buffers())["transformer.trans.model.bn1.running_var"]
    keep = rv.clone()
    rv[0] += 0.5
    with pytest.raises(mmvqa_amd.MMVQAError, match="the token cache is stale"):
        twin.check(hip)
    with torch.no_grad():                                   # an encoder weight is none of the cache's business
        rv.copy_(keep)
        hp["classifier.2.weight"].mul_(2.0)
    cache.check(hip)
